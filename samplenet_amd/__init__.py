"""samplenet_amd -- MI355X-native implementation of the SampleNet differentiable-sampling hot path.

Public surface mirrors `registration/src/__init__.py` of itailang/SampleNet for this path:
    from samplenet_amd import ChamferDistance, FPSSampler, RandomSampler, SampleNet, SoftProjection, sputils
Importing the package loads libsamplenet_hip.so (hand-written HIP for gfx950) and fails loudly if it
is missing -- there is no CPU or eager-PyTorch fallback.
"""
from . import _lib  # noqa: F401  (loads the HIP library or raises)
from . import ops, optim, sputils  # noqa: F401
from .autoencoder import PointNetAE, reconstruction_loss  # noqa: F401
from .device_data import BatchRecipe, DeviceBatchSource, DeviceCloudSet  # noqa: F401
from .classifier import PointNetCls, PointNetClsBasic, classification_loss  # noqa: F401
from .chamfer_distance import ChamferDistance, ChamferDistanceFunction  # noqa: F401
from .qtransform import QuaternionTransform, deg_to_rad, qinv, rad_to_deg  # noqa: F401
from .progressive import SampleNetProgressive, progressive_sizes  # noqa: F401
from .samplenet import SampleNet  # noqa: F401
from .evaluation import (ClassificationEvaluator, ProgressiveClassificationEvaluator,  # noqa: F401
                         ProgressiveReconstructionEvaluator, ProgressiveRetrievalEvaluator, ReconstructionEvaluator,
                         RegistrationEvaluator, RetrievalEvaluator, SegmentationEvaluator, classification_aggregates,
                         retrieval_aggregates, segmentation_aggregates)
from .samplers import FPSSampler, RandomSampler  # noqa: F401
from .segmentation import segmentation_loss  # noqa: F401
from .soft_projection import SoftProjection  # noqa: F401

__all__ = ["ChamferDistance", "ChamferDistanceFunction", "SoftProjection", "SampleNet", "FPSSampler", "RandomSampler", "SampleNetProgressive",
           "progressive_sizes", "PointNetAE", "reconstruction_loss", "PointNetCls", "PointNetClsBasic", "classification_loss",
           "sputils", "ops", "optim", "BatchRecipe", "DeviceBatchSource", "DeviceCloudSet", "QuaternionTransform", "qinv", "rad_to_deg",
           "deg_to_rad", "RegistrationEvaluator", "ClassificationEvaluator", "ReconstructionEvaluator",
           "ProgressiveClassificationEvaluator", "ProgressiveReconstructionEvaluator", "classification_aggregates",
           "RetrievalEvaluator", "ProgressiveRetrievalEvaluator", "retrieval_aggregates", "SegmentationEvaluator",
           "segmentation_aggregates", "segmentation_loss"]

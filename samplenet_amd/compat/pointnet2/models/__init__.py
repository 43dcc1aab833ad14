"""Pointnet2_PyTorch's `pointnet2.models`, on the kernels of libsamplenet_hip.so: the single-scale semantic-segmentation network."""
from .pointnet2_ssg_sem import PointNet2SemSegSSG  # noqa: F401

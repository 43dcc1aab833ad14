"""CPU-side tests of the reconstruction autoencoder: the module is exported, its state_dict is an ordinary torch one, TF-named variables load with the right transposes, no CPU route."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from torch_ae import torch_ae_copy  # noqa: E402

def test_module_is_exported_and_adds_no_c_entry():
    """The autoencoder is built from the library's existing entries (the single-launch decoder kernels the issue proposed lost to the
    sn_skinny_linear composition and were kept out, as the issue rules for that outcome): the package exports the module and the loss,
    and every entry the module calls -- itself or through the layer walk and the skinny-GEMM wrappers it drives (pointnet.py,
    task_features.py) -- is in the prototype table."""
    import inspect

    import samplenet_amd
    from samplenet_amd import _lib, autoencoder, pointnet, task_features

    assert {"PointNetAE", "reconstruction_loss"} <= set(samplenet_amd.__all__)
    assert not [n for n in _lib.PROTOTYPES if n.startswith("sn_ae_")]
    used = set(__import__("re").findall(r"lib\.(sn_[a-z0-9_]+)", "".join(inspect.getsource(m) for m in (autoencoder, pointnet, task_features))))
    assert used and used <= set(_lib.PROTOTYPES), used - set(_lib.PROTOTYPES)


def test_state_dict_is_an_ordinary_torch_one():
    from samplenet_amd import PointNetAE

    sd = PointNetAE().state_dict()
    widths = (3, 64, 128, 128, 256, 128)
    want = {}
    for i in range(1, 6):
        want["conv%d.weight" % i], want["conv%d.bias" % i] = (widths[i], widths[i - 1], 1), (widths[i],)
        for k in ("weight", "bias", "running_mean", "running_var"):
            want["bn%d.%s" % (i, k)] = (widths[i],)
        want["bn%d.num_batches_tracked" % i] = ()
    for i, (ci, co) in enumerate(((128, 256), (256, 256), (256, 6144)), 1):
        want["fc%d.weight" % i], want["fc%d.bias" % i] = (co, ci), (co,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert tuple(PointNetAE(n_pc_points=512, bottleneck_size=64).state_dict()["fc3.weight"].shape) == (1536, 256)


@pytest.mark.parametrize("conv_rank", [4, 3])
def test_load_tf_variables_matches_numpy_evaluation_of_the_tf_layout(conv_rank):
    from samplenet_amd import PointNetAE

    rng = np.random.default_rng(5)
    widths = (3, 64, 128, 128, 256, 128)
    n_pc = 32
    tf = {}
    for i in range(5):
        ci, co = widths[i], widths[i + 1]
        w = rng.standard_normal((ci, co)) / np.sqrt(ci)
        tf["single_class_ae/encoder_conv_layer_%d/W:0" % i] = w.reshape((1, 1, ci, co) if conv_rank == 4 else (1, ci, co))
        tf["single_class_ae/encoder_conv_layer_%d/b:0" % i] = 0.1 * rng.standard_normal(co)
        pre = "single_class_ae/encoder_conv_layer_%d_bnorm/" % i
        tf[pre + "gamma:0"], tf[pre + "beta:0"] = 1 + 0.1 * rng.standard_normal(co), 0.1 * rng.standard_normal(co)
        tf[pre + "moving_mean:0"], tf[pre + "moving_variance:0"] = 0.1 * rng.standard_normal(co), 0.5 + rng.random(co)
    for i, (ci, co) in enumerate(((128, 256), (256, 256), (256, 3 * n_pc))):
        tf["single_class_ae/decoder_fc_%d/W:0" % i] = rng.standard_normal((ci, co)) / np.sqrt(ci)
        tf["single_class_ae/decoder_fc_%d/b:0" % i] = 0.1 * rng.standard_normal(co)
    tf["single_class_ae/beta1_power:0"] = np.float32(0.9)  # (optimizer slots of a checkpoint are ignored)
    eps = 1e-3
    ae = PointNetAE(n_pc_points=n_pc, bn_eps=eps).load_tf_variables(tf)
    ref = torch_ae_copy(ae.state_dict(), n_pc_points=n_pc, bn_eps=eps, dtype=torch.float64).eval()
    x = rng.standard_normal((3, 20, 3))
    # the TF graph, evaluated directly on the TF layout: x @ W + b with W (Ci, Co), inference-mode batch norm, relu; max; fc
    h = x
    for i in range(5):
        pre = "single_class_ae/encoder_conv_layer_%d" % i
        h = h @ tf[pre + "/W:0"].reshape(widths[i], widths[i + 1]) + tf[pre + "/b:0"]
        h = (h - tf[pre + "_bnorm/moving_mean:0"]) / np.sqrt(tf[pre + "_bnorm/moving_variance:0"] + eps) * tf[pre + "_bnorm/gamma:0"] \
            + tf[pre + "_bnorm/beta:0"]
        h = np.maximum(h, 0)
    h = h.max(axis=1)
    for i in range(3):
        h = h @ tf["single_class_ae/decoder_fc_%d/W:0" % i] + tf["single_class_ae/decoder_fc_%d/b:0" % i]
        if i < 2:
            h = np.maximum(h, 0)
    want = h.reshape(3, n_pc, 3)
    with torch.no_grad():
        got = ref(torch.from_numpy(x)).numpy()
    # the module holds the variables in fp32: the comparison carries their rounding (2^-24 relative per weight) and nothing else
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    with pytest.raises(ValueError):
        PointNetAE(n_pc_points=n_pc).load_tf_variables({**tf, "single_class_ae/decoder_fc_0/W:0": np.zeros((256, 128))})
    with pytest.raises(KeyError):
        PointNetAE(n_pc_points=n_pc).load_tf_variables({k: v for k, v in tf.items() if "decoder_fc_2/b" not in k})


def test_no_cpu_route():
    from samplenet_amd import PointNetAE, reconstruction_loss

    ae = PointNetAE(n_pc_points=16)
    with pytest.raises(RuntimeError):
        ae(torch.zeros(2, 8, 3))
    with pytest.raises(RuntimeError):
        ae.decode(torch.zeros(2, 128))
    with pytest.raises(RuntimeError):
        reconstruction_loss(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))

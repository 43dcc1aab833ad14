"""CPU-side tests of the classification task network: the transform / regulariser entries exist, are declared and validate their
arguments without a GPU; the module's state_dict is the documented one and starts with identity transforms; no CPU route."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from torch_cls import torch_cls_copy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sn_cloud_transform_forward", "sn_cloud_transform_backward", "sn_orthogonality_loss_forward", "sn_orthogonality_loss_backward",
           "sn_bn_relu_forward", "sn_bn_relu_backward")
SN_ERR_BAD_ARGUMENT = 10001
P = 4096  # a non-NULL pointer value: argument checks come before any device work and never dereference it


def test_entries_are_exported_declared_and_prototyped():
    import samplenet_amd
    from samplenet_amd import _lib

    assert {"PointNetCls", "PointNetClsBasic", "classification_loss"} <= set(samplenet_amd.__all__)
    internal = open(os.path.join(ROOT, "include", "samplenet_hip_internal.h")).read()
    public = open(os.path.join(ROOT, "include", "samplenet_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name), name
        assert re.search(r"\bint %s\(" % name, internal), name
        assert not re.search(r"\bint %s\(" % name, public), name


def _bad(name, *args):
    from samplenet_amd import _lib

    rc = getattr(_lib.lib, name)(*args)
    msg = (_lib.lib.sn_last_error_string() or b"").decode()
    assert rc == SN_ERR_BAD_ARGUMENT, (name, args, rc)
    assert msg.startswith(name), (name, msg)


def test_bad_arguments_answer_without_a_gpu():
    from samplenet_amd import _lib

    lib = _lib.lib
    for K in (0, 4, 32, 65, -3):  # K outside {3, 64}
        _bad("sn_cloud_transform_forward", 2, 8, K, P, P, P, None)
        _bad("sn_cloud_transform_backward", 2, 8, K, P, P, P, P, P, None)
        _bad("sn_orthogonality_loss_forward", 2, K, P, P, P, None)
        _bad("sn_orthogonality_loss_backward", 2, K, P, P, P, None)
    for B, N in ((-1, 8), (2, -8)):  # negative sizes
        _bad("sn_cloud_transform_forward", B, N, 64, P, P, P, None)
        _bad("sn_cloud_transform_backward", B, N, 3, P, P, P, P, P, None)
    _bad("sn_orthogonality_loss_forward", -1, 64, P, P, P, None)
    _bad("sn_orthogonality_loss_backward", -1, 64, P, P, P, None)
    for i in range(3):  # NULL required pointers
        a = [P, P, P]
        a[i] = None
        _bad("sn_cloud_transform_forward", 2, 8, 64, *a, None)
        _bad("sn_orthogonality_loss_forward", 2, 64, *a, None)
        _bad("sn_orthogonality_loss_backward", 2, 64, *a, None)
    _bad("sn_cloud_transform_backward", 2, 8, 64, P, P, None, P, P, None)  # dY
    _bad("sn_cloud_transform_backward", 2, 8, 64, P, None, P, P, None, None)  # dX wanted, no T
    _bad("sn_cloud_transform_backward", 2, 8, 64, None, P, P, None, P, None)  # dT wanted, no X
    _bad("sn_bn_relu_forward", -1, 64, P, P, P, None)
    _bad("sn_bn_relu_forward", 4, 6, P, P, P, None)
    _bad("sn_bn_relu_forward", 4, 64, P, None, P, None)
    _bad("sn_bn_relu_backward", 4, -64, P, P, P, 0, P, None)
    _bad("sn_bn_relu_backward", 4, 64, P, P, None, 0, P, None)
    # B == 0 (no rows): a no-op that succeeds
    assert lib.sn_cloud_transform_forward(0, 8, 64, P, P, P, None) == 0
    assert lib.sn_cloud_transform_backward(0, 8, 3, P, P, P, P, P, None) == 0
    assert lib.sn_orthogonality_loss_forward(0, 64, P, P, P, None) == 0
    assert lib.sn_orthogonality_loss_backward(0, 64, P, P, P, None) == 0
    assert lib.sn_bn_relu_forward(0, 64, P, P, P, None) == 0
    assert lib.sn_bn_relu_backward(0, 64, P, P, P, 1, P, None) == 0
    # ... also for a caller that has no buffers for its empty batch
    assert lib.sn_cloud_transform_forward(0, 8, 64, None, None, None, None) == 0
    assert lib.sn_cloud_transform_backward(0, 8, 64, None, None, None, None, None, None) == 0
    assert lib.sn_orthogonality_loss_forward(0, 64, None, None, None, None) == 0
    assert lib.sn_orthogonality_loss_backward(0, 64, None, None, None, None) == 0
    assert lib.sn_bn_relu_forward(0, 64, None, None, None, None) == 0
    assert ctypes.sizeof(ctypes.c_void_p) == 8


def _want_keys(basic):
    want = {}

    def lin(name, co, ci, conv):
        want[name + ".weight"], want[name + ".bias"] = ((co, ci, 1) if conv else (co, ci)), (co,)

    def bn(name, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            want["%s.%s" % (name, k)] = (c,)
        want[name + ".num_batches_tracked"] = ()

    if not basic:
        for t, K in (("transform_net1", 3), ("transform_net2", 64)):
            w = (K, 64, 128, 1024)
            for i in range(1, 4):
                lin("%s.tconv%d" % (t, i), w[i], w[i - 1], True)
                bn("%s.bn%d" % (t, i), w[i])
            lin(t + ".tfc1", 512, 1024, False), bn(t + ".bn4", 512)
            lin(t + ".tfc2", 256, 512, False), bn(t + ".bn5", 256)
            lin(t + ".transform", K * K, 256, False)
    w = (3, 64, 64, 64, 128, 1024)
    for i in range(1, 6):
        lin("conv%d" % i, w[i], w[i - 1], True)
        bn("bn%d" % i, w[i])
    lin("fc1", 512, 1024, False), bn("bn_fc1", 512)
    lin("fc2", 256, 512, False), bn("bn_fc2", 256)
    lin("fc3", 40, 256, False)
    return want


@pytest.mark.parametrize("basic", [False, True])
def test_state_dict_is_the_documented_one_and_starts_with_identity_transforms(basic):
    from samplenet_amd import PointNetCls, PointNetClsBasic

    net = (PointNetClsBasic if basic else PointNetCls)()
    sd = net.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == _want_keys(basic)
    if not basic:
        for t, K in (("transform_net1", 3), ("transform_net2", 64)):
            assert not bool(sd[t + ".transform.weight"].any())
            assert torch.equal(sd[t + ".transform.bias"], torch.eye(K).flatten())
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            assert m.eps == 1e-3 and m.momentum == 0.1
    ref = torch_cls_copy(sd, basic=basic)  # strict=True inside
    assert set(ref.state_dict()) == set(sd)
    assert tuple(PointNetCls(num_classes=10).state_dict()["fc3.weight"].shape) == (10, 256)


def test_no_cpu_route():
    from samplenet_amd import PointNetCls, PointNetClsBasic, classification_loss
    from samplenet_amd.classifier import cloud_transform, orthogonality_loss

    with pytest.raises(RuntimeError):
        PointNetCls()(torch.zeros(2, 8, 3))
    with pytest.raises(RuntimeError):
        PointNetClsBasic()(torch.zeros(2, 8, 3))
    with pytest.raises(RuntimeError):
        classification_loss(torch.zeros(2, 40), torch.zeros(2, dtype=torch.long), {})
    with pytest.raises(RuntimeError):
        cloud_transform(torch.zeros(2, 8, 3), torch.zeros(2, 3, 3))
    with pytest.raises(RuntimeError):
        orthogonality_loss(torch.zeros(2, 64, 64))

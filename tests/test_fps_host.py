"""Farthest-point sampling without a GPU: argument validation of sn_furthest_point_sample (codes and messages before any device
work), its workspace query and variant hook, the compat / sampler surface, and the test's numpy restatement of the contract
against the fixture emulating the reference's in-tree kernel (tests/golden/make_fps_golden.py)."""
import ctypes
import importlib
import warnings

import numpy as np
import pytest
import torch

from fps_numpy import fps_restated

BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
FAKE = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch


@pytest.fixture()
def lib():
    from samplenet_amd._lib import lib

    prev = lib.sn_fps_set_variant(0)
    yield lib
    lib.sn_fps_set_variant(prev)


def _fps(lib, B, N, M, xyz=FAKE, layout=0, temp=None, idx=FAKE):
    return lib.sn_furthest_point_sample(B, N, M, xyz, layout, temp, idx, None)


def test_argument_errors_are_reported_without_a_gpu(lib):
    for B, N, M in ((-1, 10, 4), (2, -1, 4), (2, 10, -3)):
        assert _fps(lib, B, N, M) == BAD_ARGUMENT and b"negative" in lib.sn_last_error_string()
    assert _fps(lib, 2, 10, 4, layout=2) == BAD_ARGUMENT and b"layout" in lib.sn_last_error_string()
    assert _fps(lib, 2, 0, 4) == BAD_ARGUMENT and b"N = 0" in lib.sn_last_error_string()
    assert _fps(lib, 2, 10, 4, xyz=None) == BAD_ARGUMENT and b"null" in lib.sn_last_error_string()
    assert _fps(lib, 2, 10, 4, idx=None) == BAD_ARGUMENT and b"null" in lib.sn_last_error_string()
    # the streaming path needs the caller's temp; register-resident shapes do not
    assert _fps(lib, 1, 40000, 16) == BAD_ARGUMENT and b"temp" in lib.sn_last_error_string()
    # empty work is a no-op, whatever the pointers
    assert _fps(lib, 0, 10, 4, xyz=None, idx=None) == 0
    assert _fps(lib, 0, 0, 4, xyz=None, idx=None) == 0
    assert _fps(lib, 3, 10, 0, xyz=None, idx=None) == 0


def test_variant_hook_and_workspace_query(lib):
    ws = lambda B, N, M: lib.sn_workspace_bytes(b"furthest_point_sample", B, N, M, 0)  # noqa: E731
    assert ws(32, 1024, 64) == 0 and ws(50, 2048, 2048) == 0 and ws(8, 16384, 1024) == 0  # registers
    assert ws(4, 16385, 64) == 4 * 16385 * 4 and ws(1, 100000, 4096) == 100000 * 4  # streaming: B*N floats
    assert ws(0, 100000, 4) == 0 and ws(-1, 5, 5) == 0
    assert lib.sn_fps_set_variant(3) == 0
    assert ws(32, 1024, 64) == 32 * 1024 * 4  # forced streaming
    assert _fps(lib, 2, 100, 8) == BAD_ARGUMENT and b"temp" in lib.sn_last_error_string()
    assert lib.sn_fps_set_variant(1) == 3
    assert _fps(lib, 2, 2049, 8) == UNSUPPORTED and b"variant 1" in lib.sn_last_error_string()
    assert ws(2, 2049, 8) == 0
    assert lib.sn_fps_set_variant(2) == 1
    assert _fps(lib, 2, 16385, 8) == UNSUPPORTED
    assert lib.sn_fps_set_variant(7) == -1 and lib.sn_fps_set_variant(0) == 2  # out of range: no change


def test_ops_refuse_cpu_tensors():
    from samplenet_amd import ops

    with pytest.raises(RuntimeError):
        ops.furthest_point_sample(torch.zeros(2, 16, 3), 4)
    with pytest.raises(RuntimeError):
        ops.gather_operation(torch.zeros(2, 3, 16), torch.zeros(2, 4, dtype=torch.int32))


def test_compat_exposes_every_pointnet2_name_the_reference_imports():
    """registration/src/soft_projection.py:8 (grouping_operation), fps.py:4-5 (furthest_point_sample, gather_operation),
    random_sampling.py:4 (gather_operation) -- all resolve after compat.install()."""
    from samplenet_amd import compat, ops

    compat.install()
    pu = importlib.import_module("pointnet2.utils.pointnet2_utils")
    for name in ("grouping_operation", "furthest_point_sample", "gather_operation"):
        assert callable(getattr(pu, name)), name
    with pytest.raises(RuntimeError):  # the shim is the product path: GPU only
        pu.furthest_point_sample(torch.zeros(1, 8, 3), 2)
    assert ops.furthest_point_sample.__module__ == "samplenet_amd.ops"


@pytest.mark.parametrize("cls,args,name", [("FPSSampler", (16, True), "fps"), ("RandomSampler", (16,), "random")])
def test_sampler_constructors_match_the_reference(cls, args, name):
    import samplenet_amd

    S = getattr(samplenet_amd, cls)
    s = S(*args, input_shape="bnc", output_shape="bnc")
    assert s.name == name and s.num_out_points == 16 and s.input_shape == "bnc" and s.output_shape == "bnc"
    assert S(*args).input_shape == "bcn" and S(*args).output_shape == "bcn"
    with pytest.raises(ValueError):
        S(*args, input_shape="nbc")
    with pytest.raises(ValueError):
        S(*args, output_shape="bcn ")
    with pytest.warns(UserWarning):
        S(*args, input_shape="bnc", output_shape="bcn")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        S(*args, input_shape="bcn", output_shape="bcn")
    assert list(S(*args).parameters()) == []
    with pytest.raises(RuntimeError):
        s(torch.zeros(2, 32, 3))


def test_restatement_equals_the_emulated_reference_kernel(golden):
    """On tie-free clouds the reference's in-tree kernel (slot-first tie rule, 1e38 start) and this project's contract (lowest
    index, +inf start) pick the same sequence: the restatement the GPU tests hold the kernel to is the farthest-point sequence."""
    g = golden("fps_reference.npz")
    assert g["xyz_full"].shape == (2, 2048, 3) and g["xyz_64"].shape == (4, 1024, 3)
    assert np.array_equal(fps_restated(g["xyz_full"], 2048), g["idx_full"])
    assert np.array_equal(fps_restated(g["xyz_64"], 64), g["idx_64"])
    assert (g["idx_full"] >= 0).all() and len(np.unique(g["idx_full"][0])) == 2048  # a full ordering is a permutation


def test_restatement_rules():
    """The contract's corner rules, as the restatement states them: ties to the lowest index, M > N returns to 0, NaN stays
    in range."""
    sq = np.array([[[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 0]]], np.float32)  # 1, 2, 3 tie at step 1
    assert fps_restated(sq, 7)[0].tolist() == [0, 1, 2, 3, 0, 0, 0]
    nan = np.array([[[0, 0, 0], [np.nan, 0, 0], [2, 0, 0]]], np.float32)
    assert fps_restated(nan, 4)[0].tolist() == [0, 1, 1, 1]  # the NaN point's minimum stays +inf
    assert fps_restated(np.zeros((0, 5, 3), np.float32), 3).shape == (0, 3)

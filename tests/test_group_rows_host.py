"""The yardsticks of the set-abstraction entries held to what they restate (no GPU): the row-layout grouping to tests/ball_ref.py's
channel-major one (which tests/test_ball_host.py holds to the reference's compiled CPU twin), the sequential float32 sum to float64
and to the list-by-list walk over numpy's stable argsort, the centre's sum to float64, the pool yardstick to torch float64 amax /
amin; then the stand-in modules' state-dict keys and shapes, and the torch composition (fused=False) on CPU tensors."""
import numpy as np
import pytest
import torch

import ball_ref as R
import group_rows_ref as GR

SMALL = [s for s in GR.SHAPES if s[0] * s[2] * s[3] <= 5000]


@pytest.mark.parametrize("recipe", GR.RECIPES, ids=[r[0] for r in GR.RECIPES])
@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_grouping_yardstick_is_ball_refs_permuted(shape, recipe):
    b, n, m, ns = shape
    P, Q, radius = R.make_case(shape, recipe)
    feat = np.random.default_rng(1).standard_normal((b, n, 5)).astype(np.float32)
    for rule in R.RULES:
        idx, cnt = R.ball_query(P, Q, radius, ns, rule)
        if recipe[0] == "empty":
            assert not cnt.any() and not idx.any()
        for c, u in ((0, 1), (5, 0), (5, 1)):
            rows = GR.group_rows(P, Q, feat[:, :, :c], idx, u)
            want = R.group(P, Q, np.ascontiguousarray(feat[:, :, :c].transpose(0, 2, 1)), idx, u)
            assert rows.shape == (b, m, ns, 3 * u + c)
            assert np.array_equal(rows.view(np.int32), np.ascontiguousarray(want.transpose(0, 2, 3, 1)).view(np.int32))


@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_sequential_sum_is_the_list_walk_and_close_to_float64(shape):
    b, n, m, ns = shape
    rng = np.random.default_rng(R._seed(shape, 21))
    idx = rng.integers(0, n, (b, m * ns))
    idx[:, ::3] = 0                                         # a long list at point 0
    g = rng.standard_normal((b, m * ns, 4)).astype(np.float32)
    got = GR.sequential_sum(n, idx, g)
    assert np.array_equal(got.view(np.int32), GR.sequential_sum_by_lists(n, idx, g).view(np.int32))
    for start, order in GR.invert(idx, n):                  # the lists ascend, and a stable sort is what orders them
        assert all(np.all(np.diff(order[start[r]:start[r + 1]]) > 0) for r in range(n))
    s, sab, mult = GR.scatter_f64(n, idx, g)
    assert (np.abs(got - s) <= mult[:, :, None] * GR.U * sab).all()
    gi = rng.integers(-3, 4, g.shape).astype(np.float32)   # integer terms: exact in any order
    assert np.array_equal(GR.sequential_sum(n, idx, gi), GR.scatter_f64(n, idx, gi)[0])


def test_sequential_sum_depends_on_the_order():
    g = np.array([[[1.0], [2.0 ** -24], [2.0 ** -24], [-1.0]]], np.float32)
    idx = np.zeros((1, 4), np.int64)
    assert GR.sequential_sum(1, idx, g)[0, 0, 0] == 0.0     # ascending: the two small terms are rounded away one by one
    assert GR.sequential_sum(1, idx, g[:, ::-1])[0, 0, 0] != 0.0


@pytest.mark.parametrize("ns", [1, 3, 64, 69, 200])
def test_centre_sum(ns):
    rng = np.random.default_rng(ns)
    g = rng.standard_normal((2, 3, ns, 3)).astype(np.float32)
    got = GR.centre_sum(g)
    ref = -g.astype(np.float64).sum(2)
    assert (np.abs(got - ref) <= ns * GR.U * np.abs(g).astype(np.float64).sum(2)).all()
    gi = rng.integers(-3, 4, g.shape).astype(np.float32)
    assert np.array_equal(GR.centre_sum(gi), -gi.sum(2))


@pytest.mark.parametrize("S", [1, 3, 16])
def test_pool_yardstick_against_torch_float64(S):
    z, scale, shift = GR.pool_case(5, S, 7, S)
    pooled, arg, zsel = GR.group_pool(z, scale, shift)
    z64 = torch.from_numpy(z).double()
    ext = torch.where(torch.from_numpy(scale) >= 0, z64.amax(1), z64.amin(1)).numpy()
    assert np.array_equal(zsel.astype(np.float64), ext)
    assert np.array_equal(np.take_along_axis(z, arg[:, None, :].astype(np.int64), 1)[:, 0], zsel)
    for gi in range(5):                                     # the first row that holds the extreme
        for c in range(7):
            assert arg[gi, c] == np.flatnonzero(z[gi, :, c] == zsel[gi, c])[0]
    if S >= 2:
        assert (arg[:, ::2] < S - 1).all() and (scale < 0).any() and (scale > 0).any()
    ref = np.maximum(ext * scale.astype(np.float64) + shift.astype(np.float64), 0.0)
    assert (np.abs(pooled - ref) <= GR.U * np.abs(ref)).all()


def test_modules_state_dict_and_torch_composition_on_cpu():
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    msg = PM.PointnetSAModuleMSG(8, (0.3, 0.6), (4, 16), ((5, 16, 32), (5, 32, 64)))
    sd = msg.state_dict()
    assert len(msg.groupers) == 2 and len(msg.mlps) == 2
    assert sd["mlps.0.0.conv.weight"].shape == (16, 8, 1, 1) and sd["mlps.1.1.conv.weight"].shape == (64, 32, 1, 1)
    assert "mlps.0.0.conv.bias" not in sd and sd["mlps.1.0.bn.running_var"].shape == (32,)
    assert {k[len("mlps.0.0."):] for k in sd if k.startswith("mlps.0.0.")} == {
        "conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}
    one = PM.PointnetSAModule([5, 16, 32], npoint=4, radius=0.5, nsample=8, use_xyz=False)
    assert one.state_dict()["mlps.0.0.conv.weight"].shape == (16, 5, 1, 1)
    assert "mlps.0.0.conv.bias" in PM.PointnetSAModule([5, 16], bn=False).state_dict()
    # group-all: the composition a user would write runs on CPU tensors
    torch.manual_seed(0)
    ga = PM.PointnetSAModule([5, 16, 32])
    xyz, f = torch.rand(2, 9, 3), torch.rand(2, 5, 9, requires_grad=True)
    new_xyz, out = ga(xyz, f, fused=False)
    assert new_xyz is None and out.shape == (2, 32, 1)
    want = ga.mlps[0](torch.cat([xyz.transpose(1, 2), f], 1).unsqueeze(2)).amax(3)
    assert torch.allclose(out, want)
    out.sum().backward()
    assert f.grad is not None and ga.mlps[0][0].conv.weight.grad is not None
    assert "not provided" not in PM.__doc__

"""sn_rank_points called directly in guarded buffers (tests/cabi_ref.py): the order, the distinct count and the ordered points against
the numpy restatement of tests/rank_ref.py (held to sputils.nn_matching and to the reference routine by tests/test_rank_host.py) at
one shape per branch of the kernel, every recipe, both layouts; against sn_nn_matching_indexed's bits wherever that entry takes the
shape; NULL outputs, out-of-range indices, limits, determinism, and every points-per-lane setting of the measurement hook."""
import itertools

import numpy as np
import pytest
import torch

import cabi_ref as G
import rank_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def call(xyz, idx, layout, want=(True, True, True), entry="sn_rank_points"):
    lib, check = _lib()
    B, N, _ = xyz.shape
    k = idx.shape[1]
    src = G.t(xyz, layout)
    gx, gi = G.Guarded(src.shape, fill=src), G.Guarded((B, k), torch.int32, fill=idx)
    outs = [G.Guarded((B, k, 3)) if want[0] else None, G.Guarded((B, k), torch.int32) if want[1] else None,
            G.Guarded((B,), torch.int32) if want[2] else None]
    if entry == "sn_rank_points":
        check(lib.sn_rank_points(B, N, k, gx.ptr(), layout, gi.ptr(), None, *[G.arg(o) for o in outs], None), entry)
    else:
        check(lib.sn_nn_matching_indexed(B, N, k, gx.ptr(), layout, gi.ptr(), 1, *[G.arg(o) for o in outs], None), entry)
    torch.cuda.synchronize()
    assert gx.guards_intact() and gi.guards_intact()
    assert np.array_equal(gx.numpy().view(np.int32), src.view(np.int32)) and np.array_equal(gi.numpy(), idx)
    return [None if o is None else o.check(entry).cpu().numpy().copy() for o in outs]


def gathered(xyz, order):
    return np.stack([xyz[b][order[b]] for b in range(len(xyz))])


@pytest.mark.parametrize("layout", [G.BNC, G.BCN])
@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("B,N,k", R.SHAPES)
def test_order_count_and_points(B, N, k, recipe, layout):
    xyz, idx, order, n_unique = R.case(recipe, B, N, k)
    out, out_idx, nun = call(xyz, idx, layout)
    assert np.array_equal(nun, n_unique)
    assert np.array_equal(out_idx, order), "first difference at %s" % (np.argwhere(out_idx != order)[:1],)
    assert np.array_equal(out.view(np.int32), gathered(xyz, out_idx).view(np.int32))
    if recipe == "distinct" and k == N:  # distinct points, every one named once: a permutation
        assert np.array_equal(np.sort(out_idx, axis=1), np.tile(np.arange(N, dtype=np.int32), (B, 1)))
    if k <= 1024:  # the shapes the earlier kernel takes: the same bits in all three outputs
        old = call(xyz, idx, layout, entry="sn_nn_matching_indexed")
        assert np.array_equal(out.view(np.int32), old[0].view(np.int32))
        assert np.array_equal(out_idx, old[1]) and np.array_equal(nun, old[2])


@pytest.mark.parametrize("ppt", [1, 2, 4, 8])
@pytest.mark.parametrize("recipe", ["draws", "coincident", "near_tie"])
def test_every_points_per_lane_setting(ppt, recipe):
    lib, _ = _lib()
    shapes = [(3, 100, 100), (1, 1025, 1025)] if ppt > 1 else [(3, 100, 100), (2, 1024, 1024)]
    assert lib.sn_rank_points_set_ppt(3) == -1
    prev = lib.sn_rank_points_set_ppt(ppt)
    try:
        for B, N, k in shapes:
            xyz, idx, order, n_unique = R.case(recipe, B, N, k)
            out, out_idx, nun = call(xyz, idx, G.BNC)
            assert np.array_equal(out_idx, order) and np.array_equal(nun, n_unique)
            assert np.array_equal(out.view(np.int32), gathered(xyz, out_idx).view(np.int32))
        if ppt == 1:  # 1024 lanes of one point do not hold 1025 points
            x, i = torch.zeros(1, 1025, 3, device="cuda"), torch.zeros(1, 8, device="cuda", dtype=torch.int32)
            o = G.Guarded((1, 8, 3))
            assert lib.sn_rank_points(1, 1025, 8, x.data_ptr(), 0, i.data_ptr(), None, o.ptr(), None, None, None) == G.UNSUPPORTED
            assert b"sn_rank_points" in lib.sn_last_error_string()
            torch.cuda.synchronize()
            assert o.untouched()
    finally:
        assert lib.sn_rank_points_set_ppt(prev) == ppt


@pytest.mark.parametrize("B,N,k", [(3, 100, 100), (2, 2048, 64)])
def test_every_null_output_combination(B, N, k):
    xyz, idx, order, n_unique = R.case("half", B, N, k)
    full = call(xyz, idx, G.BNC)
    assert np.array_equal(full[1], order)
    for want in itertools.product((False, True), repeat=3):
        got = call(xyz, idx, G.BNC, want)
        for w, a, b in zip(want, got, full):
            assert (a is None) if not w else np.array_equal(a, b)


@pytest.mark.parametrize("layout", [G.BNC, G.BCN])
@pytest.mark.parametrize("B,N,k", [(3, 100, 100), (1, 1025, 1025), (1, 16, 40)])
def test_out_of_range_indices_are_clamped(B, N, k, layout):
    xyz, idx = R.make_case("draws", B, N, k, seed=3)
    wild = idx.astype(np.int64)
    wild[:, 0::5] -= N           # below 0
    wild[:, 1::5] += N           # at or above N
    wild[:, 2] = -2 ** 31
    wild[:, 3] = 2 ** 31 - 1
    wild[:, 4] = N
    wild = wild.astype(np.int32)
    assert (wild < 0).any() and (wild >= N).any()
    clamped = np.clip(wild, 0, N - 1).astype(np.int32)
    got, want = call(xyz, wild, layout), call(xyz, clamped, layout)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    ref = [R.rank_one(xyz[b], clamped[b], k) for b in range(B)]
    assert np.array_equal(got[1], np.stack([r[0] for r in ref])) and np.array_equal(got[2], [r[1] for r in ref])


def test_limits_and_empty_batch():
    lib, check = _lib()
    o, oi, nu = G.Guarded((2, 4, 3)), G.Guarded((2, 4), torch.int32), G.Guarded((2,), torch.int32)
    check(lib.sn_rank_points(0, 8, 4, None, 0, None, None, None, None, None, None), "B = 0")
    check(lib.sn_rank_points(0, 8, 4, None, 0, None, None, o.ptr(), oi.ptr(), nu.ptr(), None), "B = 0")
    assert lib.sn_workspace_bytes(b"rank_points", 2, 8192, 8192, 0) == 0
    x, i = torch.zeros(2, 8, 3, device="cuda"), torch.zeros(2, 4, device="cuda", dtype=torch.int32)
    args = (o.ptr(), oi.ptr(), nu.ptr(), None)
    assert lib.sn_rank_points(2, 2000, 8193, x.data_ptr(), 0, i.data_ptr(), None, *args) == G.UNSUPPORTED
    assert lib.sn_last_error_string().startswith(b"sn_rank_points")
    assert lib.sn_rank_points(2, 8193, 4, x.data_ptr(), 0, i.data_ptr(), None, *args) == G.UNSUPPORTED
    assert lib.sn_last_error_string().startswith(b"sn_rank_points")
    assert lib.sn_rank_points(2, 8, 4, x.data_ptr(), 7, i.data_ptr(), None, *args) == G.BAD_ARGUMENT
    assert lib.sn_last_error_string().startswith(b"sn_rank_points")
    assert lib.sn_rank_points(2, 8, 4, None, 0, i.data_ptr(), None, *args) == G.BAD_ARGUMENT
    assert lib.sn_rank_points(2, 8, 4, x.data_ptr(), 0, None, None, *args) == G.BAD_ARGUMENT
    assert lib.sn_rank_points(2, 0, 4, x.data_ptr(), 0, i.data_ptr(), None, *args) == G.BAD_ARGUMENT
    assert lib.sn_rank_points(2, 8, 0, x.data_ptr(), 0, i.data_ptr(), None, *args) == G.BAD_ARGUMENT
    torch.cuda.synchronize()
    assert o.untouched() and oi.untouched() and nu.untouched()


@pytest.mark.parametrize("B,N,k", [(2, 2048, 2048), (1, 4100, 1500)])
def test_same_call_twice_gives_equal_bits(B, N, k):
    xyz, idx, order, _ = R.case("coincident", B, N, k)
    a, b = call(xyz, idx, G.BCN), call(xyz, idx, G.BCN)
    assert np.array_equal(a[1], order)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int32), v.view(np.int32))


def test_ops_rank_points():
    from samplenet_amd import ops

    xyz, idx, order, n_unique = R.case("draws", 2, 2048, 2048)
    x, i = torch.from_numpy(xyz.copy()).cuda(), torch.from_numpy(idx.copy()).cuda()
    for layout, src in ((ops.BNC, x), (ops.BCN, x.permute(0, 2, 1).contiguous())):
        pts, got, nun = ops.rank_points(src, i.unsqueeze(-1), layout=layout)  # (knn's (B,k,1) indices are taken as they come)
        assert pts.dtype == torch.float32 and got.dtype == torch.int32 and nun.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), order) and np.array_equal(nun.cpu().numpy(), n_unique)
        assert torch.equal(pts, torch.gather(x, 1, got.long().unsqueeze(-1).expand(-1, -1, 3))) and not pts.requires_grad
    with pytest.raises(ValueError, match="rank_points: idx must hold k indices per cloud"):
        ops.rank_points(x, i, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rank_points(x.cpu(), i.cpu())

"""sn_nn_matching_indexed called directly: the selected indices and the distinct-neighbour count against a numpy restatement of
fps_from_given_indices / simple_projection_and_continued_fps (reconstruction/src/samplenet_pointnet_ae.py:459-549: float64 distances,
first-maximum argmax), `out` against sn_nn_matching's bits and against xyz[out_idx]; guarded buffers throughout (tests/cabi_ref.py).
Then SampleNet.sample_indices against forward's matched cloud in eval mode."""
import itertools

import numpy as np
import pytest
import torch

import cabi_ref as G

pytestmark = pytest.mark.gpu

# one to eight points per thread of the 1024-thread workgroup (N <= 1024, 2048, 4096, 8192), N no multiple of it, k = N
SHAPES = ((1, 1, 1), (2, 64, 8), (3, 100, 16), (2, 16, 16), (2, 1024, 64), (1, 1500, 32), (1, 2049, 8), (1, 4100, 4))
RECIPES = ("equal", "distinct", "half", "coincident")


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def restated(cloud, picks, k):
    """One cloud (N,3) float32, picks (k,): -> (indices (k,), number of distinct picks).  The distinct picks in order of first
    occurrence, then farthest-point picks: float64 squared distances to the chosen set, np.argmax (first maximum)."""
    pts = cloud.astype(np.float64)
    _, first = np.unique(picks, return_index=True)
    chosen = list(picks[np.sort(first)])
    n_unique = len(chosen)
    dist = np.full(len(pts), np.inf)
    for p in chosen:
        dist = np.minimum(dist, ((pts[p] - pts) ** 2).sum(1))
    while len(chosen) < k:
        far = int(np.argmax(dist))
        chosen.append(far)
        dist = np.minimum(dist, ((pts[far] - pts) ** 2).sum(1))
    return np.asarray(chosen[:k], dtype=np.int32), n_unique


def make_case(recipe, B, N, k, seed=0):
    rng = np.random.default_rng([seed, B, N, k, RECIPES.index(recipe)])
    xyz = (rng.random((B, N, 3), dtype=np.float32) - 0.5)
    if recipe == "equal":
        idx = np.repeat(rng.integers(0, N, (B, 1)), k, axis=1)
    elif recipe == "distinct":
        idx = np.stack([rng.permutation(N)[:k] for _ in range(B)])
    elif recipe == "half":
        idx = np.stack([rng.permutation(N)[:k] for _ in range(B)])
        idx[:, k // 2:] = idx[:, :k - k // 2]
    else:  # coincident points: ties of the farthest-point step go to the lowest index
        xyz[:, N // 2:] = xyz[:, :N - N // 2]
        idx = rng.integers(0, N, (B, k))
        idx[:, 1::2] = idx[:, 0:1]
    return xyz, idx.astype(np.int32)


def call(xyz, idx, layout, complete_fps, want=(True, True, True), entry="sn_nn_matching_indexed"):
    lib, check = _lib()
    B, N, _ = xyz.shape
    k = idx.shape[1]
    src = G.t(xyz, layout)
    gx, gi = G.Guarded(src.shape, fill=src), G.Guarded((B, k), torch.int32, fill=idx)
    outs = [G.Guarded((B, k, 3)) if want[0] else None, G.Guarded((B, k), torch.int32) if want[1] else None,
            G.Guarded((B,), torch.int32) if want[2] else None]
    if entry == "sn_nn_matching":
        check(lib.sn_nn_matching(B, N, k, gx.ptr(), layout, gi.ptr(), complete_fps, outs[0].ptr(), None), entry)
    else:
        check(lib.sn_nn_matching_indexed(B, N, k, gx.ptr(), layout, gi.ptr(), complete_fps, *[G.arg(o) for o in outs], None), entry)
    torch.cuda.synchronize()
    assert gx.guards_intact() and gi.guards_intact()
    assert np.array_equal(gx.numpy().view(np.int32), src.view(np.int32)) and np.array_equal(gi.numpy(), idx)
    return [None if o is None else o.check(entry).cpu().numpy().copy() for o in outs]


@pytest.mark.parametrize("layout", [G.BNC, G.BCN])
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("B,N,k", SHAPES)
def test_indices_and_unique_count(B, N, k, recipe, layout):
    xyz, idx = make_case(recipe, B, N, k)
    ref = [restated(xyz[b], idx[b], k) for b in range(B)]
    out, out_idx, n_unique = call(xyz, idx, layout, 1)
    assert np.array_equal(out_idx, np.stack([r[0] for r in ref]))
    assert np.array_equal(n_unique, np.array([r[1] for r in ref], dtype=np.int32))
    assert np.array_equal(n_unique, np.array([len(np.unique(r)) for r in idx], dtype=np.int32))
    if recipe == "equal":
        assert (n_unique == 1).all()
    plain = call(xyz, idx, layout, 1, (True, False, False), "sn_nn_matching")[0]
    assert np.array_equal(out.view(np.int32), plain.view(np.int32))
    gathered = np.stack([xyz[b][out_idx[b]] for b in range(B)])
    assert np.array_equal(out.view(np.int32), gathered.view(np.int32))
    # complete_fps = 0: a plain gather, out_idx a copy of idx, the count still computed
    out0, idx0, nun0 = call(xyz, idx, layout, 0)
    assert np.array_equal(idx0, idx) and np.array_equal(nun0, n_unique)
    assert np.array_equal(out0.view(np.int32), np.stack([xyz[b][idx[b]] for b in range(B)]).view(np.int32))
    assert np.array_equal(out0.view(np.int32), call(xyz, idx, layout, 0, (True, False, False), "sn_nn_matching")[0].view(np.int32))


@pytest.mark.parametrize("complete_fps", [0, 1])
def test_every_null_output_combination(complete_fps):
    xyz, idx = make_case("half", 3, 100, 16)
    full = call(xyz, idx, G.BNC, complete_fps)
    for want in itertools.product((False, True), repeat=3):
        got = call(xyz, idx, G.BNC, complete_fps, want)
        for w, a, b in zip(want, got, full):
            assert (a is None) if not w else np.array_equal(a, b)


def test_limits_and_empty_batch():
    lib, check = _lib()
    o, oi, nu = G.Guarded((2, 4, 3)), G.Guarded((2, 4), torch.int32), G.Guarded((2,), torch.int32)
    check(lib.sn_nn_matching_indexed(0, 8, 4, None, 0, None, 1, o.ptr(), oi.ptr(), nu.ptr(), None), "B = 0")
    x, i = torch.zeros(2, 8, 3, device="cuda"), torch.zeros(2, 4, device="cuda", dtype=torch.int32)
    assert lib.sn_nn_matching_indexed(2, 2000, 1025, x.data_ptr(), 0, i.data_ptr(), 1, o.ptr(), oi.ptr(), nu.ptr(), None) == G.UNSUPPORTED
    assert b"sn_nn_matching_indexed" in lib.sn_last_error_string()
    assert lib.sn_nn_matching_indexed(2, 8193, 4, x.data_ptr(), 0, i.data_ptr(), 1, o.ptr(), oi.ptr(), nu.ptr(), None) == G.UNSUPPORTED
    assert lib.sn_nn_matching_indexed(2, 8, 4, x.data_ptr(), 7, i.data_ptr(), 1, o.ptr(), oi.ptr(), nu.ptr(), None) == G.BAD_ARGUMENT
    assert lib.sn_nn_matching_indexed(2, 8, 4, None, 0, i.data_ptr(), 1, o.ptr(), oi.ptr(), nu.ptr(), None) == G.BAD_ARGUMENT
    torch.cuda.synchronize()
    assert o.untouched() and oi.untouched() and nu.untouched()


@pytest.mark.parametrize("shape", ["bnc", "bcn"])
@pytest.mark.parametrize("train_before", [False, True])
def test_sample_indices_is_forwards_eval_branch(shape, train_before):
    from samplenet_amd import SampleNet

    torch.manual_seed(4)
    net = SampleNet(16, 128, group_size=4, input_shape=shape, output_shape=shape).cuda()
    x = torch.rand(3, 128, 3, device="cuda") - 0.5
    x[:, 64:] = x[:, :64]  # coincident points
    xin = x if shape == "bnc" else x.permute(0, 2, 1).contiguous()
    net.eval()
    with torch.no_grad():
        simp, matched = net(xin)
    net.train(train_before)
    s2, m2, out_idx, n_unique = net.sample_indices(xin)
    assert net.training == train_before
    assert torch.equal(s2, simp) and torch.equal(m2, matched) and not m2.requires_grad
    pts = m2 if shape == "bnc" else m2.permute(0, 2, 1)
    assert out_idx.dtype == torch.int32 and tuple(out_idx.shape) == (3, 16) and tuple(n_unique.shape) == (3,)
    assert torch.equal(pts, torch.gather(x, 1, out_idx.long().unsqueeze(-1).expand(-1, -1, 3)))
    assert ((n_unique >= 1) & (n_unique <= 16)).all()
    for b in range(3):
        assert len(np.unique(out_idx[b].cpu().numpy())) == 16  # completed to 16 distinct points

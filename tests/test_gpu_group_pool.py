"""sn_group_pool_forward / sn_group_pool_backward on the device, into poisoned and guarded buffers, against the entries they stand
beside: pooled / argsel / zsel bit for bit sn_pool_forward(B = G, N = S), gsel bit for bit sn_pool_backward; argsel / zsel also
against the numpy restatement (first-row ties, the min route on a negative scale).

The block partials against float64: block k sums the groups 64 k .. 64 k + 63 of a channel as four slices (groups q, q + 4, ..
ascending) whose sums are then added in slice order, so a sum of cnt terms passes through ceil(cnt / 4) + 4 rounded additions at
most, and the second sum's terms are rounded products: k = ceil(cnt / 4) + 4 + 1, error <= k * 2^-24 * sum|terms| to first order.
kcoef after sn_bn_backward_coef against the one-launch sn_pool_backward_bn: both reduce the same terms in fixed orders of their own
(the one-launch kernel: 16 slices of ceil(G / 16) terms, 16 slice sums, possibly a fused multiply-add), so their sums s, sz differ by
at most ds = (k_new + k_old) 2^-24 sum|terms|; that is carried through dgamma = invstd (sz - mean s), k2 = -scale invstd dgamma / R,
k3 = scale (invstd mean dgamma - s) / R, plus one float32 rounding on either side (2^-24 each) and the float64 arithmetic of the
finalisation (2^-40 covers its few operations and the Newton reciprocal)."""
import numpy as np
import pytest
import torch

import group_rows_ref as GR
from cabi_ref import Guarded, stream as _stream

pytestmark = pytest.mark.gpu

_CASES = {}


def case(G, S, C):
    if (G, S, C) not in _CASES:
        z, scale, shift = GR.pool_case(G, S, C, 1000 * G + 10 * S + C)
        rng = np.random.default_rng(G + S + C)
        coef = np.stack([scale, shift, rng.standard_normal(C).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)])
        g = rng.standard_normal((G, C)).astype(np.float32)
        ref = GR.group_pool(z, scale, shift)
        for a in (z, coef, g) + ref:
            a.setflags(write=False)
        _CASES[(G, S, C)] = (z, coef, g, ref)
    return _CASES[(G, S, C)]


def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("C", [1, 64, 67, 130])
@pytest.mark.parametrize("S", [1, 3, 16, 64, 70])
@pytest.mark.parametrize("G", [1, 5, 300])
def test_group_pool_pair(G, S, C):
    from samplenet_amd._lib import lib

    z, coef, g, (want_pooled, want_arg, want_zsel) = case(G, S, C)
    dz, dcoef, dg = (torch.tensor(a, device="cuda") for a in (z, coef, g))
    pooled, argsel, zsel = Guarded((G, C)), Guarded((G, C), torch.int32), Guarded((G, C))
    assert lib.sn_group_pool_forward(G, S, C, dz.data_ptr(), dcoef.data_ptr(), pooled.ptr(), argsel.ptr(), zsel.ptr(), _stream()) == 0
    old = [torch.empty(G, C, device="cuda"), torch.empty(G, C, device="cuda", dtype=torch.int32), torch.empty(G, C, device="cuda")]
    assert lib.sn_pool_forward(G, S, C, dz.data_ptr(), dcoef.data_ptr(), *(t.data_ptr() for t in old), _stream()) == 0
    torch.cuda.synchronize()
    for new, o, what in zip((pooled, argsel, zsel), old, ("pooled", "argsel", "zsel")):
        assert torch.equal(_i32(new.check(what)), _i32(o)), what
    assert np.array_equal(argsel.numpy(), want_arg) and np.array_equal(zsel.numpy().view(np.int32), want_zsel.view(np.int32))
    assert (np.abs(pooled.numpy() - want_pooled) <= 2.0 ** -23 * np.abs(want_pooled)).all()
    if S >= 2:
        assert (coef[0] < 0).any() or C == 1   # the min route is taken (channel 0 has a negative scale)

    # backward
    nblk = lib.sn_group_pool_stats_blocks(G)
    assert nblk == -(-G // 64)
    gsel, stats = Guarded((G, C)), Guarded((nblk, 2, C))
    assert lib.sn_group_pool_backward(G, C, dg.data_ptr(), old[0].data_ptr(), old[2].data_ptr(), gsel.ptr(), stats.ptr(), _stream()) == 0
    gsel_old, stats_old = torch.empty(G, C, device="cuda"), torch.empty(2, C, device="cuda")
    assert lib.sn_pool_backward(G, C, dg.data_ptr(), old[0].data_ptr(), old[2].data_ptr(), gsel_old.data_ptr(), stats_old.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_i32(gsel.check("gsel")), _i32(gsel_old))
    gs = gsel_old.cpu().numpy().astype(np.float64)
    terms = np.stack([gs, gs * old[2].cpu().numpy().astype(np.float64)])                # (2, G, C)
    got = stats.check("stats").cpu().numpy()
    worst = 0.0
    for k in range(nblk):
        blk = terms[:, 64 * k:64 * (k + 1)]
        kk = -(-blk.shape[1] // 4) + 4 + 1
        err, bound = np.abs(got[k] - blk.sum(1)), kk * GR.U * np.abs(blk).sum(1)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    print("stats blocks: worst error / bound %.3g" % worst)
    # a NULL stats: gsel alone (the fixed-statistics backward)
    gsel2 = Guarded((G, C))
    assert lib.sn_group_pool_backward(G, C, dg.data_ptr(), old[0].data_ptr(), old[2].data_ptr(), gsel2.ptr(), None, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gsel2.raw, gsel.raw)

    # the BatchNorm backward of the two routes
    Rn = G * S
    new_o = [torch.empty(C, device="cuda") for _ in range(3)] + [torch.empty(3, C, device="cuda")]
    old_o = [torch.empty(C, device="cuda") for _ in range(3)] + [torch.empty(3, C, device="cuda")]
    assert lib.sn_bn_backward_coef(nblk, C, Rn, stats.ptr(), dcoef.data_ptr(), *(t.data_ptr() for t in new_o), _stream()) == 0
    g3 = torch.empty(G, C, device="cuda")
    assert lib.sn_pool_backward_bn(G, C, Rn, dg.data_ptr(), old[0].data_ptr(), old[2].data_ptr(), g3.data_ptr(), dcoef.data_ptr(),
                                   *(t.data_ptr() for t in old_o), _stream()) == 0
    torch.cuda.synchronize()
    A = np.abs(terms).sum(1)                                                             # (2, C)
    k_new, k_old = -(-min(G, 64) // 4) + 4 + 1, -(-G // 16) + 16 + 1
    ds, dsz = (k_new + k_old) * GR.U * A[0], (k_new + k_old) * GR.U * A[1]
    scale, mean, invstd = (np.abs(coef[i]).astype(np.float64) for i in (0, 2, 3))
    ddg = invstd * (dsz + mean * ds)
    kn, ko = new_o[3].cpu().numpy().astype(np.float64), old_o[3].cpu().numpy().astype(np.float64)
    RND = 2.0 ** -23 + 2.0 ** -40
    rnd = RND * np.maximum(np.abs(kn), np.abs(ko))
    assert np.array_equal(kn[0], ko[0])
    assert (np.abs(kn[1] - ko[1]) <= scale * invstd * ddg / Rn + rnd[1]).all()
    assert (np.abs(kn[2] - ko[2]) <= scale * (invstd * mean * ddg + ds) / Rn + rnd[2]).all()
    dgn, dgo = new_o[0].cpu().numpy().astype(np.float64), old_o[0].cpu().numpy().astype(np.float64)
    assert (np.abs(dgn - dgo) <= ddg + RND * np.maximum(np.abs(dgn), np.abs(dgo))).all()
    dbn, dbo = new_o[1].cpu().numpy().astype(np.float64), old_o[1].cpu().numpy().astype(np.float64)
    assert (np.abs(dbn - dbo) <= ds + RND * np.maximum(np.abs(dbn), np.abs(dbo))).all()


def test_argument_errors():
    from samplenet_amd._lib import lib

    t = torch.zeros(8, device="cuda")
    p, st = t.data_ptr(), _stream()
    assert lib.sn_group_pool_forward(0, 2, 2, p, p, p, p, p, st) == 10001 and lib.sn_group_pool_forward(2, 2, 2, p, p, None, p, p, st) == 10001
    assert lib.sn_group_pool_backward(2, 0, p, p, p, p, p, st) == 10001 and lib.sn_group_pool_backward(2, 2, p, p, p, None, p, st) == 10001
    assert lib.sn_group_pool_stats_blocks(0) == 0 and lib.sn_group_pool_stats_blocks(64) == 1 and lib.sn_group_pool_stats_blocks(65) == 2

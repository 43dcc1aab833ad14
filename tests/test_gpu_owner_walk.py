"""The ordered owner sum of the Chamfer backward kernels (csrc/chamfer_owner.h: owner_sum), called through the raw C ABI in guarded
buffers (tests/cabi_ref.py).  A query's gradient is its own term followed by one subtraction per cloud point it owns, in ascending
point index; the kernels run that sum as a chain over the lanes of a wave, 16 list entries per chunk, from a list of CAP entries
per wave; a query that owns more passes the slots once more per CAP owners.  The clouds are clusters around the queries, built so
that ONE chosen query owns exactly c points, for every c that crosses a chunk, list or slot boundary, in three placements (from
point 0 on; up to the last point; one per slot of 64 points); the other points go round-robin to the other queries, so every call
also checks many ordinary owner counts (at M = 4 the others own a third of the cloud each: two passes at N >= 1024).

  a. sn_chamfer_backward with explicit upstream gradients: both outputs bit for bit a numpy float32 restatement of the sequential
     loop (every numpy float32 operation is one IEEE operation, so equality is exact);
  b. sn_sampler_step_loss_backward on the same clouds: bit for bit fp32(sn_simplification_loss_backward) +
     fp32(sn_soft_project_backward), the identity the fused kernel promises;
  every output sits between intact guard words and is fully written."""
import functools

import numpy as np
import pytest
import torch

import step_loss_ref as S
from cabi_ref import BCN, BNC, Guarded

pytestmark = pytest.mark.gpu
I32 = torch.int32

CAP = 256  # kOwnerCap: entries of a wave's list (a query that owns more passes the slots again, once per CAP owners)
COUNTS = sorted({0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, CAP - 1, CAP, CAP + 1})
BS, MS, NS = (1, 3), (1, 4, 64), (64, 65, 256, 1024, 1088)  # N: one slot, a ragged second, 4, 16 and 17 of 32 slots
PLACEMENTS = ("front", "back", "spread")
K = 4
SCALARS = S.SCALARS["base"]
SHAPES = [(b, m, n) for b in BS for m in MS for n in NS]


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    return t if dtype is None else t.to(dtype)


def scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def _same_bits(what, a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert not len(bad), "%s: %d of %d elements differ, first at %s: %#x against %#x" % (
        what, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])] & 0xFFFFFFFF, b[tuple(bad[0])] & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the clouds
def recipes(M, N):
    """(c, placement) of every cloud of a shape; c == N once (every placement is the same cloud), M == 1 owns everything."""
    if M == 1:
        return [(N, "front")]
    out = [(0, "front")]
    out += [(c, p) for c in COUNTS if 0 < c < N for p in PLACEMENTS]
    out += [(N, "front"), (17, "ties")]
    return out


def owner_points(N, c, placement):
    """The c point indices the chosen query owns."""
    if placement == "front":  # slot 0 from lane 0 on (and on into the next slots once c passes 64)
        return np.arange(c)
    if placement == "back":  # ... ending at the last valid lane of the last slot
        return np.arange(N - c, N)
    order = sorted(range(N), key=lambda i: (i % 64, i // 64))  # one per slot, then the next lane of every slot
    return np.sort(np.array(order[:c], dtype=np.int64))


def make_cloud(M, N, c, placement, rng):
    """-> P (N, 3), Q (M, 3) float32, the chosen query, the points it must own (None: whatever the ties give)."""
    jb = M // 2
    Q = np.zeros((M, 3))
    Q[:, 0] = 3.0 * np.arange(M)
    Q += rng.uniform(-0.3, 0.3, (M, 3))
    ties = placement == "ties"
    if ties:
        Q[jb + 1] = Q[jb]  # two coincident queries: the lower one owns what lies around them
    mine = owner_points(N, c, "spread" if ties else placement)
    owner = np.full(N, -1)
    owner[mine] = jb
    rest = np.flatnonzero(owner < 0)
    others = np.array([j for j in range(M) if j != jb])
    if len(rest):
        owner[rest] = others[np.arange(len(rest)) % len(others)]
    Q = Q.astype(np.float32)
    P = (Q[owner].astype(np.float64) + rng.uniform(-0.4, 0.4, (N, 3))).astype(np.float32)
    if ties:
        P[mine[1:4]] = P[mine[0]]  # coincident points: equal contributions one after the other
        P[mine[5]] = Q[jb]  # a point ON its query: a contribution of zeros
        return P, Q, jb, None
    return P, Q, jb, mine


def chamfer_backward_np32(T, S_, gT, idxT, gS, idxS, own_first):
    """grad of the targets T (C, nt, 3) against the sources S_ (C, ns, 3) as the sequential loop adds it, one float32 operation at a
    time: the own term 2 gT (t - s_idxT), and a = a - (2 gS_l) (s_l - t_idxS[l]) for l ascending; the own term enters first or last."""
    C, nt, ns = T.shape[0], T.shape[1], S_.shape[1]
    ar = np.arange(C)
    two = np.float32(2)
    own = (gT * two)[..., None] * (T - S_[ar[:, None], idxT])
    a = np.zeros((C, nt, 3), np.float32)
    if own_first:
        a = a + own
    gg = gS * two
    for l in range(ns):
        j = idxS[:, l]
        a[ar, j] = a[ar, j] - gg[:, l, None] * (S_[:, l] - T[ar, j])
    if not own_first:
        a = a + own
    assert a.dtype == np.float32 and own.dtype == np.float32
    return a


@functools.lru_cache(maxsize=None)
def clouds(M, N):
    """Every cloud of a shape, its scan in float32 and the restated gradients; built once, shared by all tests, read-only."""
    rng = np.random.default_rng(1000 * M + N)
    rec = recipes(M, N)
    made = [make_cloud(M, N, c, placement, rng) for c, placement in rec]
    P, Q = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
    scan = S.scan_np32(P, Q, K)
    for i, (c, placement) in enumerate(rec):  # the clusters are what they were built to be
        jb, mine = made[i][2:]
        got = np.flatnonzero(scan["ip"][i] == jb)
        if mine is None:
            assert len(got) > c and not (scan["ip"][i] == jb + 1).any(), (M, N, c, placement)
        else:
            assert np.array_equal(got, mine), (M, N, c, placement)
    gq = rng.standard_normal((len(rec), M)).astype(np.float32)
    gp = rng.standard_normal((len(rec), N)).astype(np.float32)
    gp[:, ::7] = 0  # (a few owners contribute exact zeros)
    ref_q = chamfer_backward_np32(Q, P, gq, scan["iq"], gp, scan["ip"], True)
    ref_p = chamfer_backward_np32(P, Q, gp, scan["ip"], gq, scan["iq"], False)
    out = dict(P=P, Q=Q, gq=gq, gp=gp, ref_q=ref_q, ref_p=ref_p, rec=rec, **scan)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def batches(n, B):
    """The clouds of a shape B at a time (the last batch repeats the last cloud)."""
    return [[min(i + k, n - 1) for k in range(B)] for i in range(0, n, B)]


# ------------------------------------------------------------------------------------------------ a. bitwise against numpy
@pytest.mark.parametrize("B,M,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_chamfer_backward_is_the_sequential_loop(B, M, N):
    """sn_chamfer_backward (queries = xyz1: own term first, owners in ascending point index; cloud = xyz2: owners first) bit for bit
    chamfer_backward_np32, every cloud of the shape."""
    lib, check = _lib()
    c = clouds(M, N)
    for sel in batches(len(c["rec"]), B):
        g1, g2 = Guarded((B, M, 3)), Guarded((B, N, 3))
        t = [dev(c[k][sel]) for k in ("Q", "P", "gq", "iq", "gp", "ip")]
        check(lib.sn_chamfer_backward(B, M, t[0].data_ptr(), N, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                      t[5].data_ptr(), g1.ptr(), g2.ptr(), None), "sn_chamfer_backward")
        torch.cuda.synchronize()
        g1.check("grad_xyz1"), g2.check("grad_xyz2")
        tag = "%dx%dx%d clouds %s %s: " % (B, M, N, sel, [c["rec"][i] for i in sel])
        _same_bits(tag + "grad of the queries", g1.numpy(), c["ref_q"][sel])
        _same_bits(tag + "grad of the cloud", g2.numpy(), c["ref_p"][sel])


# ------------------------------------------------------------------------------------------------ b. fused against op by op
@pytest.mark.parametrize("B,M,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_fused_backward_is_the_two_launches(B, M, N):
    """sn_sampler_step_loss_backward (chamfer_soft_bwd_kernel) against sn_simplification_loss_backward + sn_soft_project_backward
    (chamfer_bwd_reg_kernel, soft_bwd_kernel) on the same clouds and indices: grad_Q and the sigma partials bit for bit."""
    lib, check = _lib()
    c = clouds(M, N)
    T, ms, alpha, lmbda, weight, g = SCALARS
    dT, dg = scalar(T), scalar(g)
    up = scalar(np.float32(alpha) * np.float32(g))
    splits = S.soft_bwd_splits(B, M)
    gproj = torch.full((B, M, 3), float(np.float32(g) / np.float32(B * 3 * M)), dtype=torch.float32, device="cuda")
    for sel in batches(len(c["rec"]), B):
        dP, dQ = dev(c["P"][sel]), dev(c["Q"][sel].transpose(0, 2, 1))  # (B, N, 3) and (B, 3, M), the FC head's layout
        knn, iq, ip, am = (dev(c[k][sel]) for k in ("knn", "iq", "ip", "am"))
        o = dict(gQ=Guarded((B, 3, M)), gsig=Guarded((B * splits,)), gT=Guarded((1,)), cham=Guarded((B, 3, M)), soft=Guarded((B, 3, M)),
                 gsig2=Guarded((B * splits,)))
        check(lib.sn_sampler_step_loss_backward(B, N, M, K, dP.data_ptr(), BNC, dQ.data_ptr(), knn.data_ptr(), iq.data_ptr(), ip.data_ptr(),
                                                am.data_ptr(), dT.data_ptr(), ms, alpha, lmbda, weight, dg.data_ptr(), o["gQ"].ptr(),
                                                o["gsig"].ptr(), o["gT"].ptr(), None, None, None), "sn_sampler_step_loss_backward")
        check(lib.sn_simplification_loss_backward(B, M, dQ.data_ptr(), N, dP.data_ptr(), iq.data_ptr(), ip.data_ptr(), am.data_ptr(), weight,
                                                  up.data_ptr(), o["cham"].ptr(), None, 1, None), "sn_simplification_loss_backward")
        check(lib.sn_soft_project_backward(B, N, M, K, dP.data_ptr(), BNC, dQ.data_ptr(), BCN, knn.data_ptr(), dT.data_ptr(), ms,
                                           gproj.data_ptr(), BNC, o["soft"].ptr(), BCN, None, o["gsig2"].ptr(), None),
              "sn_soft_project_backward")
        torch.cuda.synchronize()
        for name, buf in o.items():
            buf.check(name)
        tag = "%dx%dx%d clouds %s %s: " % (B, M, N, sel, [c["rec"][i] for i in sel])
        _same_bits(tag + "grad_Q against the two launches", o["gQ"].numpy(), o["cham"].numpy() + o["soft"].numpy())
        _same_bits(tag + "sigma partials against sn_soft_project_backward", o["gsig"].numpy(), o["gsig2"].numpy())

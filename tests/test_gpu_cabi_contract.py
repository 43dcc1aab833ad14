"""The public C header's contract, entry point by entry point (include/samplenet_hip.h, geometric half): every test here calls
samplenet_amd._lib.lib with raw device pointers -- the way a ctypes / dlopen / pybind binding of the reference would -- and
checks one sentence of the header against a plain reference (tests/cabi_ref.py in fp64, or the CPU oracle where the bar is
bit-exactness):

  1. optional outputs ("may be NULL") and "overwritten without a memset": poison-and-guard buffers;
  2. the products no wrapper requests: the pair scan's `weights`, the ACCUMULATING atomic gradients;
  3. every layout selector, on transposed copies of the same data;
  4. the pair scan's routing limits as a grid (N x K x M x B x workspace form) against the oracle;
  5. any stream, hipGraph capture, several host threads.

Bars: indices / squared distances / anything "same kernel, same order": bit for bit.  proj and weights: 1e-6 absolute (the bar
test_soft_project_fused_vs_oracle holds proj to).  Gradients summed by float atomics: rtol 1e-4, atol 1e-5 (that test's bar for
the same gradient).  Plain elementwise results against fp64 (rotation, head, loss gradients): rtol 1e-5, atol 1e-6 -- a
handful of fp32 roundings (2^-24 each) on values of unit scale.  Index-adds by atomics: hits * 2^-24 * sum|terms| per
destination, the first-order bound of a recursive fp32 sum in ANY order."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import cabi_ref as R
from cabi_ref import BAD_ARGUMENT, BCN, BNC, Guarded, arg, back, clouds, sigma_of, surface_queries, t, tie_clouds

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
ATOMIC = dict(rtol=1e-4, atol=1e-5)
PLAIN = dict(rtol=1e-5, atol=1e-6)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args, expect=0):
    from samplenet_amd._lib import lib

    rc = getattr(lib, name)(*[arg(a) for a in args])
    assert rc == expect, "%s returned %d: %s" % (name, rc, (lib.sn_last_error_string() or b"").decode())
    return rc


def same_bits(a, b):
    a = a.view() if isinstance(a, Guarded) else a
    b = b.view() if isinstance(b, Guarded) else b
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ================================================================================================ the pair scan, raw
PRODUCTS = ("knn_idx", "knn_dist", "dist_q", "idx_q", "dist_p", "idx_p", "proj", "weights")


def pairscan(P, Q, B, N, M, K, want=PRODUCTS, pl=BNC, ql=BNC, projl=BNC, T=None, min_sigma=1e-2, form="ws"):
    """One raw call.  P / Q: device tensors already in layouts pl / ql.  want: the products requested (the others are NULL).
    form: "ws" = sn_pairscan_forward_ws with the reported workspace, "null" = sn_pairscan_forward (no workspace), "ws-null" =
    the _ws entry with workspace NULL, "short" = a workspace one byte too small.  Every buffer is poisoned and guarded; returns
    {product: Guarded} after checking that each was written completely and that no guard changed."""
    from samplenet_amd._lib import lib

    shapes = {"knn_idx": ((B, M, K), I32), "knn_dist": ((B, M, K), F32), "dist_q": ((B, M), F32), "idx_q": ((B, M), I32),
              "dist_p": ((B, N), F32), "idx_p": ((B, N), I32), "proj": ((B, M, 3) if projl == BNC else (B, 3, M), F32),
              "weights": ((B, M, K), F32)}
    out = {k: Guarded(*shapes[k]) for k in want}
    o = lambda k: out.get(k)
    head = (B, N, M, K, P, pl, Q, ql, o("knn_idx"), o("knn_dist"), o("dist_q"), o("idx_q"), o("dist_p"), o("idx_p"), o("proj"), projl,
            o("weights"), T, float(min_sigma))
    ws = None
    if form == "null":
        call("sn_pairscan_forward", *head, stream())
    else:
        wb = int(lib.sn_pairscan_workspace_bytes(B, N, M))
        assert wb >= 0 and wb % 4 == 0
        if form == "ws-null" or wb == 0:
            call("sn_pairscan_forward_ws", *head, None, 0, stream())
        else:
            ws = Guarded((wb // 4,), I32)
            call("sn_pairscan_forward_ws", *head, ws, wb if form == "ws" else wb - 1, stream())
    torch.cuda.synchronize()
    for k, g in out.items():
        g.check("%s (%s)" % (k, form))
    if ws is not None:
        assert ws.guards_intact(), "the workspace was written beyond its reported size"
    return out


def scan_inputs(seed, B, N, M, recipe=tie_clouds):
    Pn, Qn = recipe(seed, B, N, M)
    return Pn, Qn, dev(Pn), dev(Qn), torch.tensor(0.5, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. optional outputs
SUBSETS = [("knn_idx",), ("knn_dist",), ("dist_q", "idx_q"), ("dist_p", "idx_p"), ("proj",), ("weights",),
           ("weights", "knn_idx"), ("idx_p",), ("dist_p",), ("idx_q",), ("dist_q",), ("knn_dist", "dist_p"), ("proj", "idx_q", "idx_p"),
           ("knn_idx", "knn_dist", "proj", "weights")]


@pytest.mark.parametrize("shape", [(3, 1024, 64, 8), (2, 200, 33, 17), (2, 64, 5, 1), (2, 2048, 70, 64), (2, 2500, 70, 16),
                                   (33, 300, 40, 9)])
def test_pairscan_any_output_may_be_null(oracle, shape):
    """"Any output pointer may be NULL to skip that product": each product alone and mixed subsets equal the all-outputs call
    bit for bit, every requested buffer is written completely, nothing outside it -- and the all-outputs call is the oracle's."""
    B, N, M, K = shape
    Pn, Qn, P, Q, T = scan_inputs(N + M + K, B, N, M)
    full = pairscan(P, Q, B, N, M, K, T=T)
    od, oi = oracle.knn(K, Pn, Qn)
    assert np.array_equal(full["knn_idx"].numpy(), oi) and np.array_equal(full["knn_dist"].numpy(), od)
    cq, ciq, cp, cip = oracle.chamfer_forward(Qn, Pn)
    for k, ref in (("dist_q", cq), ("idx_q", ciq), ("dist_p", cp), ("idx_p", cip)):
        assert np.array_equal(full[k].numpy(), ref), k
    for form in ("ws", "null"):
        for sub in SUBSETS:
            got = pairscan(P, Q, B, N, M, K, want=sub, T=T, form=form)
            for k in sub:
                assert same_bits(got[k], full[k]), (k, sub, form)
        # Chamfer products with K = 0 (no kNN, no projection)
        got = pairscan(P, Q, B, N, M, 0, want=("dist_q", "idx_q", "dist_p", "idx_p"), T=None, form=form)
        for k in got:
            assert same_bits(got[k], full[k]), (k, "K = 0", form)
        got = pairscan(P, Q, B, N, M, 0, want=("idx_p",), T=None, form=form)
        assert same_bits(got["idx_p"], full["idx_p"])


@pytest.mark.parametrize("shape", [(2, 100, 37), (3, 64, 1024), (2, 1024, 64), (1, 2049, 70), (1, 70, 2049), (2, 513, 515)])
def test_chamfer_forward_and_knn_optional_outputs(oracle, shape):
    """sn_chamfer_forward / sn_knn through their own entries: outputs against the oracle; sn_knn's dist may be NULL."""
    b, n, m = shape
    x1n, x2n = clouds(n * 31 + m, b, n, m)
    x1, x2 = dev(x1n), dev(x2n)
    g = [Guarded((b, n), F32), Guarded((b, n), I32), Guarded((b, m), F32), Guarded((b, m), I32)]
    call("sn_chamfer_forward", b, n, x1, m, x2, *g, stream())
    torch.cuda.synchronize()
    for got, ref in zip(g, oracle.chamfer_forward(x1n, x2n)):
        assert np.array_equal(got.check("chamfer_forward").cpu().numpy(), ref)
    k = min(n, 9)
    od, oi = oracle.knn(k, x1n, x2n)
    for l1 in (BNC, BCN):
        for l2 in (BNC, BCN):
            gi, gd, gi2 = Guarded((b, m, k), I32), Guarded((b, m, k), F32), Guarded((b, m, k), I32)
            call("sn_knn", b, n, m, k, dev(t(x1n, l1)), l1, dev(t(x2n, l2)), l2, gi, gd, stream())
            call("sn_knn", b, n, m, k, dev(t(x1n, l1)), l1, dev(t(x2n, l2)), l2, gi2, None, stream())
            torch.cuda.synchronize()
            assert np.array_equal(gi.check("knn idx").cpu().numpy(), oi) and np.array_equal(gd.check("knn dist").cpu().numpy(), od)
            assert same_bits(gi2.check("knn idx alone"), gi)


# ------------------------------------------------------------------------------------------------ 1. "overwritten"
@pytest.mark.parametrize("shape", [(2, 64, 1024), (3, 100, 37), (1, 1, 1), (2, 513, 515), (1, 2049, 70), (1, 70, 2049), (32, 64, 1024)])
def test_chamfer_backward_overwrites_and_either_gradient_may_be_null(oracle, shape):
    """"grad_xyz1 / grad_xyz2 are fully overwritten (no memset needed); either may be NULL": stale poison never shows, the rows
    no minimum names come out as the oracle's (zero contributions included), and dropping one output leaves the other's bits."""
    b, n, m = shape
    x1n, x2n = clouds(n * 7 + m, b, n, m)
    d1, i1, d2, i2 = oracle.chamfer_forward(x1n, x2n)
    rng = np.random.default_rng(n + m)
    g1n, g2n = rng.standard_normal((b, n)).astype(np.float32), rng.standard_normal((b, m)).astype(np.float32)
    g1n[:, ::3] = 0.0  # rows whose incoming gradient is zero still receive what the OTHER direction sends them
    g2n[:, 1::4] = 0.0
    o1, o2 = oracle.chamfer_backward(x1n, x2n, g1n, i1, g2n, i2)
    x1, x2, g1, g2, di1, di2 = dev(x1n), dev(x2n), dev(g1n), dev(g2n), dev(i1), dev(i2)
    a1, a2 = Guarded((b, n, 3)), Guarded((b, m, 3))
    call("sn_chamfer_backward", b, n, x1, m, x2, g1, di1, g2, di2, a1, a2, stream())
    torch.cuda.synchronize()
    assert np.array_equal(a1.check("grad_xyz1").cpu().numpy(), o1) and np.array_equal(a2.check("grad_xyz2").cpu().numpy(), o2)
    b1, b2 = Guarded((b, n, 3)), Guarded((b, m, 3))
    call("sn_chamfer_backward", b, n, x1, m, x2, g1, di1, g2, di2, b1, None, stream())
    call("sn_chamfer_backward", b, n, x1, m, x2, g1, di1, g2, di2, None, b2, stream())
    torch.cuda.synchronize()
    assert same_bits(b1.check("grad_xyz1 alone"), a1) and same_bits(b2.check("grad_xyz2 alone"), a2)
    # an all-zero upstream gradient gives an all-zero (not a stale) result
    z1, z2 = Guarded((b, n, 3)), Guarded((b, m, 3))
    call("sn_chamfer_backward", b, n, x1, m, x2, torch.zeros_like(g1), di1, torch.zeros_like(g2), di2, z1, z2, stream())
    torch.cuda.synchronize()
    assert not z1.check("zero upstream").any() and not z2.check("zero upstream").any()


# index-add shapes: (b, n, c, m, nsample); the last runs the atomic route ((n + 63) / 64 * m * nsample > 2^26 index loads)
GROUP_SHAPES = [(2, 50, 3, 20, 4), (3, 1000, 5, 64, 8), (1, 7, 1, 300, 9), (2, 300, 64, 33, 16), (1, 65536, 2, 2048, 33)]


def _group_idx(b, n, m, ns, seed):
    idx = np.random.default_rng(seed).integers(0, n, size=(b, m, ns)).astype(np.int32)
    idx[:, : min(m, 50), 0] = min(7, n - 1)  # one hot destination
    return idx


@pytest.mark.parametrize("shape", GROUP_SHAPES)
@pytest.mark.parametrize("channel_major", [False, True])
def test_group_gathers_and_their_gradients_overwrite(oracle, shape, channel_major):
    """sn_group_point[_grad] / sn_grouping_operation[_grad]: the gather is the oracle's bit for bit; the gradient is
    "overwritten (zero-filled inside)" on the ordered route (bit-identical to the oracle) and on the atomic route (within the
    summation bound): rows no index names are zero, not stale."""
    b, n, c, m, ns = shape
    atomic = ((n + 63) // 64) * m * ns > (1 << 26)
    idx = _group_idx(b, n, m, ns, n + c)
    idx[idx == 3 % n] = 4 % n  # destination 3 is named by nobody (when n > 4): it must come out 0
    rng = np.random.default_rng(c)
    if channel_major:
        X = rng.standard_normal((b, c, n)).astype(np.float32)
        go = rng.standard_normal((b, c, m, ns)).astype(np.float32)
        ref_out, ref_g = oracle.grouping_operation(X, idx), oracle.grouping_operation_grad((b, c, n), idx, go)
        out, g = Guarded((b, c, m, ns)), Guarded((b, c, n))
        call("sn_grouping_operation", b, c, n, m, ns, dev(X), dev(idx), out, stream())
        call("sn_grouping_operation_grad", b, c, n, m, ns, dev(go), dev(idx), g, stream())
        src = go.reshape(b, c, m * ns).transpose(0, 2, 1)
    else:
        X = rng.standard_normal((b, n, c)).astype(np.float32)
        go = rng.standard_normal((b, m, ns, c)).astype(np.float32)
        ref_out, ref_g = oracle.group_point(X, idx), oracle.group_point_grad((b, n, c), idx, go)
        out, g = Guarded((b, m, ns, c)), Guarded((b, n, c))
        call("sn_group_point", b, n, c, m, ns, dev(X), dev(idx), out, stream())
        call("sn_group_point_grad", b, n, c, m, ns, dev(go), dev(idx), g, stream())
        src = go.reshape(b, m * ns, c)
    torch.cuda.synchronize()
    assert np.array_equal(out.check("gather").cpu().numpy(), ref_out)
    got = g.check("gradient").cpu().numpy()
    if not atomic:
        assert np.array_equal(got, ref_g)
    f64, hits, sab = R.index_add(n, idx.reshape(b, m * ns), src)
    if channel_major:
        f64, sab = f64.transpose(0, 2, 1), sab.transpose(0, 2, 1)
        bound = hits[:, None, :] * 2.0 ** -24 * sab
        untouched = got.transpose(0, 2, 1)[hits == 0]
    else:
        bound = hits[:, :, None] * 2.0 ** -24 * sab
        untouched = got[hits == 0]
    print("max |grad - fp64| = %.3g, max bound %.3g" % (np.abs(got - f64).max(), bound.max()))
    assert (np.abs(got - f64) <= bound + 1e-30).all()
    assert untouched.size > 0 and not untouched.any()


# ================================================================================================ 2. weights
WEIGHT_CASES = [(1024, 64, 8, 1.0), (1024, 64, 7, 0.3), (2048, 64, 16, 0.05), (33, 7, 16, 1.0), (300, 40, 64, 0.05), (4100, 20, 33, 0.1)]


@pytest.mark.parametrize("cfg", WEIGHT_CASES)
def test_pairscan_weights_against_fp64_softmax(oracle, cfg):
    """`weights (B,M,K) optional softmax weights`: fp64 softmax over the kernel's own neighbours (= the oracle's) to 1e-6, rows
    sum to 1 to 1e-6, proj = the fp64 weighted sum of P[idx] with these weights to 1e-6; sn_soft_weights_forward on the same
    indices agrees to the same bar; `weights` without `proj` is the same bits."""
    N, M, K, T = cfg
    B, min_sigma = 2, 1e-2
    Pn, Qn = surface_queries(N * 3 + K, B, N, M)
    P, Q, Tt = dev(Pn), dev(Qn), torch.tensor(T, device="cuda")
    full = pairscan(P, Q, B, N, M, K, T=Tt, min_sigma=min_sigma)
    _, oi = oracle.knn(K, Pn, Qn)
    idx = full["knn_idx"].numpy()
    assert np.array_equal(idx, oi)
    sigma = sigma_of(T, min_sigma)
    w64 = R.soft_weights(Pn, Qn, idx, sigma)
    w = full["weights"].numpy()
    print("max |w - fp64| = %.3g" % np.abs(w - w64).max())
    np.testing.assert_allclose(w, w64, rtol=0, atol=1e-6)
    assert np.abs(w.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    nb = Pn.astype(np.float64)[np.arange(B)[:, None, None], idx]
    np.testing.assert_allclose(full["proj"].numpy(), (w.astype(np.float64)[..., None] * nb).sum(2), rtol=0, atol=1e-6)
    np.testing.assert_allclose(full["proj"].numpy(), R.soft_project(Pn, Qn, idx, sigma)[0], rtol=0, atol=1e-6)
    alone = pairscan(P, Q, B, N, M, K, want=("weights",), T=Tt, min_sigma=min_sigma)
    assert same_bits(alone["weights"], full["weights"])
    # the split entry (channel-major clouds) on the same indices
    w2 = Guarded((B, M, K))
    call("sn_soft_weights_forward", B, N, M, K, dev(t(Pn, BCN)), dev(t(Qn, BCN)), full["knn_idx"], Tt, min_sigma, w2, stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(w2.check("soft_weights_forward").cpu().numpy(), w64, rtol=0, atol=1e-6)
    np.testing.assert_allclose(w2.numpy(), w, rtol=0, atol=1e-6)
    # ... and the gather of sn_weighted_gather_forward with them is the projection
    pr = Guarded((B, 3, M))
    call("sn_weighted_gather_forward", B, 3, N, M, K, dev(t(Pn, BCN)), full["knn_idx"], w2, pr, stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(pr.check("weighted_gather_forward").cpu().numpy(), R.weighted_gather(t(Pn, BCN), idx, w2.numpy()), rtol=0,
                               atol=1e-6)


# ================================================================================================ 2. atomic accumulation
def _soft_case(seed, b, n, m, k):
    Pn, Qn = surface_queries(seed, b, n, m, cluster=True)
    from oracle import oracle as O

    _, idx = O.knn(k, Pn, Qn)
    return Pn, Qn, idx


@pytest.mark.parametrize("k", [1, 8, 16, 17, 64])
def test_soft_project_backward_accumulates_with_atomics(k):
    """sn_soft_project_backward: "grad_P optional (atomics)" ACCUMULATES -- g0 + gradient, twice gives g0 + 2 x gradient, g0 = 0
    agrees with the ordered entry; grad_Q and the b * sn_soft_bwd_splits(b, m) sigma partials are overwritten, identical bits
    in both forms and with grad_P NULL; the ordered entry overwrites grad_P."""
    from samplenet_amd._lib import lib

    b, n, m, T, min_sigma = 3, 300, 90, 0.3, 1e-2
    Pn, Qn, idx = _soft_case(k, b, n, m, k)
    sigma = sigma_of(T, min_sigma)
    gpn = np.random.default_rng(9 + k).standard_normal((b, m, 3)).astype(np.float32)
    _, _, rP, rQ, rs = R.soft_project(Pn, Qn, idx, sigma, gpn)
    g0n = np.random.default_rng(k).standard_normal((b, n, 3)).astype(np.float32)
    P, Q, I, gp, Tt = dev(Pn), dev(Qn), dev(idx), dev(gpn), torch.tensor(T, device="cuda")
    ns = lib.sn_soft_bwd_splits(b, m)

    def run(entry, g0, times=1):
        gQ, gs = Guarded((b, m, 3)), Guarded((b * ns,))
        gP = None if g0 is None else Guarded((b, n, 3), fill=g0)
        extra = (Guarded((b * m * k * 3,)),) if entry.endswith("ordered") else ()
        for _ in range(times):
            call(entry, b, n, m, k, P, BNC, Q, BNC, I, Tt, min_sigma, gp, BNC, gQ, BNC, gP, gs, *extra, stream())
        torch.cuda.synchronize()
        gQ.check(entry + " grad_Q"), gs.check(entry + " sigma partials")
        if gP is not None:
            gP.check(entry + " grad_P")
        for e in extra:
            assert e.guards_intact()
        return gQ, gs, gP

    aQ, aS, aP = run("sn_soft_project_backward", g0n)
    np.testing.assert_allclose(aP.numpy(), g0n.astype(np.float64) + rP, **ATOMIC)
    np.testing.assert_allclose(aQ.numpy(), rQ, **ATOMIC)
    np.testing.assert_allclose(aS.numpy().astype(np.float64).sum(), rs, **ATOMIC)
    _, _, a2 = run("sn_soft_project_backward", g0n, times=2)
    np.testing.assert_allclose(a2.numpy(), g0n.astype(np.float64) + 2 * rP, **ATOMIC)
    zQ, zS, zP = run("sn_soft_project_backward", np.zeros_like(g0n))
    oQ, oS, oP = run("sn_soft_project_backward_ordered", g0n)  # stale g0 must not leak: OVERWRITTEN
    np.testing.assert_allclose(oP.numpy(), rP, **ATOMIC)
    np.testing.assert_allclose(zP.numpy(), oP.numpy(), **ATOMIC)
    nQ, nS, _ = run("sn_soft_project_backward", None)
    for q, s in ((zQ, zS), (oQ, oS), (nQ, nS)):
        assert same_bits(q, aQ) and same_bits(s, aS)
    # optional grad_Q / sigma partials: the remaining outputs keep their bits
    gP = Guarded((b, n, 3), fill=np.zeros_like(g0n))
    sc = Guarded((b * m * k * 3,))
    call("sn_soft_project_backward_ordered", b, n, m, k, P, BNC, Q, BNC, I, Tt, min_sigma, gp, BNC, None, BNC, gP, None, sc, stream())
    torch.cuda.synchronize()
    assert same_bits(gP.check("ordered grad_P alone"), oP)
    # d loss / dT from the partials in one launch
    gT = Guarded((1,))
    call("sn_sigma_grad", b * ns, aS, Tt, min_sigma, gT, stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(gT.check("grad_T")[0]), rs * 2 * T if T * T > min_sigma else 0.0, **ATOMIC)


@pytest.mark.parametrize("k", [1, 8, 16, 17, 64])
def test_soft_weights_backward_accumulates_with_atomics(k):
    """sn_soft_weights_backward: grad_Q "[overwritten]", grad_P "[ACCUMULATED with atomics; may be NULL]", grad_sigma_partial
    "[overwritten]" -- and the `weights` argument is not read (recomputed): NULL gives the same bits."""
    from samplenet_amd._lib import lib

    b, n, m, T, min_sigma = 2, 300, 90, 0.3, 1e-2
    Pn, Qn, idx = _soft_case(100 + k, b, n, m, k)
    sigma = sigma_of(T, min_sigma)
    gwn = np.random.default_rng(k).standard_normal((b, m, k)).astype(np.float32)
    rP, rQ, rs = R.soft_weights_backward(Pn, Qn, idx, sigma, gwn)
    g0n = np.random.default_rng(k + 1).standard_normal((b, 3, n)).astype(np.float32)
    P, Q, I, gw, Tt = dev(t(Pn, BCN)), dev(t(Qn, BCN)), dev(idx), dev(gwn), torch.tensor(T, device="cuda")
    w = Guarded((b, m, k))
    call("sn_soft_weights_forward", b, n, m, k, P, Q, I, Tt, min_sigma, w, stream())
    ns = lib.sn_soft_bwd_splits(b, m)

    def run(entry, g0, times=1, weights=w):
        gQ, gs = Guarded((b, 3, m)), Guarded((b * ns,))
        gP = None if g0 is None else Guarded((b, 3, n), fill=g0)
        extra = (Guarded((b * m * k * 3,)),) if entry.endswith("ordered") else ()
        for _ in range(times):
            call(entry, b, n, m, k, P, Q, I, Tt, min_sigma, weights, gw, gQ, gP, gs, *extra, stream())
        torch.cuda.synchronize()
        gQ.check(entry + " grad_Q"), gs.check(entry + " sigma partials")
        if gP is not None:
            gP.check(entry + " grad_P")
        return gQ, gs, gP

    rPc = rP.transpose(0, 2, 1)
    aQ, aS, aP = run("sn_soft_weights_backward", g0n)
    np.testing.assert_allclose(aP.numpy(), g0n.astype(np.float64) + rPc, **ATOMIC)
    np.testing.assert_allclose(aQ.numpy(), rQ.transpose(0, 2, 1), **ATOMIC)
    np.testing.assert_allclose(aS.numpy().astype(np.float64).sum(), rs, **ATOMIC)
    _, _, a2 = run("sn_soft_weights_backward", g0n, times=2)
    np.testing.assert_allclose(a2.numpy(), g0n.astype(np.float64) + 2 * rPc, **ATOMIC)
    zQ, zS, zP = run("sn_soft_weights_backward", np.zeros_like(g0n), weights=None)
    oQ, oS, oP = run("sn_soft_weights_backward_ordered", g0n)
    np.testing.assert_allclose(oP.numpy(), rPc, **ATOMIC)
    np.testing.assert_allclose(zP.numpy(), oP.numpy(), **ATOMIC)
    nQ, nS, _ = run("sn_soft_weights_backward", None)
    for q, s in ((zQ, zS), (oQ, oS), (nQ, nS)):
        assert same_bits(q, aQ) and same_bits(s, aS)


@pytest.mark.parametrize("c", [1, 3, 5, 64])
@pytest.mark.parametrize("k", [1, 8, 17])
def test_weighted_gather_backward_accumulates_with_atomics(c, k):
    """sn_weighted_gather_backward: grad_w "[overwritten, may be NULL]", grad_X "[ACCUMULATED with atomics, may be NULL]"."""
    b, n, m = 2, 300, 90
    Pn, Qn, idx = _soft_case(7 * c + k, b, n, m, k)
    rng = np.random.default_rng(c * 100 + k)
    Xn = rng.standard_normal((b, c, n)).astype(np.float32)
    gon = rng.standard_normal((b, c, m)).astype(np.float32)
    wn = R.soft_weights(Pn, Qn, idx, 0.09).astype(np.float32)
    g0n = rng.standard_normal((b, c, n)).astype(np.float32)
    rw, rX = R.weighted_gather_backward(Xn, idx, wn, gon)
    X, I, w, go = dev(Xn), dev(idx), dev(wn), dev(gon)
    out = Guarded((b, c, m))
    call("sn_weighted_gather_forward", b, c, n, m, k, X, I, w, out, stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.check("forward").cpu().numpy(), R.weighted_gather(Xn, idx, wn), **ATOMIC)

    def run(entry, g0, times=1, want_gw=True):
        gw = Guarded((b, m, k)) if want_gw else None
        gX = None if g0 is None else Guarded((b, c, n), fill=g0)
        extra = (Guarded((b * c * m * k,)),) if entry.endswith("ordered") else ()
        for _ in range(times):
            call(entry, b, c, n, m, k, X, I, w, go, gw, gX, *extra, stream())
        torch.cuda.synchronize()
        if gw is not None:
            gw.check(entry + " grad_w")
        if gX is not None:
            gX.check(entry + " grad_X")
        return gw, gX

    aw, aX = run("sn_weighted_gather_backward", g0n)
    np.testing.assert_allclose(aX.numpy(), g0n.astype(np.float64) + rX, **ATOMIC)
    np.testing.assert_allclose(aw.numpy(), rw, **ATOMIC)
    _, a2 = run("sn_weighted_gather_backward", g0n, times=2)
    np.testing.assert_allclose(a2.numpy(), g0n.astype(np.float64) + 2 * rX, **ATOMIC)
    zw, zX = run("sn_weighted_gather_backward", np.zeros_like(g0n))
    ow, oX = run("sn_weighted_gather_backward_ordered", g0n)
    np.testing.assert_allclose(oX.numpy(), rX, **ATOMIC)
    np.testing.assert_allclose(zX.numpy(), oX.numpy(), **ATOMIC)
    nw, _ = run("sn_weighted_gather_backward", None)
    _, xX = run("sn_weighted_gather_backward_ordered", g0n, want_gw=False)
    assert same_bits(zw, aw) and same_bits(ow, aw) and same_bits(nw, aw) and same_bits(xX, oX)


# ================================================================================================ 3. layout selectors
@pytest.mark.parametrize("shape", [(2, 50, 40, 8), (2, 200, 40, 8), (2, 700, 40, 16), (2, 1500, 40, 17), (2, 3000, 40, 8)])
def test_pairscan_layout_selectors(shape):
    """p_layout x q_layout x proj_layout, one shape per points-per-lane class (1 / 4 / 16 / 32 / multi-chunk): every product
    bit-identical after transposing back."""
    B, N, M, K = shape
    Pn, Qn = tie_clouds(N + K, B, N, M)
    T = torch.tensor(0.4, device="cuda")
    base = pairscan(dev(Pn), dev(Qn), B, N, M, K, T=T)
    for pl in (BNC, BCN):
        for ql in (BNC, BCN):
            for jl in (BNC, BCN):
                got = pairscan(dev(t(Pn, pl)), dev(t(Qn, ql)), B, N, M, K, pl=pl, ql=ql, projl=jl, T=T)
                for k in PRODUCTS:
                    g = got[k].view()
                    if k == "proj":
                        g = back(g, jl).contiguous()
                    assert same_bits(g, base[k].view()), (k, pl, ql, jl)


@pytest.mark.parametrize("k", [8, 17])
def test_soft_project_backward_layout_selectors(k):
    """p_layout x q_layout x gproj_layout x gq_layout on both forms: grad_Q and the sigma partials bit-identical, the ordered
    grad_P bit-identical, the atomic grad_P within its bar."""
    from samplenet_amd._lib import lib

    b, n, m, T, min_sigma = 2, 300, 45, 0.3, 1e-2
    Pn, Qn, idx = _soft_case(k, b, n, m, k)
    gpn = np.random.default_rng(k).standard_normal((b, m, 3)).astype(np.float32)
    I, Tt, ns = dev(idx), torch.tensor(T, device="cuda"), lib.sn_soft_bwd_splits(b, m)
    base = None
    for pl in (BNC, BCN):
        for ql in (BNC, BCN):
            for gl in (BNC, BCN):
                for gql in (BNC, BCN):
                    P, Q, gp = dev(t(Pn, pl)), dev(t(Qn, ql)), dev(t(gpn, gl))
                    res = []
                    for entry in ("sn_soft_project_backward_ordered", "sn_soft_project_backward"):
                        gQ = Guarded((b, m, 3) if gql == BNC else (b, 3, m))
                        gP = Guarded((b, n, 3) if pl == BNC else (b, 3, n), fill=np.zeros((b, n, 3) if pl == BNC else (b, 3, n), np.float32))
                        gs = Guarded((b * ns,))
                        extra = (Guarded((b * m * k * 3,)),) if entry.endswith("ordered") else ()
                        call(entry, b, n, m, k, P, pl, Q, ql, I, Tt, min_sigma, gp, gl, gQ, gql, gP, gs, *extra, stream())
                        torch.cuda.synchronize()
                        res += [back(gQ.check("grad_Q"), gql).contiguous(), gs.check("partials"), back(gP.check("grad_P"), pl).contiguous()]
                    if base is None:
                        base = res
                        _, _, rP, rQ, _ = R.soft_project(Pn, Qn, idx, sigma_of(T, min_sigma), gpn)
                        np.testing.assert_allclose(res[0].cpu().numpy(), rQ, **ATOMIC)
                        np.testing.assert_allclose(res[2].cpu().numpy(), rP, **ATOMIC)
                    for i in (0, 1, 2, 3, 4):
                        assert same_bits(res[i], base[i]), (i, pl, ql, gl, gql)
                    assert same_bits(res[3], res[0]) and same_bits(res[4], res[1])  # atomic and ordered form: same kernel
                    np.testing.assert_allclose(res[5].cpu().numpy(), base[2].cpu().numpy(), **ATOMIC)
    for pos in (5, 7, 12, 14):  # a selector other than 0 / 1 is refused before any launch
        a = [b, n, m, k, P, pl, Q, ql, I, Tt, min_sigma, gp, gl, gQ, gql, gP, gs]
        a[pos] = 2
        call("sn_soft_project_backward", *a, stream(), expect=BAD_ARGUMENT)


@pytest.mark.parametrize("shape", [(4, 64, 1024), (2, 33, 300), (3, 128, 2500), (1, 1, 5)])
def test_simplification_and_chamfer_mean_loss(oracle, shape):
    """sn_simplification_loss_* / sn_chamfer_mean_loss_*: value and both gradients against fp64; layout1 = 1 on a transposed
    sample gives grad_xyz1's bits transposed; either gradient may be NULL; layout1 = 1 with grad_xyz2 is SN_ERR_BAD_ARGUMENT;
    outputs are overwritten."""
    B, n1, n2 = shape
    x2n, x1n = clouds(n1 + n2, B, n2, n1)
    d1n, i1n, d2n, i2n = oracle.chamfer_forward(x1n, x2n)
    x1, x2, d1, i1, d2, i2 = dev(x1n), dev(x2n), dev(d1n), dev(i1n), dev(d2n), dev(i2n)
    weight, gl = 1.5, torch.tensor(0.7, device="cuda")
    for with_max in (True, False):
        part, am, loss = Guarded((B * 3,)), Guarded((B,), I32), Guarded((1,))
        if with_max:
            call("sn_simplification_loss_forward", B, n1, n2, d1, d2, weight, part, am, loss, stream())
        else:
            call("sn_chamfer_mean_loss_forward", B, n1, n2, d1, d2, part, am, loss, stream())
        torch.cuda.synchronize()
        part.check("partial"), am.check("argmax1")
        w = weight if with_max else 1.0
        rl, r1, r2 = R.simplification_loss(x1n, x2n, i1n, i2n, w, with_max=with_max, grad_loss=0.7)
        np.testing.assert_allclose(float(loss.check("loss")[0]), rl, rtol=1e-5, atol=1e-7)
        assert np.array_equal(am.numpy(), d1n.argmax(1))

        def bwd(g1, g2, xa=x1, layout1=0, expect=0):
            if with_max:
                return call("sn_simplification_loss_backward", B, n1, xa, n2, x2, i1, i2, am, weight, gl, g1, g2, layout1, stream(),
                            expect=expect)
            return call("sn_chamfer_mean_loss_backward", B, n1, xa, n2, x2, i1, i2, gl, g1, g2, stream(), expect=expect)

        g1, g2 = Guarded((B, n1, 3)), Guarded((B, n2, 3))
        bwd(g1, g2)
        h1, h2 = Guarded((B, n1, 3)), Guarded((B, n2, 3))
        bwd(h1, None), bwd(None, h2)
        torch.cuda.synchronize()
        np.testing.assert_allclose(g1.check("grad_xyz1").cpu().numpy(), r1, **PLAIN)
        np.testing.assert_allclose(g2.check("grad_xyz2").cpu().numpy(), r2, **PLAIN)
        assert same_bits(h1.check("grad_xyz1 alone"), g1) and same_bits(h2.check("grad_xyz2 alone"), g2)
        if with_max:
            c1 = Guarded((B, 3, n1))
            bwd(c1, None, xa=dev(t(x1n, BCN)), layout1=1)
            torch.cuda.synchronize()
            assert same_bits(c1.check("channel-major grad_xyz1").transpose(1, 2).contiguous(), g1)
            bwd(c1, g2, xa=dev(t(x1n, BCN)), layout1=1, expect=BAD_ARGUMENT)
            bwd(g1, g2, layout1=2, expect=BAD_ARGUMENT)


@pytest.mark.parametrize("B", [1, 7, 300])
def test_pcrnet_head_and_qrot_optional_pointers(B):
    """sn_pcrnet_head_forward/backward ("quat optional", "qnorm NULL: not wanted", "each may be NULL") and sn_qrot_* ("either may
    be NULL"): fp64 values, and every NULL combination leaves the remaining outputs' bits."""
    rng = np.random.default_rng(B)
    yn = rng.standard_normal((B, 7)).astype(np.float32)
    gtn, gqn = rng.standard_normal((B, 7)).astype(np.float32), rng.standard_normal((B, 4)).astype(np.float32)
    y, gt, gq, gn = dev(yn), dev(gtn), dev(gqn), torch.tensor(0.3, device="cuda")
    tw, qu, qn = Guarded((B, 7)), Guarded((B, 4)), Guarded((1,))
    call("sn_pcrnet_head_forward", B, y, tw, qu, qn, stream())
    torch.cuda.synchronize()
    rt, rq, rn, _ = R.pcrnet_head(yn)
    np.testing.assert_allclose(tw.check("twist").cpu().numpy(), rt, **PLAIN)
    np.testing.assert_allclose(qu.check("quat").cpu().numpy(), rq, **PLAIN)
    np.testing.assert_allclose(float(qn.check("qnorm")[0]), rn, rtol=1e-5)
    for want_q, want_n in ((False, False), (True, False), (False, True)):
        tw2, qu2, qn2 = Guarded((B, 7)), Guarded((B, 4)) if want_q else None, Guarded((1,)) if want_n else None
        call("sn_pcrnet_head_forward", B, y, tw2, qu2, qn2, stream())
        torch.cuda.synchronize()
        assert same_bits(tw2.check("twist"), tw)
        assert qu2 is None or same_bits(qu2.check("quat"), qu)
        assert qn2 is None or same_bits(qn2.check("qnorm"), qn)
    for a, b_, c in ((gt, gq, gn), (gt, None, None), (None, gq, None), (None, None, gn), (gt, gq, None), (None, None, None)):
        gy = Guarded((B, 7))
        call("sn_pcrnet_head_backward", B, y, a, b_, c, gy, stream())
        torch.cuda.synchronize()
        ref = R.pcrnet_head(yn, gtn if a is not None else None, gqn if b_ is not None else None, 0.3 if c is not None else None)[3]
        np.testing.assert_allclose(gy.check("g_y").cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref).max()))
    # rotation
    N = 130
    qn_ = rq.astype(np.float32)
    vn, gon = rng.standard_normal((B, N, 3)).astype(np.float32), rng.standard_normal((B, N, 3)).astype(np.float32)
    q, v, go = dev(qn_), dev(vn), dev(gon)
    out, gqt, gv = Guarded((B, N, 3)), Guarded((B, 4)), Guarded((B, N, 3))
    call("sn_qrot_forward", B, N, q, v, out, stream())
    call("sn_qrot_backward", B, N, q, v, go, gqt, gv, stream())
    g1, g2 = Guarded((B, 4)), Guarded((B, N, 3))
    call("sn_qrot_backward", B, N, q, v, go, g1, None, stream())
    call("sn_qrot_backward", B, N, q, v, go, None, g2, stream())
    torch.cuda.synchronize()
    ro, rgq, rgv = R.qrot(qn_, vn, gon)
    np.testing.assert_allclose(out.check("qrot").cpu().numpy(), ro, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gv.check("grad_v").cpu().numpy(), rgv, rtol=1e-5, atol=1e-5)
    # grad_quat sums N terms of unit scale per cloud: N * 2^-24 * sum|terms| <= N * 2^-24 * (8 N) on these inputs
    np.testing.assert_allclose(gqt.check("grad_quat").cpu().numpy(), rgq, rtol=1e-4, atol=1e-4)
    assert same_bits(g1.check("grad_quat alone"), gqt) and same_bits(g2.check("grad_v alone"), gv)


# ================================================================================================ 4. routing grid
GRID_N = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4100]
GRID_K = [1, 2, 8, 9, 16, 17, 33, 64]


def _grid():
    cases = []
    for N in GRID_N:
        for M in (1, 64):
            for B in (1, 32):
                if B == 32 and N > 2048:  # the oracle is a CPU loop over B x M x N: 32 clouds only up to one chunk
                    continue
                cases.append((B, N, M))
    for N in (64, 2048, 2049):  # the swapped scan above 2048 points on either side
        for B in (1, 32):
            if B == 32 and N > 2048:
                continue
            cases.append((B, N, 2100))
    for B in (16, 17, 512, 513):  # pairscan_ysplit: many workgroups per cloud -> one; B >= 512 switches the 4-wave workgroups on
        cases.append((B, 1024, 64))
    return [(B, N, M, K) for (B, N, M) in cases for K in GRID_K if K <= N]


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "B%d-N%d-M%d-K%d" % c)
def test_pairscan_routing_grid(oracle, case):
    """sn_pairscan_forward_ws, all products, against the oracle (indices and squared distances bit-exact, proj 1e-6) across
    every kernel instantiation the dispatch chooses between -- with the reported workspace, without one (both entries), and
    with one a byte too small (the one-workgroup-per-cloud fallback): identical bits.

    Measured on an MI355X (the figures this test prints), over the 464 cases: proj is within 8.4e-7 of the oracle and within
    1.8e-7 of fp64; the oracle itself (an fp32 loop) is within 8.4e-7 of fp64, at K = 64.  The kernel's sums of more than 16
    terms run in fp64 for that reason: as fp32 running sums they were as far from fp64 as the oracle's, and two cases (B = 512 /
    513, N = 1024, M = 64, K = 64) had one element each 1.3e-6 / 1.2e-6 from the oracle."""
    B, N, M, K = case
    Pn, Qn, P, Q, T = scan_inputs(N * 5 + M + K, B, N, M)
    full = pairscan(P, Q, B, N, M, K, T=T, form="ws")
    od, oi = oracle.knn(K, Pn, Qn)
    assert np.array_equal(full["knn_idx"].numpy(), oi)
    assert np.array_equal(full["knn_dist"].numpy(), od)
    cq, ciq, cp, cip = oracle.chamfer_forward(Qn, Pn)
    for k, ref in (("dist_q", cq), ("idx_q", ciq), ("dist_p", cp), ("idx_p", cip)):
        assert np.array_equal(full[k].numpy(), ref), k
    oproj, _, _ = oracle.softproj_forward(t(Pn, BCN), t(Qn, BCN), oi, sigma_of(0.5, 1e-2))
    p64 = R.soft_project(Pn, Qn, oi, sigma_of(0.5, 1e-2))[0]
    print("proj: max |kernel - oracle| = %.3g, |kernel - fp64| = %.3g, |oracle - fp64| = %.3g" % (
        np.abs(full["proj"].numpy() - oproj.transpose(0, 2, 1)).max(), np.abs(full["proj"].numpy() - p64).max(),
        np.abs(oproj.transpose(0, 2, 1) - p64).max()))
    np.testing.assert_allclose(full["proj"].numpy(), oproj.transpose(0, 2, 1), rtol=0, atol=1e-6)
    np.testing.assert_allclose(full["weights"].numpy(), R.soft_weights(Pn, Qn, oi, sigma_of(0.5, 1e-2)), rtol=0, atol=1e-6)
    for form in ("null", "ws-null", "short"):
        got = pairscan(P, Q, B, N, M, K, T=T, form=form)
        for k in PRODUCTS:
            assert same_bits(got[k], full[k]), (k, form)


@pytest.mark.parametrize("cfg", [(2, 700, 300, (1, 7, 64, 300)), (1, 2500, 64, (64,)), (33, 100, 40, tuple(range(1, 31, 2)) + (40,))])
def test_prefix_point_minima_raw(oracle, cfg):
    """sn_prefix_point_minima: slice j equals the Chamfer per-point side of Q[:, :s_j] bit for bit; (nprefix, B, N) overwritten."""
    B, N, M, sizes = cfg
    Pn, Qn = clouds(N + M, B, N, M)
    hs = (ctypes.c_int * len(sizes))(*sizes)
    d, i = Guarded((len(sizes), B, N)), Guarded((len(sizes), B, N), I32)
    call("sn_prefix_point_minima", B, N, M, len(sizes), ctypes.cast(hs, ctypes.c_void_p), dev(Pn), dev(Qn), d, i, stream())
    torch.cuda.synchronize()
    d.check("dist"), i.check("idx")
    for j, s in enumerate(sizes):
        _, _, rd, ri = oracle.chamfer_forward(Qn[:, :s], Pn)
        assert np.array_equal(d.numpy()[j], rd) and np.array_equal(i.numpy()[j], ri), s


@pytest.mark.parametrize("cfg", [(3, 1024, 64, BNC), (2, 3000, 100, BCN), (1, 8192, 1024, BNC), (2, 50, 64, BCN)])
def test_nn_matching_raw(oracle, cfg):
    """sn_nn_matching: out (B,k,3) overwritten, exact parity with the float64 numpy completion, both layouts, both modes."""
    B, N, k, layout = cfg
    Pn, _ = clouds(N + k, B, N, 13)
    idx = np.random.default_rng(k).integers(0, N, size=(B, k)).astype(np.int32)
    idx[:, 1::2] = idx[:, ::2][:, : idx[:, 1::2].shape[1]]  # duplicates: the completion has work to do
    for fps in (1, 0):
        out = Guarded((B, k, 3))
        call("sn_nn_matching", B, N, k, dev(t(Pn, layout)), layout, dev(idx), fps, out, stream())
        torch.cuda.synchronize()
        ref = oracle.nn_matching(Pn, idx, k, complete_fps=bool(fps))
        assert np.array_equal(out.check("nn_matching").cpu().numpy().astype(np.float64), ref)


# ================================================================================================ 5. streams, capture, threads
class Family:
    """A group of entries on fixed buffers: load(seed) refills the inputs in place, launch() enqueues every entry on torch's
    current stream, results() names the outputs -- `exact` ones must reproduce bit for bit, `atomic` ones within ATOMIC."""

    atomic = ()

    def load(self, seed):
        for k, v in self.make(seed).items():
            if k in self.inp:
                self.inp[k].copy_(dev(v))
            else:
                self.inp[k] = dev(v)

    def __init__(self, seed=0):
        self.inp, self.out = {}, {}
        self.load(seed)
        self.alloc()

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.view().clone() for k, v in self.out.items()}

    def compare(self, got, ref, what):
        for k in ref:
            if k in self.atomic:
                np.testing.assert_allclose(got[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg="%s: %s" % (what, k), **ATOMIC)
            else:
                assert same_bits(got[k], ref[k]), "%s: %s differs" % (what, k)


class ScanFamily(Family):
    B, N, M, K = 4, 1024, 64, 8
    sizes = (8, 32, 64)

    def make(self, seed):
        P, Q = tie_clouds(seed, self.B, self.N, self.M)
        return {"P": P, "Q": Q, "T": np.float32(0.5 + 0.01 * (seed % 7))}

    def alloc(self):
        from samplenet_amd._lib import lib

        B, N, M, K = self.B, self.N, self.M, self.K
        shp = {"knn_idx": ((B, M, K), I32), "knn_dist": ((B, M, K), F32), "dist_q": ((B, M), F32), "idx_q": ((B, M), I32),
               "dist_p": ((B, N), F32), "idx_p": ((B, N), I32), "proj": ((B, M, 3), F32), "weights": ((B, M, K), F32)}
        for tag in ("ws", "nows"):
            for k, (s, d) in shp.items():
                self.out[tag + "." + k] = Guarded(s, d)
        self.wb = int(lib.sn_pairscan_workspace_bytes(B, N, M))
        self.ws = Guarded((max(self.wb, 4) // 4,), I32)
        for k in ("cd1", "cd2"):
            self.out[k] = Guarded((B, M) if k == "cd1" else (B, N), F32)
            self.out[k + "i"] = Guarded((B, M) if k == "cd1" else (B, N), I32)
        self.out["knn.idx"], self.out["knn.dist"] = Guarded((B, M, K), I32), Guarded((B, M, K), F32)
        self.out["pre.d"], self.out["pre.i"] = Guarded((len(self.sizes), B, N)), Guarded((len(self.sizes), B, N), I32)
        self.hs = (ctypes.c_int * len(self.sizes))(*self.sizes)

    def launch(self):
        B, N, M, K = self.B, self.N, self.M, self.K
        i, o, s = self.inp, self.out, stream()
        for tag in ("ws", "nows"):
            a = [B, N, M, K, i["P"], BNC, i["Q"], BNC] + [o[tag + "." + k] for k in PRODUCTS[:6]] + [o[tag + ".proj"], BNC, o[tag + ".weights"],
                                                                                                  i["T"], 1e-2]
            if tag == "ws":
                call("sn_pairscan_forward_ws", *a, self.ws if self.wb else None, self.wb, s)
            else:
                call("sn_pairscan_forward", *a, s)
        call("sn_chamfer_forward", B, M, i["Q"], N, i["P"], o["cd1"], o["cd1i"], o["cd2"], o["cd2i"], s)
        call("sn_knn", B, N, M, K, i["P"], BNC, i["Q"], BNC, o["knn.idx"], o["knn.dist"], s)
        call("sn_prefix_point_minima", B, N, M, len(self.sizes), ctypes.cast(self.hs, ctypes.c_void_p), i["P"], i["Q"], o["pre.d"],
             o["pre.i"], s)


class SoftFamily(Family):
    b, n, m, k, c = 3, 300, 60, 8, 5
    atomic = ("a.gP", "w.gP", "g.gX")

    def make(self, seed):
        from oracle import oracle as O

        P, Q = surface_queries(seed, self.b, self.n, self.m, cluster=True)
        rng = np.random.default_rng(seed)
        sn = lambda *s: rng.standard_normal(s).astype(np.float32)
        return {"P": t(P, BCN), "Q": t(Q, BCN), "idx": O.knn(self.k, P, Q)[1], "T": np.float32(0.3), "gproj": sn(self.b, 3, self.m),
                "gw": sn(self.b, self.m, self.k), "X": sn(self.b, self.c, self.n), "go": sn(self.b, self.c, self.m)}

    def alloc(self):
        from samplenet_amd._lib import lib

        b, n, m, k, c = self.b, self.n, self.m, self.k, self.c
        self.ns = lib.sn_soft_bwd_splits(b, m)
        o = self.out
        o["w"], o["gather"] = Guarded((b, m, k)), Guarded((b, c, m))
        for tag in ("a", "o", "w", "wo"):  # fused atomic / ordered, split atomic / ordered
            o[tag + ".gQ"], o[tag + ".gP"], o[tag + ".gs"] = Guarded((b, 3, m)), Guarded((b, 3, n)), Guarded((b * self.ns,))
        for tag in ("g", "go"):
            o[tag + ".gw"], o[tag + ".gX"] = Guarded((b, m, k)), Guarded((b, c, n))
        o["gT"] = Guarded((1,))
        self.scratch = Guarded((b * max(c, 3) * m * k,))

    def launch(self):
        b, n, m, k, c = self.b, self.n, self.m, self.k, self.c
        i, o, s = self.inp, self.out, stream()
        for tag in ("a", "w"):
            o[tag + ".gP"].view().zero_()  # the accumulating forms start from zero (a memset node on the same stream)
        o["g.gX"].view().zero_()
        call("sn_soft_weights_forward", b, n, m, k, i["P"], i["Q"], i["idx"], i["T"], 1e-2, o["w"], s)
        call("sn_weighted_gather_forward", b, c, n, m, k, i["X"], i["idx"], o["w"], o["gather"], s)
        pre = (b, n, m, k, i["P"], BCN, i["Q"], BCN, i["idx"], i["T"], 1e-2, i["gproj"], BCN)
        call("sn_soft_project_backward", *pre, o["a.gQ"], BCN, o["a.gP"], o["a.gs"], s)
        call("sn_soft_project_backward_ordered", *pre, o["o.gQ"], BCN, o["o.gP"], o["o.gs"], self.scratch, s)
        pre = (b, n, m, k, i["P"], i["Q"], i["idx"], i["T"], 1e-2, o["w"], i["gw"])
        call("sn_soft_weights_backward", *pre, o["w.gQ"], o["w.gP"], o["w.gs"], s)
        call("sn_soft_weights_backward_ordered", *pre, o["wo.gQ"], o["wo.gP"], o["wo.gs"], self.scratch, s)
        pre = (b, c, n, m, k, i["X"], i["idx"], o["w"], i["go"])
        call("sn_weighted_gather_backward", *pre, o["g.gw"], o["g.gX"], s)
        call("sn_weighted_gather_backward_ordered", *pre, o["go.gw"], o["go.gX"], self.scratch, s)
        call("sn_sigma_grad", b * self.ns, o["o.gs"], i["T"], 1e-2, o["gT"], s)


class GroupFamily(Family):
    b, n, c, m, ns, k = 2, 500, 6, 40, 8, 32

    def make(self, seed):
        rng = np.random.default_rng(seed)
        sn = lambda *s: rng.standard_normal(s).astype(np.float32)
        b, n, c, m, ns = self.b, self.n, self.c, self.m, self.ns
        return {"pts": sn(b, n, c), "feat": sn(b, c, n), "idx": _group_idx(b, n, m, ns, seed), "go": sn(b, m, ns, c), "gof": sn(b, c, m, ns),
                "xyz": sn(b, n, 3), "midx": rng.integers(0, n // 4, size=(b, self.k)).astype(np.int32)}

    def alloc(self):
        b, n, c, m, ns = self.b, self.n, self.c, self.m, self.ns
        self.out.update({"gp": Guarded((b, m, ns, c)), "gpg": Guarded((b, n, c)), "gr": Guarded((b, c, m, ns)), "grg": Guarded((b, c, n)),
                         "nm": Guarded((b, self.k, 3)), "nm0": Guarded((b, self.k, 3))})

    def launch(self):
        b, n, c, m, ns = self.b, self.n, self.c, self.m, self.ns
        i, o, s = self.inp, self.out, stream()
        call("sn_group_point", b, n, c, m, ns, i["pts"], i["idx"], o["gp"], s)
        call("sn_group_point_grad", b, n, c, m, ns, i["go"], i["idx"], o["gpg"], s)
        call("sn_grouping_operation", b, c, n, m, ns, i["feat"], i["idx"], o["gr"], s)
        call("sn_grouping_operation_grad", b, c, n, m, ns, i["gof"], i["idx"], o["grg"], s)
        call("sn_nn_matching", b, n, self.k, i["xyz"], BNC, i["midx"], 1, o["nm"], s)
        call("sn_nn_matching", b, n, self.k, i["xyz"], BNC, i["midx"], 0, o["nm0"], s)


class LossFamily(Family):
    B, n1, n2 = 4, 64, 700

    def make(self, seed):
        from oracle import oracle as O

        x2, x1 = clouds(seed, self.B, self.n2, self.n1)
        d1, i1, d2, i2 = O.chamfer_forward(x1, x2)
        rng = np.random.default_rng(seed)
        sn = lambda *s: rng.standard_normal(s).astype(np.float32)
        return {"x1": x1, "x2": x2, "d1": d1, "i1": i1, "d2": d2, "i2": i2, "g1": sn(self.B, self.n1), "g2": sn(self.B, self.n2),
                "gl": np.float32(0.7), "y": sn(self.B, 7), "gt": sn(self.B, 7), "gq": sn(self.B, 4), "gn": np.float32(0.3),
                "go": sn(self.B, self.n2, 3)}

    def alloc(self):
        B, n1, n2 = self.B, self.n1, self.n2
        o = self.out
        o["cb1"], o["cb2"] = Guarded((B, n1, 3)), Guarded((B, n2, 3))
        for tag in ("s", "m"):
            o[tag + ".part"], o[tag + ".am"], o[tag + ".loss"] = Guarded((B * 3,)), Guarded((B,), I32), Guarded((1,))
            o[tag + ".g1"], o[tag + ".g2"] = Guarded((B, n1, 3)), Guarded((B, n2, 3))
        o["twist"], o["quat"], o["qnorm"], o["gy"] = Guarded((B, 7)), Guarded((B, 4)), Guarded((1,)), Guarded((B, 7))
        o["rot"], o["rgq"], o["rgv"] = Guarded((B, n2, 3)), Guarded((B, 4)), Guarded((B, n2, 3))

    def launch(self):
        B, n1, n2 = self.B, self.n1, self.n2
        i, o, s = self.inp, self.out, stream()
        call("sn_chamfer_backward", B, n1, i["x1"], n2, i["x2"], i["g1"], i["i1"], i["g2"], i["i2"], o["cb1"], o["cb2"], s)
        call("sn_simplification_loss_forward", B, n1, n2, i["d1"], i["d2"], 1.5, o["s.part"], o["s.am"], o["s.loss"], s)
        call("sn_simplification_loss_backward", B, n1, i["x1"], n2, i["x2"], i["i1"], i["i2"], o["s.am"], 1.5, i["gl"], o["s.g1"], o["s.g2"],
             0, s)
        call("sn_chamfer_mean_loss_forward", B, n1, n2, i["d1"], i["d2"], o["m.part"], o["m.am"], o["m.loss"], s)
        call("sn_chamfer_mean_loss_backward", B, n1, i["x1"], n2, i["x2"], i["i1"], i["i2"], i["gl"], o["m.g1"], o["m.g2"], s)
        call("sn_pcrnet_head_forward", B, i["y"], o["twist"], o["quat"], o["qnorm"], s)
        call("sn_pcrnet_head_backward", B, i["y"], i["gt"], i["gq"], i["gn"], o["gy"], s)
        call("sn_qrot_forward", B, n2, o["quat"], i["x2"], o["rot"], s)
        call("sn_qrot_backward", B, n2, o["quat"], i["x2"], i["go"], o["rgq"], o["rgv"], s)


FAMILIES = [ScanFamily, SoftFamily, GroupFamily, LossFamily]


def test_the_families_reach_every_entry_in_scope():
    import inspect
    import re

    from test_cabi_arguments import ENTRIES

    text = "".join(inspect.getsource(f.launch) + inspect.getsource(f.alloc) for f in FAMILIES)
    called = set(re.findall(r"\"(sn_[a-z0-9_]+)\"", text)) | set(re.findall(r"lib\.(sn_[a-z0-9_]+)", text))
    assert not set(ENTRIES) - called, set(ENTRIES) - called
    assert {"sn_pairscan_workspace_bytes", "sn_soft_bwd_splits"} <= called


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_any_stream_gives_the_default_stream_result(family):
    """"work is enqueued on `stream`": every entry on a side stream, while the default stream is kept busy with unrelated work,
    gives the bits of the default-stream call; every output is overwritten and guarded."""
    fam = family(seed=3)
    fam.launch()
    ref = fam.snapshot()
    for g in fam.out.values():
        g.check(family.__name__)
        g.words().fill_(R.POISON)
    side = torch.cuda.Stream()
    busy = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    for _ in range(8):
        busy = busy @ busy * 1e-3  # the default stream has work in flight while the side stream runs
    with torch.cuda.stream(side):
        fam.launch()
    side.synchronize()
    got = {k: v.check(family.__name__ + " side stream").clone() for k, v in fam.out.items()}
    fam.compare(got, ref, "side stream")
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_entries_are_safe_under_stream_capture(family):
    """"the call returns without synchronising (safe under hipGraph stream capture)": one captured graph per family, replayed
    twice on changed input contents, equals the eager calls on the same inputs."""
    fam = family(seed=5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fam.launch()  # warm-up outside the capture (first-use runtime work)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fam.launch()
    for seed in (11, 12):
        fam.load(seed)
        for g in fam.out.values():
            g.words().fill_(R.POISON)
        torch.cuda.synchronize()
        graph.replay()
        got = fam.snapshot()
        for k, g in fam.out.items():
            g.check("%s replay: %s" % (family.__name__, k))
        fam.launch()
        fam.compare(got, fam.snapshot(), "replay of seed %d" % seed)


def test_four_host_threads_with_their_own_streams():
    """"re-entrant; any number of streams / host threads": four threads, each looping a different family twenty times on its
    own stream and buffers while the others run, reproduce the serial results; the error text is per thread: each thread first
    provokes its own SN_ERR_BAD_ARGUMENT (a negative size: rejected on the host, no device work) and still reads its own message
    after the loop, while every other call of every thread returned 0."""
    from samplenet_amd._lib import lib

    fams = [f(seed=20 + i) for i, f in enumerate(FAMILIES)]
    serial = []
    for f in fams:
        f.launch()
        serial.append(f.snapshot())
    provoke = [("sn_knn", (-1, 8, 4, 2, None, 0, None, 0, None, None, None)),
               ("sn_soft_weights_forward", (1, 8, -4, 2, None, None, None, None, 0.0, None, None)),
               ("sn_group_point", (1, -8, 3, 4, 2, None, None, None, None)),
               ("sn_qrot_forward", (-1, 8, None, None, None, None))]
    errors, barrier = [None] * 4, threading.Barrier(4)

    def work(i):
        try:
            torch.cuda.set_device(0)
            name, args = provoke[i]
            assert getattr(lib, name)(*args) == BAD_ARGUMENT
            barrier.wait(timeout=120)
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(20):
                    fams[i].launch()  # (call() asserts that every entry returned 0)
            st.synchronize()
            msg = (lib.sn_last_error_string() or b"").decode()
            assert msg.startswith(name + ":"), "thread %d reads %r" % (i, msg)
        except BaseException as e:  # noqa: BLE001 -- reported in the main thread
            errors[i] = e
            try:
                barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not any(th.is_alive() for th in threads)
    for e in errors:
        if e is not None:
            raise e
    for f, ref in zip(fams, serial):
        f.compare(f.snapshot(), ref, type(f).__name__ + " threaded")
        for g in f.out.values():
            assert g.guards_intact()

"""The one-batch task-evaluation entries, called directly, edge by edge (BASELINE configs[4]: the registration task on every prefix of
the progressive sampler as ONE batch): sn_cyclic_pad_cat / _backward, sn_chamfer_forward_valid, sn_chamfer_mean_loss_*_grouped,
sn_pcrnet_head_rot_*_grouped and the ungrouped sn_pcrnet_head_rot_* they share kernels with.

Every call goes through samplenet_amd._lib.lib with raw pointers, so that NULL arguments and guarded buffers can be said: every output
lives between poisoned guard words (tests/cabi_ref.py: Guarded), which turns an out-of-range store into a failed assertion and an
element left unwritten -- or one that the header says STAYS unwritten -- into a visible one.  Three yardsticks, each independent of the
route under test: (1) the header's promise "equals the evaluation's own ungrouped call on the unpadded cloud, bit for bit";
(2) plain restatements (tests/task_batch_ref.py: torch indexing, a sequential float32 sum, the scan as float32 numpy), bit for bit;
(3) fp64 references under bounds counted from the kernels' own operations (same file), never looser than the bars the suite already
holds the ungrouped forms to.  The shape tables in the helper say which branch each row reaches."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cabi_ref as R  # noqa: E402
import task_batch_ref as T  # noqa: E402
from cabi_ref import POISON, Guarded, arg  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
PLAIN = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_cabi_contract.py: plain elementwise results against fp64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    from samplenet_amd._lib import check, lib

    check(getattr(lib, name)(*[arg(a) for a in args]), name)


def ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[arg(b) for b in bufs])


def bits(a):
    a = a.view() if isinstance(a, Guarded) else a
    return a.contiguous().view(torch.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


# ================================================================================================ 1. sn_cyclic_pad_cat / _backward
_pad_id = lambda c: "B%d-C%d-%dclouds-len%d" % (c[0], c[1], len(c[2]), max(c[2]))


@pytest.mark.parametrize("case", T.PAD_CASES, ids=_pad_id)
def test_cyclic_pad_cat_forward_is_a_pure_copy(case):
    """out[(j B + b), m, :] = src_j[b, m mod s_j, :]: equal to torch indexing, every element written, no guard word changed."""
    B, C, sizes = case
    L, E = max(sizes), len(sizes)
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + C + L)
    cl = [torch.randn(B, s, C, device="cuda", generator=g) for s in sizes]
    out = Guarded((E * B, L, C))
    call("sn_cyclic_pad_cat", B, L, C, E, ints(sizes), ptrs(cl), out, stream())
    torch.cuda.synchronize()
    assert torch.equal(out.check("padded batch"), torch.cat([T.pad(c, L) for c in cl], dim=0))


def _pad_backward(B, C, sizes, gout, null=()):
    L, E = max(sizes), len(sizes)
    grads = [None if j in null else Guarded((B, s, C)) for j, s in enumerate(sizes)]
    decoys = [Guarded((B, sizes[j], C)) for j in null]  # where a stray store of the skipped cloud is likeliest to land
    call("sn_cyclic_pad_cat_backward", B, L, C, E, ints(sizes), gout, ptrs(grads), stream())
    torch.cuda.synchronize()
    for d in decoys:
        assert d.untouched(), "a NULL entry of grads was written somewhere"
    return [None if gb is None else gb.check("grads[%d]" % j) for j, gb in enumerate(grads)]


@pytest.mark.parametrize("case", T.PAD_CASES, ids=_pad_id)
def test_cyclic_pad_cat_backward_adds_the_copies_in_order(case):
    """grads[j] = the original's gradient, then its copies' in ascending order, in fp32: bit for bit a sequential float32 sum; integer
    gradients with |g| <= 8 (every partial sum exact) equal fp64 exactly; real data within (n - 1) 2^-24 sum|g| per element, n =
    ceil(len / size) terms -- the bound of an n-term sequential sum; a size equal to len hands the gradient through unchanged; a NULL
    entry is skipped (the others keep their bits, a guarded decoy of the skipped cloud's size stays untouched)."""
    B, C, sizes = case
    L, E = max(sizes), len(sizes)
    g = torch.Generator(device="cuda").manual_seed(B * 77 + C * 5 + L)
    gi = torch.randint(-8, 9, (E * B, L, C), device="cuda", generator=g).float()
    gr = torch.randn(E * B, L, C, device="cuda", generator=g)
    for gout, exact in ((gi, True), (gr, False)):
        got = _pad_backward(B, C, sizes, gout)
        gn = gout.cpu().numpy()
        seq32, ref64, mag = T.pad_backward(gn, B, sizes, np.float32), T.pad_backward(gn, B, sizes, np.float64), T.pad_backward_abs(gn, B, sizes)
        for j, s in enumerate(sizes):
            a = got[j].cpu().numpy()
            assert np.array_equal(a.view(np.int32), seq32[j].view(np.int32)), (j, s)
            if exact:
                assert np.array_equal(a.astype(np.float64), ref64[j]), (j, s)
            n = -(-L // s)
            assert bool((np.abs(a.astype(np.float64) - ref64[j]) <= (n - 1) * T.U * mag[j]).all()), (j, s)
            if s == L:
                assert same_bits(got[j], gout[j * B:(j + 1) * B])
        for null in ((E // 2,), tuple(range(E))) if E > 1 else ((0,),):
            part = _pad_backward(B, C, sizes, gout, null=null)
            for j in range(E):
                assert (part[j] is None) == (j in null)
                assert part[j] is None or same_bits(part[j], got[j]), (null, j)


# ================================================================================================ 2. sn_chamfer_forward_valid
def _valid_scan(R_, m, n, small, large, qv, q_group, form):
    from samplenet_amd._lib import lib

    wsb = int(lib.sn_pairscan_workspace_bytes(R_, n, m))
    assert wsb > 0 and wsb % 8 == 0  # (every case of the table is spread over several workgroups a cloud when it may be)
    ws = None if form == "null" else Guarded((wsb // 4,), dtype=I32)
    out = dict(ds=Guarded((R_, m)), is_=Guarded((R_, m), dtype=I32), dl=Guarded((R_, n)), il=Guarded((R_, n), dtype=I32))
    call("sn_chamfer_forward_valid", R_, m, small, n, large, qv, q_group, out["ds"], out["is_"], out["dl"], out["il"], ws,
         {"ws": wsb, "null": 0, "short": wsb - 1}[form], stream())
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in out.values()) and (ws is None or ws.guards_intact()), form
    out["dl"].check("dist_large"), out["il"].check("idx_large")
    return out


@pytest.mark.parametrize("case", T.VALID_CASES, ids=lambda c: "R%d-group%d-m%d-n%d" % (c[0], c[1], c[3], c[4]))
def test_chamfer_forward_valid(case):
    """Only the first q_valid[b / q_group] points of the padded cloud are scanned: for every cloud the valid queries' dist / idx and the
    large cloud's dist / idx equal sn_chamfer_forward on the UNPADDED pair and a float32 numpy restatement of the header's expression
    (distances bit for bit, first minimum), idx_large never names a copy, the copies' words of dist_small / idx_small still hold the
    poison they were filled with, and no guard word changes -- with the reported workspace, with none, and with one a byte short (the
    one-workgroup-per-cloud fallback): identical bits.  With 1, 2, 3, 5 valid queries most workgroups of a cloud scan nothing and still
    owe colmin_finalize_kernel their (empty) partials."""
    R_, q_group, q_valid, m, n = case
    assert len(q_valid) == -(-R_ // q_group) and max(q_valid) <= m <= n
    x1, large = T.task_clouds(R_ * 31 + n, R_, m, n)
    valid = [q_valid[b // q_group] for b in range(R_)]
    small = np.stack([x1[b][np.arange(m) % valid[b]] for b in range(R_)])
    sm, lg, qv = dev(small), dev(large), dev(np.asarray(q_valid, dtype=np.int32))
    runs = {form: _valid_scan(R_, m, n, sm, lg, qv, q_group, form) for form in ("ws", "null", "short")}
    for form in ("null", "short"):
        for k in runs["ws"]:
            assert torch.equal(runs[form][k].words(), runs["ws"][k].words()), (form, k)
    got = {k: b.view().cpu().numpy() for k, b in runs["ws"].items()}
    words = {k: runs["ws"][k].words().view(R_, m).cpu().numpy() for k in ("ds", "is_")}
    for b, v in enumerate(valid):
        # the library's own scan of the unpadded pair
        d1, i1, d2, i2 = Guarded((1, v)), Guarded((1, v), dtype=I32), Guarded((1, n)), Guarded((1, n), dtype=I32)
        call("sn_chamfer_forward", 1, v, sm[b, :v].contiguous(), n, lg[b].contiguous(), d1, i1, d2, i2, stream())
        torch.cuda.synchronize()
        lib_ref = [x.check("unpadded").cpu().numpy()[0] for x in (d1, i1, d2, i2)]
        np_ref = T.chamfer_np32(small[b, :v], large[b])
        for ref, what in ((lib_ref, "sn_chamfer_forward"), (np_ref, "numpy")):
            assert np.array_equal(got["ds"][b, :v].view(np.int32), ref[0].view(np.int32)), (b, v, what)
            assert np.array_equal(got["is_"][b, :v], ref[1]), (b, v, what)
            assert np.array_equal(got["dl"][b].view(np.int32), ref[2].view(np.int32)), (b, v, what)
            assert np.array_equal(got["il"][b], ref[3]), (b, v, what)
        assert int(got["il"][b].max()) < v and int(got["il"][b].min()) >= 0
        assert bool((words["ds"][b, v:] == POISON).all()) and bool((words["is_"][b, v:] == POISON).all()), (b, v)
        assert not bool((words["ds"][b, :v] == POISON).any()) and not bool((words["is_"][b, :v] == POISON).any()), (b, v)


# ================================================================================================ 3. the grouped Chamfer-mean loss
LOSS_CASES = [(nev, group, n1, n2) for (n1, n2) in T.LOSS_PAIRS for (nev, group) in T.LOSS_GROUPS] + [T.LOSS_WIDE]


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "nev%d-group%d-n%d-%d" % c)
def test_chamfer_mean_loss_grouped(case):
    """dist / idx of sn_chamfer_forward on the padded batch, the copies' dist1 then set to NaN and their idx1 to INT_MAX (nothing may
    read them).  Every loss and every gradient row equals the evaluation's own sn_chamfer_mean_loss_forward / _backward on the UNPADDED
    clouds bit for bit; the copies' gradient rows are exactly 0; either gradient may be NULL without the other changing; everything is
    written and no guard word changes.  Against fp64 mean(d1[:, :nv]) + mean(d2) on the same float32 points and its autograd gradient:
      loss     : |err| <= loss_bound_units(nv, n2, group) 2^-24 (|mean d1| + |mean d2|)   [5 roundings a distance + the additions a term
                 passes: strided partial, 8-level tree, `group` clouds + quotient + final sum] and <= 2e-6 |loss|,
      gradients: per element |err| <= (4 + hits + 1) 2^-24 sum|terms|   [4 roundings a term, `hits` = the sources that chose the target
                 = the additions it passes, 1 for second order] and, per evaluation, max|err| <= 1e-6 max|gradient|
    -- the 2e-6 / 1e-6 are the bars tests/test_gpu_mlp.py holds the ungrouped loss to."""
    nev, group, n1, n2 = case
    Rr = nev * group
    nvalid, gl = T.nvalid_of(nev, n1), T.grad_loss_of(nev)
    assert nev == 1 or (1 in nvalid and n1 in nvalid and 0.0 in gl and min(gl) < 0)
    b1, x2n = T.task_clouds(n1 * 7 + n2 + nev, Rr, n1, n2)
    x1n = T.pad_rows(b1, group, nvalid)
    x1, x2, gld = dev(x1n), dev(x2n), dev(np.asarray(gl, dtype=np.float32))
    dist1, idx1, dist2, idx2 = Guarded((Rr, n1)), Guarded((Rr, n1), dtype=I32), Guarded((Rr, n2)), Guarded((Rr, n2), dtype=I32)
    call("sn_chamfer_forward", Rr, n1, x1, n2, x2, dist1, idx1, dist2, idx2, stream())
    torch.cuda.synchronize()
    for buf in (dist1, idx1, dist2, idx2):
        buf.check("scan of the padded batch")
    for e, nv in enumerate(nvalid):  # the copies' products: unwritten by the valid scan, read by nobody
        dist1.view()[e * group:(e + 1) * group, nv:] = float("nan")
        idx1.view()[e * group:(e + 1) * group, nv:] = POISON
        assert int(idx2.view()[e * group:(e + 1) * group].max()) < nv  # (a copy never wins a minimum: the lowest index does)
    nvh = ints(nvalid)
    partial, loss = Guarded((2 * Rr,)), Guarded((nev,))
    call("sn_chamfer_mean_loss_forward_grouped", Rr, n1, n2, group, nev, nvh, dist1, dist2, partial, loss, stream())
    g1, g2, g1only, g2only = Guarded((Rr, n1, 3)), Guarded((Rr, n2, 3)), Guarded((Rr, n1, 3)), Guarded((Rr, n2, 3))
    for a, b in ((g1, g2), (g1only, None), (None, g2only)):
        call("sn_chamfer_mean_loss_backward_grouped", Rr, n1, x1, n2, x2, group, nev, nvh, idx1, idx2, gld, a, b, stream())
    torch.cuda.synchronize()
    partial.check("partial")
    losses = loss.check("loss").cpu().numpy()
    G1, G2 = g1.check("grad_xyz1"), g2.check("grad_xyz2")
    assert same_bits(g1only.check("grad_xyz1 alone"), G1) and same_bits(g2only.check("grad_xyz2 alone"), G2)
    assert bool(torch.isfinite(G1).all()) and bool(torch.isfinite(G2).all()) and bool(np.isfinite(losses).all())
    for e, nv in enumerate(nvalid):
        rows = slice(e * group, (e + 1) * group)
        xv, xe = x1[rows, :nv].contiguous(), x2[rows].contiguous()
        # ---- the evaluation's own ungrouped calls on the unpadded clouds
        d1, i1, d2, i2 = Guarded((group, nv)), Guarded((group, nv), dtype=I32), Guarded((group, n2)), Guarded((group, n2), dtype=I32)
        call("sn_chamfer_forward", group, nv, xv, n2, xe, d1, i1, d2, i2, stream())
        sp, am, sl = Guarded((3 * group,)), Guarded((group,), dtype=I32), Guarded((1,))
        call("sn_chamfer_mean_loss_forward", group, nv, n2, d1, d2, sp, am, sl, stream())
        s1, s2 = Guarded((group, nv, 3)), Guarded((group, n2, 3))
        call("sn_chamfer_mean_loss_backward", group, nv, xv, n2, xe, i1, i2, gld[e:e + 1], s1, s2, stream())
        torch.cuda.synchronize()
        assert same_bits(d1.check(), dist1.view()[rows, :nv]) and torch.equal(i1.check(), idx1.view()[rows, :nv]), e
        assert same_bits(d2.check(), dist2.view()[rows]) and torch.equal(i2.check(), idx2.view()[rows]), e
        assert same_bits(sl.check("loss")[0], loss.view()[e]), (e, nv, float(sl.view()[0]), float(losses[e]))
        assert same_bits(s1.check("grad_xyz1"), G1[rows, :nv]), (e, nv)
        assert same_bits(s2.check("grad_xyz2"), G2[rows]), (e, nv)
        assert bool((G1[rows, nv:] == 0).all()), (e, nv)  # the copies: exactly zero
        # ---- fp64 on the same float32 points, the scan's own indices
        i1n, i2n = i1.numpy(), i2.numpy()
        ref_loss, ra, rb = R.simplification_loss(x1n[rows, :nv], x2n[rows], i1n, i2n, 1.0, with_max=False, grad_loss=gl[e])
        a64, c64 = x1n[rows, :nv].astype(np.float64), x2n[rows].astype(np.float64)
        ar = np.arange(group)[:, None]
        m1, m2 = ((a64 - c64[ar, i1n]) ** 2).sum(-1).mean(), ((c64 - a64[ar, i2n]) ** 2).sum(-1).mean()
        assert abs(ref_loss - (m1 + m2)) <= 1e-12 * (m1 + m2) + 1e-300
        err = abs(float(losses[e]) - ref_loss)
        assert err <= T.loss_bound_units(nv, n2, group) * T.U * (m1 + m2), (e, nv, err, m1 + m2)
        assert err <= 2e-6 * abs(ref_loss), (e, nv, err, ref_loss)
        c1, c2 = 1.0 / (group * nv), 1.0 / (group * n2)
        for got, ref, (gr, hits, mag) in ((G1[rows, :nv], ra, T.grad_terms(a64, c64, i1n, i2n, c1, c2, gl[e])),
                                          (G2[rows], rb, T.grad_terms(c64, a64, i2n, i1n, c2, c1, gl[e]))):
            assert np.abs(gr - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)  # (the terms restate the autograd gradient)
            d = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert bool((d <= T.grad_bound_units(hits)[..., None] * T.U * mag).all()), (e, nv, float((d / np.maximum(mag, 1e-300)).max()))
            assert d.max() <= 1e-6 * np.abs(ref).max(), (e, nv, d.max(), np.abs(ref).max())
            if nv > 24 and n2 > 24 and n1 > 24:
                assert hits.max() >= min(nv, 8)  # the cluster: a ballot with many bits set


@pytest.mark.parametrize("n1,n2,route", [(77, 130, "valid-scan"), (300, 64, "fallback")])
def test_chamfer_mean_loss_grouped_wrapper(n1, n2, route):
    """ops.chamfer_mean_loss_grouped on its valid-scan route (n1 <= n2: a _QVALID entry is made) and on the chamfer_forward_impl
    fallback (n1 > n2): losses and both gradients equal the per-evaluation ops.chamfer_mean_loss under torch.equal."""
    from samplenet_amd import ops

    group, nvalid = 3, [1, 40, n1]
    w = [0.7, 0.0, -1.1]
    b1, x2n = T.task_clouds(n1 + n2, group * len(nvalid), n1, n2)
    x1 = dev(T.pad_rows(b1, group, nvalid)).requires_grad_(True)
    x2 = dev(x2n).requires_grad_(True)
    key = (n1, n2, tuple(nvalid), x1.device)
    assert key not in ops._QVALID
    losses = ops.chamfer_mean_loss_grouped(x1, x2, group, nvalid)
    assert (key in ops._QVALID) == (route == "valid-scan")
    ga, gb = torch.autograd.grad(sum(wi * l for wi, l in zip(w, losses.unbind(0))), [x1, x2])
    for e, nv in enumerate(nvalid):
        rows = slice(e * group, (e + 1) * group)
        a = x1.detach()[rows, :nv].contiguous().requires_grad_(True)
        c = x2.detach()[rows].contiguous().requires_grad_(True)
        one = ops.chamfer_mean_loss(a, c)
        assert torch.equal(one, losses[e]), (e, float(one), float(losses[e]))
        ra, rc = torch.autograd.grad(w[e] * one, [a, c])
        assert torch.equal(ga[rows, :nv], ra) and torch.equal(gb[rows], rc), e
        assert bool((ga[rows, nv:] == 0).all())


# ================================================================================================ 4. head + rotation
_HEAD_SUBSETS = [s for k in range(5) for s in itertools.combinations("otqn", k)]  # grad_out, grad_twist, grad_quat, grad_qnorm


def _head_inputs(Rr, N, nv, zero_row=None):
    rng = np.random.default_rng(Rr * 1009 + N)
    y = rng.standard_normal((Rr, 7)).astype(np.float32)
    if zero_row is not None:
        y[zero_row, :4] = 0.0
    v = (rng.random((nv, N, 3), dtype=np.float32) - 0.5)
    up = dict(o=rng.standard_normal((Rr, N, 3)).astype(np.float32), t=rng.standard_normal((Rr, 7)).astype(np.float32),
              q=rng.standard_normal((Rr, 4)).astype(np.float32))
    return y, v, up


def _check_head_fp64(yn, vn, up, gn, fw, gy_of, subsets):
    """One evaluation (B rows, its own template clouds vn (B, N, 3)) against cabi_ref's fp64 head and rotation, under the bars of
    test_pcrnet_head_and_qrot_optional_pointers: twist / quat rtol 1e-5 atol 1e-6, the regulariser rtol 1e-5, the rotated cloud rtol
    1e-5 atol 1e-5, grad_y rtol 1e-5 atol 1e-5 max(1, max|ref|) -- row by row, so that the row of the clamped quaternion (gradient
    1e12 x upstream) does not excuse the others.  Where grad_out comes in, the quaternion's gradient is a fixed-order fp32 sum over N
    points: its bound quat_sum_units(N) 2^-24 sum|terms| reaches grad_y through (g - q (q . g)) / max(|p|, 1e-12), whose rows sum to at
    most 3 / max(|p|, 1e-12) in magnitude, and is added to the bar."""
    twist, quat, qnorm, out = fw
    rt, rq, rn, _ = R.pcrnet_head(yn)
    np.testing.assert_allclose(twist, rt, **PLAIN)
    np.testing.assert_allclose(quat, rq, **PLAIN)
    assert np.isfinite(twist).all() and np.isfinite(out).all()
    if qnorm is not None:
        np.testing.assert_allclose(qnorm, rn, rtol=1e-5)
    np.testing.assert_allclose(out, R.qrot(quat, vn), rtol=1e-5, atol=1e-5)
    N = vn.shape[1]
    terms = T.qrot_quat_terms(quat, vn, up["o"])
    rgq, mag = terms.sum(1), np.abs(terms).sum(1)
    nrm = np.maximum(np.sqrt((yn[:, :4].astype(np.float64) ** 2).sum(1)), 1e-12)
    for sub in subsets:
        gq = (up["q"].astype(np.float64) if "q" in sub else 0.0) + (rgq if "o" in sub else 0.0)
        ref = R.pcrnet_head(yn, up["t"] if "t" in sub else None, gq if ("q" in sub or "o" in sub) else None, gn if "n" in sub else None)[3]
        got = gy_of(sub).astype(np.float64)
        assert np.isfinite(got).all(), sub
        tol = 1e-5 * np.abs(ref) + 1e-5 * np.maximum(1.0, np.abs(ref).max(1, keepdims=True))
        if "o" in sub:
            tol = tol + (3.0 / nrm * T.quat_sum_units(N) * T.U * mag.max(1))[:, None]
        assert bool((np.abs(got - ref) <= tol).all()), (sub, float((np.abs(got - ref) / tol).max()))


@pytest.mark.parametrize("case", T.HEAD_CASES, ids=lambda c: "R%d-N%d-group%d" % c)
def test_head_rot_grouped(case):
    """Rows [e group, (e + 1) group) are evaluation e, row b rotates v[b % group], one regulariser and one grad_qnorm per evaluation:
    twist, quat, out, qnorm and grad_y equal the ungrouped sn_pcrnet_head_rot_* run evaluation by evaluation bit for bit -- for every
    subset of {grad_out, grad_twist, grad_quat, grad_qnorm} left NULL, and with qnorm NULL -- and meet the fp64 references; all outputs
    between guard words.  One row of the (6, 7, 2) case has y[:, :4] = 0: F.normalize's eps = 1e-12, finite everywhere."""
    Rr, N, group = case
    E = Rr // group
    yn, vn, up = _head_inputs(Rr, N, group, zero_row=3 if case == (6, 7, 2) else None)
    gnn = np.asarray([0.3, -1.7, 0.0, 2.5][:E] if E <= 4 else np.linspace(-1, 1, E), dtype=np.float32)
    y, v, gn = dev(yn), dev(vn), dev(gnn)
    upd = {k: dev(a) for k, a in up.items()}
    tw, qu, qn, out = Guarded((Rr, 7)), Guarded((Rr, 4)), Guarded((E,)), Guarded((Rr, N, 3))
    call("sn_pcrnet_head_rot_forward_grouped", Rr, N, group, y, v, tw, qu, qn, out, stream())
    tw2, qu2, out2 = Guarded((Rr, 7)), Guarded((Rr, 4)), Guarded((Rr, N, 3))
    call("sn_pcrnet_head_rot_forward_grouped", Rr, N, group, y, v, tw2, qu2, None, out2, stream())
    torch.cuda.synchronize()
    fw = [b.check(w) for b, w in ((tw, "twist"), (qu, "quat"), (qn, "qnorm"), (out, "out"))]
    assert same_bits(tw2.check("twist"), tw) and same_bits(qu2.check("quat"), qu) and same_bits(out2.check("out"), out)
    gy = {}
    for sub in _HEAD_SUBSETS:
        gb = Guarded((Rr, 7))
        call("sn_pcrnet_head_rot_backward_grouped", Rr, N, group, y, qu, v, upd["o"] if "o" in sub else None, upd["t"] if "t" in sub else None,
             upd["q"] if "q" in sub else None, gn if "n" in sub else None, gb, stream())
        torch.cuda.synchronize()
        gy[sub] = gb.check("grad_y %s" % (sub,))
    for e in range(E):
        rows = slice(e * group, (e + 1) * group)
        ye = y[rows].contiguous()
        t1, q1, n1_, o1 = Guarded((group, 7)), Guarded((group, 4)), Guarded((1,)), Guarded((group, N, 3))
        call("sn_pcrnet_head_rot_forward", group, N, ye, v, t1, q1, n1_, o1, stream())
        torch.cuda.synchronize()
        assert same_bits(t1.check("twist"), fw[0][rows]) and same_bits(q1.check("quat"), fw[1][rows]), e
        assert same_bits(n1_.check("qnorm")[0], fw[2][e]) and same_bits(o1.check("out"), fw[3][rows]), e
        for sub in _HEAD_SUBSETS:
            g1 = Guarded((group, 7))
            sl = lambda k: upd[k][rows].contiguous() if k in sub else None
            call("sn_pcrnet_head_rot_backward", group, N, ye, q1, v, sl("o"), sl("t"), sl("q"), gn[e:e + 1] if "n" in sub else None, None, g1,
                 stream())
            torch.cuda.synchronize()
            assert same_bits(g1.check("grad_y"), gy[sub][rows]), (e, sub)
        fp64_subsets = _HEAD_SUBSETS if N <= 300 else [(), ("o",), ("o", "t", "q", "n"), ("t", "n")]  # (the per-point terms of 16500 points: four will do)
        _check_head_fp64(yn[rows], vn, {k: a[rows] for k, a in up.items()}, float(gnn[e]),
                         [a[rows].cpu().numpy() for a in (fw[0], fw[1])] + [float(fw[2][e])] + [fw[3][rows].cpu().numpy()],
                         lambda sub: gy[sub][rows].cpu().numpy(), fp64_subsets)
    if case == (6, 7, 2):
        assert bool((fw[0][3, :4] == 0).all()) and same_bits(fw[3][3], v[3 % group])  # q = 0 / 1e-12 = 0: the cloud comes back as it is


def test_head_rot_ungrouped_strided_loop():
    """The ungrouped pair at (2, 16500): ceil(N / 256) = 65 workgroups wanted, 64 launched -- the last 116 points are a second trip of
    the strided loop -- against fp64, grad_v included, with and without it (grad_y keeps its bits), qnorm NULL or not."""
    B, N = 2, 16500
    yn, vn, up = _head_inputs(B, N, B)
    y, v = dev(yn), dev(vn)
    upd = {k: dev(a) for k, a in up.items()}
    gn = dev(np.asarray([0.3], dtype=np.float32))
    tw, qu, qn, out = Guarded((B, 7)), Guarded((B, 4)), Guarded((1,)), Guarded((B, N, 3))
    call("sn_pcrnet_head_rot_forward", B, N, y, v, tw, qu, qn, out, stream())
    tw2, qu2, out2 = Guarded((B, 7)), Guarded((B, 4)), Guarded((B, N, 3))
    call("sn_pcrnet_head_rot_forward", B, N, y, v, tw2, qu2, None, out2, stream())
    gv, gy, gy2 = Guarded((B, N, 3)), Guarded((B, 7)), Guarded((B, 7))
    call("sn_pcrnet_head_rot_backward", B, N, y, qu, v, upd["o"], upd["t"], upd["q"], gn, gv, gy, stream())
    call("sn_pcrnet_head_rot_backward", B, N, y, qu, v, upd["o"], upd["t"], upd["q"], gn, None, gy2, stream())
    torch.cuda.synchronize()
    fw = [b.check(w).cpu().numpy() for b, w in ((tw, "twist"), (qu, "quat"), (qn, "qnorm"), (out, "out"))]
    assert same_bits(tw2.check("twist"), tw) and same_bits(qu2.check("quat"), qu) and same_bits(out2.check("out"), out)
    assert same_bits(gy2.check("grad_y without grad_v"), gy.check("grad_y"))
    full = ("o", "t", "q", "n")
    _check_head_fp64(yn, vn, up, 0.3, [fw[0], fw[1], float(fw[2][0]), fw[3]], lambda sub: gy.numpy(), [full])
    np.testing.assert_allclose(gv.check("grad_v").cpu().numpy(), R.qrot(fw[1], vn, up["o"])[2], rtol=1e-5, atol=1e-5)


# ================================================================================================ 5. end to end at odd sizes
@pytest.mark.parametrize("prefixes", [(40, 77, 100), (5, 100), (5, 6, 100)], ids=lambda p: "-".join(map(str, p)))
def test_task_term_one_batch_at_odd_sizes(prefixes):
    """pcrnet_chamfer_loss_multi against evaluation-by-evaluation pcrnet_chamfer_loss at B = 3, N = 300: losses, regularisers, twists
    and the gradient to every prefix agree under torch.equal -- in one batch at (40, 77, 100), where PCRNet._one_batch_ok holds
    (3 x 100 <= 2.5 x 217), and by the fallback at (5, 100) and (5, 6, 100), where it does not.  (5, 100) is the case that found the
    few-row defect: 3 clouds of 5 points are 15 rows, which the extractor runs on its few-row kernels -- not the bits the same cloud gets
    inside a padded batch of 600 rows -- so neither _one_batch_ok nor _feat_multi may pad a cloud whose own pass has 64 rows or fewer;
    (5, 6, 100) fails the 2.5 x rule as well (3 x 100 > 2.5 x 111)."""
    from samplenet_amd import task_features as TF

    torch.manual_seed(11)
    pcr = TF.PCRNet(bottleneck_size=1024, input_shape="bnc").cuda().eval()
    for p in pcr.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device="cuda").manual_seed(5)
    B, N = 3, 300
    template = torch.rand(B, N, 3, device="cuda", generator=g) - 0.5
    cloud = torch.rand(B, max(prefixes), 3, device="cuda", generator=g) - 0.5
    qs = [cloud[:, :s, :].contiguous().requires_grad_(True) for s in prefixes]
    assert pcr._one_batch_ok(template, qs) == (prefixes == (40, 77, 100))
    many = TF.pcrnet_chamfer_loss_multi(pcr, template, qs)
    one = [TF.pcrnet_chamfer_loss(pcr, template, q) for q in qs]
    for (la, qa, ta), (lb, qb, tb) in zip(one, many):
        assert torch.equal(la, lb) and torch.equal(qa, qb) and torch.equal(ta, tb)
    wl = [0.3, -1.0, 0.0][:len(prefixes)]
    ga = torch.autograd.grad(sum(w * (l + 0.1 * q) for w, (l, q, _) in zip(wl, one)), qs)
    gb = torch.autograd.grad(sum(w * (l + 0.1 * q) for w, (l, q, _) in zip(wl, many)), qs)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)

"""sn_pose_error_forward / sn_pose_error_backward / sn_chamfer_mean_per_cloud called directly, against the fp64 restatement and the
counted bounds of tests/pose_ref.py.  Inputs and outputs sit in guarded buffers (tests/cabi_ref.py: poisoned words on both sides,
checked after every call).  Every test prints its largest observed error beside the bound (`pytest -s`; recorded in
profiles/pose/errors.txt)."""
import itertools

import numpy as np
import pytest
import torch

import cabi_ref as R
import pose_ref as P

pytestmark = pytest.mark.gpu

TWO_PI32 = np.float32(2 * np.pi)  # = 2 float32(pi): the largest value 2 acosf can return


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def _report(what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if err.size:
        i = np.argmax(err / np.maximum(bound, 1e-300))
        print("POSE_ERR %-44s observed %.3e  bound %.3e  ratio %.3f" % (what, err.flat[i], bound.flat[i], err.flat[i] / max(bound.flat[i], 1e-300)))


def _within(what, got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    _report(what, err, bound)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d outside the bound, worst %.3e against %.3e" % (what, bad.sum(), err[bad].max(), np.broadcast_to(bound, err.shape)[bad].min())


def forward(est, gt, want=(True, True, True, True)):
    """One guarded call -> [rot, nrm, trn, means] as numpy (None where not asked for)."""
    lib, check = _lib()
    B = est.shape[0]
    ge, gg = R.Guarded((B, 7), fill=est), R.Guarded((B, 7), fill=gt)
    outs = [R.Guarded((n,)) if w else None for n, w in zip((B, B, B, 3), want)]
    check(lib.sn_pose_error_forward(B, ge.ptr(), gg.ptr(), *[R.arg(o) for o in outs], None), "sn_pose_error_forward")
    torch.cuda.synchronize()
    assert ge.guards_intact() and gg.guards_intact()
    assert np.array_equal(ge.numpy().view(np.int32), est.view(np.int32)) and np.array_equal(gg.numpy().view(np.int32), gt.view(np.int32))
    return [None if o is None else o.check("forward output").cpu().numpy().copy() for o in outs]


def backward(est, gt, gm, gn, gtr):
    lib, check = _lib()
    B = est.shape[0]
    ge, gg = R.Guarded((B, 7), fill=est), R.Guarded((B, 7), fill=gt)
    ins = [None if a is None else R.Guarded(a.shape, fill=a) for a in (gm, gn, gtr)]
    out = R.Guarded((B, 7))
    check(lib.sn_pose_error_backward(B, ge.ptr(), gg.ptr(), *[R.arg(i) for i in ins], out.ptr(), None), "sn_pose_error_backward")
    torch.cuda.synchronize()
    assert all(i is None or i.guards_intact() for i in ins) and ge.guards_intact() and gg.guards_intact()
    return out.check("g_est").cpu().numpy().copy()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


CASES = [(B, r) for B in P.BATCHES for r in P.RECIPES]


@pytest.mark.parametrize("B,recipe", CASES, ids=["%d-%s" % c for c in CASES])
def test_forward_against_fp64(B, recipe):
    est, gt = P.make_case(recipe, B)
    T = P.pose_terms(est, gt)
    rot, nrm, trn, means = forward(est, gt)
    tag = "%s B=%d " % (recipe, B)
    bn, bt = P.bound_norm_err(T["norm_err"]), P.bound_trans_err(T["trans_err"])
    _within(tag + "norm_err", nrm, T["norm_err"], bn)
    _within(tag + "trans_err", trn, T["trans_err"], bt)
    assert np.isfinite(rot).all() and (rot >= 0).all() and (rot <= TWO_PI32).all()
    ok = P.rot_admitted(T)
    if P.RECIPES[recipe]:
        assert 1.0 - ok.mean() <= P.ROT_EXCLUDED_CAP
        br = P.bound_rot_err({k: v[ok] for k, v in T.items()})
        _within(tag + "rot_err", rot[ok], T["rot_err"][ok], br)
        if ok.all():
            _within(tag + "mean rot_err", means[0], T["rot_err"].mean(), P.bound_mean(B, T["rot_err"], br))
    _within(tag + "mean norm_err", means[1], T["norm_err"].mean(), P.bound_mean(B, T["norm_err"], bn))
    _within(tag + "mean trans_err", means[2], T["trans_err"].mean(), P.bound_mean(B, T["trans_err"], bt))
    # the means are the kernel's own per-cloud values added in the documented order, bit for bit
    for k, v in enumerate((rot, nrm, trn)):
        assert _bits(means[k]) == _bits(P.means_in_kernel_order(v)), (k, means[k], P.means_in_kernel_order(v))
    # a second run is bit-identical
    for a, b in zip((rot, nrm, trn, means), forward(est, gt)):
        assert np.array_equal(_bits(a), _bits(b))
    if recipe == "same":
        assert (rot < 1e-2).all()  # (the reference returns NaN for a fifth of these rows)
        assert not trn.any()
    if recipe == "negated":
        same_rot = forward(-est * np.array([1, 1, 1, 1, -1, -1, -1], dtype=np.float32), gt)[0]
        assert np.array_equal(_bits(rot), _bits(same_rot))  # d -> -d: the same 2 d^2 - 1
    if recipe == "antipodal":
        assert (rot > TWO_PI32 - 1e-2).all()


def test_null_outputs_are_honoured():
    est, gt = P.make_case("unit", 257)
    full = forward(est, gt)
    for want in itertools.product((True, False), repeat=4):
        got = forward(est, gt, want)
        for w, g, f in zip(want, got, full):
            assert (g is None) == (not w)
            if w:
                assert np.array_equal(_bits(g), _bits(f)), want


def test_zero_batch_is_a_no_op():
    lib, check = _lib()
    outs = [R.Guarded((n,)) for n in (4, 4, 4, 3, 7)]
    check(lib.sn_pose_error_forward(0, None, None, *[o.ptr() for o in outs[:4]], None), "forward")
    check(lib.sn_pose_error_backward(0, None, None, None, None, None, outs[4].ptr(), None), "backward")
    check(lib.sn_chamfer_mean_per_cloud(0, 5, 5, None, None, outs[0].ptr(), None), "per cloud")
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


@pytest.mark.parametrize("where", ["quat_est", "quat_gt", "trans"])
def test_nan_stays_in_its_row_and_poisons_the_means(where):
    est, gt = P.make_case("unit", 65)
    clean = forward(est, gt)
    est, gt = est.copy(), gt.copy()
    row = 17
    if where == "quat_est":
        est[row, 2] = np.nan
    elif where == "quat_gt":
        gt[row, 0] = np.nan
    else:
        est[row, 5] = np.nan
    rot, nrm, trn, means = forward(est, gt)
    hit = (trn,) if where == "trans" else (rot, nrm)
    for k, (v, c) in enumerate(zip((rot, nrm, trn), clean[:3])):
        others = np.arange(65) != row
        assert np.array_equal(_bits(v[others]), _bits(c[others]))
        if any(v is h for h in hit):
            assert np.isnan(v[row]) and np.isnan(means[k])
        else:
            assert _bits(v[row]) == _bits(c[row]) and _bits(means[k]) == _bits(clean[3][k])
    g = backward(est, gt, None, np.ones(65, dtype=np.float32), np.ones(65, dtype=np.float32))
    gc = backward(*P.make_case("unit", 65), None, np.ones(65, dtype=np.float32), np.ones(65, dtype=np.float32))
    assert np.array_equal(_bits(g[others]), _bits(gc[others]))
    assert np.isnan(g[row, 4:] if where == "trans" else g[row, :4]).any()


@pytest.mark.parametrize("B,recipe", CASES, ids=["%d-%s" % c for c in CASES])
def test_backward_against_fp64(B, recipe):
    est, gt = P.make_case(recipe, B)
    gm, gn, gtr = P.upstream_case(B)
    tag = "%s B=%d " % (recipe, B)
    for use in itertools.product((True, False), repeat=3):
        a = [v if u else None for v, u in zip((gm, gn, gtr), use)]
        got = backward(est, gt, *a)
        ref, bound = P.pose_backward(est, gt, *a), P.bound_backward(est, gt, *a)
        assert np.isfinite(got).all()  # (g_means[0] is a NaN: it was not read)
        if use == (True, True, True):
            _within(tag + "g_est quaternion", got[:, :4], ref[:, :4], bound[:, :4])
            _within(tag + "g_est translation", got[:, 4:], ref[:, 4:], bound[:, 4:])
            assert np.array_equal(_bits(got), _bits(backward(est, gt, *a)))  # two runs
        else:
            assert (np.abs(got - ref) <= bound).all(), use
        if not (use[0] or use[1]):
            assert not got[:, :4].any()
        if not (use[0] or use[2]):
            assert not got[:, 4:].any()
        if recipe == "same":
            assert not got[:, 4:].any()  # sign(0) = 0: exactly no translation gradient (the reference: NaN)
        if recipe == "zero":
            assert not got[:, :4].any()
        if recipe == "unit":  # every 5th row shares its y translation: that component alone is exactly 0
            assert not got[::5, 5].any()


def test_ops_pose_errors_agree_with_autograd_of_the_fp64_restatement():
    """ops.pose_errors (forward values, non-differentiable rot_err, gradients of norm_err / trans_err to est, none to gt) against
    torch autograd through the fp64 torch restatement of the same formulas -- no finite differences on the fp32 kernel."""
    from samplenet_amd import QuaternionTransform, ops

    B = 65
    for recipe in ("unit", "nonunit"):
        est_np, gt_np = P.make_case(recipe, B)
        _, gn, gtr = P.upstream_case(B)
        est = torch.from_numpy(est_np).cuda().requires_grad_(True)
        gt = torch.from_numpy(gt_np).cuda().requires_grad_(True)
        rot, nrm, trn = ops.pose_errors(est, gt)
        assert not rot.requires_grad and nrm.requires_grad and trn.requires_grad
        wn, wt = torch.from_numpy(gn).cuda(), torch.from_numpy(gtr).cuda()
        ((wn * nrm).sum() + (wt * trn).sum()).backward()
        assert gt.grad is None
        e64 = torch.from_numpy(est_np).double().requires_grad_(True)
        _, n64, t64 = P.pose_terms_torch(e64, torch.from_numpy(gt_np))
        (g64,) = torch.autograd.grad((wn.cpu().double() * n64).sum() + (wt.cpu().double() * t64).sum(), e64)
        _within("ops.pose_errors %s gradient" % recipe, est.grad.cpu().numpy(), g64.numpy(), P.bound_backward(est_np, gt_np, None, gn, gtr))
        # compute_errors: the batch means as scalars, gradient through means[1] and means[2] only
        est.grad = None
        r, n, t = QuaternionTransform(est).compute_errors(QuaternionTransform(gt.detach()))
        assert r.dim() == n.dim() == t.dim() == 0 and not r.requires_grad
        (n + 2 * t).backward()
        gm = np.array([np.nan, 1.0, 2.0], dtype=np.float32)
        _within("compute_errors %s gradient" % recipe, est.grad.cpu().numpy(), P.pose_backward(est_np, gt_np, gm), P.bound_backward(est_np, gt_np, gm))
        full = forward(est_np, gt_np)
        assert np.array_equal(_bits([r.item(), n.item(), t.item()]), _bits(full[3]))
        assert np.array_equal(_bits(nrm.detach().cpu().numpy()), _bits(full[1]))


CH_CASES = [(B, n1, n2) for B in P.CHAMFER_BATCHES for n1, n2 in P.CHAMFER_SIZES]


@pytest.mark.parametrize("B,n1,n2", CH_CASES)
def test_chamfer_mean_per_cloud(B, n1, n2):
    lib, check = _lib()
    rng = np.random.default_rng([B, n1, n2])
    d1 = (rng.random((B, n1), dtype=np.float32) ** 2 * 3).astype(np.float32)
    d2 = (rng.random((B, n2), dtype=np.float32) ** 2 * 3).astype(np.float32)
    d1[:, 0] = 0.0
    g1, g2, out = R.Guarded((B, n1), fill=d1), R.Guarded((B, n2), fill=d2), R.Guarded((B,))
    check(lib.sn_chamfer_mean_per_cloud(B, n1, n2, g1.ptr(), g2.ptr(), out.ptr(), None), "sn_chamfer_mean_per_cloud")
    torch.cuda.synchronize()
    assert g1.guards_intact() and g2.guards_intact()
    got = out.check("out").cpu().numpy().copy()
    m1, m2 = P.chamfer_mean(d1, d2)
    bound = P.bound_chamfer_mean(n1, n2, m1, m2)
    _within("chamfer_mean_per_cloud B=%d %dx%d" % (B, n1, n2), got, m1 + m2, bound)
    out2 = R.Guarded((B,))
    check(lib.sn_chamfer_mean_per_cloud(B, n1, n2, g1.ptr(), g2.ptr(), out2.ptr(), None), "sn_chamfer_mean_per_cloud")
    assert np.array_equal(_bits(got), _bits(out2.check("out").cpu().numpy()))
    # the batch mean of the per-cloud values against the loss entry's scalar: both within the fixed-order bound of the exact
    # value (the loss entry adds the B clouds' sums one after the other: B more roundings)
    part, am, loss = R.Guarded((3 * B,)), R.Guarded((B,), dtype=torch.int32), R.Guarded((1,))
    check(lib.sn_chamfer_mean_loss_forward(B, n1, n2, g1.ptr(), g2.ptr(), part.ptr(), am.ptr(), loss.ptr(), None), "sn_chamfer_mean_loss_forward")
    exact = (m1 + m2).mean()
    extra = 1.01 * (B + 1) * P.U * exact
    _within("... against sn_chamfer_mean_loss_forward", loss.check("loss").cpu().numpy()[0], exact, bound.mean() + extra)
    assert abs(got.astype(np.float64).mean() - loss.numpy()[0]) <= 2 * bound.mean() + extra


def test_ops_chamfer_mean_per_cloud_matches_the_loss_per_item():
    """ops.chamfer_mean_per_cloud on real clouds: every item equals chamfer_mean_loss of that item alone within the bound."""
    from samplenet_amd import ops

    x1, x2 = R.clouds(3, 3, 77, 130)
    a, b = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    got = ops.chamfer_mean_per_cloud(a, b).cpu().numpy()
    d = ((x1.astype(np.float64)[:, :, None] - x2.astype(np.float64)[:, None]) ** 2).sum(-1)
    m1, m2 = d.min(2).mean(1), d.min(1).mean(1)
    # (each fp32 squared distance ((dx dx + dy dy) + dz dz) of exact inputs: a subtraction, a square and up to two additions on
    #  non-negative terms -- relative 5 U; the minimum of perturbed values moves by no more than their perturbation)
    slack = 1.01 * 5 * P.U * (m1 + m2)
    _within("ops.chamfer_mean_per_cloud", got, m1 + m2, P.bound_chamfer_mean(77, 130, m1, m2) + slack)
    for i in range(3):
        one = ops.chamfer_mean_loss(a[i:i + 1].contiguous(), b[i:i + 1].contiguous()).item()
        assert abs(one - got[i]) <= 2 * P.bound_chamfer_mean(77, 130, m1[i], m2[i])

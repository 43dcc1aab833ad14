"""tests/interp_ref.py, the yardstick of sn_three_nn and of the interpolation on top of it, held to its own row-loop twin and to float64 torch
(cdist, topk, gather) where no tie occurs; the recipes' promises; the counted weight bounds; the shape table against the restated
launch rule; and the host half of the entry's contract: argument errors and no-op cases in a child process that sees no GPU,
RuntimeError on CPU tensors, the prototypes, PointnetFPModule's construction.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import interp_ref as R
from cabi_runner import check_case, run_cases

LOOP_SHAPES = [s for s in R.SHAPES if s[0] * s[1] * s[2] <= 70000]  # the row loop is Python: every row but the three largest clouds (two queries of those)


@pytest.mark.parametrize("recipe", R.RECIPES)
def test_vectorised_restatement_is_the_row_loop(recipe):
    for shape in R.SHAPES:
        u, k = R.make_case(shape, recipe)
        if shape not in LOOP_SHAPES:
            u = u[:, :2]
        a, b = R.three_nn(u, k), R.three_nn_by_loop(u, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        assert a[0].dtype == np.int32 and a[1].dtype == np.float32 and ((a[0] >= 0) & (a[0] < shape[2])).all()


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_restatement_is_float64_torch_where_nothing_ties(shape):
    b, n, m, c2, c1 = shape
    u, k = R.make_case(shape, "rand")
    kf, uf, _ = R.make_feats(shape)
    idx, d2 = R.three_nn(u, k)
    kk = min(3, m)
    d64 = torch.cdist(torch.from_numpy(u).double(), torch.from_numpy(k).double())
    top = torch.topk(d64, kk + 1 if m > kk else kk, dim=2, largest=False)
    # the premise: the float64 distances of the first kk + 1 neighbours are apart by far more than float32 can blur
    gaps = (top.values[:, :, 1:] - top.values[:, :, :-1]).numpy()
    assert kk == 1 or (gaps > 1e-6 * top.values[:, :, 1:].numpy()).all(), "a near-tie in the rand recipe"
    assert np.array_equal(idx[:, :, :kk], top.indices[:, :, :kk].numpy().astype(np.int32))
    assert np.allclose(np.sqrt(d2[:, :, :kk].astype(np.float64)), top.values[:, :, :kk].numpy(), rtol=1e-5, atol=1e-7)
    for rule in R.RULES:
        w = R.weights(d2, rule)
        dist = top.values[:, :, :kk]
        r = 1.0 / (dist + 1e-8) if rule == R.SQRT_EPS else 1.0 / torch.clamp(dist * dist, min=1e-10)
        w64 = torch.zeros(b, n, 3, dtype=torch.float64)
        w64[:, :, :kk] = r / r.sum(-1, keepdim=True)
        assert np.allclose(w, w64.numpy(), rtol=1e-4, atol=1e-7)
        li = torch.from_numpy(idx.astype(np.int64)).view(b, 1, n * 3).expand(b, c2, n * 3)
        g = torch.gather(torch.from_numpy(kf).double(), 2, li).view(b, c2, n, 3)
        ref = torch.cat([(g * w64[:, None]).sum(-1), torch.from_numpy(uf).double()], 1).numpy()
        _, _, out = R.propagate(u, k, uf, kf, rule)
        assert out.shape == (b, c2 + c1, n) and np.allclose(out, ref, rtol=1e-4, atol=1e-5)
        assert np.array_equal(out[:, c2:], uf)


def test_the_recipes_reach_what_they_promise():
    for shape in R.SHAPES:
        b, n, m, _, _ = shape
        for recipe in R.RECIPES:
            u, k = R.make_case(shape, recipe)
            idx, d2 = R.three_nn(u, k)
            full = R.dist2(u, k)
            if recipe == "lattice" and m > 3:
                # rows with another point exactly as far as the third neighbour: they occur at every shape with a choice to make,
                # and are most rows once the known cloud has 64 points (9^3 lattice sites, few distinct distances)
                tied = ((full == d2[:, :, 2:3]).sum(-1) > 1).mean()
                assert tied > (0.5 if m >= 64 else 0.0), (shape, tied)
            if recipe == "dup":
                assert (d2[:, :, 0] == 0).all()
                for rule in R.RULES:
                    w = R.weights(d2, rule)
                    assert np.isfinite(w).all() and (w[:, :, 0] > 0).all()
            if recipe == "same":
                assert (idx == np.arange(3)[None, None, :] * (np.arange(3) < m)).all()
            if recipe == "nan":
                assert not (idx == m // 2).any() or m // 2 == 0       # never selected (index 0 is also the filler)
                assert (np.isfinite(d2[:, :, :min(3, m - 1)])).all() and not np.isnan(d2).any()
                for rule in R.RULES:
                    assert np.isnan(R.weights(d2, rule)).any() == (m == 1)   # NaN only where every candidate is
            if m < 3 and recipe in ("rand", "lattice", "big"):
                assert np.isinf(d2[:, :, m:]).all() and (idx[:, :, m:] == 0).all()
                for rule in R.RULES:
                    assert (R.weights(d2, rule)[:, :, m:] == 0).all()


@pytest.mark.parametrize("rule", R.RULES)
def test_float32_weights_stay_within_the_counted_bound(rule):
    worst = worst_sum = 0.0
    for shape in R.SHAPES:
        for recipe in R.RECIPES:
            u, k = R.make_case(shape, recipe)
            _, d2 = R.three_nn(u, k)
            w, w64 = R.weights(d2, rule), R.weights64(d2, rule)
            ok = ~np.isnan(w64)
            assert np.array_equal(np.isnan(w), ~ok)
            err = np.abs(w[ok].astype(np.float64) - w64[ok])
            assert (err <= R.WEIGHT_BOUND[rule] * w64[ok]).all()
            rows = ok.all(-1)
            s = np.abs(w[rows].astype(np.float64).sum(-1) - 1.0)
            assert (s <= R.WEIGHT_SUM_BOUND).all()
            pos = w64[ok] > 0
            if pos.any():
                worst = max(worst, float((err[pos] / w64[ok][pos]).max() / R.U))
            worst_sum = max(worst_sum, float(s.max() / R.U) if len(s) else 0.0)
    print("rule %d: worst weight error %.2f units of 2^-24 (bound %g), worst |sum - 1| %.2f units (bound 3)"
          % (rule, worst, R.WEIGHT_BOUND[rule] / R.U, worst_sum))


def test_backward_reference_is_the_gradient_of_the_forward():
    shape = (2, 257, 65, 16, 1)
    b, n, m, c2, c1 = shape
    u, k = R.make_case(shape, "lattice")
    kf, uf, g = R.make_feats(shape)
    idx, d2 = R.three_nn(u, k)
    w = R.weights(d2, R.SQRT_EPS)
    f64 = torch.from_numpy(kf).double().requires_grad_(True)
    li = torch.from_numpy(idx.astype(np.int64)).view(b, 1, n * 3).expand(b, c2, n * 3)
    out = (torch.gather(f64, 2, li).view(b, c2, n, 3) * torch.from_numpy(w).double()[:, None]).sum(-1)
    assert np.allclose(out.detach().numpy(), R.interpolate64(kf, idx, w), rtol=0, atol=1e-12)
    (gk,) = torch.autograd.grad(out, [f64], torch.from_numpy(g[:, :c2]).double())
    grad, ab, mult = R.backward64(m, c2, idx, w, g)
    assert np.allclose(gk.numpy(), grad, rtol=0, atol=1e-12) and (ab >= np.abs(grad) - 1e-12).all()
    assert np.array_equal(mult, np.stack([np.bincount(idx[i].ravel(), minlength=m) for i in range(b)])) and mult.sum() == idx.size


def test_the_table_reaches_every_launch_rule_branch():
    S, Q = R.STAGE, R.QUERIES
    assert (S, Q) == (1024, 64)
    assert {R.waves(s[0], s[1]) for s in R.SHAPES} == {4, 8, 16}
    assert [R.waves(1, q) for q in (1, 64 * 511, 64 * 511 + 1, 64 * 1023, 64 * 1023 + 1)] == [16, 16, 8, 8, 4]
    ms, ns = {s[2] for s in R.SHAPES}, {s[1] for s in R.SHAPES}
    assert {1, 2, 3, S + 1, 2 * S + 1} <= ms and {1, Q, Q + 1, 2 * Q + 1} <= ns and any(s[0] > 64 for s in R.SHAPES)


# ------------------------------------------------------------------------------------------------ argument checks, no GPU
BAD = 10001
P_ = "PTR"  # a non-NULL device pointer that is never dereferenced
N_BASE = [1, 8, 4, P_, P_, None, None, P_, None]                                # sn_three_nn


def _with(base, changes):
    out = list(base)
    for k, v in changes.items():
        out[k] = v
    return out


def _cases():
    q = "sn_three_nn"
    out = []
    for pos in (0, 1, 2):
        out.append(("%s-negative-%d" % (q, pos), q, _with(N_BASE, {pos: -1}), BAD, "negative size"))
    for pos in (3, 4, 7):
        out.append(("%s-null-%d" % (q, pos), q, _with(N_BASE, {pos: None}), BAD, "null pointer"))
    out.append((q + "-empty-known", q, _with(N_BASE, {2: 0}), BAD, "m == 0"))
    # the documented no-ops: nothing is dereferenced, nothing launched (every pointer NULL)
    nq = N_BASE[:3] + [None] * 6
    for tag, ch in (("b0", {0: 0}), ("n0", {1: 0}), ("n0-m0", {1: 0, 2: 0})):
        out.append((q + "-noop-" + tag, q, _with(nq, ch), 0, None))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def results():
    return run_cases(CASES)


def test_the_tables_match_the_prototypes():
    from samplenet_amd import _lib

    for name, base in (("sn_three_nn", N_BASE),):
        proto = _lib.PROTOTYPES[name]
        assert len(proto) == len(base), name
        for ty, a in zip(proto, base):
            assert (ty is ctypes.c_void_p) == (a is None or a == P_), name
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_table(results, case):
    check_case(results, case)


def test_cpu_tensors_raise():
    from samplenet_amd import ops
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    u, k, kf, uf = torch.zeros(1, 8, 3), torch.zeros(1, 4, 3), torch.zeros(1, 5, 4), torch.zeros(1, 2, 8)
    idx, w = torch.zeros(1, 8, 3, dtype=torch.int32), torch.zeros(1, 8, 3)
    for call in (lambda: ops.three_nn(u, k), lambda: PU.three_nn(u, k), lambda: ops.three_interpolate(kf, idx, w),
                 lambda: PU.three_interpolate(kf, idx, w), lambda: PM.PointnetFPModule([7, 4])(u, k, uf, kf)):
        with pytest.raises(RuntimeError):
            call()


def test_fp_module_constructs_with_the_layers_asked_for():
    from samplenet_amd import compat

    compat.install()
    from pointnet2.utils.pointnet2_modules import PointnetFPModule
    from pointnet2.utils.pointnet2_utils import three_interpolate, three_nn  # noqa: F401

    fp = PointnetFPModule([7, 16, 4])
    convs = [l for l in fp.mlp.modules() if isinstance(l, torch.nn.Conv2d)]
    assert [(c.in_channels, c.out_channels, c.kernel_size, c.bias is None) for c in convs] == [(7, 16, (1, 1), True), (16, 4, (1, 1), True)]
    assert sum(isinstance(l, torch.nn.BatchNorm2d) for l in fp.mlp.modules()) == 2 and sum(isinstance(l, torch.nn.ReLU) for l in fp.mlp.modules()) == 2
    plain = PointnetFPModule([7, 4], bn=False)
    assert not any(isinstance(l, torch.nn.BatchNorm2d) for l in plain.mlp.modules())
    assert all(c.bias is not None for c in plain.mlp.modules() if isinstance(c, torch.nn.Conv2d))
    # known is None: known_feats (B,C2,1) is expanded over n and concatenated -- plain torch, runs anywhere
    out = plain(torch.zeros(2, 9, 3), None, torch.ones(2, 3, 9), torch.ones(2, 4, 1))
    assert out.shape == (2, 4, 9)

"""tests/ball_ref.py, the yardstick of sn_ball_query / sn_ball_group_*, held to the reference's own CPU twin (query_ball_point_cpu,
classification/grouping/test/query_ball_point.cpp:19-47, as built into oracle/_ref/libgroup_point_ref.so) on every recipe and shape
row; the boundary recipe's premise; and the host half of the three entries' contract: argument errors and no-op cases in a child
process that sees no GPU, RuntimeError on CPU tensors.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ball_ref as R
from cabi_runner import check_case, run_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = os.path.join(ROOT, "oracle", "_ref", "libgroup_point_ref.so")
SENTINEL = -77
SHAPE_IDS = ["x".join(map(str, s[0])) for s in R.SHAPES]


def _twin(P, Q, radius, nsample):
    fn = ctypes.CDLL(TWIN)._Z20query_ball_point_cpuiiifiPKfS0_Pi
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 3
    fn.restype = None
    b, n, _ = P.shape
    m = Q.shape[1]
    P, Q = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(Q, np.float32)
    idx = np.full((b, m, nsample), SENTINEL, np.int32)
    fn(b, n, m, float(radius), nsample, P.ctypes.data, Q.ctypes.data, idx.ctypes.data)
    return idx


@pytest.mark.skipif(not os.path.exists(TWIN), reason="oracle/_ref is built only where the reference tree is present")
@pytest.mark.parametrize("recipe", R.RECIPES, ids=R.RECIPE_IDS)
@pytest.mark.parametrize("row", R.SHAPES, ids=SHAPE_IDS)
def test_restatement_is_the_reference_twin(row, recipe):
    shape = row[0]
    P, Q, radius = R.make_case(shape, recipe)
    idx, cnt = R.ball_query(P, Q, radius, shape[3], R.SQRT)
    ref = _twin(P, Q, radius, shape[3])
    full = cnt > 0
    assert np.array_equal(idx[full], ref[full])
    assert (ref[~full] == SENTINEL).all() and (idx[~full] == 0).all()  # the reference leaves an empty ball's row unwritten
    assert ((0 <= idx) & (idx < shape[1])).all() and (cnt <= shape[3]).all()


@pytest.mark.parametrize("recipe", R.RECIPES, ids=R.RECIPE_IDS)
def test_vectorised_restatement_is_the_row_loop(recipe):
    for row in R.SHAPES[:8]:
        P, Q, radius = R.make_case(row[0], recipe)
        for rule in R.RULES:
            a, b = R.ball_query(P, Q, radius, row[0][3], rule), R.ball_query_by_loop(P, Q, radius, row[0][3], rule)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == np.int32 and a[1].dtype == np.int32


def test_the_table_reaches_every_launch_rule():
    """the rows marked 2W+1 have m one more than twice a workgroup's queries at 1, 2 and 4 queries per wave"""
    assert [R.queries_per_wave(s[0], s[2]) for s in R.TWO_W_PLUS_ONE] == [1, 2, 4]
    for b, n, m, ns in R.TWO_W_PLUS_ONE:
        assert m == 2 * R.WAVES_PER_WORKGROUP * R.queries_per_wave(b, m) + 1 and (b, n, m, ns) in [row[0] for row in R.SHAPES]
    assert [R.queries_per_wave(1, q) for q in (1, 8192, 8193, 16384, 16385, 24577, 10 ** 6)] == [1, 1, 2, 2, 3, 4, 4]


def test_the_recipes_reach_their_branches():
    """what the recipe texts promise, over the whole table: empty, short and overflowing balls all occur, the grid's forced pair sits
    exactly on the radius and is excluded under both rules, the floor separates the rules on zero distances."""
    seen = set()
    for row in R.SHAPES:
        shape = row[0]
        b, n, m, ns = shape
        for recipe in R.RECIPES:
            P, Q, radius = R.make_case(shape, recipe)
            d2 = R.dist2(P, Q)
            for rule in R.RULES:
                idx, cnt = R.ball_query(P, Q, radius, ns, rule)
                total = R.passes(d2, radius, rule).sum(-1)
                seen |= {"empty"} if (cnt == 0).any() else set()
                seen |= {"short"} if ((cnt > 0) & (cnt < ns)).any() else set()
                seen |= {"overflow"} if (total > ns).any() else set()
                seen |= {"exact"} if ((total == ns) & (cnt == ns)).any() else set()
                if recipe[0].startswith("grid"):
                    assert d2[0, 0, n - 1] == radius * radius and not R.passes(d2, radius, rule)[0, 0, n - 1]
                if recipe[0] == "fill-late":
                    assert (total == min(3, n)).all() and (idx[:, :, 0] == max(n - 3, 0)).all()
                if recipe[0] in ("fill-last63", "fill-last64", "fill-lastn"):
                    last = min({"fill-last63": 63, "fill-last64": 64, "fill-lastn": n - 1}[recipe[0]], n - 1)
                    assert (total == min(ns, last + 1)).all() and (idx.max(-1) == last).all()
                if recipe[0] == "clusters" and ns < 64 < n:
                    assert (total[:, ::2] > ns).all() and (idx[:, ::2].max(-1) < 64).all()
            if recipe[0].startswith("copies"):
                zero = d2[0, 0, 0] == 0
                a = R.passes(d2, radius, R.SQRT)[0, 0, 0]
                c = R.passes(d2, radius, R.SQUARED)[0, 0, 0]
                assert zero and bool(a) == (radius > np.float32(1e-20)) and bool(c)  # 1e-20: the floor keeps a zero distance out
    assert seen == {"empty", "short", "overflow", "exact"}


@pytest.mark.parametrize("row", R.SHAPES, ids=SHAPE_IDS)
def test_boundary_recipe_splits_the_rules(row):
    """recipe 3's premise: under its committed seed the two rules give at least one query different rows."""
    shape = row[0]
    P, Q, radius = R.boundary(shape)
    assert R.rules_differ(P, Q, radius, shape[3])
    a, ca = R.ball_query(P, Q, radius, shape[3], R.SQRT)
    c, cc = R.ball_query(P, Q, radius, shape[3], R.SQUARED)
    assert ca[0, 0] == 0 and cc[0, 0] == 1  # the pair the radius was taken from: excluded by r < r, included by d2 < fl(r * r)


def test_group_backward_reference_is_the_gradient_of_group():
    """the float64 gradient reference against torch autograd of the gather composition (float64), multiplicities against a count"""
    shape, c = (2, 65, 7, 3), 5
    P, Q, radius = R.make_case(shape, R.RECIPES[1])
    idx, _ = R.ball_query(P, Q, radius, shape[3], R.SQUARED)
    rng = np.random.default_rng(5)
    feat, g = rng.standard_normal((2, c, 65)), rng.standard_normal((2, 3 + c, 7, 3))
    x, q, f = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (P, Q, feat))
    li = torch.from_numpy(idx).long()
    ar = torch.arange(2).view(2, 1, 1)
    out = torch.cat([(x[ar, li] - q[:, :, None, :]).permute(0, 3, 1, 2), f.transpose(1, 2)[ar, li].permute(0, 3, 1, 2)], 1)
    assert np.array_equal(out.detach().numpy().astype(np.float32), R.group(P, Q, feat.astype(np.float32), idx, True))
    gx, gq, gf = torch.autograd.grad(out, [x, q, f], torch.from_numpy(g))
    ref = R.group_backward(65, c, True, idx, g)
    for got, key in ((gx, "grad_xyz"), (gq, "grad_new_xyz"), (gf, "grad_features")):
        assert np.allclose(got.numpy(), ref[key], rtol=0, atol=1e-12), key
    assert np.array_equal(ref["mult"], np.stack([np.bincount(idx[i].ravel(), minlength=65) for i in range(2)]))
    assert ref["mult"].sum() == idx.size


# ------------------------------------------------------------------------------------------------ argument checks, no GPU
BAD = 10001
P_ = "PTR"  # a non-NULL device pointer that is never dereferenced
Q_BASE = [1, 8, 4, 0.5, 2, 0, P_, 0, P_, 0, P_, None, None]                      # sn_ball_query
F_BASE = [1, 8, 4, 3, 0.5, 2, 1, 1, P_, P_, P_, P_, None, P_, None]              # sn_ball_group_forward
B_BASE = [1, 8, 4, 3, 2, 1, P_, P_, None, None, None, None]                      # sn_ball_group_backward


def _with(base, changes):
    out = list(base)
    for k, v in changes.items():
        out[k] = v
    return out


def _cases():
    q, f, g = "sn_ball_query", "sn_ball_group_forward", "sn_ball_group_backward"
    out = []
    for name, base, sizes in ((q, Q_BASE, (0, 1, 2)), (f, F_BASE, (0, 1, 2, 3)), (g, B_BASE, (0, 1, 2, 3))):
        for pos in sizes:
            out.append(("%s-negative-%d" % (name, pos), name, _with(base, {pos: -1}), BAD, "negative size"))
    for name, base, pos in ((q, Q_BASE, 4), (f, F_BASE, 5), (g, B_BASE, 4)):
        for ns in (0, -3):
            out.append(("%s-nsample%d" % (name, ns), name, _with(base, {pos: ns}), BAD, "nsample"))
    for name, base, pos in ((q, Q_BASE, 5), (f, F_BASE, 6)):
        for rule in (-1, 2):
            out.append(("%s-rule%d" % (name, rule), name, _with(base, {pos: rule}), BAD, "bad rule"))
    for pos in (7, 9):
        for layout in (-1, 2):
            out.append(("%s-layout%d-%d" % (q, pos, layout), q, _with(Q_BASE, {pos: layout}), BAD, "bad layout"))
    for name, base, pos in ((f, F_BASE, 7), (g, B_BASE, 5)):
        out.append((name + "-use_xyz2", name, _with(base, {pos: 2}), BAD, "use_xyz"))
        out.append((name + "-no-channel", name, _with(base, {3: 0, pos: 0}), BAD, "no output channel"))
    for name, base, required in ((q, Q_BASE, (6, 8, 10)), (f, F_BASE, (8, 9, 10, 11, 13)), (g, B_BASE, (6, 7))):
        for pos in required:
            out.append(("%s-null-%d" % (name, pos), name, _with(base, {pos: None}), BAD, "null pointer"))
    out.append((q + "-empty-dataset", q, _with(Q_BASE, {1: 0}), BAD, "n == 0"))
    out.append((f + "-empty-dataset", f, _with(F_BASE, {1: 0}), BAD, "n == 0"))
    # the documented no-ops: nothing is dereferenced, nothing launched (every pointer NULL)
    nq, nf, nb = [1, 8, 4, 0.5, 2, 0] + [None, 0, None, 0, None, None, None], F_BASE[:8] + [None] * 7, B_BASE[:6] + [None] * 6
    for tag, ch in (("b0", {0: 0}), ("m0", {2: 0}), ("b0-n0", {0: 0, 1: 0})):
        out.append((q + "-noop-" + tag, q, _with(nq, ch), 0, None))
        out.append((f + "-noop-" + tag, f, _with(nf, ch), 0, None))
    out.append((g + "-noop-b0", g, _with(nb, {0: 0}), 0, None))
    out.append((g + "-noop-m0-no-output", g, _with(nb, {2: 0}), 0, None))
    # any float radius is legal: these fail on the NEXT check (a NULL pointer), not on the radius
    for r in (float("nan"), -1.0, 0.0, float("inf")):
        out.append(("%s-radius-%r" % (q, r), q, _with(Q_BASE, {3: r, 6: None}), BAD, "null pointer"))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def results():
    return run_cases(CASES)


def test_the_tables_match_the_prototypes():
    from samplenet_amd import _lib

    for name, base in (("sn_ball_query", Q_BASE), ("sn_ball_group_forward", F_BASE), ("sn_ball_group_backward", B_BASE)):
        proto = _lib.PROTOTYPES[name]
        assert len(proto) == len(base), name
        for ty, a in zip(proto, base):
            assert (ty is ctypes.c_void_p) == (a is None or a == P_), name
            assert (ty is ctypes.c_float) == isinstance(a, float), name
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_table(results, case):
    check_case(results, case)


def test_cpu_tensors_raise():
    from samplenet_amd import ops
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    xyz, new = torch.zeros(1, 8, 3), torch.zeros(1, 2, 3)
    with pytest.raises(RuntimeError):
        ops.ball_query(0.5, 4, xyz, new)
    with pytest.raises(RuntimeError):
        ops.query_ball_point(0.5, 4, xyz, new)
    with pytest.raises(RuntimeError):
        ops.ball_group(0.5, 4, xyz, new, torch.zeros(1, 3, 8))
    with pytest.raises(RuntimeError):
        PU.ball_query(0.5, 4, xyz, new)
    with pytest.raises(RuntimeError):
        PU.QueryAndGroup(0.5, 4)(xyz, new, None)
    with pytest.raises(ValueError):
        ops.ball_query(0.5, 4, xyz, new, rule="cube")
    with pytest.raises(ValueError):
        PU.QueryAndGroup(0.5, 4, use_xyz=False)(xyz, new, None)
    # GroupAll is plain tensor ops: it runs anywhere
    f = torch.arange(16.0).view(1, 2, 8)
    out = PU.GroupAll()(xyz + 1, None, f)
    assert out.shape == (1, 5, 1, 8) and bool((out[:, :3] == 1).all()) and torch.equal(out[:, 3:, 0], f)
    assert PU.GroupAll(use_xyz=False)(xyz, None, f).shape == (1, 2, 1, 8) and PU.GroupAll()(xyz, None).shape == (1, 3, 1, 8)

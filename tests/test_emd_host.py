"""Host-side half of the direct EMD tests (no GPU): the table of tests/emd_ref.py is honest -- every case it lists meets the admission
rule (the fp32 oracle and the CPU model of the fast exponential stay within 1/4 of every bar the case is asserted under), every shape
row and every recipe keeps a case, the plans the rows are named for are the plans emd_seg_plan makes --, the float64 reference is
sane on its own (marginals, sign, gradient against a finite difference), and the workspace sizes the library reports cover the layout
emd_loss_impl lays out: level vectors, segment partials and counters, cost partials, then P1 at a 16-byte offset, then P2."""
import numpy as np
import pytest

import emd_ref as E


@pytest.fixture(scope="module")
def lib():
    from built_lib import ensure_built

    ensure_built()
    from samplenet_amd._lib import lib as L

    return L


# ------------------------------------------------------------------------------------------------ the table
def test_table_covers_every_row_and_recipe():
    cs = E.cases()
    assert {c[0] for c in cs} == {s for s, _ in E.SHAPES}
    assert {c[1] for c in cs} == set(E.RECIPES)
    assert set(E.CASE_SEEDS) | set(E.NOT_ADMITTED) == {(s, r) for s, _ in E.SHAPES for r in E.RECIPES}
    assert (2, 64, 64) in {c[0] for c in E.cases(recipes=("same",))}  # the diagonal property needs n = m


def test_rows_reach_the_plans_they_are_named_for():
    """(ranges of pass k over xyz2, ranges of pass l over xyz1) as emd_seg_plan cuts them."""
    plans = {s: (E.seg_ranges(s[0], s[1], s[2]), E.seg_ranges(s[0], s[2], s[1])) for s, _ in E.SHAPES}
    for s in ((3, 7, 5), (2, 64, 64), (2, 65, 129), (2, 100, 300)):
        assert plans[s] == ((s[2],), (s[1],)), s
    assert plans[(1, 600, 300)] == ((300,), (320, 280))
    assert plans[(1, 300, 600)] == ((320, 280), (300,))
    assert plans[(1, 520, 600)] == ((320, 280), (320, 200))
    assert plans[(1, 100, 800)] == ((320, 320, 160), (100,))
    assert plans[(1, 1030, 70)] == ((70,), (320, 320, 320, 70))
    assert {s for s, p in plans.items() if len(p[0]) > 1 or len(p[1]) > 1} == set(E.SEGMENTED)
    assert E.multis(100, 300) == (3.0, 1.0) and E.multis(100, 800) == (8.0, 1.0) and E.multis(65, 129) == (1.0, 1.0)
    assert E.multis(7, 5) == (1.0, 1.0) and E.multis(1030, 70) == (1.0, 14.0)


@pytest.mark.parametrize("case", E.cases(), ids=E.case_id)
def test_every_case_of_the_table_is_admitted(oracle, case):
    """The admission rule, as a condition: the references alone within 1/4 of every bar the device is asserted under."""
    ref = E.reference(*case)
    ok, fo, ff = E.admitted(oracle, ref)
    print(E.show(E.case_id(case) + " oracle", fo))
    print(E.show(E.case_id(case) + " fast model", ff))
    assert ok, (E.misses(fo, 0.25), E.misses(ff, 0.25))
    if ref.shape[1] * ref.shape[2] < E.MEAN_FROM:
        assert "match mean" not in fo  # declared "not asserted" below n m = 4096


# ------------------------------------------------------------------------------------------------ the float64 reference itself
@pytest.mark.parametrize("case", E.cases(recipes=("cube", "sphere", "cluster", "big")), ids=E.case_id)
def test_fp64_plan_is_a_transport_plan(case):
    ref = E.reference(*case)
    b, n, m = ref.shape
    multiL, multiR = E.multis(n, m)
    assert ref.match.min() >= 0.0
    # the level-0 pass (exp = 1) ships whatever is left of the side with less total mass: n multiL on the left, m multiR on the right.
    # Column sums (over l) are what xyz1 points ship, row sums (over k) what xyz2 points receive.  With n >= m and m | n both sides
    # hold n: every column sums to multiL = 1; at 7 x 5 or 1030 x 70 the right side (5, 980) is the short one and fills instead.
    if n * multiL <= m * multiR:
        np.testing.assert_allclose(ref.match.sum(1), multiL, rtol=0, atol=1e-6)
    if n * multiL >= m * multiR:
        np.testing.assert_allclose(ref.match.sum(2), multiR, rtol=0, atol=1e-6)
    assert (ref.match.sum(2) <= multiR + 1e-9).all() and (ref.match.sum(1) <= multiL + 1e-9).all()
    for rl, rr, _ in ref.ratios:
        assert rl.min() >= 0.0 and rr.min() >= 0.0 and rr.max() <= multiR


def test_fp64_level_table_and_recipes():
    assert E.LEVELS == (-16384.0, -4096.0, -1024.0, -256.0, -64.0, -16.0, -4.0, -1.0, -0.25, 0.0)
    x1, x2 = E.make("same", 2, 65, 129, 0)
    assert np.array_equal(x1, x2[:, :65]) and x1.dtype == np.float32
    x1, x2 = E.make("cluster", 1, 7, 5, 0)
    assert (x1[:, :2] == x1[:, :1]).all() and (x2[:, :2] == x2[:, :1]).all() and not (x1[:, 2] == x1[:, 0]).all()
    x1, x2 = E.make("sphere", 2, 100, 300, 0)
    assert x1.min() < -0.5 and np.linalg.norm(x2, axis=2).max() <= 1.0 + 1e-6
    x1, x2 = E.make("noisy", 1, 600, 300, 0)
    assert np.abs(x1 - x2[:, np.arange(600) % 300]).max() < 0.06
    assert E.make("apart", 1, 7, 5, 0)[1].min() >= 3.0 and E.make("big", 1, 7, 5, 0)[0].max() > 10.0


def test_fp64_gradient_is_the_derivative_of_the_cost_at_fixed_match():
    b, n, m = 2, 9, 6
    x1, x2 = E.make("sphere", b, n, m, 3)
    x1, x2 = x1.astype(np.float64), x2.astype(np.float64)
    match, _ = E.approx_match_fp64(x1, x2)
    g1, g2 = E.match_cost_grad_fp64(x1, x2, match)
    h = 1e-6
    for x, g, which in ((x1, g1, 0), (x2, g2, 1)):
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            cp = E.match_cost_fp64(*((xp, x2) if which == 0 else (x1, xp)), match)
            cm = E.match_cost_fp64(*((xm, x2) if which == 0 else (x1, xm)), match)
            assert abs((cp - cm)[idx[0]] / (2 * h) - g[idx]) <= 1e-8, (which, idx)


def test_fast_exp_model_rounds_only_the_argument():
    """fast_exp=True is the same computation: at level 0 the argument is 0 either way, and the plan moves by rounding only."""
    ref = E.reference((2, 100, 300), "cube", 0)
    mt, rat = E.approx_match_fp64(ref.x1, ref.x2, fast_exp=True)
    assert 0.0 < np.abs(mt - ref.match).max() < 1e-4
    assert mt.min() >= 0.0 and len(rat) == 10


def test_ratio_vectors_define_the_match():
    """match_from_ratios(ratio_block()) is the reference's own match, and the figures it feeds are zero for the reference itself."""
    ref = E.reference((2, 65, 129), "sphere", 0)
    blk = ref.ratio_block()
    assert blk.shape == (2, 10 * (65 + 129))
    np.testing.assert_allclose(E.match_from_ratios(ref.x1, ref.x2, blk), ref.match, rtol=0, atol=1e-15)
    fig = E.figures(ref, ratios=blk)
    assert fig["ratioR"][0] == 0.0 and fig["ratioL held"][0] == 0.0 and fig["ratios as match"][0] <= 1e-15
    slip = blk.copy()
    slip[:, 65:130] = blk[:, 0:65]  # the second level's ratioL overwritten with the first's: a layout slip is seen
    assert E.misses(E.figures(ref, ratios=slip))
    slip = blk.copy()
    slip[:, 650 + 5 * 129:650 + 6 * 129] = blk[:, 650 + 4 * 129:650 + 5 * 129]  # the sixth level's ratioR replaced by the fifth's
    assert "ratioR" in E.misses(E.figures(ref, ratios=slip))


@pytest.mark.parametrize("case", E.cases(), ids=E.case_id)
def test_ratio_elements_asserted_one_by_one(case):
    """Which ratioL elements the float64 run calls well-posed: all of level 1 and, except where the plan is sharp (`noisy`, `same`:
    nearly every point is served at level 1, so 0 .. 23 % remain), at least 15 % of levels 2-10 (measured 16 .. 89 %) -- and the plain
    float32 evaluation stays within the bars on them and on every ratioR element (within 1/4: the admission test above)."""
    ref = E.reference(*case)
    n = ref.shape[1]
    wp = ref.well_posed()
    assert wp.shape == (ref.shape[0], 10 * n) and wp[:, :n].all()
    share = float(wp[:, n:].mean())
    print("%s: %.0f %% of ratioL at levels 2-10 asserted element by element" % (E.case_id(case), 100 * share))
    assert share >= 0.15 or ref.recipe in ("noisy", "same")
    assert not E.misses(E.fp32_ratio_figures(ref))


# ------------------------------------------------------------------------------------------------ workspace sizes
def seg_floats(b, n, m):
    """segment partials + arrival counters behind the level vectors (emd_seg_floats)."""
    (sk, _), (sl, _) = E.seg_plan(b, n, m), E.seg_plan(b, m, n)
    if sk <= 1 and sl <= 1:
        return 0
    psum = max(b * sk * 2 * n, b * sl * m)
    ctr = b * max((n + 255) // 256, (m + 255) // 256)
    return psum + (ctr + 63) // 64 * 64


@pytest.mark.parametrize("shape", [s for s, _ in E.SHAPES] + [(5, 3, 2), (1, 1, 1), (2, 2048, 2048)], ids=str)
def test_workspace_bytes_cover_the_layout(lib, shape):
    b, n, m = shape
    am = lib.sn_workspace_bytes(b"approxmatch", b, n, m, 0)
    el = lib.sn_workspace_bytes(b"emd_loss", b, n, m, 0)
    mc = lib.sn_workspace_bytes(b"matchcost", b, n, m, 0)
    assert am == 4 * (b * 11 * (n + m) + seg_floats(b, n, m))
    assert mc == 4 * b * ((n + 255) // 256)
    nkt, nlt = (n + 63) // 64, (m + 63) // 64
    sweep = 4 * b * (nlt * n * 4 + nkt * m * 3)  # P1 [b][tiles_l][n][4], P2 [b][tiles_k][m][3]
    assert el >= am + 4 * b * ((n + 255) // 256) + sweep
    assert am % 4 == 0 and el % 4 == 0 and mc % 4 == 0
    # P1 is read and written as float4: its offset is rounded up to 16 bytes, and the size grows by exactly that padding
    p1 = am + 4 * b * ((n + 255) // 256)
    assert el == (p1 + 15) // 16 * 16 + sweep


@pytest.mark.parametrize("shape", [(3, 50, 0), (3, 0, 4), (0, 5, 4), (2, 0, 0), (1, 600, 0), (1, 0, 600)], ids=str)
def test_workspace_bytes_of_an_empty_cloud(lib, shape):
    """ops.emd_loss asks for the workspace of whatever shape it is given: an empty cloud has no ranges to cut (the plan used to
    divide by a range length of zero) and needs no more than the level vectors and cost partials of the other one."""
    b, n, m = shape
    for op in (b"approxmatch", b"matchcost", b"emd_loss"):
        wb = lib.sn_workspace_bytes(op, b, n, m, 0)
        assert 0 <= wb <= 4 * (b * 11 * (n + m) + b * ((n + 255) // 256) + 3) and wb % 4 == 0, (op, wb)


def test_workspace_p1_padding_is_needed_at_the_ragged_row(lib):
    """(3, 7, 5): 3 * 11 * 12 + 0 + 3 * 1 = 399 floats in front of P1 -- not a multiple of 4."""
    am = lib.sn_workspace_bytes(b"approxmatch", 3, 7, 5, 0)
    assert (am // 4 + 3) % 4 == 3
    assert lib.sn_workspace_bytes(b"emd_loss", 3, 7, 5, 0) == 4 * (400 + 3 * (1 * 7 * 4 + 1 * 5 * 3))

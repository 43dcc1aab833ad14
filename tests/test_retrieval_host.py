"""tests/retrieval_ref.py, the yardstick of sn_retrieval_metrics, held to the worked example of the contract, its float32 restatement
to its float64 one on the grid recipes (where float32 is exact in any order), its shortcuts to the definitions they abbreviate, and
evaluation.retrieval_aggregates to its edge cases.  No GPU."""
import numpy as np
import pytest

import retrieval_ref as R


def test_worked_example():
    """C = 1, a = [0, 1, 3, 7], labels = [0, 0, 1, 0], L = 2: AP = [5/6, 5/6, NaN, 7/12], map = 0.75, precision of query 0 =
    [1, 2/3], of query 3 = [1/2, 2/3], n_relevant = [2, 2, 0, 2]."""
    a = np.array([[0.0], [1.0], [3.0], [7.0]], np.float32)
    labels = np.array([0, 0, 1, 0], np.int32)
    ref = R.reference(a, labels, 2)
    assert np.array_equal(ref["d"], [[0, 1, 9, 49], [1, 0, 4, 36], [9, 4, 0, 16], [49, 36, 16, 0]])
    assert np.array_equal(ref["order"], [[1, 2, 3], [0, 2, 3], [1, 0, 3], [2, 1, 0]])
    assert np.array_equal(ref["sorted_dist"], [[1, 9, 49], [1, 4, 36], [4, 9, 16], [16, 36, 49]])
    assert np.array_equal(ref["n_relevant"], [2, 2, 0, 2])
    # the float64 values of the formulas as written: (1/1 + 2/3) / 2 and (1/2 + 2/3) / 2
    assert np.array_equal(ref["ap"], [(1.0 + 2.0 / 3.0) / 2.0, (1.0 + 2.0 / 3.0) / 2.0, np.nan, (0.5 + 2.0 / 3.0) / 2.0], equal_nan=True)
    assert np.array_equal(ref["ap"].astype(np.float32), np.array([5 / 6, 5 / 6, np.nan, 7 / 12], np.float32), equal_nan=True)
    assert np.array_equal(ref["prec"], [[1.0, 2.0 / 3.0], [1.0, 2.0 / 3.0], [np.nan, np.nan], [0.5, 2.0 / 3.0]], equal_nan=True)
    assert abs(np.nanmean(ref["ap"]) - 0.75) <= 2.0 ** -52

    from samplenet_amd.evaluation import retrieval_aggregates

    agg = retrieval_aggregates(ref["ap"], ref["prec"], ref["n_relevant"])
    assert abs(agg["map"] - 0.75) <= 2.0 ** -52 and agg["n_valid"] == 3
    assert np.allclose(agg["pr_curve"], [(1 + 1 + 0.5) / 3, 2 / 3], rtol=0, atol=2.0 ** -52)
    assert abs(agg["auc"] - (2.5 / 3 + 2 / 3) / 2) <= 2.0 ** -52


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("n,C", [(1, 3), (2, 1), (9, 64), (33, 65), (40, 255), (24, 256)])
def test_float32_restatement_is_exact_on_the_grid(recipe, n, C):
    desc, labels = R.make_case(recipe, 2, n, C)
    q = desc.astype(np.float64) * 16
    assert np.array_equal(q, np.round(q)) and np.abs(desc).max() <= 2 and C <= 256  # the recipe's premises
    for s in range(2):
        d64, d32 = R.dist64(desc[s]), R.dist32(desc[s])
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64)
        assert np.array_equal(R.dist64_grid(desc[s]), d64)
        assert np.array_equal(d32, d32.T) and (np.diag(d64) == 0).all()
        assert d64.max(initial=0) <= 4096 and np.array_equal(d64 * 256, np.round(d64 * 256))
        assert np.array_equal(R.dist32(desc[s], rows=[n - 1, 0]), d32[[n - 1, 0]])


def test_float32_restatement_on_real_values():
    """off the grid: symmetric bit for bit, exactly zero on the diagonal and for duplicated rows, and within the counted bound of C
    products and C - 1 additions of float64: (C + 2) 2^-24 relative (a difference's rounding enters twice through its square)"""
    desc, _ = R.normal_case(50, 256, 5)
    a = desc[0]
    a[7] = a[31]
    d64, d32 = R.dist64(a), R.dist32(a)
    assert np.array_equal(d32, d32.T) and (np.diag(d32) == 0).all() and d32[7, 31] == 0
    assert (np.abs(d32.astype(np.float64) - d64) <= (256 + 2) * 2.0 ** -24 * d64).all()
    assert not np.array_equal(d32.astype(np.float64), d64)  # (the restatement does round)


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("n,L", [(2, 1), (3, 20), (23, 7), (40, 64)])
def test_vectorised_scores_are_the_rank_loop(recipe, n, L):
    desc, labels = R.make_case(recipe, 1, n, 5, classes=3)
    ref = R.reference(desc[0], labels, L, exact_grid=True)
    ap, prec, rel = R.scores_by_loop(ref["order"], labels, L)
    assert np.array_equal(ref["n_relevant"], rel)
    assert np.array_equal(ref["ap"], ap, equal_nan=True) and np.array_equal(ref["prec"], prec, equal_nan=True)
    assert R.order_is_the_ranking(ref["d"], ref["order"])
    if n > 2:
        swapped = ref["order"].copy()
        swapped[n // 2, [0, 1]] = swapped[n // 2, [1, 0]]
        assert not R.order_is_the_ranking(ref["d"], swapped)
        twice = ref["order"].copy()
        twice[0, 1] = twice[0, 0]
        assert not R.order_is_the_ranking(ref["d"], twice)
    if recipe == "identical":
        assert np.array_equal(ref["order"], [[j for j in range(n) if j != i] for i in range(n)])
    if recipe == "distinct_labels":
        assert np.isnan(ref["ap"]).all() and np.isnan(ref["prec"]).all() and (rel == 0).all()
    if recipe == "singleton":
        assert rel[n // 2] == 0 and np.isnan(ref["ap"][n // 2])
        if n > 3:  # (with 2 or 3 shapes taking one out of a class of the alternating labels leaves another alone too)
            assert np.isnan(ref["ap"]).sum() == 1
    if recipe == "one_label":
        assert (ref["ap"] == 1).all() and (ref["prec"] == 1).all() and (rel == n - 1).all()


def test_single_shape():
    ref = R.reference(np.ones((1, 4), np.float32), np.array([2], np.int32), 3)
    assert ref["order"].shape == (1, 0) and np.isnan(ref["ap"]).all() and np.isnan(ref["prec"]).all() and ref["n_relevant"][0] == 0


def test_aggregates_edge_cases():
    from samplenet_amd.evaluation import retrieval_aggregates

    nan = np.nan
    none = retrieval_aggregates(np.full(4, nan), np.full((4, 3), nan), np.zeros(4, np.int64))
    assert none["n_valid"] == 0 and np.isnan(none["map"]) and np.isnan(none["auc"])
    assert none["pr_curve"].shape == (3,) and np.isnan(none["pr_curve"]).all()
    one = retrieval_aggregates(np.array([nan, 0.25, nan], np.float32), np.array([[nan, nan], [0.5, 0.125], [nan, nan]], np.float32), [0, 3, 0])
    assert one["n_valid"] == 1 and one["map"] == 0.25 and np.array_equal(one["pr_curve"], [0.5, 0.125]) and one["auc"] == 0.3125
    assert one["pr_curve"].dtype == np.float64
    two = retrieval_aggregates([0.5, nan, 1.0], [[1.0], [nan], [0.5]], [1, 0, 2])
    assert two == {"map": 0.75, "pr_curve": two["pr_curve"], "auc": 0.75, "n_valid": 2} and np.array_equal(two["pr_curve"], [0.75])

"""numpy restatement of sn_retrieval_metrics (include/samplenet_hip_internal.h): all-against-all retrieval inside one labelled set.
The reference tree has no retrieval script, so the definitions here ARE the yardstick (tests/test_retrieval_host.py holds them to a
worked example; tests/test_gpu_retrieval.py holds the kernel to them).

    d(i, j)  = sum_c (a_ic - a_jc)^2                                  dist64: float64;  dist32: float32 in the kernel's order
    ranking  = all j != i ascending by (d(i, j), j)                    numpy's stable argsort with the query removed
    R_i      = others with the query's label,  H(r) = those among the first r ranks
    AP_i     = (sum over relevant ranks r of H(r) / r) / R_i           float64, the terms added in ascending rank
    prec_il  = H(r*) / r*, r* the smallest r with H(r) >= (l R_i + L - 1) // L,  l = 1..L
    R_i == 0 -> NaN

The kernel's fp32 summation order, mirrored by dist32: with the channels padded by zeros to a multiple of 64, partial sum l < 64 adds
the squares of the channels l, l + 64, l + 128, .. in ascending order; the 64 partial sums are then added as a balanced tree of
adjacent pairs (six halvings).  A padded channel adds +0, which changes nothing.

The grid recipe makes fp32 exact in ANY order: descriptors are multiples of 2^-4 in [-2, 2] and C <= 256, so a difference is a
multiple of 2^-4 of at most 4, a square a multiple of 2^-8 of at most 16, and every partial sum a multiple of 2^-8 of at most 4096:
20 bits."""
import bisect

import numpy as np

GRID_STEP = 1.0 / 16.0
RECIPES = ("grid", "identical", "duplicates", "one_label", "distinct_labels", "singleton")


# ------------------------------------------------------------------------------------------------ inputs
def grid_desc(rng, S, n, C):
    """(S, n, C) float32, multiples of 2^-4 in [-2, 2]"""
    return (rng.integers(-32, 33, size=(S, n, C)) * GRID_STEP).astype(np.float32)


def make_case(recipe, S, n, C, classes=5, seed=0):
    """-> desc (S, n, C) float32 on the grid, labels (n,) int32"""
    rng = np.random.default_rng([seed, S, n, C, RECIPES.index(recipe)])
    desc = grid_desc(rng, S, n, C)
    labels = rng.integers(0, classes, size=n).astype(np.int32)
    if recipe == "identical":        # every distance ties at 0: the order must be 0..n-1 without the query
        desc[:] = desc[:, :1]
    elif recipe == "duplicates":     # duplicated rows at scattered indices: zero distances and ties on the index
        src = rng.integers(0, n, size=max(1, n // 3))
        dst = rng.integers(0, n, size=max(1, n // 3))
        desc[:, dst] = desc[:, src]
        desc[:, n - 1] = desc[:, 0]  # (whatever was drawn: the first and the last shape are one)
    elif recipe == "one_label":
        labels[:] = 3
    elif recipe == "distinct_labels":  # every query invalid
        labels = (np.arange(n)[::-1] * 7 - 5).astype(np.int32)
    elif recipe == "singleton":      # one class with a single member: that query alone is invalid
        labels = (np.arange(n) % 2).astype(np.int32)
        labels[n // 2] = 9
    return desc, labels


def normal_case(n, C, classes, seed=0):
    rng = np.random.default_rng([seed, n, C, classes])
    return rng.standard_normal((1, n, C)).astype(np.float32), rng.integers(0, classes, size=n).astype(np.int32)


# ------------------------------------------------------------------------------------------------ distances
def _rows(rows, n):
    return np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)


def dist64(a, rows=None):
    """(n, C) -> (len(rows), n) float64, the definition: channel by channel.  rows: the queries wanted, default all"""
    a = np.asarray(a, dtype=np.float64)
    rows = _rows(rows, len(a))
    d = np.zeros((len(rows), len(a)))
    for c in range(a.shape[1]):
        d += np.subtract.outer(a[rows, c], a[:, c]) ** 2
    return d


def dist64_grid(a, rows=None):
    """dist64 for GRID descriptors through integers (16 a is an integer of at most 32, every sum below 2^53: float64 holds the
    expansion exactly).  Only a shortcut of this file for large n; the kernel never expands the square."""
    q = np.asarray(a, dtype=np.float64) * 16.0
    assert np.array_equal(q, np.round(q)) and np.abs(q).max(initial=0.0) <= 32
    rows = _rows(rows, len(q))
    sq = (q * q).sum(1)
    return (sq[rows, None] + sq[None, :] - 2.0 * (q[rows] @ q.T)) / 256.0


def dist32(a, rows=None):
    """(n, C) float32 -> (len(rows), n) float32 in the kernel's summation order (module docstring); rows default: all"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, C = a.shape
    rows = _rows(rows, n)
    M = (C + 63) // 64
    pad = np.zeros((n, M * 64), np.float32)
    pad[:, :C] = a
    out = np.empty((len(rows), n), np.float32)
    for lo in range(0, len(rows), 32):
        r = rows[lo:lo + 32]
        u = pad[r][:, None, :] - pad[None, :, :]          # a_i - a_j
        sq = (u * u).reshape(len(r), n, M, 64)
        p = sq[:, :, 0, :].copy()
        for k in range(1, M):
            p = p + sq[:, :, k, :]
        while p.shape[-1] > 1:
            p = p[..., 0::2] + p[..., 1::2]
        out[lo:lo + 32] = p[..., 0]
    return out


# ------------------------------------------------------------------------------------------------ ranking and scores
def ranking(d, rows=None):
    """d (len(rows), n): the distances of the queries `rows` (default all) -> order (len(rows), n-1): per query the others ascending
    by (distance, index)"""
    n = d.shape[1]
    rows = _rows(rows, n)
    full = np.argsort(d, axis=1, kind="stable")
    return full[full != rows[:, None]].reshape(len(rows), n - 1)


def order_is_the_ranking(d, order, rows=None):
    """True iff order[i] holds every j != rows[i] once and (d[i, order[i]], order[i]) ascends strictly: the ranking is the only such
    arrangement, so this is ranking(d, rows) == order without the sort."""
    n = d.shape[1]
    rows = _rows(rows, n)
    order = np.asarray(order).astype(np.int64)
    if order.shape != (len(rows), n - 1) or (order < 0).any() or (order >= n).any():
        return False
    seen = np.zeros((len(rows), n), bool)
    seen[np.arange(len(rows))[:, None], order] = True
    others = np.ones((len(rows), n), bool)
    others[np.arange(len(rows)), rows] = False
    if not np.array_equal(seen, others):
        return False
    ds = np.take_along_axis(np.asarray(d), order, axis=1)
    a, b, i, j = ds[:, :-1], ds[:, 1:], order[:, :-1], order[:, 1:]
    return bool(((a < b) | ((a == b) & (i < j))).all())


def scores(order, labels, L, rows=None):
    """order (len(rows), n-1): the rankings of the queries `rows` (default all), labels (n,) -> ap (len(rows),) float64, prec
    (len(rows), L) float64, n_relevant (len(rows),) int64.  No rounding to float32 here."""
    order, labels = np.asarray(order).astype(np.int64), np.asarray(labels)
    rows = _rows(rows, len(labels))
    n, m = len(rows), len(labels) - 1
    ap, prec, R = np.full(n, np.nan), np.full((n, L), np.nan), np.zeros(n, np.int64)
    if m == 0:
        return ap, prec, R
    rel = labels[order] == labels[rows][:, None]
    H = np.cumsum(rel, axis=1)
    R = H[:, -1].astype(np.int64)
    ranks = np.arange(1, m + 1, dtype=np.float64)
    terms = np.where(rel, H / ranks, 0.0)
    total = np.cumsum(terms, axis=1)[:, -1]          # ascending rank, one float64 addition per term (+0.0 for the others)
    ok = R > 0
    ap[ok] = total[ok] / R[ok]
    # rank_of[i, h]: the rank at which H first reaches h (H steps by one)
    rank_of = np.zeros((n, m + 1), np.int64)
    qi, pos = np.nonzero(rel)
    rank_of[qi, H[qi, pos]] = pos + 1
    for l in range(1, L + 1):
        t = (l * R + L - 1) // L
        r_star = rank_of[np.arange(n), t]
        prec[ok, l - 1] = t[ok].astype(np.float64) / r_star[ok].astype(np.float64)    # H(r*) == t
    return ap, prec, R


def scores_by_loop(order, labels, L):
    """scores() as the plain rank loop of the definition, one query at a time (the host route tools/retrieval_bench.py times)"""
    n = len(labels)
    ap, prec, R = np.full(n, np.nan), np.full((n, L), np.nan), np.zeros(n, np.int64)
    for i in range(n):
        rel = labels[order[i]] == labels[i]
        R[i] = Ri = int(rel.sum())
        if Ri == 0:
            continue
        h, total, H = 0, 0.0, []
        for r, ok in enumerate(rel, start=1):
            h += int(ok)
            H.append(h)
            if ok:
                total += h / r
        ap[i] = total / Ri
        for l in range(1, L + 1):
            t = (l * Ri + L - 1) // L
            r_star = bisect.bisect_left(H, t) + 1          # the smallest r with H(r) >= t (H does not decrease)
            prec[i, l - 1] = H[r_star - 1] / r_star
    return ap, prec, R


def reference(desc, labels, L, exact_grid=False, rows=None):
    """One set (n, C), the queries `rows` (default all): -> dict d (float64), order, sorted_dist (float64), ap, prec (float64),
    n_relevant"""
    d = dist64_grid(desc, rows) if exact_grid else dist64(desc, rows)
    order = ranking(d, rows)
    ap, prec, R = scores(order, labels, L, rows)
    return {"d": d, "order": order, "sorted_dist": np.take_along_axis(d, order, axis=1), "ap": ap, "prec": prec, "n_relevant": R}

"""Test helper of the inverted-index gradient of the weighted gather (tests/test_gather_inv_host.py, tests/test_gpu_gather_invert.py,
tests/test_gpu_three_interpolate_backward.py): numpy restatements, written from the contract in include/samplenet_hip_internal.h, of
sn_gather_invert (per destination row the entries that name it, ascending) and of sn_weighted_gather_backward_inverted (the
sequential float32 sum in list order, and float64 with a counted bound), the shape table, the index and value recipes and a cache
that computes every reference once.
Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np

import interp_ref as R

F = np.float32
U = 2.0 ** -24

TILE = 4096           # csrc/feature_propagate.hip: kInvTile, destination rows counted in LDS at a time
CHANNELS = 8          # kGbChannels, channels a thread of the walk accumulates
WORK = 1 << 26        # kInvWork: sn_gather_invert_supported(n, ne) iff ceil(n / 64) * ne <= WORK

# (b, c, n destination rows, m queries, k)
SHAPES = (
    (1, 1, 1, 1, 3),             # one row takes everything
    (2, 3, 2, 5, 3),             # the m < 3 filling of three-NN: a query names row 0 twice
    (1, 17, 64, 64, 3),
    (2, 16, 65, 257, 3),         # rows across a wave boundary
    (70, 2, 5, 3, 3),            # more than 64 clouds
    (1, 2, 1025, 130, 3),
    (1, 5, 4, 4100, 3),          # lists of about 3000 entries
    (1, 4 * CHANNELS + 1, 16, 65, 3),  # channels not a multiple of the walk's channel block
    (1, 3, 40, 9, 1),
    (1, 3, 40, 9, 8),
    (1, 2, 16385, 5, 3),         # five count tiles, the last of one row
    (1, 2, TILE + 1, 700, 3),    # a second count tile of one row, with entries in both
)
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
INDEX_RECIPES = ("nn", "same", "uniform", "descending", "oob", "empty")
VALUE_RECIPES = ("int", "mixed")


def supported(n, ne):
    return -(-n // 64) * ne <= WORK


# ------------------------------------------------------------------------------------------------ the restatement
def invert(idx, n):
    """idx (b,ne) or (b,m,k) -> start (b,n+1) int32, order (b,ne) int32: a plain walk over the entries in ascending order"""
    idx = np.asarray(idx)
    b = idx.shape[0]
    idx = idx.reshape(b, -1)
    ne = idx.shape[1]
    start, order = np.zeros((b, n + 1), np.int32), np.full((b, ne), -1, np.int32)
    for i in range(b):
        lists = {}
        for e in range(ne):
            r = int(idx[i, e])
            if 0 <= r < n:
                lists.setdefault(r, []).append(e)
        count = np.zeros(n, np.int64)
        for r, l in lists.items():
            count[r] = len(l)
        start[i, 1:] = np.cumsum(count)
        for r, l in lists.items():
            order[i, start[i, r]:start[i, r] + len(l)] = l
    return start, order


def backward32(c, n, k, weights, grad_out, start, order, reverse=False):
    """grad_X (b,c,n) float32: per row the sequential sum from +0, in list order, of fl(grad_out[:, e // k] * weights[e]); all
    channels of a row at once, one entry at a time.  reverse: every list walked backwards (a wrong order, for the host test)."""
    w = np.asarray(weights, F)
    g = np.asarray(grad_out, F)
    b = g.shape[0]
    w = w.reshape(b, -1)
    out = np.zeros((b, c, n), F)
    for i in range(b):
        for r in np.nonzero(start[i, 1:] > start[i, :-1])[0]:
            acc = np.zeros(c, F)
            entries = order[i, start[i, r]:start[i, r + 1]]
            for e in (entries[::-1] if reverse else entries):
                term = g[i, :, e // k] * w[i, e]
                acc = acc + term
                assert term.dtype == F and acc.dtype == F
            out[i, :, r] = acc
    return out


def backward64(c, n, k, weights, grad_out, start, order):
    """-> grad_X (b,c,n) float64 and its bound: (L + 1) * 2^-24 * sum|term| for a row of L entries (one rounding for each product,
    L additions, to first order)"""
    g = np.asarray(grad_out, np.float64)
    b = g.shape[0]
    w = np.asarray(weights, np.float64).reshape(b, -1)
    out, bound = np.zeros((b, c, n)), np.zeros((b, c, n))
    for i in range(b):
        for r in np.nonzero(start[i, 1:] > start[i, :-1])[0]:
            e = order[i, start[i, r]:start[i, r + 1]].astype(np.int64)
            terms = g[i][:, e // k] * w[i, e][None, :]      # (c, L)
            out[i, :, r] = terms.sum(1)
            bound[i, :, r] = (len(e) + 1) * U * np.abs(terms).sum(1)
    return out, bound


# ------------------------------------------------------------------------------------------------ recipes
def _seed(shape, salt):
    b, c, n, m, k = shape
    return ((((b * 1009 + c) * 1013 + n) * 1019 + m) * 1021 + k) * 31 + salt


def make_idx(shape, recipe):
    """-> idx (b,m,k) int32.
    nn: the k nearest of n known points for m unknown ones (interp_ref's three-NN at k = 3, with its filling at n < 3).
    same: every query names rows 0, 1, 2 (as far as n has them).  uniform: random rows.  descending: the row falls as the entry
    number rises, so list order and memory order disagree.  oob: uniform with about 10 % of the entries -1 or n.
    empty: only even rows are named, so at n >= 2 every odd row is empty."""
    b, c, n, m, k = shape
    rng = np.random.default_rng(_seed(shape, 1 + INDEX_RECIPES.index(recipe)))
    if recipe == "nn":
        u, kn = R.make_case((b, m, n, c, 0), "rand")
        if k == 3:
            idx = R.three_nn(u, kn)[0]
        else:
            idx = np.argsort(R.dist2(u, kn), axis=-1, kind="stable")[:, :, np.arange(k) % n]
    elif recipe == "same":
        idx = np.broadcast_to((np.arange(k) % 3) % n, (b, m, k))
    elif recipe == "descending":
        ne = m * k
        idx = np.broadcast_to(((ne - 1 - np.arange(ne)) * n // ne).reshape(m, k), (b, m, k))
    elif recipe == "empty":
        idx = 2 * rng.integers(0, (n + 1) // 2, (b, m, k))
    else:
        idx = rng.integers(0, n, (b, m, k))
        if recipe == "oob":
            bad = rng.random((b, m, k)) < 0.1
            idx = np.where(bad, np.where(rng.random((b, m, k)) < 0.5, -1, n), idx)
    return np.ascontiguousarray(idx, np.int32)


def make_values(shape, recipe, salt=0):
    """-> weights (b,m,k), grad_out (b,c,m) float32.  int: small integers (every sum exact in any order: a missing or doubled term
    shows).  mixed: normal values times 10^u, u uniform in [-1, 1] (another order gives other bits).  salt: other draws of the same
    recipe (case() gives every index recipe its own)."""
    b, c, n, m, k = shape
    rng = np.random.default_rng(_seed(shape, 20 + VALUE_RECIPES.index(recipe) + 2 * salt))
    if recipe == "int":
        return rng.integers(-3, 4, (b, m, k)).astype(F), rng.integers(-3, 4, (b, c, m)).astype(F)
    w = rng.standard_normal((b, m, k)) * 10.0 ** rng.uniform(-1, 1, (b, m, k))
    g = rng.standard_normal((b, c, m)) * 10.0 ** rng.uniform(-1, 1, (b, c, m))
    return w.astype(F), g.astype(F)


_CASES = {}


def case(shape, index_recipe, value_recipe=None):
    """the shared, read-only reference of one case: idx, start, order [, weights, grad_out, grad32, grad64, bound]"""
    key = (shape, index_recipe)
    if key not in _CASES:
        idx = make_idx(shape, index_recipe)
        start, order = invert(idx, shape[2])
        _CASES[key] = _frozen(dict(idx=idx, start=start, order=order))
    if value_recipe is None:
        return _CASES[key]
    vkey = key + (value_recipe,)
    if vkey not in _CASES:
        b, c, n, m, k = shape
        d = dict(_CASES[key])
        d["weights"], d["grad_out"] = make_values(shape, value_recipe, INDEX_RECIPES.index(index_recipe))
        d["grad32"] = backward32(c, n, k, d["weights"], d["grad_out"], d["start"], d["order"])
        d["grad64"], d["bound"] = backward64(c, n, k, d["weights"], d["grad_out"], d["start"], d["order"])
        _CASES[vkey] = _frozen(d)
    return _CASES[vkey]


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d

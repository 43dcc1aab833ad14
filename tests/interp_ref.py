"""Test helper of the feature-propagation pieces (tests/test_interp_host.py, tests/test_gpu_three_nn.py,
tests/test_gpu_three_interpolate.py): a numpy float32 restatement of sn_three_nn written from the contract in
include/samplenet_hip_internal.h, its plain row-loop twin, the inverse-distance weights and the three-term interpolation in
float32 and in float64 ON THE float32-SELECTED indices and float32 d2 (teacher-forced selection: no case is ever left out for a
near-tie), the float64 gradient with per-destination contribution counts, the input recipes, the shape table, the counted bounds
and a restatement of the kernel's launch rule.
Pointnet2_PyTorch's source is not at hand: the tie order, the m < 3 filling and both weight rules are as recalled, unpinned.
Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np

SQRT_EPS, SQUARED_CLAMP = 0, 1  # 1 / (dist + 1e-8), PointnetFPModule's; 1 / max(dist^2, 1e-10), the TF PointNet++ module's
RULES = (SQRT_EPS, SQUARED_CLAMP)
RULE_NAMES = {SQRT_EPS: "sqrt_eps", SQUARED_CLAMP: "squared_clamp"}
F = np.float32
U = 2.0 ** -24
EPS, CLAMP = F(1e-8), F(1e-10)

# counted bounds, relative and to first order, in units of U = 2^-24 (each float32 operation costs one).
#   SQRT_EPS:  r = 1 / (sqrt(d2) + eps): sqrt, add, div = 3;  norm = (r0 + r1) + r2: 3 + 2 = 5;  w = r / norm: 3 + 5 + 1 = 9
#   SQUARED_CLAMP: r = 1 / max(d2, c): div = 1;  norm: 1 + 2 = 3;  w: 1 + 3 + 1 = 5
# the sum of the three weights: (r0 + r1 + r2) / norm32 is within 2 of 1, each final division adds 1: 3
WEIGHT_BOUND = {SQRT_EPS: 9 * U, SQUARED_CLAMP: 5 * U}
WEIGHT_SUM_BOUND = 3 * U

# ------------------------------------------------------------------------------------------------ the launch rule, restated
STAGE = 1024          # csrc/feature_propagate.hip: kFpStage, known points per LDS stage
QUERIES = 64          # kFpQueries, queries per workgroup


def waves(b, n):
    """fp_waves: waves per workgroup from the number of workgroups b * ceil(n / 64)"""
    g = b * -(-n // QUERIES)
    return 4 if g >= 1024 else (8 if g >= 512 else 16)


# (b, n, m, c2, c1)
SHAPES = (
    (1, 1, 1, 1, 0),
    (2, 5, 2, 3, 0),            # m < 3
    (1, 7, 3, 1, 2),
    (3, 65, 4, 5, 0),
    (1, 64, 64, 17, 3),
    (2, 257, 65, 16, 1),
    (70, 3, 5, 2, 1),           # more than 64 clouds
    (1, 130, STAGE + 1, 2, 0),  # a second LDS stage of one point
    (1, QUERIES + 1, 16, 1, 0),
    (1, 2 * QUERIES + 1, 16, 1, 0),
    (1, 9, 2 * STAGE + 1, 9, 0),  # three stages, the last of one point
    (1, 5, 16385, 2, 0),        # seventeen stages, n small
    (520, 3, 5, 2, 1),          # 520 workgroups: 8 waves each
    (1030, 3, 5, 2, 1),         # 1030 workgroups: 4 waves each
)
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


# ------------------------------------------------------------------------------------------------ the restatement
def dist2(unknown, known):
    """d2[b,j,k] = ((dx*dx) + (dy*dy)) + (dz*dz), differences unknown - known, every operation in float32"""
    u, k = np.asarray(unknown, F), np.asarray(known, F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [u[:, :, None, c] - k[:, None, :, c] for c in range(3)]
        assert all(x.dtype == F for x in d)
        return ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])


def three_nn(unknown, known):
    """-> idx (b,n,3) int32, d2 (b,n,3) float32: the three smallest by (d2, index), a stable sort on d2; a NaN (or +inf) d2 is
    never selected; unfilled slots hold index 0 and +inf."""
    d2 = dist2(unknown, known)
    b, n, m = d2.shape
    key = np.where(d2 < F(np.inf), d2, F(np.inf))              # NaN and +inf: not selectable
    order = np.argsort(key, axis=-1, kind="stable")[:, :, :3]
    got = np.take_along_axis(key, order, -1)
    if m < 3:
        order = np.pad(order, ((0, 0), (0, 0), (0, 3 - m)))
        got = np.pad(got, ((0, 0), (0, 0), (0, 3 - m)), constant_values=np.inf)
    idx = np.where(got < F(np.inf), order, 0).astype(np.int32)
    return idx, got.astype(F)


def three_nn_by_loop(unknown, known):
    """the same as the ascending walk with strict < reads, row by row: what three_nn abbreviates"""
    d2 = dist2(unknown, known)
    b, n, m = d2.shape
    idx, out = np.zeros((b, n, 3), np.int32), np.full((b, n, 3), np.inf, F)
    for i in range(b):
        for j in range(n):
            best = [(F(np.inf), 0)] * 3
            for k in range(m):
                d = d2[i, j, k]
                if d < best[2][0]:
                    if d < best[1][0]:
                        best = [(d, k), best[0], best[1]] if d < best[0][0] else [best[0], (d, k), best[1]]
                    else:
                        best[2] = (d, k)
            for t in range(3):
                out[i, j, t], idx[i, j, t] = best[t]
    return idx, out


def weights(d2, rule):
    """float32: r_t = 1 / (sqrt(d2_t) + 1e-8f) or 1 / max(d2_t, 1e-10f); norm = (r_0 + r_1) + r_2; w_t = r_t / norm"""
    d2 = np.asarray(d2, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = F(1) / (np.sqrt(d2) + EPS) if rule == SQRT_EPS else F(1) / np.maximum(d2, CLAMP)
        norm = (r[..., 0] + r[..., 1]) + r[..., 2]
        w = r / norm[..., None]
    assert w.dtype == F
    return w


def weights64(d2, rule):
    """the same expression in float64 on the float32 d2 (the float32 constants, widened)"""
    d2 = np.asarray(d2, F).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = 1.0 / (np.sqrt(d2) + np.float64(EPS)) if rule == SQRT_EPS else 1.0 / np.maximum(d2, np.float64(CLAMP))
        return r / r.sum(-1, keepdims=True)


def _gather(feats, idx):
    """feats (b,c,m), idx (b,n,3) -> (b,c,n,3)"""
    b = feats.shape[0]
    return feats[np.arange(b)[:, None, None, None], np.arange(feats.shape[1])[None, :, None, None], idx[:, None, :, :].astype(np.int64)]


def interpolate(known_feats, idx, w):
    """float32 ((w_0*f_0) + (w_1*f_1)) + (w_2*f_2) -> (b,c2,n)"""
    f = _gather(np.asarray(known_feats, F), idx)
    w = np.asarray(w, F)[:, None]
    with np.errstate(invalid="ignore"):
        out = ((w[..., 0] * f[..., 0]) + (w[..., 1] * f[..., 1])) + (w[..., 2] * f[..., 2])
    assert out.dtype == F
    return out


def interpolate64(known_feats, idx, w):
    f = _gather(np.asarray(known_feats, np.float64), idx)
    return (np.asarray(w, np.float64)[:, None] * f).sum(-1)


def propagate(unknown, known, unknown_feats, known_feats, rule):
    """-> idx, weight, out (b,c2+c1,n): the whole forward"""
    idx, d2 = three_nn(unknown, known)
    w = weights(d2, rule)
    out = interpolate(known_feats, idx, w)
    if unknown_feats is not None and unknown_feats.shape[1]:
        out = np.concatenate([out, np.asarray(unknown_feats, F)], axis=1)
    return idx, w, np.ascontiguousarray(out)


def backward64(m, c2, idx, w, grad_out):
    """float64 gradient towards known_feats for grad_out (b,c2+c1,n): grad (b,c2,m), the sum of |terms| behind every element
    (abs) and mult (b,m): how many (j,t) contribute to each known point"""
    idx = np.asarray(idx).astype(np.int64)
    b, n, _ = idx.shape
    g = np.asarray(grad_out, np.float64)[:, :c2]                      # (b,c2,n)
    terms = g[:, :, :, None] * np.asarray(w, np.float64)[:, None]     # (b,c2,n,3)
    grad, ab, mult = np.zeros((b, c2, m)), np.zeros((b, c2, m)), np.zeros((b, m))
    flat = idx.reshape(b, n * 3)
    cloud = np.arange(b)[:, None]
    np.add.at(mult, (cloud, flat), 1.0)
    where = (cloud[:, :, None], np.arange(c2)[None, :, None], flat[:, None, :])
    np.add.at(grad, where, terms.reshape(b, c2, n * 3))
    np.add.at(ab, where, np.abs(terms).reshape(b, c2, n * 3))
    return grad, ab, mult


# ------------------------------------------------------------------------------------------------ recipes
RECIPES = ("rand", "lattice", "dup", "same", "big", "nan")


def _seed(shape, salt):
    b, n, m, c2, c1 = shape
    return (((b * 1009 + n) * 1013 + m) * 1019 + c2) * 1021 + c1 + 7919 * salt


def make_case(shape, recipe):
    """-> unknown (b,n,3), known (b,m,3) float32.
    rand: uniform - 0.5.  lattice: integer coordinates in [-4,4] divided by 8, every d2 exact, ties at the third neighbour in most
    rows.  dup: every unknown point is a copy of a known one (d2 = 0: the epsilon or the clamp decides).  same: all known points
    identical (idx 0, 1, 2).  big: rand x 1e3.  nan: one known point per cloud is NaN."""
    b, n, m, _, _ = shape
    rng = np.random.default_rng(_seed(shape, RECIPES.index(recipe) + 1))
    if recipe == "lattice":
        u, k = rng.integers(-4, 5, (b, n, 3)).astype(F) / F(8), rng.integers(-4, 5, (b, m, 3)).astype(F) / F(8)
    else:
        u, k = rng.random((b, n, 3), dtype=F) - F(0.5), rng.random((b, m, 3), dtype=F) - F(0.5)
    if recipe == "dup":
        u = k[:, np.arange(n) % m].copy()
    elif recipe == "same":
        k[:] = k[:, :1]
    elif recipe == "big":
        u, k = u * F(1e3), k * F(1e3)
    elif recipe == "nan":
        k[:, m // 2] = np.nan
    assert u.dtype == F and k.dtype == F
    return np.ascontiguousarray(u), np.ascontiguousarray(k)


def make_feats(shape, integer=False, salt=50):
    """-> known_feats (b,c2,m), unknown_feats (b,c1,n), grad_out (b,c2+c1,n): randn, or small integers"""
    b, n, m, c2, c1 = shape
    rng = np.random.default_rng(_seed(shape, salt + integer))
    dims = ((b, c2, m), (b, c1, n), (b, c2 + c1, n))
    if integer:
        return tuple(rng.integers(-3, 4, d).astype(F) for d in dims)
    return tuple(rng.standard_normal(d).astype(F) for d in dims)

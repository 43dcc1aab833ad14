"""Test helper of the row-layout feature propagation (tests/test_fp_rows_host.py, tests/test_gpu_interp_rows.py,
tests/test_gpu_bn_relu_stats.py): numpy float32 restatements, written from the contract in include/samplenet_hip_internal.h, of
sn_interp_rows_forward (tests/interp_ref.py's weights and interpolation on the row layout, the skip columns beside them), of
sn_interp_rows_backward (tests/gather_inv_ref.py's sequential sum in list order on transposed operands) and of
sn_bn_relu_backward_stats (the activation's mask and the block / slice order of the partial sums), their float64 twins with
counted bounds, the shape tables and a cache that computes every reference once.
Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np

import gather_inv_ref as G
import interp_ref as R

F = np.float32
U = 2.0 ** -24

# (b, n, m, c2, c1)
SHAPES = (
    (1, 1, 1, 1, 0),
    (2, 5, 2, 3, 0),        # m < 3: infinite slots, weight 0
    (2, 65, 3, 5, 3),       # a lane group straddling the c2 boundary
    (2, 257, 65, 16, 1),
    (2, 64, 4, 70, 0),      # more than 64 columns, NULL skip
    (1, 130, 17, 64, 67),   # width 131
    (3, 33, 5, 1, 128),
)
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
RECIPES = ("rand", "lattice", "dup", "same")
INDEX_RECIPES = ("nn", "same", "empty", "oob")


def lane_group(cols):
    """the power of two covering `cols`, 64 at most: lanes per row of both interpolation kernels"""
    lg = 1
    while lg < cols and lg < 64:
        lg *= 2
    return lg


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------ forward
def forward32(known_rows, skip_rows, idx, d2, rule):
    """-> weights (b,n,3), rows (b,n,c2+c1) float32: interp_ref's weights and three-term interpolation, the skip row beside it"""
    w = R.weights(d2, rule)
    kf = np.ascontiguousarray(np.asarray(known_rows, F).transpose(0, 2, 1))           # (b,c2,m)
    out = R.interpolate(kf, idx, w).transpose(0, 2, 1)                                 # (b,n,c2)
    if skip_rows is not None and skip_rows.shape[2]:
        out = np.concatenate([out, np.asarray(skip_rows, F)], axis=2)
    return w, np.ascontiguousarray(out)


def forward64(known_rows, idx, d2, rule):
    """the interpolated columns in float64 on the float32 idx / d2 -> (b,n,c2)"""
    kf = np.asarray(known_rows, np.float64).transpose(0, 2, 1)
    return R.interpolate64(kf, idx, R.weights64(d2, rule)).transpose(0, 2, 1)


_FWD = {}


def forward_case(shape, recipe):
    """the shared, read-only inputs and references of one forward case, both rules"""
    key = (shape, recipe)
    if key not in _FWD:
        b, n, m, c2, c1 = shape
        u, k = R.make_case(shape, recipe)
        idx, d2 = R.three_nn(u, k)
        kf, sf, _ = R.make_feats(shape)
        d = dict(unknown=u, known=k, idx=idx, d2=d2, known_rows=np.ascontiguousarray(kf.transpose(0, 2, 1)),
                 skip_rows=np.ascontiguousarray(sf.transpose(0, 2, 1)))
        for rule in R.RULES:
            d["w%d" % rule], d["rows%d" % rule] = forward32(d["known_rows"], d["skip_rows"], idx, d2, rule)
        _FWD[key] = _frozen(d)
    return _FWD[key]


# ------------------------------------------------------------------------------------------------ backward
def gshape(shape):
    """gather_inv_ref's (b, c, n destination rows, m queries, k) of a (b, n, m, c2, c1) case"""
    b, n, m, c2, c1 = shape
    return (b, c2, m, n, 3)


def backward32(m, c2, weights, grad_rows, start, order):
    """grad_known (b,m,c2) float32: per row the sequential sum from +0, in list order, of fl(grad_rows[e // 3, :c2] * weights[e])"""
    g = np.ascontiguousarray(np.asarray(grad_rows, F)[:, :, :c2].transpose(0, 2, 1))   # (b,c2,n)
    return np.ascontiguousarray(G.backward32(c2, m, 3, weights, g, start, order).transpose(0, 2, 1))


def backward64(m, c2, weights, grad_rows, start, order):
    """-> grad_known (b,m,c2) float64 and its bound (L + 1) * 2^-24 * sum|term| for a row of L entries"""
    g = np.ascontiguousarray(np.asarray(grad_rows, F)[:, :, :c2].transpose(0, 2, 1))
    out, bound = G.backward64(c2, m, 3, weights, g, start, order)
    return out.transpose(0, 2, 1), bound.transpose(0, 2, 1)


_BWD = {}


def backward_case(shape, recipe, integer=False):
    """idx (b,n,3) of gather_inv_ref's recipe, start / order, weights, grad_rows (b,n,c2+c1) and the references; integer: small
    integer weights and gradients, every sum exact"""
    key = (shape, recipe, integer)
    if key not in _BWD:
        b, n, m, c2, c1 = shape
        gs = gshape(shape)
        ref = G.case(gs, recipe)
        rng = np.random.default_rng(G._seed(gs, 40 + G.INDEX_RECIPES.index(recipe) + 100 * integer))
        if integer:
            w, g = rng.integers(-3, 4, (b, n, 3)).astype(F), rng.integers(-3, 4, (b, n, c2 + c1)).astype(F)
        else:
            w = (rng.standard_normal((b, n, 3)) * 10.0 ** rng.uniform(-1, 1, (b, n, 3))).astype(F)
            g = (rng.standard_normal((b, n, c2 + c1)) * 10.0 ** rng.uniform(-1, 1, (b, n, c2 + c1))).astype(F)
        d = dict(idx=ref["idx"], start=ref["start"], order=ref["order"], weights=w, grad_rows=g)
        d["grad32"] = backward32(m, c2, w, g, ref["start"], ref["order"])
        d["grad64"], d["bound"] = backward64(m, c2, w, g, ref["start"], ref["order"])
        _BWD[key] = _frozen(d)
    return _BWD[key]


# ------------------------------------------------------------------------------------------------ top activation backward + sums
BLOCK_ROWS = 256      # csrc/feature_rows.hip: kBsRows, rows per block of partial sums
STATS_R = (1, 63, 64, 65, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 2 * BLOCK_ROWS + 3)
STATS_C = (4, 8, 68, 260)


def stats_blocks(rows):
    return 0 if rows < 1 else -(-rows // BLOCK_ROWS)


def stats_slices(C):
    """S: slices per block.  LR = the power of two covering C / 4, 64 at most; S = 256 / LR"""
    return 256 // lane_group(C // 4)


def mask_dy(z, coef, g):
    """dy = g . [fma(z, scale, shift) > 0] -- the fused multiply-add evaluated in float64 and rounded once: z * scale is exact in
    float64 and the sum's double rounding cannot be told from one rounding by the sign test except at |.| below 2^-149"""
    y = np.asarray(z, np.float64) * np.asarray(coef[0], np.float64) + np.asarray(coef[1], np.float64)
    return np.where(y.astype(F) > 0, np.asarray(g, F), F(0)).astype(F)


def block_sums(dy, z):
    """stats [nblk][2][C] float32 in the kernel's order: per block, slice q adds rows q, q + S, .. ascending from +0, the S slice
    sums are then added in slice order from +0; (sum dy, sum fl(dy * z))"""
    dy, z = np.asarray(dy, F), np.asarray(z, F)
    rows, C = dy.shape
    S = stats_slices(C)
    terms = np.stack([dy, dy * z])                         # (2, rows, C), the product rounded
    assert terms.dtype == F
    out = np.zeros((stats_blocks(rows), 2, C), F)
    for k in range(out.shape[0]):
        blk = terms[:, k * BLOCK_ROWS:(k + 1) * BLOCK_ROWS]
        tot = np.zeros((2, C), F)
        for q in range(S):
            acc = np.zeros((2, C), F)
            for r in range(q, blk.shape[1], S):
                acc = acc + blk[:, r]
            tot = tot + acc
        assert tot.dtype == F
        out[k] = tot
    return out


def block_sums_by_row_loop(dy, z):
    """the same order spelled as one loop over the rows: row r of a block goes to slice r % S"""
    dy, z = np.asarray(dy, F), np.asarray(z, F)
    rows, C = dy.shape
    S = stats_slices(C)
    out = np.zeros((stats_blocks(rows), 2, C), F)
    for k in range(out.shape[0]):
        acc = np.zeros((S, 2, C), F)
        for r in range(k * BLOCK_ROWS, min(rows, (k + 1) * BLOCK_ROWS)):
            q = (r - k * BLOCK_ROWS) % S
            acc[q, 0] = acc[q, 0] + dy[r]
            acc[q, 1] = acc[q, 1] + dy[r] * z[r]
        tot = np.zeros((2, C), F)
        for q in range(S):
            tot = tot + acc[q]
        out[k] = tot
    return out


def block_sum_roundings(C):
    """roundings behind one element of a block's sum, to first order: the product, ceil(256 / S) adds of a slice, S adds of slices"""
    S = stats_slices(C)
    return 1 + -(-BLOCK_ROWS // S) + S


def stats_case(rows, C, seed=0):
    """z, g (rows, C), coef (4, C): scales of both signs, mean and invstd as a BatchNorm's; about half the activations are off"""
    rng = np.random.default_rng(rows * 1009 + C * 17 + seed)
    z = rng.standard_normal((rows, C)).astype(F)
    g = rng.standard_normal((rows, C)).astype(F)
    coef = np.stack([(rng.random(C) + 0.5) * np.where(np.arange(C) % 3 == 0, -1, 1), rng.standard_normal(C) * 0.3,
                     rng.standard_normal(C) * 0.2, rng.random(C) + 0.5]).astype(F)
    return z, coef, g

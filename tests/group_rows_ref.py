"""Test helper of the set-abstraction entries (tests/test_group_rows_host.py, tests/test_gpu_group_rows.py,
tests/test_gpu_group_pool.py): numpy restatements written from the contracts in include/samplenet_hip_internal.h -- the row-layout
grouping on tests/ball_ref.py's index rows, the sequential float32 sum over a destination row's entries in ascending order, the
lane-strided + xor-tree sum of the centre's gradient, the group max-pool with first-row ties and the min route -- and the shape
tables and recipes of the GPU tests.  Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np

import ball_ref as R

F = np.float32
U = 2.0 ** -24

# (b, n, m, nsample)
SHAPES = (
    (1, 1, 1, 1),
    (2, 70, 5, 3),
    (2, 200, 33, 69),     # more slots than lanes
    (3, 257, 9, 16),
    (500, 3, 17, 2),      # several queries per wave (8500 queries)
    (1, 16385, 2, 2),
)
CHANNELS = ((0, 1), (1, 0), (1, 1), (5, 1), (67, 0), (131, 1))  # (c, use_xyz)


def empty(shape, _=None):
    """every ball empty: the dataset lies beyond 10, the queries in the unit cube, radius 0.1 -- every slot names point 0"""
    b, n, m, _ns = shape
    rng = np.random.default_rng(R._seed(shape, 8))
    return rng.random((b, n, 3), dtype=F) + F(10), rng.random((b, m, 3), dtype=F), F(0.1)


RECIPES = [r for r in R.RECIPES if r[0] in ("uniform-0.3", "grid-2", "clusters", "fill-lastn")] + [("empty", empty, None)]


def group_rows(xyz, new_xyz, feat_bnc, idx, use_xyz):
    """-> (b, m, nsample, 3 use_xyz + c) float32: xyz[idx] - new_xyz (one float32 subtraction), then feat_bnc[idx]."""
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    ar = np.arange(xyz.shape[0])[:, None, None]
    parts = []
    if use_xyz:
        g = xyz[ar, idx] - new_xyz[:, :, None, :]
        assert g.dtype == F
        parts.append(g)
    if feat_bnc is not None and feat_bnc.shape[2] > 0:
        parts.append(np.asarray(feat_bnc, F)[ar, idx])
    return np.ascontiguousarray(np.concatenate(parts, axis=3))


def invert(idx_flat, n):
    """sn_gather_invert's lists: per cloud (start (n+1,), order (ne,)) -- the valid entries by a stable sort of their index."""
    out = []
    for row in np.asarray(idx_flat):
        valid = np.flatnonzero((row >= 0) & (row < n))
        order = valid[np.argsort(row[valid], kind="stable")]
        start = np.concatenate([[0], np.cumsum(np.bincount(row[valid], minlength=n))])
        out.append((start.astype(np.int64), order.astype(np.int64)))
    return out


def sequential_sum(n, idx_flat, grad):
    """idx_flat (b,ne), grad (b,ne,C) float32 -> (b,n,C) float32: per destination row the sum, from +0, of the entries that name it
    in ascending entry order, every add rounded to float32.  Step t adds the t-th entry of every list at once (distinct rows)."""
    grad = np.asarray(grad, F)
    b, ne, C = grad.shape
    out = np.zeros((b, n, C), F)
    for i, (start, order) in enumerate(invert(idx_flat, n)):
        rows = np.asarray(idx_flat[i])[order]
        rank = np.arange(len(order)) - start[rows]
        for t in range(int(rank.max()) + 1 if len(order) else 0):
            sel = rank == t
            out[i, rows[sel]] = out[i, rows[sel]] + grad[i, order[sel]]
    assert out.dtype == F
    return out


def sequential_sum_by_lists(n, idx_flat, grad):
    """the same, list by list as the contract reads: what sequential_sum abbreviates"""
    grad = np.asarray(grad, F)
    b, ne, C = grad.shape
    out = np.zeros((b, n, C), F)
    for i, (start, order) in enumerate(invert(idx_flat, n)):
        for r in range(n):
            acc = np.zeros(C, F)
            for e in order[start[r]:start[r + 1]]:
                acc = acc + grad[i, e]
            out[i, r] = acc
    return out


def scatter_f64(n, idx_flat, grad):
    """float64 sums, the sums of |terms| and the list lengths (b,n) behind sequential_sum"""
    g = np.asarray(grad, np.float64)
    b, ne, C = g.shape
    s, sab, mult = np.zeros((b, n, C)), np.zeros((b, n, C)), np.zeros((b, n))
    cloud = np.arange(b)[:, None]
    np.add.at(s, (cloud, idx_flat), g)
    np.add.at(sab, (cloud, idx_flat), np.abs(g))
    np.add.at(mult, (cloud, idx_flat), 1.0)
    return s, sab, mult


def centre_sum(grad_xyz_rows):
    """grad_xyz_rows (b,m,nsample,3) float32 -> (b,m,3) float32: lane l of 64 adds slots l, l + 64, .. ascending from +0, the lane
    sums meet by the xor tree (offsets 32, 16, .. 1; both partners form a + b, which commutes), one negation."""
    g = np.asarray(grad_xyz_rows, F)
    b, m, ns, _ = g.shape
    lanes = np.zeros((b, m, 64, 3), F)
    for s in range(ns):
        lanes[:, :, s % 64] = lanes[:, :, s % 64] + g[:, :, s]
    o = 32
    while o:
        lanes = lanes + lanes[:, :, np.arange(64) ^ o]
        o >>= 1
    assert lanes.dtype == F
    return -lanes[:, :, 0]


def group_pool(z, scale, shift):
    """z (G,S,C), scale / shift (C,) float32 -> pooled (G,C), argsel (G,C) int32, zsel (G,C): per channel the maximum (scale >= 0) or
    minimum (scale < 0) over the S rows, the FIRST row on a tie (numpy's argmax / argmin), pooled = relu(fma(zsel, scale, shift)) --
    the fma through float64 (the product is exact there; the sum is rounded twice, which can differ from one rounding in the last
    bit only when the float64 sum lies within 2^-53 relative of a float32 tie: the GPU tests hold pooled to sn_pool_forward)."""
    z = np.asarray(z, F)
    up = np.asarray(scale, F) >= 0
    arg = np.where(up[None, :], z.argmax(1), z.argmin(1))
    zsel = np.take_along_axis(z, arg[:, None, :], 1)[:, 0]
    v = (zsel.astype(np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)).astype(F)
    return np.where(v < 0, F(0), v).astype(F), arg.astype(np.int32), zsel


def pool_case(G, S, C, seed):
    """z with planted ties 1 and S - 1 rows apart at the extreme of some channels, scales of both signs (channel 0 negative)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((G, S, C)).astype(F)
    scale = (rng.random(C) + 0.5).astype(F) * np.where(np.arange(C) % 3 == 0, F(-1), F(1)).astype(F)
    shift = (rng.standard_normal(C) * 0.3).astype(F)
    if S >= 2:
        for gi in range(G):
            for c in range(0, C, 2):      # the extreme twice: rows 0 and S - 1 (S - 1 apart), or rows r and r + 1
                big = F(9.0) if scale[c] >= 0 else F(-9.0)
                if (gi + c // 2) % 2 == 0:
                    z[gi, 0, c] = z[gi, S - 1, c] = big
                else:
                    r = (gi + c) % (S - 1)
                    z[gi, r, c] = z[gi, r + 1, c] = big
    return z, scale, shift

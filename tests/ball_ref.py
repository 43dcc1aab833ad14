"""Test helper of the ball-query entries (tests/test_ball_host.py, tests/test_gpu_ball_query.py, tests/test_gpu_ball_group.py): a numpy
float32 restatement of sn_ball_query's two rules written from the contract in include/samplenet_hip_internal.h -- the semantics of
query_ball_point_gpu / query_ball_point_cpu (classification/grouping/tf_grouping_g.cu:3-36, test/query_ball_point.cpp:19-47; the
comparison is :24-25 / :32-33, the first-hit padding :26-29 / :34-37, the early stop :16-17 / :24-25) --, the grouped tensor of
sn_ball_group_forward, float64 gradient references with per-element multiplicities, the input recipes and the shape table.
Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np

SQRT, SQUARED = 0, 1  # SN_BALL_RULE_*
RULES = (SQRT, SQUARED)
BNC, BCN = 0, 1
F = np.float32

WAVES_PER_WORKGROUP = 4  # csrc/ball_query.hip: kBallWaves


def queries_per_wave(b, m):
    """csrc/ball_query.hip: ball_queries_per_wave -- one query per wave up to 8192 queries (the chip's wave slots), then 2, 3, 4"""
    return min(4, max(1, -(-(b * m) // 8192)))


# (b, n, m, nsample), the branch the row exercises, the (layout1, layout2) pairs it runs under.  The kernel stages no dataset tile,
# so there is no "one past the tile" row.  A workgroup holds 4 x queries_per_wave queries: the rows marked 2W+1 have m one more than
# twice that, at each of the three values the launch rule takes in this table (tests/test_ball_host.py asserts it).
_ALL = ((BNC, BNC), (BCN, BNC), (BNC, BCN), (BCN, BCN))
SHAPES = (
    ((1, 1, 1, 1), "one point, one query, one slot: a single masked round", ((BNC, BNC),)),
    ((2, 63, 5, 4), "one round with a masked tail lane; a second wave with one query", _ALL),
    ((2, 64, 4, 64), "one full round, a row as wide as the wave, one wave", ((BNC, BNC),)),
    ((2, 65, 7, 3), "a second round of one lane; two waves, the second short", _ALL),
    ((1, 130, 1, 1), "three rounds, exit after the first hit", ((BNC, BNC),)),
    ((2, 200, 33, 70), "rows wider than a wave (strided padding), m = 2 workgroups + 1", ((BNC, BNC),)),
    ((3, 257, 9, 16), "five rounds, the last of one lane; 2W+1 at one query per wave: a third workgroup with one query", _ALL),
    ((1, 40, 33, 5), "nine workgroups, the last with one query", ((BNC, BNC),)),
    ((500, 3, 17, 2), "2W+1 at two queries per wave (8500 queries)", ((BNC, BNC),)),
    ((800, 2, 33, 1), "2W+1 at four queries per wave (26400 queries)", ((BNC, BNC), (BCN, BCN))),
)
TWO_W_PLUS_ONE = ((3, 257, 9, 16), (500, 3, 17, 2), (800, 2, 33, 1))


# ------------------------------------------------------------------------------------------------ the restatement
def dist2(xyz1, xyz2):
    """d2[b,j,k] = ((dx*dx) + (dy*dy)) + (dz*dz), differences query - dataset, every operation in float32."""
    P, Q = np.asarray(xyz1, F), np.asarray(xyz2, F)
    d = [Q[:, :, None, c] - P[:, None, :, c] for c in range(3)]
    assert all(x.dtype == F for x in d)
    return ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])


def passes(d2, radius, rule):
    radius = F(radius)
    with np.errstate(invalid="ignore"):
        if rule == SQRT:
            s = np.sqrt(d2)  # float32 in, float32 out: correctly rounded
            assert s.dtype == F
            s = np.where(s < F(1e-20), F(1e-20), s)  # std::max(s, 1e-20f): a NaN stays
            return s < radius
        if not radius > 0:
            return np.zeros(d2.shape, bool)
        return d2 < F(radius * radius)


def ball_query(xyz1, xyz2, radius, nsample, rule):
    """xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries -> idx (b,m,nsample) int32, pts_cnt (b,m) int32; empty balls are rows of zeros."""
    ok = passes(dist2(xyz1, xyz2), radius, rule)
    b, m, n = ok.shape
    cnt = np.minimum(ok.sum(-1), nsample).astype(np.int32)
    order = np.argsort(~ok, axis=-1, kind="stable")[:, :, :nsample]    # the passing indices first, ascending (a stable sort)
    order = np.pad(order, ((0, 0), (0, 0), (0, nsample - order.shape[2])))
    first = np.where(cnt > 0, order[:, :, 0], 0)                         # an empty ball: zeros
    idx = np.where(np.arange(nsample) < cnt[:, :, None], order, first[:, :, None])
    return idx.astype(np.int32), cnt


def ball_query_by_loop(xyz1, xyz2, radius, nsample, rule):
    """the same, row by row as the reference's loop reads (test/query_ball_point.cpp:22-41): what ball_query abbreviates"""
    ok = passes(dist2(xyz1, xyz2), radius, rule)
    b, m, n = ok.shape
    idx, cnt = np.zeros((b, m, nsample), np.int32), np.zeros((b, m), np.int32)
    for i in range(b):
        for j in range(m):
            hits = np.flatnonzero(ok[i, j])[:nsample]
            if len(hits):
                idx[i, j] = hits[0]
                idx[i, j, :len(hits)] = hits
                cnt[i, j] = len(hits)
    return idx, cnt


def group(xyz, new_xyz, features, idx, use_xyz):
    """-> (b, 3 use_xyz + c, m, nsample) float32: xyz[idx] - new_xyz (one float32 subtraction), then features[:, :, idx]."""
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    b = xyz.shape[0]
    ar = np.arange(b)[:, None, None]
    parts = []
    if use_xyz:
        g = xyz[ar, idx] - new_xyz[:, :, None, :]          # (b,m,ns,3)
        assert g.dtype == F
        parts.append(g.transpose(0, 3, 1, 2))
    if features is not None and features.shape[1] > 0:
        f = np.asarray(features, F).transpose(0, 2, 1)     # (b,n,c)
        parts.append(f[ar, idx].transpose(0, 3, 1, 2))
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def group_backward(n, c, use_xyz, idx, grad_out):
    """float64 gradients of group() for grad_out (b, 3 use_xyz + c, m, ns): a dict with grad_features (b,c,n), grad_xyz (b,n,3),
    grad_new_xyz (b,m,3), the sums of |terms| behind each (abs_*), and mult (b,n): how many slots name each dataset point."""
    idx = np.asarray(idx).astype(np.int64)
    g = np.asarray(grad_out, np.float64)
    b, m, ns = idx.shape
    u = 3 if use_xyz else 0
    out = {k: np.zeros((b, c, n)) for k in ("grad_features", "abs_features")}
    out.update({k: np.zeros((b, n, 3)) for k in ("grad_xyz", "abs_xyz")})
    out["mult"] = np.zeros((b, n))
    flat = idx.reshape(b, m * ns)
    cloud = np.arange(b)[:, None]
    np.add.at(out["mult"], (cloud, flat), 1.0)
    if use_xyz:
        src = g[:, :3].reshape(b, 3, m * ns).transpose(0, 2, 1)
        np.add.at(out["grad_xyz"], (cloud, flat), src)
        np.add.at(out["abs_xyz"], (cloud, flat), np.abs(src))
    if c:
        src = g[:, u:].reshape(b, c, m * ns)
        where = (cloud[:, :, None], np.arange(c)[None, :, None], flat[:, None, :])
        np.add.at(out["grad_features"], where, src)
        np.add.at(out["abs_features"], where, np.abs(src))
    gx = g[:, :3] if use_xyz else np.zeros((b, 3, m, ns))
    out["grad_new_xyz"] = -gx.sum(-1).transpose(0, 2, 1)
    out["abs_new_xyz"] = np.abs(gx).sum(-1).transpose(0, 2, 1)
    return out


# ------------------------------------------------------------------------------------------------ recipes
def _seed(shape, salt):
    b, n, m, ns = shape
    return ((b * 1009 + n) * 1013 + m) * 1019 + ns + 7919 * salt


def uniform(shape, radius):
    """1: uniform [0,1)^3 -- radius 0.05 mostly empty or short balls, 0.3 mixed, 2.0 every point in the ball."""
    b, n, m, _ = shape
    rng = np.random.default_rng(_seed(shape, 1))
    return rng.random((b, n, 3), dtype=F), rng.random((b, m, 3), dtype=F), F(radius)


_GRID_OFFSET = {1: (1, 0, 0), 2: (0, 2, 0), 3: (1, 2, 2), 5: (3, 4, 0)}


def grid(shape, radius):
    """2: integer grid [-4,4]^3, radius 1, 2, 3 or 5.  Distances equal to the radius occur; one is forced: query 0 sits at the
    origin and the last dataset point at an offset of exactly that length -- (3,4,0) for 5 --, excluded under both rules."""
    b, n, m, _ = shape
    rng = np.random.default_rng(_seed(shape, 2))
    P, Q = rng.integers(-4, 5, (b, n, 3)).astype(F), rng.integers(-4, 5, (b, m, 3)).astype(F)
    Q[:, 0] = 0
    P[:, n - 1] = _GRID_OFFSET[int(radius)]
    return P, Q, F(radius)


# 3: the seed per shape, chosen on the CPU so that the two rules give query 0 of cloud 0 different rows (tests/test_ball_host.py
# asserts it): the radius is the realised float32 distance r = sqrt(d2) from query 0 to its nearest dataset point, which the
# reference's rule excludes (r < r is false) and the squared rule includes exactly when fl(r * r) > d2
BOUNDARY_SEEDS = {(1, 1, 1, 1): 1000, (2, 63, 5, 4): 1002, (2, 64, 4, 64): 1002, (2, 65, 7, 3): 1000, (1, 130, 1, 1): 1002,
                  (2, 200, 33, 70): 1002, (3, 257, 9, 16): 1008, (1, 40, 33, 5): 1004, (500, 3, 17, 2): 1002,
                  (800, 2, 33, 1): 1009}


def boundary(shape, seed=None):
    b, n, m, _ = shape
    rng = np.random.default_rng(BOUNDARY_SEEDS[shape] if seed is None else seed)
    P, Q = rng.random((b, n, 3), dtype=F), rng.random((b, m, 3), dtype=F)
    d2 = dist2(P[:1], Q[:1, :1])[0, 0]
    return P, Q, np.sqrt(d2.min())


def rules_differ(P, Q, radius, nsample):
    """a query's result (its index row or its count: a one-point cloud has only index 0 to give) differs between the rules"""
    a, ca = ball_query(P, Q, radius, nsample, SQRT)
    c, cc = ball_query(P, Q, radius, nsample, SQUARED)
    return bool(((a != c).any(axis=2) | (ca != cc)).any())


def copies(shape, radius):
    """4: queries copied from the dataset (d = 0), radius 1e-20, 1e-19 or 1e-3: the reference's 1e-20 floor."""
    b, n, m, _ = shape
    P = np.random.default_rng(_seed(shape, 4)).random((b, n, 3), dtype=F)
    return P, P[:, np.arange(m) % n].copy(), F(radius)


def clusters(shape, _=None):
    """5: the first min(n, 64) dataset points coincide and every other query sits on them: the ball overflows nsample inside the
    first round (nsample < 64), or fills it exactly there (nsample = 64)."""
    b, n, m, _ns = shape
    rng = np.random.default_rng(_seed(shape, 5))
    P, Q = rng.random((b, n, 3), dtype=F), rng.random((b, m, 3), dtype=F)
    P[:, :min(n, 64)] = P[:, :1]
    Q[:, ::2] = P[:, :1]
    return P, Q, F(0.1)


def fill(shape, variant):
    """6: late and exact fill.  Every dataset point is far away (beyond 10) except the chosen ones, which lie within 0.02 of the
    queries; radius 0.5.  "late": the only hits are the last three indices.  "last63" / "last64" / "lastn": exactly nsample hits
    (fewer where the cloud has fewer points up to there) whose last sits at index min(63, n-1), min(64, n-1) or n-1."""
    b, n, m, ns = shape
    rng = np.random.default_rng(_seed(shape, 6))
    P = rng.random((b, n, 3), dtype=F) + F(10)
    Q = (rng.random((b, m, 3), dtype=F) * F(0.01)).astype(F)
    if variant == "late":
        near = np.arange(max(n - 3, 0), n)
    else:
        last = min({"last63": 63, "last64": 64, "lastn": n - 1}[variant], n - 1)
        near = np.sort(np.append(rng.choice(last, min(ns - 1, last), replace=False), last)).astype(np.int64)
    P[:, near] = (rng.random((b, len(near), 3), dtype=F) * F(0.01)).astype(F)
    return P, Q, F(0.5)


RECIPES = ([("uniform-%g" % r, uniform, r) for r in (0.05, 0.3, 2.0)] + [("grid-%d" % r, grid, r) for r in (1, 2, 3, 5)] +
           [("boundary", boundary, None)] + [("copies-%g" % r, copies, r) for r in (1e-20, 1e-19, 1e-3)] +
           [("clusters", clusters, None)] + [("fill-" + v, fill, v) for v in ("late", "last63", "last64", "lastn")])
RECIPE_IDS = [r[0] for r in RECIPES]


def make_case(shape, recipe):
    """-> xyz1 (b,n,3), xyz2 (b,m,3) float32, radius (float32 scalar)."""
    _, fn, arg = recipe
    P, Q, r = fn(shape, arg)
    assert P.dtype == F and Q.dtype == F and P.shape == (shape[0], shape[1], 3) and Q.shape == (shape[0], shape[2], 3)
    return P, Q, F(r)


def lay(x, layout):
    """(b,n,3) -> contiguous array in the selected layout."""
    return np.ascontiguousarray(x if layout == BNC else x.transpose(0, 2, 1))

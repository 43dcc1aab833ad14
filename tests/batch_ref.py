"""Numpy restatement of sn_batch_assemble, written from the text above its prototype in include/samplenet_hip_internal.h (item order,
Philox draw layout, the nine stages) -- it calls nothing of the library.  Integers (items, labels, point order, dropout's choice, the
clips) are reproduced exactly; the float stages are evaluated in fp64 from the exact 24-bit uniforms, and every value carries an
ERROR BOUND for the kernel's fp32 result counted operation by operation: one rounding (2^-24 relative) per fp32 operation the header
writes out, inherited errors propagated to first order plus their products, and for each library call (logf, sqrtf, sincosf) an
allowance in ulps of its result (ULPS below; tests/test_gpu_batch_assemble.py sets it from the measured figures).

Imported by tests/test_batch_host.py and tests/test_gpu_batch_assemble.py."""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
TINY = 2.0 ** -149      # one subnormal step: what an underflowing product may lose
TWO_PI = float(np.float32(6.28318530717958647692))  # the fp32 constant the header names, as a number
# Allowed error of the device's library calls, in ulps of the result (1 ulp <= 2^-23 |result|).  The defaults are the bounds HIP's
# math API documents for its fp32 functions (logf 1, sinf / cosf 1 -- sincosf is the pair --, sqrtf 1), doubled.
ULPS = {"logf": 2.0, "sqrtf": 2.0, "sincosf": 2.0}
STREAM_SORT, STREAM_JITTER, STREAM_DROPOUT, STREAM_PAIR_NOISE, STREAM_CLOUD, STREAM_ANGLES, STREAM_ORDER = range(7)
THREADS = 256


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Counter words and key words (anything that broadcasts) -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & 0xFFFFFFFF for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # (32 x 32 bits: fits 64)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def draw(index, stream, item, epoch, seed):
    return philox(index, stream, item, int(epoch) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)


def uniform(x):
    """Exact: a 24-bit integer times 2^-24 (also exact as float32)."""
    return (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


# ---- the item order --------------------------------------------------------------------------------------------------------------
def feistel_bits(lset):
    k = 2
    while (1 << k) < lset:
        k += 2
    return k


def _mix(v):
    v ^= v >> 16
    v = (v * 0x7FEB352D) & 0xFFFFFFFF
    v ^= v >> 15
    v = (v * 0x846CA68B) & 0xFFFFFFFF
    return v ^ (v >> 16)


def perm(seed, epoch, x, lset):
    """The keyed bijection of [0, lset) at one point, and the number of Feistel applications the cycle walk took."""
    h = feistel_bits(lset) // 2
    mask = (1 << h) - 1
    rk = [int(w) for w in draw(0, STREAM_ORDER, 0, epoch, seed)]
    steps = 0
    while True:
        l, r = x >> h, x & mask
        for i in range(4):
            l, r = r, l ^ (_mix((r + rk[i]) & 0xFFFFFFFF) & mask)
        x = (l << h) | r
        steps += 1
        if x < lset:
            return x, steps


def item_at(seed, g, lset, sequential=False):
    """-> (item, epoch) of global position g."""
    epoch, r = divmod(g, lset)
    return (r if sequential else perm(seed, epoch, r, lset)[0]), epoch


# ---- values with error bounds ----------------------------------------------------------------------------------------------------
class V:
    """fp64 value(s) with a bound on |the kernel's fp32 value - this value|."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def _rounded(self, v, prop):
        return V(v, prop + U * (np.abs(v) + prop) + TINY)

    def __add__(self, o):
        o = V.of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = V.of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = V.of(o)
        den = np.abs(o.v) - o.e
        assert np.all(den > 0), "divisor not bounded away from zero"
        q = self.v / o.v
        return self._rounded(q, (self.e + np.abs(q) * o.e) / den)

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.e)

    def clip(self, c):
        """min(max(x, -c), c): exact operations, 1-Lipschitz; a value beyond the clip by more than its error gives the clip exactly."""
        return V(np.clip(self.v, -c, c), np.where(np.abs(self.v) - self.e >= c, 0.0, self.e))

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])


def _lib_err(name, val):
    return ULPS[name] * 2.0 * U * np.abs(val)


def v_log(a):
    assert np.all(a.v - a.e > 0)
    val = np.log(a.v)
    return V(val, a.e / (a.v - a.e) + _lib_err("logf", val))


def v_sqrt(a):
    val = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(a.e > 0, np.minimum(np.sqrt(a.e), a.e / np.where(val > 0, val, 1.0)), 0.0)
    return V(val, prop + _lib_err("sqrtf", val))


def v_sincos(a):
    s, c = np.sin(a.v), np.cos(a.v)
    return V(s, a.e + _lib_err("sincosf", s)), V(c, a.e + _lib_err("sincosf", c))


def gauss2(xa, xb):
    u1 = ((np.asarray(xa, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = uniform(xb)
    rad = v_sqrt(V(-2.0) * v_log(V(u1)))
    s, c = v_sincos(V(TWO_PI) * V(u2))
    return rad * c, rad * s


def gauss3(x):
    g0, g1 = gauss2(x[0], x[1])
    g2, _ = gauss2(x[2], x[3])
    return g0, g1, g2


def _f32(x):
    return float(np.float32(x))


# ---- the recipe ------------------------------------------------------------------------------------------------------------------
class Recipe:
    """The stages as plain fields (the names of samplenet_amd.device_data.BatchRecipe: either object serves)."""

    def __init__(self, order="shuffled", shuffle_points=False, unit_cube=False, scale=None, rotate_axis=None, perturb=None,
                 translate=None, jitter=None, dropout=None, pair_noise=None):
        self.order, self.shuffle_points, self.unit_cube, self.scale, self.rotate_axis = order, shuffle_points, unit_cube, scale, rotate_axis
        self.perturb, self.translate, self.jitter, self.dropout, self.pair_noise = perturb, translate, jitter, dropout, pair_noise


def unit_cube(x):
    """Stage 2 on V points (N, 3)."""
    n = x.v.shape[0]
    ext = V(x.v.max(0), x.e.max(0)) - V(x.v.min(0), x.e.max(0))
    k = int(np.argmax(ext.v))
    s = V(ext.v[k], ext.e.max())
    v = x / s
    depth = (n + THREADS - 1) // THREADS + 8  # additions a term passes through: its thread's chain, six xor steps, three wave sums
    tot = v.v.sum(0)
    tot_e = v.e.sum(0) + 1.01 * depth * U * (np.abs(v.v).sum(0) + v.e.sum(0))
    mean = V(tot, tot_e) / V(float(n))
    return v - V(mean.v[None, :], mean.e[None, :])


def axis_matrix(axis, s, c):
    """Stage 4's R from the recipe's axis (fp32 values) and V sine / cosine -> 3 x 3 nested list of V."""
    a64 = np.asarray([_f32(t) for t in axis], dtype=np.float64)
    a = (a64 / np.sqrt((a64 * a64).sum())).astype(np.float32).astype(np.float64)  # normalised in fp64, rounded to fp32: exact here
    K = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    t = V(1.0) - c
    return [[(c * V(1.0 if i == j else 0.0) + s * V(K[i][j])) + (t * V(a[i])) * V(a[j]) for j in range(3)] for i in range(3)]


def apply_matrix(R, x):
    cols = [x[:, 0], x[:, 1], x[:, 2]]
    out = [(R[i][0] * cols[0] + R[i][1] * cols[1]) + R[i][2] * cols[2] for i in range(3)]
    return V(np.stack([o.v for o in out], 1), np.stack([o.e for o in out], 1))


def perturb_apply(sc, x):
    """Stage 5: sc = [(s, c)] about x, y, z; three plane rotations."""
    px, py, pz = x[:, 0], x[:, 1], x[:, 2]
    (s, c) = sc[0]
    py, pz = c * py - s * pz, s * py + c * pz
    (s, c) = sc[1]
    px, pz = c * px + s * pz, c * pz - s * px
    (s, c) = sc[2]
    px, py = c * px - s * py, s * px + c * py
    return V(np.stack([px.v, py.v, pz.v], 1), np.stack([px.e, py.e, pz.e], 1))


def perturb_matrix(angles):
    """Rz Ry Rx as a plain fp64 matrix (what perturb_apply applies)."""
    x = V(np.eye(3))
    sc = [(V(np.sin(a)), V(np.cos(a))) for a in angles]
    return perturb_apply(sc, x).v.T


def qrot(q, x):
    """sn_qrot_forward's expression on V points (N, 3); q: four fp32 values (w, x, y, z)."""
    w, u = V(float(q[0])), [V(float(t)) for t in q[1:]]
    p = [x[:, 0], x[:, 1], x[:, 2]]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
    uv = cross(u, p)
    uuv = cross(u, uv)
    out = [p[c] + V(2.0) * (w * uv[c] + uuv[c]) for c in range(3)]
    return V(np.stack([o.v for o in out], 1), np.stack([o.e for o in out], 1))


def point_order(seed, item, epoch, n):
    keys = draw(np.arange(n), STREAM_SORT, item, epoch, seed)[0].astype(np.uint64)
    comp = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return (np.sort(comp) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def cloud(points, item, epoch, recipe, n, seed, quat=None):
    """One output cloud.  points (P, 3) float32: the item's cloud.  -> dict with order (n), p0 / p1 as V (n, 3), dropped (n) bool,
    jitter / angles (the clipped draws, V) where the stage is on."""
    rc, out = recipe, {}
    order = point_order(seed, item, epoch, n) if rc.shuffle_points else np.arange(n)
    x = V(points[order].astype(np.float64))
    cs = draw(0, STREAM_CLOUD, item, epoch, seed)
    if rc.unit_cube:
        x = unit_cube(x)
    if rc.scale is not None:
        lo, hi = _f32(rc.scale[0]), _f32(rc.scale[1])
        x = x * (V(lo) + V(uniform(cs[0])) * (V(hi) - V(lo)))
    if rc.rotate_axis is not None:
        s, c = v_sincos(V(uniform(cs[1])) * V(TWO_PI))
        x = apply_matrix(axis_matrix(rc.rotate_axis, s, c), x)
    if rc.perturb is not None:
        sigma, clip = _f32(rc.perturb[0]), _f32(rc.perturb[1])
        ang = [(V(sigma) * g).clip(clip) for g in gauss3(draw(0, STREAM_ANGLES, item, epoch, seed))]
        out["angles"] = ang
        x = perturb_apply([v_sincos(a) for a in ang], x)
    if rc.translate is not None:
        t = _f32(rc.translate)
        x = x + (V(uniform(cs[2])) * (V(t) + V(t)) - V(t))
    if rc.jitter is not None:
        std, clip = _f32(rc.jitter[0]), _f32(rc.jitter[1])
        g = gauss3(draw(np.arange(n), STREAM_JITTER, item, epoch, seed))
        d = [(V(std) * t).clip(clip) for t in g]
        x = x + V(np.stack([t.v for t in d], 1), np.stack([t.e for t in d], 1))
    dropped = np.zeros(n, dtype=bool)
    if rc.dropout is not None and n > 0:
        ratio = np.float32(uniform(cs[3])) * np.float32(rc.dropout)  # one fp32 product: the kernel's, bit for bit
        uj = uniform(draw(np.arange(n), STREAM_DROPOUT, item, epoch, seed)[0]).astype(np.float32)
        dropped = uj <= ratio
        x = V(np.where(dropped[:, None], x.v[0], x.v), np.where(dropped[:, None], x.e[0], x.e))
    out.update(order=order, p0=x, dropped=dropped)
    if quat is not None:
        y = qrot(quat, x)
        if rc.pair_noise is not None:
            g = gauss3(draw(np.arange(n), STREAM_PAIR_NOISE, item, epoch, seed))
            d = [V(_f32(rc.pair_noise)) * t for t in g]
            y = y + V(np.stack([t.v for t in d], 1), np.stack([t.e for t in d], 1))
        out["p1"] = y
    return out


def batch(points, labels, recipe, B, n, seed=0, rank=0, world=1, position=0, repeat=1, pair_quat=None):
    """The batch at `position`.  -> dict: items (B), labels (B), order (B, n), p0 / p0_err (B, n, 3) [, p1 / p1_err, igt (B, 7)],
    dropped (B, n)."""
    L = points.shape[0]
    lset = L * repeat
    res = {k: [] for k in ("items", "labels", "order", "p0", "p0_err", "p1", "p1_err", "igt", "dropped")}
    for b in range(B):
        item, epoch = item_at(seed, position + rank * B + b, lset, recipe.order == "sequential")
        c = cloud(points[item % L], item, epoch, recipe, n, seed, None if pair_quat is None else pair_quat[item])
        res["items"].append(item)
        res["labels"].append(int(labels[item % L]))
        res["order"].append(c["order"])
        res["dropped"].append(c["dropped"])
        res["p0"].append(c["p0"].v)
        res["p0_err"].append(c["p0"].e)
        if pair_quat is not None:
            res["p1"].append(c["p1"].v)
            res["p1_err"].append(c["p1"].e)
            res["igt"].append(np.concatenate([np.asarray(pair_quat[item], dtype=np.float32), np.zeros(3, np.float32)]))
    return {k: np.asarray(v) for k, v in res.items() if v}


# ---- the fixed pair table (qdataset.py:122-145) ----------------------------------------------------------------------------------
def fixed_pair_quaternions(lset, seed=0, max_deg=45.0):
    """np.random.seed(seed); per item: uniform(-max, max, [1, 3]) Euler angles, then the never-used translation draw
    uniform(-0, 0, [1, 3]); Euler "xyz" -> quaternion (w, x, y, z): the product qx qy qz, negated (quaternion.py:166-210), in fp64,
    cast to float32.  Uses numpy's GLOBAL generator like the reference."""
    mx = np.pi / 180 * max_deg
    np.random.seed(seed)
    out = np.empty((lset, 4), dtype=np.float64)

    def qmul(q, r):  # Hamilton product
        return np.array([q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3], q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2],
                         q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1], q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0]])

    for i in range(lset):
        e = np.random.uniform(-mx, mx, [1, 3])[0]
        np.random.uniform(-0.0, 0.0, [1, 3])
        qx = np.array([np.cos(e[0] / 2), np.sin(e[0] / 2), 0.0, 0.0])
        qy = np.array([np.cos(e[1] / 2), 0.0, np.sin(e[1] / 2), 0.0])
        qz = np.array([np.cos(e[2] / 2), 0.0, 0.0, np.sin(e[2] / 2)])
        out[i] = -qmul(qmul(qx, qy), qz)
    return out.astype(np.float32)

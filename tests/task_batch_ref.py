"""Test helper for tests/test_gpu_task_batch.py: the shape tables, input recipes and plain references of the one-batch task
evaluation (sn_cyclic_pad_cat*, sn_chamfer_forward_valid, sn_chamfer_mean_loss_*_grouped, sn_pcrnet_head_rot_*[_grouped]).  The fp64
restatements of the PCRNet head, the quaternion rotation and the Chamfer-mean loss are tests/cabi_ref.py's; what is added here is
what those entries do on top: the cyclic copies (plain indexing), their gradient (a sequential sum, in float32 as the kernel adds and
in float64), the nearest-neighbour scan as float32 numpy, and the rounding bounds counted from the kernels' own operations.  Every
table says which branch of the code each row reaches.  Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np
import torch

import cabi_ref as R

U = 2.0 ** -24  # unit roundoff of float32

# ------------------------------------------------------------------------------------------------ 1. cyclic padding
# (B, C, sizes): len = max(sizes).  The pad kernels launch min((len C + 255) / 256, 16) workgroups of 256 threads per cloud.
PAD_CASES = (
    (1, 1, (1,)),                      # smallest case: one workgroup, one element, no copies (size == len)
    (5, 3, (3, 7, 8, 20)),             # sizes that do not divide len: the last round of copies is partial
    (2, 4, tuple(range(1, 17))),       # 16 clouds (kMaxPrefixes); size 1: every point of the padded cloud is the same row, 16 terms a sum
    (4, 3, (32, 64, 128, 256)),        # the BASELINE configs[4] prefix ladder
    (3, 64, (5, 70)),                  # len C = 4480 > 16 x 256 = 4096: the strided loop takes a second trip (forward and, for 70, backward)
    (2, 3, (1500, 2048)),              # largest clouds: 6144 elements a cloud, two trips; 2048 % 1500 != 0
)


def pad(c, length):
    """(B, s, C) -> (B, length, C) by cyclic repetition: plain torch indexing, not the kernel under test."""
    return c[:, torch.arange(length, device=c.device) % c.shape[1]]


def pad_backward(g, B, sizes, dtype):
    """The gradient of pad() for every cloud, as cyclic_pad_cat_bwd_kernel adds: acc = 0, then the original, then its copies in
    ascending order -- one `dtype` addition each.  g (E B, len, C) numpy -> list of (B, s, C) arrays of `dtype`."""
    g = np.asarray(g).astype(dtype)
    L = g.shape[1]
    outs = []
    for j, s in enumerate(sizes):
        blk = g[j * B:(j + 1) * B]
        acc = np.zeros((B, s, g.shape[2]), dtype=dtype)
        for r in range(0, L, s):
            seg = blk[:, r:r + s]
            acc[:, :seg.shape[1]] = acc[:, :seg.shape[1]] + seg
        outs.append(acc)
    return outs


def pad_backward_abs(g, B, sizes):
    """sum of |terms| of pad_backward, float64."""
    return pad_backward(np.abs(np.asarray(g, dtype=np.float64)), B, sizes, np.float64)


# ------------------------------------------------------------------------------------------------ inputs
def task_clouds(seed, b, n1, n2):
    """cabi_ref.tie_clouds (uniform clouds, exact duplicates, one zero distance; 40 coincident points above 300) plus, at every size
    above 24 points, a cluster of coincident points on either side and one point of the OTHER cloud on top of it: every point of the
    cluster names that one target (the backward's ballot then holds several bits -- up to a whole wave's --, summed in ascending source
    order), and the targets' own nearest neighbour is a tie among the cluster that must go to its lowest index.
    -> x1 (b, n1, 3), x2 (b, n2, 3) float32."""
    x1, x2 = R.tie_clouds(seed, b, n1, n2)
    if n1 > 24 and n2 > 24:
        k1, k2 = min(70, n1 // 3), min(70, n2 // 3)
        x1[:, 14:14 + k1] = x1[:, 14:15]
        x2[:, 1] = x1[:, 14]
        x2[:, 16:16 + k2] = x2[:, 16:17]
        x1[:, 1] = x2[:, 16]
    return x1, x2


def pad_rows(x, group, nvalid):
    """x (E group, n, 3) numpy: rows of evaluation e keep their first nvalid[e] points and repeat them cyclically up to n."""
    out = x.copy()
    n = x.shape[1]
    for e, v in enumerate(nvalid):
        out[e * group:(e + 1) * group] = x[e * group:(e + 1) * group][:, np.arange(n) % v]
    return out


# ------------------------------------------------------------------------------------------------ 2. the valid-query scan
# (R, q_group, q_valid, m, n): pairscan_dispatch picks the points per lane by n (<= 64: 1, <= 256: 4, <= 1024: 16, <= 2048: 32) and
# spreads the m queries of a cloud over min(ceil(512 / R), ceil(m / waves)) workgroups; the kernel splits the VALID queries over them.
VALID_CASES = (
    (6, 2, (1, 5, 64), 64, 64),              # 1 point per lane; 1 and 5 valid queries over 8 workgroups: most scan nothing; 64 = m: no copies
    (4, 1, (3, 40, 100, 256), 256, 256),     # 4 points per lane; q_group 1; 3 valid queries over 32 workgroups
    (3, 3, (200,), 256, 1000),               # 16 points per lane (the variant the suite already runs), n no multiple of 64, one group
    (16, 1, (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 256, 256, 7, 64), 256, 1024),  # 16 counts, 1 .. m, n a whole 16 x 64
    (2, 2, (70,), 128, 2048),                # 32 points per lane, the largest n
)


def chamfer_np32(a, b):
    """Nearest neighbours both ways of a (na, 3) and b (nb, 3) as float32 numpy: d = ((dx dx + dy dy) + dz dz), one rounding per
    operation (numpy never contracts), first minimum.  -> dist_a (na,), idx_a, dist_b (nb,), idx_b."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    ia, ib = d.argmin(1), d.argmin(0)
    return d[np.arange(len(a)), ia], ia.astype(np.int32), d[ib, np.arange(len(b))], ib.astype(np.int32)


# ------------------------------------------------------------------------------------------------ 3. the grouped Chamfer-mean loss
# (n1, n2): chamfer_bwd_grouped_kernel<PPL> keeps the SOURCE side in registers, PPL = 1 / 4 / 16 / 32 for ns <= 64 / 256 / 1024 / 2048;
# grad_xyz1 has ns = n2, grad_xyz2 has ns = n1.
LOSS_PAIRS = (
    (7, 64),        # grad_xyz1: PPL 1 (ns = 64, the edge),  grad_xyz2: PPL 1 (ns = 7)
    (64, 200),      # grad_xyz1: PPL 4,                      grad_xyz2: PPL 1 (ns = 64, the edge)
    (256, 257),     # grad_xyz1: PPL 16 (just above 256),    grad_xyz2: PPL 4 (ns = 256, the edge)
    (300, 1024),    # grad_xyz1: PPL 16 (ns = 1024, edge),   grad_xyz2: PPL 16
    (1024, 1100),   # grad_xyz1: PPL 32,                     grad_xyz2: PPL 16 (the edge)
    (2048, 2048),   # grad_xyz1: PPL 32,                     grad_xyz2: PPL 32: the largest size either side
    (300, 64),      # n1 > n2: grad_xyz1: PPL 1, grad_xyz2: PPL 16; the Python wrapper's chamfer_forward_impl route
)
# (nev, group): R = nev group rows; the backward spreads a cloud's targets over min((nt + 3) / 4, ceil(1024 / R)) workgroups
LOSS_GROUPS = (
    (1, 1),     # one evaluation of one cloud: y-split (nt + 3) / 4 up to 1024
    (3, 2),     # R = 6: y-split min((nt + 3) / 4, 171)
    (16, 1),    # kMaxPrefixes evaluations: y-split min((nt + 3) / 4, 64)
)
LOSS_WIDE = (16, 65, 8, 8)  # (nev, group, n1, n2): R = 1040 > 1024 -> y-split 1; 65 partials a sum in the final kernel


def nvalid_of(nev, n1, seed=0):
    """Valid counts of the evaluations: 1 and n1 (no copies at all) whenever there are two evaluations or more."""
    if nev == 1:
        return [(n1 + 1) // 2]
    rng = np.random.default_rng(seed * 7919 + nev * 131 + n1)
    return [1] + [int(v) for v in rng.integers(1, n1 + 1, nev - 2)] + [n1]


def grad_loss_of(nev):
    """One upstream gradient per evaluation: holds a 0 and a negative value from three evaluations on."""
    base = (0.75, -1.3, 0.0, 1.0, 0.37, 2.0, -0.5, 1.0)
    return [-1.3] if nev == 1 else [base[e % len(base)] for e in range(nev)]


def loss_bound_units(nv, n2, group):
    """The grouped loss in units of 2^-24 (|mean d1| + |mean d2|), counted from chamfer_mean_grouped_partial_kernel / _final_kernel: a
    squared distance is 5 roundings away from the fp64 one formed on the same float32 points (each difference 1, each square 1 -> 3 a
    product, the two additions 1 each; all terms positive, so relative errors add); it then passes ceil(n / 256) - 1 additions of its
    thread's strided partial, 8 levels of the halving tree over 256 threads and up to `group` additions over the evaluation's clouds;
    the quotient by (group n) rounds once [(float)group (float)n is exact below 2^24] and the final sum of the two means once."""
    n = max(nv, n2)
    return 5 + ((n + 255) // 256 - 1) + 8 + group + 1 + 1


def grad_terms(xt, xs, it, i_s, ct, cs, gl):
    """The terms of one side's gradient as chamfer_bwd_grouped_kernel forms them, in float64: target j receives its own term
    2 gl ct (t_j - s[it_j]) and, from every source k with i_s[k] == j, -2 gl cs (s_k - t_j).  xt (G, nt, 3), xs (G, ns, 3), it (G, nt),
    i_s (G, ns) -> (gradient, number of sources that chose each target (G, nt), sum of |terms| (G, nt, 3))."""
    xt, xs = np.asarray(xt, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    G = xt.shape[0]
    ar = np.arange(G)[:, None]
    own = 2.0 * gl * ct * (xt - xs[ar, np.asarray(it).astype(np.int64)])
    src = -2.0 * gl * cs * (xs - xt[ar, np.asarray(i_s).astype(np.int64)])
    add, hits, sab = R.index_add(xt.shape[1], i_s, src)
    return own + add, hits, np.abs(own) + sab


# Per gradient element, in units of 2^-24 sum|terms|: the coefficient (gl c) 2 carries 2 roundings (1 / (group n) on the host, the
# product with the upstream gradient; the doubling is exact), the difference of the coordinates 1, the term's product 1 -> 4 a term; the
# own term and the `hits` sources that chose the target are added one by one (the first addition, onto 0, is exact): at most `hits`
# additions over any term.  One more unit absorbs the second-order terms of (1 + u)^(4 + hits): (4 + hits)^2 2^-25 of a unit, far below one at any size here.
grad_bound_units = lambda hits: 4.0 + hits + 1.0


# ------------------------------------------------------------------------------------------------ 4. head + rotation, grouped
# (R, N, group): the forward launches min((N + 255) / 256, 64) workgroups per row
HEAD_CASES = (
    (1, 1, 1),        # smallest case
    (6, 7, 2),        # three evaluations of two rows; one row carries a ZERO pre-normalised quaternion (F.normalize's eps = 1e-12 branch)
    (12, 300, 3),     # two workgroups a row; N no multiple of 256
    (128, 64, 32),    # the BASELINE configs[4] shape: 4 evaluations of 32 rows, the regulariser's tree over 32 rows
    (2, 16500, 1),    # ceil(16500 / 256) = 65 > 64: grid.x capped, the strided loop takes a second trip; group 1
)


def qrot_quat_terms(quat, v, grad_out):
    """The per-POINT terms of the quaternion's gradient through out = qrot(quat, v) in float64: (B, N, 4); their sum over the points is
    cabi_ref.qrot's grad_quat, the sum of their magnitudes the scale of the kernel's fixed-order sum."""
    q = torch.from_numpy(np.asarray(quat)).double()
    x = torch.from_numpy(np.asarray(v)).double()
    qr = q[:, None, :].expand(-1, x.shape[1], -1).clone().requires_grad_(True)
    qv = qr[..., 1:]
    uv = torch.cross(qv, x, dim=2)
    out = x + 2 * (qr[..., :1] * uv + torch.cross(qv, uv, dim=2))
    (g,) = torch.autograd.grad(out, [qr], torch.from_numpy(np.asarray(grad_out)).double())
    return g.numpy()


def quat_sum_units(N):
    """The quaternion gradient's sum over N points in units of 2^-24 sum|terms| (pcrnet_head_rot_bwd_kernel): ceil(N / 256) - 1
    additions of the thread's strided partial, 6 butterfly levels, 2 additions over the 4 waves, and at most 8 roundings inside a term
    (cross and dot products of float32 operands, the scalings by 2 and 4 exact)."""
    return ((N + 255) // 256 - 1) + 6 + 2 + 8

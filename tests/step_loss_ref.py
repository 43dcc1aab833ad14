"""Test helper for tests/test_gpu_step_loss.py and tests/test_step_loss_host.py: the shape table, input recipes, scalar cases, plain
references and counted bounds of the sampler step's fused loss entries (include/samplenet_hip_internal.h: sn_pairscan_forward_partial
/ _partial_fc / _keys, sn_sampler_step_loss_forward / _forward_direct / _backward / _keys, sn_surface_values_keys,
sn_surface_gather_upstream, sn_sampler_loss_forward / _backward, sn_sigma_forward, sn_pairscan_colmin_splits).

Two references.  (1) The scan restated in float32 numpy, one rounding per operation in the order of `sqdist` in csrc/pairscan.hip, with
the kernels' tie rules: indices and distances are then comparable bit for bit and no case needs an admission rule.  (2) The step in
float64 on the float32 inputs with the indices FIXED to (1)'s: loss value, gradient to the queries split into its Chamfer terms, its
soft-projection term and the per-query terms of d / d sigma, so that a bound can be formed per element.  The softmax, the projection,
the simplification loss and the index-add are tests/cabi_ref.py's, the Chamfer terms tests/task_batch_ref.py's; none of those is
restated.  What IS restated by hand, because the table and the bounds need them without a library: the two launch plans scan_plan()
(pairscan_ysplit / pairscan_dispatch) and soft_bwd_splits() (sn_soft_bwd_splits); tests/test_step_loss_host.py holds both to the
library's own answers on every row.
Every table says which branch of the code each row reaches.  Lives in tests/ on purpose: nothing here is a product route."""
import functools

import numpy as np
import torch

import cabi_ref as R
import task_batch_ref as TB

U = 2.0 ** -24  # unit roundoff of float32

# ------------------------------------------------------------------------------------------------ 1. the shape table
# ((B, N, M, K), G, why) with G = sn_pairscan_colmin_splits(B, N, M), evaluated by hand from pairscan_ysplit (csrc/pairscan.hip):
# points per lane 1 / 4 / 16 / 32 for N <= 64 / 256 / 1024 / 2048, at most 16 / 16 / 8 / 4 waves a workgroup with column minima,
# G = min(ceil(512 / B), ceil(M / waves)).  tests/test_step_loss_host.py holds every G against the library's answer.
SPLIT_ROWS = (
    ((1, 1, 17, 1), 2, "one point, M > N, K = 1 (LOGG 0), B = 1"),
    ((2, 64, 33, 8), 3, "one point per lane at its edge N = 64; M % 4 = 1"),
    ((3, 200, 20, 5), 2, "4 points per lane, N no multiple of 64"),
    ((2, 256, 40, 16), 3, "4 per lane at its edge; K = 16, the edge of the DPP-scan softmax"),
    ((2, 1000, 37, 17), 5, "16 per lane; K = 17, the first K on the fp64-sum branch; M odd"),
    ((1, 1024, 64, 64), 8, "16 per lane at its edge; the largest K"),
    ((2, 1100, 9, 8), 3, "32 per lane; workgroups of 3 waves"),
    ((86, 1100, 25, 3), 6, "5 queries per workgroup, so workgroup 5 gets NO query; B > 64: lanes of the one-wave finals carry two clouds"),
    ((2, 2048, 10, 16), 3, "the largest N of the split routes"),
)
# one workgroup per cloud (G <= 1): the partial / fc / keys entries answer SN_ERR_UNSUPPORTED
DIRECT_ROWS = (
    ((3, 64, 16, 8), "M equal to the waves of one workgroup"),
    ((2, 1024, 8, 8), "small M"),
    ((2, 2048, 4, 8), "small M, largest N"),
    ((512, 64, 17, 4), "a batch that fills the chip: want = 1, workgroups capped at 4 waves"),
    ((2, 2112, 5, 8), "N > 2048: the swapped second scan forward, the three-launch branch of the backward; the keys entry is UNSUPPORTED"),
)
SPLIT = tuple(r[0] for r in SPLIT_ROWS)
DIRECT = tuple(r[0] for r in DIRECT_ROWS)
ROWS = SPLIT + DIRECT
G_OF = {r[0]: r[1] for r in SPLIT_ROWS}
NO_QUERY_ROW = (86, 1100, 25, 3)
MAX_PAIRS = 2_400_000
FC_ROWS = ((2, 64, 33, 8), (2, 1000, 37, 17))
FC_K = (4, 256, 260)  # one lane, exactly one trip of the 64 lanes x 4, one lane of a second trip
SURFACE_ROWS = ((3, 200, 20, 5), (2, 1000, 37, 17), (86, 1100, 25, 3))
GATHER_SIZES = (1, 255, 256, 257, 6144)
SCALAR_SIZES = (1, 1023, 1024, 1025, 6144)


def row_id(s):
    return "%dx%dx%dx%d" % tuple(s)


def scan_plan(B, N, M):
    """(G, queries per workgroup, waves per workgroup) as pairscan_ysplit / pairscan_dispatch (column minima wanted) make them."""
    if N > 2048:
        return 1, M, min(16, M)
    ppl = 1 if N <= 64 else 4 if N <= 256 else 16 if N <= 1024 else 32
    maxw = (256 if ppl >= 32 else 512 if ppl == 16 else 1024) // 64
    G = max(1, min((512 + B - 1) // B, (M + maxw - 1) // maxw))
    qpb = (M + G - 1) // G
    waves = max(1, min(maxw, qpb))
    if G == 1 and B >= 512:
        waves = min(waves, 4)
    return G, qpb, waves


def partial_ws_bytes(shape):
    """The workspace of sn_pairscan_forward_partial: [B][G][N] 64-bit keys, nothing else."""
    B, N, M, K = shape
    return B * G_OF[shape] * N * 8


def soft_bwd_splits(B, M):
    """sn_soft_bwd_splits as the header's formula."""
    return max(1, min((M + 3) // 4, (1024 + B - 1) // B))


# ------------------------------------------------------------------------------------------------ 2. inputs
RECIPES = ("cube", "surface", "on_points", "coincident", "shifted")


def _seed(shape, recipe):
    B, N, M, K = shape
    return 1000 * RECIPES.index(recipe) + (B * 7 + N * 3 + M * 5 + K) % 997


def make_case(shape, recipe):
    """-> P (B, N, 3), Q (B, M, 3) float32.
    cube      : cabi_ref.clouds (exact duplicates, one zero distance) and, from 8 points on, points [N/2, N/2 + 4) copied from [0, 4):
                ties between the scan's workgroups (a point pair that lands in different lanes and, at 16 / 32 per lane, slots)
    surface   : cabi_ref.surface_queries(cluster=True): many queries name the same points
    on_points : the queries ARE cloud points: every dist_q is 0 and the arg-max is query 0 by the tie rule
    coincident: all queries equal: every point's nearest query is a tie that resolves to query 0
    shifted   : cube + 0.5: mean(proj) is O(1) and carries weight in the loss"""
    B, N, M, K = shape
    seed = _seed(shape, recipe)
    if recipe == "surface":
        P, Q = R.surface_queries(seed, B, N, M, cluster=True)
    else:
        P, Q = R.clouds(seed, B, N, M)
        if N >= 8:
            P[:, N // 2:N // 2 + 4] = P[:, 0:4]
    if recipe == "on_points":
        Q = P[:, np.arange(M) % N].copy()
    elif recipe == "coincident":
        Q = np.repeat(Q[:, :1], M, axis=1)
    elif recipe == "shifted":
        P, Q = P + np.float32(0.5), Q + np.float32(0.5)
    return np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)


# (T, min_sigma, alpha, lmbda, weight, grad_loss); the first runs on every row, the others on SCALAR_ROWS
SCALARS = {
    "base": (0.6, 1e-2, 0.3, 0.7, 1.64, 1.0),
    "clamped": (0.05, 1e-2, 0.3, 0.7, 1.64, 1.0),     # min_sigma active: grad_T exactly 0
    "tie": (0.25, 0.0625, 0.3, 0.7, 1.64, 1.0),        # T^2 == min_sigma exactly: factor 0.5
    "alpha0": (0.6, 1e-2, 0.0, 0.7, 1.64, 1.0),
    "lmbda0": (0.6, 1e-2, 0.3, 0.0, 1.64, 1.0),
    "negative_g": (0.6, 1e-2, 0.3, 0.7, 1.64, -1.3),
    "zero_g": (0.6, 1e-2, 0.3, 0.7, 1.64, 0.0),        # every gradient +-0
}
SCALAR_ROWS = ((3, 200, 20, 5), (2, 1000, 37, 17))  # both split (both backward entries run); K <= 16 and K > 16


def sigma_factor(T, min_sigma):
    """sigma_grad_block's rule (csrc/step_tail.h) on float32 operands: d max(T^2, min_sigma) / d (T^2) = 1 / 0.5 / 0 for T^2 >, ==, <."""
    t2, ms = np.float32(T) * np.float32(T), np.float32(min_sigma)
    return 1.0 if t2 > ms else (0.5 if t2 == ms else 0.0)


# ------------------------------------------------------------------------------------------------ 3. the scan in float32
def scan_np32(P, Q, K):
    """The pair scan of one batch as float32 numpy.  d[j, n] = ((dx dx + dy dy) + dz dz) with dx = p - q (sqdist), one rounding per
    operation.  K nearest of a query: ascending in the key (distance, point index) -- a stable sort on the distance; dist_q / idx_q:
    the first of them; dist_p / idx_p: the minimum over the queries of the key (distance, query index) -- the first minimum, so the
    lowest query wins a tie; argmax1: the first maximum of dist_q.
    -> dict knn (B, M, K) int32, dq (B, M), iq, dp (B, N), ip, am (B,)."""
    P, Q = np.asarray(P, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    B, N, M = P.shape[0], P.shape[1], Q.shape[1]
    out = dict(knn=np.empty((B, M, K), np.int32), dq=np.empty((B, M), np.float32), iq=np.empty((B, M), np.int32),
               dp=np.empty((B, N), np.float32), ip=np.empty((B, N), np.int32), am=np.empty((B,), np.int32))
    for b in range(B):
        dx = P[b, None, :, 0] - Q[b, :, None, 0]
        dy = P[b, None, :, 1] - Q[b, :, None, 1]
        dz = P[b, None, :, 2] - Q[b, :, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32 and d.shape == (M, N)
        order = np.argsort(d, axis=1, kind="stable")[:, :K]
        out["knn"][b] = order
        out["iq"][b] = order[:, 0]
        out["dq"][b] = d[np.arange(M), order[:, 0]]
        ip = d.argmin(0)
        out["ip"][b] = ip
        out["dp"][b] = d[ip, np.arange(N)]
        out["am"][b] = out["dq"][b].argmax()
    return out


# ------------------------------------------------------------------------------------------------ 4. the step in float64
def sigma_terms(P, Q, idx, sigma, grad_proj):
    """Per-QUERY terms of d (sum grad_proj . proj) / d sigma in float64 (B, M): cabi_ref.soft_project's expression with one sigma
    per query, so that autograd keeps the queries apart; their sum is cabi_ref.soft_project's grad_sigma (held by the host test)."""
    Pt, Qt = torch.from_numpy(np.array(P)).double(), torch.from_numpy(np.array(Q)).double()  # (copies: the shared references are read-only)
    sg = torch.full(Qt.shape[:2], float(sigma), dtype=torch.float64, requires_grad=True)
    nb = R._gather(Pt, torch.from_numpy(np.array(idx)))
    d = ((nb - Qt[:, :, None, :]) ** 2).sum(-1)
    proj = (torch.softmax(-d / sg[..., None], dim=-1)[..., None] * nb).sum(2)
    (gs,) = torch.autograd.grad(proj, [sg], torch.from_numpy(np.asarray(grad_proj)).double())
    return gs.numpy()


def step_loss(P, Q, scan, scalars, with_proj=True):
    """L = alpha L_simp + lmbda max(T^2, min_sigma) + [mean(proj)] in float64 on the given indices -> (L, L_simp, parts) with parts
    = (mean dq, mean_b max dq, mean dp, mean proj, sigma, per-cloud [sum dq, max dq, sum dp, sum proj] (B, 4), proj (B, M, 3))."""
    T, ms, alpha, lmbda, weight, _ = scalars
    P64, Q64 = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    ar = np.arange(P64.shape[0])[:, None]
    d1 = ((Q64 - P64[ar, scan["iq"].astype(np.int64)]) ** 2).sum(-1)
    d2 = ((P64 - Q64[ar, scan["ip"].astype(np.int64)]) ** 2).sum(-1)
    sigma = R.sigma_of(T, ms)
    proj, _ = R.soft_project(P64, Q64, np.array(scan["knn"]), sigma)
    c12, cmax, c21 = d1.mean(), d1.max(1).mean(), d2.mean()
    lsimp = c12 + cmax + float(np.float32(weight)) * c21
    L = float(np.float32(alpha)) * lsimp + float(np.float32(lmbda)) * sigma + (proj.mean() if with_proj else 0.0)
    per = np.stack([d1.sum(1), d1.max(1), d2.sum(1), proj.sum((1, 2))], 1)
    return L, lsimp, (c12, cmax, c21, proj.mean(), sigma, per, proj)


def step_grads(P, Q, scan, scalars, grad_proj=None, grad_sigma=None):
    """Gradients of grad_loss * L in float64 on the fixed indices.  The Chamfer part as task_batch_ref.grad_terms forms it (own term
    2 (alpha g) (1 / (B M) + [j == argmax1] / B) (q_j - p[iq_j]), and -2 (alpha g) weight / (B N) (p_n - q_j) from every point n
    that chose query j), the soft part by autograd through cabi_ref.soft_project with the upstream gradient g / (3 B M) (or the explicit
    grad_proj (B, M, 3)), the temperature by sigma_grad_block's rule with the direct term lmbda g (or grad_sigma).
    -> dict cham (B, M, 3), hits (B, M), cham_abs (B, M, 3), soft (B, M, 3), gp_max, sig_terms (B, M), direct, grad_T, grad_T_abs."""
    T, ms, alpha, lmbda, weight, g = scalars
    B, N, M = P.shape[0], P.shape[1], Q.shape[1]
    g, alpha, lmbda, weight = float(np.float32(g)), float(np.float32(alpha)), float(np.float32(lmbda)), float(np.float32(weight))
    ct = 1.0 / (B * M) + (np.arange(M)[None, :] == scan["am"][:, None]) / B
    cham, hits, cham_abs = TB.grad_terms(Q, P, scan["iq"], scan["ip"], ct[..., None], weight / (B * N), alpha * g)
    gp = np.full((B, M, 3), g / (3.0 * B * M)) if grad_proj is None else np.asarray(grad_proj, dtype=np.float64)
    sigma = R.sigma_of(T, ms)
    _, _, _, soft, gs = R.soft_project(np.array(P), np.array(Q), np.array(scan["knn"]), sigma, gp)
    sig = sigma_terms(P, Q, scan["knn"], sigma, gp)
    assert abs(sig.sum() - gs) <= 1e-9 * (np.abs(sig).sum() + 1e-300)
    T32, f = float(np.float32(T)), sigma_factor(T, ms)
    direct = (lmbda * g if grad_sigma is None else float(np.float32(grad_sigma))) * 2.0 * T32 * f
    return dict(cham=cham, hits=hits, cham_abs=cham_abs, soft=soft, gp_max=float(np.abs(gp).max()), sig_terms=sig, direct=direct,
                grad_T=sig.sum() * 2.0 * T32 * f + direct, grad_T_abs=np.abs(sig).sum() * 2.0 * abs(T32) * f + abs(direct))


# ------------------------------------------------------------------------------------------------ 5. the counted bounds
def _tree(n, nt):
    """Additions over any term of a sum of n terms reduced by nt threads: the thread's strided partial, then log2(nt) tree levels."""
    return max(0, (n + nt - 1) // nt - 1) + int(np.log2(nt))


def _final(B):
    """step_loss_final / step_loss_keys_final / surface_values_final_kernel: lane b carries clouds b, b + 64, ..., then a 6-level tree."""
    return max(0, (B + 63) // 64 - 1) + 6


def query_sum_depth(B, N, M):
    """Additions over any dist_q on its way into a cloud's sum, the longest of the three routes: step_loss_partial_kernel (1024
    threads, halving tree), step_loss_partial_direct_kernel (256 threads) and, in keys mode, the scan's own sum -- a wave adds its
    ceil(qpb / waves) queries one by one, wave 0 adds the waves in order, the consumer adds the G workgroups in order."""
    G, qpb, waves = scan_plan(B, N, M)
    keys = ((qpb + waves - 1) // waves + waves + G) if G > 1 else 0
    return max(_tree(M, 1024), _tree(M, 256), keys)


def loss_bound(shape, scalars, parts, with_proj=True):
    """|L - L64| and |L_simp - L_simp64|, counted, for any of the three routes -> (bound L, bound L_simp, bounds of the three means
    mean dq, mean_b max dq, mean dp).
    A squared distance is 5 roundings away from the fp64 one on the same float32 points (each difference 1, each square 1 more -> 3 a
    product, the two additions 1 each; all terms positive, so relative errors add: task_batch_ref.loss_bound_units).  mean dq: its
    terms pass query_sum_depth additions a cloud and _final(B) over the clouds, the quotient rounds once.  mean max dq: the maximum is
    exact, _final(B) additions, one quotient.  mean dp: _tree(N, 1024) / _tree(N, 256) / (strided over 256 threads, 6 levels, 3 over the
    waves) additions a cloud, _final(B), one quotient, one product with the weight.  L_simp adds the three: 2 more over any term.  L:
    alpha L_simp and lmbda sigma round once each (sigma itself is the float32 value on both sides), the two additions 2 over any term;
    mean(proj) is charged in units of sum|proj| / (3 B M) -- its sum's depth (3 M terms a cloud; in keys mode two additions inside a
    query, then the dist_q path), the quotient -- plus the 1e-6 every projected coordinate may be off.  One more unit a term absorbs
    the second-order terms."""
    B, N, M, K = shape
    T, ms, alpha, lmbda, weight, _ = scalars
    c12, cmax, c21, mp, sigma, per, proj = parts
    dq_units = 5 + query_sum_depth(B, N, M) + _final(B) + 1 + 1
    mx_units = 5 + _final(B) + 1 + 1
    dp_units = 5 + max(_tree(N, 1024), _tree(N, 256), (N + 255) // 256 - 1 + 6 + 3) + _final(B) + 2 + 1
    w = abs(float(np.float32(weight)))
    lsimp_abs = c12 + cmax + w * c21
    b_lsimp = U * (dq_units * c12 + mx_units * cmax + dp_units * w * c21 + 2 * lsimp_abs)
    means = (U * dq_units * c12, U * mx_units * cmax, U * dp_units * c21)
    a, l = abs(float(np.float32(alpha))), abs(float(np.float32(lmbda)))
    pj_units = max(_tree(3 * M, 1024), _tree(3 * M, 256), query_sum_depth(B, N, M) + 2) + _final(B) + 1 + 1
    mp_abs = np.abs(proj).sum() / (3.0 * B * M) if with_proj else 0.0
    b_L = a * b_lsimp + U * (a * lsimp_abs + l * sigma) + 2 * U * (a * lsimp_abs + l * sigma + mp_abs)
    if with_proj:
        b_L += U * pj_units * mp_abs + 1e-6
    return b_L, b_lsimp, means


def proj_bound(P, Q, knn, sigma, proj, w):
    """Per element of proj (B, M, 3) against cabi_ref.soft_project on the same float32 points and neighbours: the 1e-6 the scan is
    held to next to the cloud, plus what the float32 DISTANCES cost when the queries lie far from it (the head's last layer on standard
    normal operands puts them tens of units away, |q - p|^2 in the hundreds).  A float32 squared distance is 5 roundings away from the
    float64 one (loss_bound), so every exponent s_k = -d_k / sigma is off by at most e = (5 + 1) 2^-24 d_max / sigma (+ 1: the quotient);
    a softmax whose exponents move by at most e moves every weight by at most a factor exp(2 e), |dw_k| <= w_k (exp(2 e) - 1); the
    projection sum_k w_k p_k with sum_k dw_k = 0 then moves by at most sum_k |dw_k| |p_k - proj|.  Next to the cloud (d ~ 0.1) this
    term is ~1e-8: section a.'s bar is unchanged by it."""
    P64, Q64 = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nb = P64[np.arange(P64.shape[0])[:, None, None], np.asarray(knn).astype(np.int64)]       # (B, M, K, 3)
    dmax = ((nb - Q64[:, :, None, :]) ** 2).sum(-1).max(-1)                                   # (B, M)
    e = 6 * U * dmax / sigma
    spread = (np.asarray(w)[..., None] * np.abs(nb - np.asarray(proj)[:, :, None, :])).sum(2)  # (B, M, 3)
    return 1e-6 + np.expm1(2 * e)[..., None] * spread


def partial_bound(shape, per, proj):
    """partial [B][4] = sum dq, max dq, sum dp, sum proj of a cloud against fp64 -> (B, 4): the counting of loss_bound without the
    clouds' final sum and the quotients."""
    B, N, M, K = shape
    dq = U * (5 + query_sum_depth(B, N, M) + 1) * per[:, 0]
    mx = U * (5 + 1) * per[:, 1]
    dp = U * (5 + max(_tree(N, 1024), _tree(N, 256), (N + 255) // 256 - 1 + 6 + 3) + 1) * per[:, 2]
    pj = U * (max(_tree(3 * M, 1024), _tree(3 * M, 256), query_sum_depth(B, N, M) + 2) + 1) * np.abs(proj).sum((1, 2)) + 3 * M * 1e-6
    return np.stack([dq, mx, dp, pj], 1)


def dpsum_bound(shape, per):
    """dpsum [B] of the keys entries (chamfer_soft_bwd_kernel / surface_cloud_values_kernel: strided over 256 threads, 6 tree levels,
    the four waves in a fixed pairing) against fp64."""
    B, N, M, K = shape
    return U * (5 + (N + 255) // 256 - 1 + 6 + 2 + 1) * per[:, 2]


def qpart_bound(shape, per, proj):
    """The scan's per-cloud query-side sums added over G against fp64: sum dist_q within (5 + query_sum_depth + 1) 2^-24 sum dq; sum
    proj within (query_sum_depth + 2 + 1) 2^-24 sum|proj| plus 1e-6 for each of the cloud's 3 M projected coordinates.  -> (B,), (B,)."""
    B, N, M, K = shape
    dep = query_sum_depth(B, N, M)
    return U * (5 + dep + 1) * per[:, 0], U * (dep + 3) * np.abs(proj).sum((1, 2)) + 3 * M * 1e-6


CHAM_UNITS = lambda hits: TB.grad_bound_units(hits) + 1.0  # + the product alpha * g in front (gscale: rounded once)
SOFT_RTOL, SOFT_ATOL = 1e-4, 1e-5  # tests/test_gpu_cabi_contract.py's ATOMIC, the bar sn_soft_project_backward is held to
GRAD_T_RTOL = 1e-4


def grad_q_bound(ref):
    """Per element of grad_Q (B, M, 3): (task_batch_ref.grad_bound_units(hits) + 1) 2^-24 sum|Chamfer terms| for the Chamfer part --
    its coefficient carries one rounding more than the grouped kernel's, the product alpha * g --, plus for the soft part rtol 1e-4 on
    the term and atol 1e-5 max|upstream grad_proj| (the closing addition of the two parts is not charged)."""
    return CHAM_UNITS(ref["hits"])[..., None] * U * ref["cham_abs"] + SOFT_RTOL * np.abs(ref["soft"]) + SOFT_ATOL * ref["gp_max"]


def grad_t_bound(ref):
    """1e-4 (sum_j |query j's sigma term| 2 |T| factor + |direct term|): ATOMIC's rtol on the sum of magnitudes, so that cancellation
    between the queries cannot fail a right kernel."""
    return GRAD_T_RTOL * ref["grad_T_abs"]


# ------------------------------------------------------------------------------------------------ 6. the head inside the scan
def fc_case(shape, Kfc, seed=0):
    """z (B, Kfc), scale, shift (Kfc), W (3 M, Kfc), bias (3 M): standard normal; the shift is moved so that a third of the
    pre-activations z scale + shift are negative (the ReLU is exercised either way)."""
    B, N, M, K = shape
    rng = np.random.default_rng(4242 + seed + Kfc + M)
    z, scale, shift = rng.standard_normal((B, Kfc)), rng.standard_normal(Kfc), rng.standard_normal(Kfc)
    pre = z * scale
    shift = shift - np.quantile(pre + shift, 1.0 / 3.0)
    W, bias = rng.standard_normal((3 * M, Kfc)), rng.standard_normal(3 * M)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(z), f(scale), f(shift), f(W), f(bias)


def fc_ref(z, scale, shift, W, bias):
    """q (B, 3 M) = bias + relu(z scale + shift) W^T in float64 and sum of |terms| + |bias| (B, 3 M)."""
    z, scale, shift, W, bias = (np.asarray(a, dtype=np.float64) for a in (z, scale, shift, W, bias))
    a = np.maximum(z * scale + shift, 0.0)
    return a @ W.T + bias, np.abs(a) @ np.abs(W).T + np.abs(bias)


def fc_bound(Kfc, mag):
    """tests/test_gpu_skinny.py's ceiling: (K + 8) 2^-24 (|bias| + sum|terms|) -- every product and every addition of a K-term dot
    product rounds at most once over any term, the activation's fma once, the closing tree and the bias a handful more."""
    return (Kfc + 8) * U * mag


# ------------------------------------------------------------------------------------------------ cached references
@functools.lru_cache(maxsize=None)
def reference(shape, recipe):
    """(P, Q, scan) of a table case; computed once, shared, never written to."""
    P, Q = make_case(shape, recipe)
    scan = scan_np32(P, Q, shape[3])
    for a in (P, Q) + tuple(scan.values()):
        a.setflags(write=False)
    return P, Q, scan


@functools.lru_cache(maxsize=None)
def reference_loss(shape, recipe, scalar):
    P, Q, scan = reference(shape, recipe)
    return step_loss(P, Q, scan, SCALARS[scalar])


@functools.lru_cache(maxsize=None)
def reference_grads(shape, recipe, scalar):
    P, Q, scan = reference(shape, recipe)
    return step_grads(P, Q, scan, SCALARS[scalar])


def decode_inverted(keys):
    """colmin_keys (u64, INVERTED): ~key has the distance's float32 bits in the high word and the query index in the low word."""
    k = ~np.asarray(keys, dtype=np.uint64)
    return (k >> np.uint64(32)).astype(np.uint32).view(np.float32), (k & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def qmax_expected(shape, dq):
    """qmax [B][G] as the scan leaves it: per workgroup the key (dist_q bits, ~query) of its FIRST maximum; 0 for a workgroup
    without queries.  qpb = ceil(M / G)."""
    B, N, M, K = shape
    G, qpb, _ = scan_plan(B, N, M)
    out = np.zeros((B, G), np.uint64)
    for g in range(G):
        q0, q1 = g * qpb, min(M, (g + 1) * qpb)
        if q0 >= q1:
            continue
        j = q0 + dq[:, q0:q1].argmax(1)
        bits = dq[np.arange(B), j].view(np.uint32).astype(np.uint64)
        out[:, g] = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - j.astype(np.uint64))
    return out

"""Test helper for the pose-term tests (tests/test_pose_host.py, tests/test_gpu_pose_terms.py, tests/test_gpu_pose_loss.py,
tests/test_gpu_evaluation.py): the fp64 restatement of sn_pose_error_* and sn_chamfer_mean_per_cloud as include/samplenet_hip_internal.h
specifies them, their analytic gradients, the aggregates of registration/main.py:461-483 transcribed literally, the case table, and
the error bounds -- every bound COUNTED from the roundings of samplenet_amd/csrc/pose_terms.hip (compiled without contraction: one
rounding per written operation), none fitted to an observed error.  The observed maxima are recorded beside them in
profiles/pose/errors.txt.  Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of float32
EPS_NORM = 1e-12

# Error of the device's acosf in ulps of its result: MEASURED against fp64 on an MI355X over 2^22 arguments across [-1, 1], dense at
# both ends (tools/micro/acosf_error.hip: 1.418 ulp at worst; profiles/pose/errors.txt), rounded up to a whole ulp -- not assumed.
ACOSF_ULP = 2.0

# rot_err's VALUE is compared only where the fp64 reference has |x| <= 1 - 2^-10 (x = 2 d^2 - 1): acos' condition number
# 1 / sqrt(1 - x^2) is unbounded at the ends; elsewhere the result must be finite and in [0, 2 pi].
ROT_ADMIT = 1.0 - 2.0 ** -10
ROT_EXCLUDED_CAP = 0.10


# ------------------------------------------------------------------------------------------------ the terms, fp64
def quat_to_matrix(n):
    """(B,4) unit quaternions (w, x, y, z) -> (B,3,3) rotation matrices."""
    w, x, y, z = n[:, 0], n[:, 1], n[:, 2], n[:, 3]
    R = np.empty((n.shape[0], 3, 3), dtype=n.dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def normalize(q):
    den = np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), EPS_NORM)
    return q / den, den


def pose_terms(est, gt):
    """est, gt (B,7) -> dict of float64 arrays: rot_err, norm_err, trans_err (B,), x = 2 d^2 - 1 before the clamp, d, and the
    intermediates the bounds and gradients read (n1, den1, R2, D)."""
    est, gt = np.asarray(est, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    q1, q2 = est[:, :4], gt[:, :4]
    d = (q1 * q2).sum(1)
    x = 2 * d * d - 1
    with np.errstate(invalid="ignore"):
        rot = 2 * np.arccos(np.where(np.isnan(x), x, np.clip(x, -1.0, 1.0)))
    n1, den1 = normalize(q1)
    n2, _ = normalize(q2)
    R1, R2 = quat_to_matrix(n1), quat_to_matrix(n2)
    D = R1 @ R2.transpose(0, 2, 1) - np.eye(3)
    dt = est[:, 4:] - gt[:, 4:]
    return {"rot_err": rot, "norm_err": (D * D).sum((1, 2)), "trans_err": np.abs(dt).sum(1) / 3, "x": x, "d": d,
            "absdot": (np.abs(q1) * np.abs(q2)).sum(1), "n1": n1, "den1": den1, "R2": R2, "D": D, "dt": dt}


def upstream(B, g_means, g_norm_err, g_trans_err):
    """The per-cloud upstream weights (wn, wt) of sn_pose_error_backward and the sums of their parts' magnitudes (Wn, Wt), fp64."""
    z = np.zeros(B)
    am = (z if g_means is None else z + float(g_means[1]) / B, z if g_means is None else z + float(g_means[2]) / B)
    an = z if g_norm_err is None else np.asarray(g_norm_err, dtype=np.float64)
    at = z if g_trans_err is None else np.asarray(g_trans_err, dtype=np.float64)
    return am[0] + an, am[1] + at, np.abs(am[0]) + np.abs(an), np.abs(am[1]) + np.abs(at)


def pose_backward(est, gt, g_means=None, g_norm_err=None, g_trans_err=None):
    """Analytic fp64 gradient g_est (B,7) of sum_b wn[b] norm_err[b] + wt[b] trans_err[b]: d norm_err / d R1 = 2 D R2, through the
    matrix to the normalised quaternion, through the normalisation (g - n (n . g)) / max(||q||, 1e-12); sign(dt) / 3, sign(0) = 0."""
    T = pose_terms(est, gt)
    B = T["D"].shape[0]
    wn, wt, _, _ = upstream(B, g_means, g_norm_err, g_trans_err)
    G = wn[:, None, None] * 2 * (T["D"] @ T["R2"])
    n = T["n1"]
    w, x, y, z = n[:, 0], n[:, 1], n[:, 2], n[:, 3]
    g = lambda i, k: G[:, i, k]  # noqa: E731
    gn = np.stack([
        2 * (z * (g(1, 0) - g(0, 1)) + y * (g(0, 2) - g(2, 0)) + x * (g(2, 1) - g(1, 2))),
        2 * (y * (g(0, 1) + g(1, 0)) + z * (g(0, 2) + g(2, 0)) + w * (g(2, 1) - g(1, 2)) - 2 * x * (g(1, 1) + g(2, 2))),
        2 * (x * (g(0, 1) + g(1, 0)) + z * (g(1, 2) + g(2, 1)) + w * (g(0, 2) - g(2, 0)) - 2 * y * (g(0, 0) + g(2, 2))),
        2 * (x * (g(0, 2) + g(2, 0)) + y * (g(1, 2) + g(2, 1)) + w * (g(1, 0) - g(0, 1)) - 2 * z * (g(0, 0) + g(1, 1))),
    ], axis=1)
    gq = (gn - n * (n * gn).sum(1, keepdims=True)) / T["den1"]
    gtr = wt[:, None] * np.sign(T["dt"]) / 3
    return np.concatenate([gq, gtr], axis=1)


def pose_terms_torch(est, gt):
    """The same three terms as differentiable fp64 torch (any device) -> rot_err, norm_err, trans_err (B,): what autograd
    differentiates in the agreement tests.  |dt| (not sqrt(dt^2)): subgradient 0 at 0, the documented choice."""
    est, gt = est.double(), gt.double()

    def mat(q):
        n = q / q.norm(dim=1, keepdim=True).clamp_min(EPS_NORM)
        w, x, y, z = n.unbind(1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)

    d = (est[:, :4] * gt[:, :4]).sum(1)
    rot = 2 * torch.acos((2 * d * d - 1).clamp(-1, 1))
    D = mat(est[:, :4]) @ mat(gt[:, :4]).transpose(1, 2) - torch.eye(3, dtype=torch.float64, device=est.device)
    return rot, (D * D).sum((1, 2)), (est[:, 4:] - gt[:, 4:]).abs().sum(1) / 3


# ------------------------------------------------------------------------------------------------ the bounds, counted
# Notation: U the unit roundoff; gamma_k ~ k U (1 + small): a chain of k roundings; all bounds carry a factor 1.01 for second order.
def _g(k):
    return 1.01 * k * U


# normalisation: four squares + three additions (every term <= 4 roundings), sqrt (halves the relative error, + 1), division (+ 1):
# n_i = q_i / ||q|| (1 + delta), |delta| <= (4 / 2 + 1 + 1) U = 4 U.
_DN = 4
# matrix entries of the normalised quaternion, |n| = 1: a product of two components carries 2 _DN + 1 = 9 roundings.
#   diagonal 1 - 2 (aa + bb): (9 + 1) U (aa + bb) <= 10 U, doubled exactly -> 20 U, the subtraction's rounding U |R_ii| <= U:  21 U
#   off-diagonal 2 (ab +- cd): |ab| + |cd| <= 1/2, so 9 U / 2, the difference's rounding U / 2, doubled:                       10 U
EPS_R = _g(21)
# D = R1 R2^T - I: perturbed operands, eps_R (sum_k |R2_jk| + sum_k |R1_ik|) <= 2 sqrt(3) eps_R; a three-term dot product of rows of
# orthogonal matrices (sum |R1||R2| <= 1): gamma_3; the diagonal's - 1: U |D_ii| <= 2 U.
EPS_D = 2 * np.sqrt(3) * EPS_R + _g(3) + _g(2)


def bound_norm_err(N):
    """|norm_err - N|: D~ = D + e, |e| <= EPS_D: sum |2 D e| <= 2 EPS_D sum |D| <= 6 EPS_D sqrt(N), + 9 EPS_D^2; nine squares and eight
    additions, every term through at most 9 roundings: gamma_9 N."""
    N = np.asarray(N, dtype=np.float64)
    return 6 * EPS_D * np.sqrt(N) + 9 * EPS_D ** 2 + _g(9) * N


def bound_trans_err(T):
    """Three subtractions (1 rounding each), two additions, one division: every |dt_c| through at most 4 roundings; + the smallest
    subnormal for a difference that underflows."""
    return _g(4) * np.asarray(T, dtype=np.float64) + 2.0 ** -149


def eps_x(terms):
    """|x~ - x| for x = 2 d^2 - 1: d a four-term dot product, |d~ - d| <= gamma_4 A with A = sum |q1_i||q2_i|; d d: (2 |d| e + e^2) and
    one rounding U d^2; doubled exactly; the subtraction's rounding U |x|."""
    e = _g(4) * terms["absdot"]
    d = np.abs(terms["d"])
    return 2 * (2 * d * e + e * e + _g(1) * d * d) + _g(1) * np.abs(terms["x"])


def rot_admitted(terms):
    return np.abs(terms["x"]) <= ROT_ADMIT


def bound_rot_err(terms):
    """(admitted rows) the argument's error times acos' condition 1 / sqrt(1 - x^2) at the worst point of [x - eps, x + eps], doubled
    with the result; + the library call's ACOSF_ULP ulps of its result (ulp(v) <= 2 U |v|)."""
    ex = eps_x(terms)
    xm = np.minimum(np.abs(terms["x"]) + ex, 1.0 - 2.0 ** -12)
    return 2 * ex / np.sqrt(1 - xm * xm) + ACOSF_ULP * 2 * U * terms["rot_err"] + 2.0 ** -149


def bound_mean(B, values, bounds):
    """A batch mean: the mean of the per-cloud bounds, + the fixed-order sum's roundings -- at most ceil(B / 256) additions in a
    thread, 8 levels of the tree, one division -- on non-negative terms."""
    k = (B + 255) // 256 + 8 + 1
    return np.sum(bounds) / B + _g(k) * np.sum(np.abs(values)) / B


def means_in_kernel_order(values, threads=256):
    """float32 (B,) -> the batch mean as pose_error_fwd_kernel adds it: thread t's partial over clouds t, t + 256, ... in ascending
    order from 0, a halving tree over the partials, one float32 division by B."""
    v = np.asarray(values, dtype=np.float32)
    part = np.zeros(threads, dtype=np.float32)
    for b in range(len(v)):
        part[b % threads] = part[b % threads] + v[b]
    s = threads // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return np.float32(part[0] / np.float32(len(v)))


def bound_backward(est, gt, g_means=None, g_norm_err=None, g_trans_err=None):
    """(B,7) bound on |g_est - pose_backward|.
    Quaternion part.  W = |g_means[1] / B| + |g_norm_err[b]| (the weight's own two roundings: 2 U W); r = max row sum of |D|.
      G = w 2 (D R2): perturbed operands sqrt(3) EPS_D + EPS_R r, three-term sum + the two scalings 5 U r:
          eps_G = 2 W (sqrt(3) EPS_D + (EPS_R + gamma_7) r),  |G| <= Gmax = 2 W r
      g_n = J^T G with sum |J| <= S = sqrt(112) (rows of +-2 n and -4 n, |n| = 1); every path <= 7 roundings, n itself 4 U:
          eps_gn = S (eps_G + gamma_11 Gmax),  |g_n| <= S Gmax
      n . g_n: sum |n_i| <= 2: 2 eps_gn + gamma_8 2 S Gmax;  |n . g_n| <= 2 S Gmax
      (g_n - n (n . g_n)) / den: eps_gn + |n_i| (2 eps_gn + gamma_16 S Gmax) + gamma_5 2 S Gmax + U 3 S Gmax, over den, + 4 U |g|
          (den: 3 roundings, the division 1)
    Translation part.  w (sg / 3): the weight's two roundings on W_t, the division and the product: gamma_4 W_t / 3."""
    T = pose_terms(est, gt)
    B = T["D"].shape[0]
    _, _, Wn, Wt = upstream(B, g_means, g_norm_err, g_trans_err)
    r = np.abs(T["D"]).sum(2).max(1)
    S = np.sqrt(112.0)
    eps_G = 2 * Wn * (np.sqrt(3) * EPS_D + (EPS_R + _g(7)) * r)
    Gmax = 2 * Wn * r
    eps_gn = S * (eps_G + _g(11) * Gmax)
    num = 3 * eps_gn + (_g(16) + 2 * _g(5) + 3 * _g(1)) * S * Gmax
    ref = pose_backward(est, gt, g_means, g_norm_err, g_trans_err)
    bq = num[:, None] / T["den1"] + _g(4) * np.abs(ref[:, :4]) + 2.0 ** -149
    bt = np.repeat((_g(4) * Wt / 3)[:, None], 3, axis=1) + 2.0 ** -149
    return np.concatenate([bq, bt], axis=1)


def bound_chamfer_mean(n1, n2, m1, m2):
    """out = s1 / n1 + s2 / n2 on non-negative distances: a side's sum runs ceil(n / 256) additions in a thread and 8 tree levels, then
    the division and the final addition."""
    k = lambda n: (n + 255) // 256 + 8 + 2  # noqa: E731
    return _g(k(n1)) * m1 + _g(k(n2)) * m2


def chamfer_mean(d1, d2):
    d1, d2 = np.asarray(d1, dtype=np.float64), np.asarray(d2, dtype=np.float64)
    return d1.mean(1), d2.mean(1)


# ------------------------------------------------------------------------------------------------ the cases
# B: 1, 2 (fewer clouds than a wave), 63 / 64 / 65 (around a wave), 257 (the strided loop's second trip: one thread takes two
# clouds), 700 (above the 256 clouds one pass serves: third trip, partial).
BATCHES = (1, 2, 63, 64, 65, 257, 700)
# recipe -> does its rot_err take part in the VALUE comparison (then at most ROT_EXCLUDED_CAP of its rows may fall outside the
# admission rule); the others sit on an edge of acos, or leave its domain, on purpose: finiteness and range only.
RECIPES = {
    "unit": True,        # random unit pairs, random translations; every 5th row shares a translation component (dt = 0)
    "nonunit": False,    # est of norm 1e-3 .. 1e3 against unit gt: normalisation and its gradient; x = 2 d^2 - 1 leaves [-1, 1]
    "same": False,       # est == gt: x = 1 up to rounding (the reference's NaN); norm_err ~ 0; dt = 0 everywhere
    "negated": False,    # est == -gt: the same rotation, d = -1
    "antipodal": False,  # rotations half a turn apart: d = 0, x = -1, rot_err = 2 pi
    "zero": False,       # est's quaternion all zero: the clamped denominator
}
CHAMFER_SIZES = ((1, 1), (1, 130), (64, 64), (77, 1024), (300, 64))
CHAMFER_BATCHES = (1, 3)


def _unit(rng, B):
    q = rng.standard_normal((B, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _qmul(q, r):
    w1, x1, y1, z1 = q.T
    w2, x2, y2, z2 = r.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def make_case(recipe, B, seed=0):
    """-> est, gt (B,7) float32."""
    rng = np.random.default_rng([seed, B, sorted(RECIPES).index(recipe)])
    q2 = _unit(rng, B)
    t1, t2 = rng.uniform(-1, 1, (B, 3)), rng.uniform(-1, 1, (B, 3))
    if recipe == "unit":
        q1 = _unit(rng, B)
        t1[::5, 1] = t2[::5, 1]
    elif recipe == "nonunit":
        q1 = _unit(rng, B) * 10.0 ** rng.uniform(-3, 3, (B, 1))
    elif recipe == "same":
        q1, t1 = q2.copy(), t2.copy()
    elif recipe == "negated":
        q1 = -q2
    elif recipe == "antipodal":
        u = rng.standard_normal((B, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        q1 = _qmul(q2, np.concatenate([np.zeros((B, 1)), u], axis=1))
    elif recipe == "zero":
        q1 = np.zeros((B, 4))
    else:
        raise KeyError(recipe)
    est = np.concatenate([q1, t1], axis=1).astype(np.float32)
    gt = np.concatenate([q2, t2], axis=1).astype(np.float32)
    return est, gt


def upstream_case(B, seed=1):
    """-> g_means (3,), g_norm_err (B,), g_trans_err (B,) float32; g_means[0] is a NaN: it must not be read."""
    rng = np.random.default_rng([seed, B])
    gm = rng.uniform(-2, 2, 3).astype(np.float32)
    gm[0] = np.nan
    return gm, rng.uniform(-2, 2, B).astype(np.float32), rng.uniform(-2, 2, B).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the aggregates
def aggregates_transcribed(rotation_errors, trans_errs, consistency_errors, losses=None):
    """registration/main.py:461-483 line by line (n_samples = len(testloader) = the number of items at its batch size 1), and the two
    running averages of eval_1 (main.py:400-407) over the same items."""
    rotation_errors = np.array(rotation_errors)
    trans_errs = np.array(trans_errs)
    consistency_errors = np.array(consistency_errors)
    n_samples = len(rotation_errors)
    x = np.arange(0.0, 180.0, 0.5)
    y = np.zeros(len(x))
    for idx, err in enumerate(x):
        precision = np.sum(rotation_errors <= err) / n_samples
        y[idx] = precision
    auc = np.sum(y) / len(x)
    out = {"thresholds": x, "precision": y, "auc": auc,
           "mean_rotation_error": np.mean(rotation_errors), "std_rotation_error": np.std(rotation_errors),
           "mean_trans_error": np.mean(trans_errs), "std_trans_error": np.std(trans_errs),
           "mean_consistency_error": np.mean(consistency_errors), "std_consistency_error": np.std(consistency_errors)}
    gloss, count = 0.0, 0
    for e in rotation_errors.tolist():  # (rotation_error.item(): Python floats)
        gloss += e
        count += 1
    out["ave_gloss"] = float(gloss) / count
    if losses is not None:
        vloss = 0.0
        for v in np.array(losses).tolist():
            vloss += v
        out["ave_vloss"] = float(vloss) / count
    return out

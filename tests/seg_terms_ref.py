"""Test helper for the segmentation-term tests (tests/test_seg_host.py, tests/test_gpu_seg_terms.py, tests/test_gpu_segmentation.py):
the fp64 restatement of sn_segmentation_terms_forward / _backward as include/samplenet_hip_internal.h specifies them, the shape
table, the input recipes, the evaluator's aggregates as a plain per-cloud loop, and the error bounds -- every bound COUNTED from the
order of operations written at the head of samplenet_amd/csrc/seg_terms.hip (compiled without contraction: one rounding per written
operation), none fitted to an observed error.  The expf / logf figures are cls_terms_ref's (measured in profiles/eval/errors.txt).
The observed maxima are recorded beside the bounds in profiles/seg/errors.txt.  Lives in tests/ on purpose: nothing here is a
product route."""
import numpy as np

from cls_terms_ref import FLUSH, TINY, U, ULPS, _g, same_kind  # noqa: F401

THREADS, PASSES = 256, 4   # a workgroup's threads and passes (seg_terms.hip: kSegThreads, kSegPasses)
LDS_CLASSES = 128          # the LDS counting route serves C <= this when rows_per_cloud >= rows_per_block(C)


def group_lanes(C):
    """lanes that own a row: the power of two covering C, at most 64"""
    g = 1
    while g < C and g < 64:
        g *= 2
    return g


def rows_per_block(C):
    return PASSES * (THREADS // group_lanes(C))


def blocks(R, C):
    return (R + rows_per_block(C) - 1) // rows_per_block(C)


# ------------------------------------------------------------------------------------------------ the terms, fp64
def terms(logits, labels, rows_per_cloud, weights=None):
    """logits (R,C) float32, labels (R,), weights (C,) float32 or None -> dict of fp64 / int64 arrays as the header defines them: ce
    (0 on an ignored row), pred, cloud_counts (R / rows_per_cloud, C, 3), means (3,), and the intermediates the bounds read."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    R, C = x.shape
    w_c = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    nan_row = np.isnan(x).any(1)
    valid = (lab >= 0) & (lab < C)
    safe = np.where(valid, lab, 0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mm = np.max(np.where(np.isnan(x), -np.inf, x), axis=1) if R else np.zeros(0)
        e = np.exp(x - mm[:, None])
        s = e.sum(1)
        lse = np.log(s) + mm
        xl = x[np.arange(R), safe]
        ce = np.where(valid, np.where(nan_row, np.nan, lse - xl), 0.0)
        w = np.where(valid, w_c[safe], 0.0)
        t = np.where(valid, w * ce, 0.0)
    pred = np.array([int(np.argmax(np.isnan(r))) if np.isnan(r).any() else int(np.argmax(r)) for r in x], dtype=np.int64).reshape(R)
    clouds = R // rows_per_cloud
    counts = np.zeros((clouds, C, 3), dtype=np.int64)
    cloud = np.arange(R) // rows_per_cloud
    ok = valid & (pred == lab)
    np.add.at(counts, (cloud[valid], lab[valid], 0), 1)
    np.add.at(counts, (cloud[valid], pred[valid], 1), 1)
    np.add.at(counts, (cloud[ok], lab[ok], 2), 1)
    nvalid, den = int(valid.sum()), float(w.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        means = np.array([np.float64(t.sum()) / np.float64(den), ok.sum() / nvalid if nvalid else 0.0, den])
    return {"ce": ce, "pred": pred, "cloud_counts": counts, "means": means, "m": mm, "s": s, "e": e, "lse": lse, "valid": valid,
            "x": x, "labels": lab, "w": w, "t": t, "weighted": weights is not None}


def upstream_coefficient(T, g_means, g_ce):
    """k_r = g_means[0] w_label / means[2] + g_ce[r] on the valid rows (a missing part left out) and K_r = the sum of the parts'
    magnitudes, fp64; 0 on the ignored rows."""
    R = len(T["ce"])
    z = np.zeros(R)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = z if g_means is None else np.where(T["valid"], float(g_means[0]) * T["w"] / T["means"][2], 0.0)
    c = z if g_ce is None else np.where(T["valid"], np.asarray(g_ce, dtype=np.float64), 0.0)
    return a + c, np.abs(a) + np.abs(c), np.abs(a)


def backward(T, g_means=None, g_ce=None):
    """fp64 g_logits (R,C) = k_r (softmax(x_r)_c - [c == label_r]); an ignored row is exactly zero."""
    R, C = T["x"].shape
    k, _, _ = upstream_coefficient(T, g_means, g_ce)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = T["e"] / T["s"][:, None]
        onehot = (np.arange(C)[None, :] == T["labels"][:, None]).astype(np.float64)
        g = k[:, None] * (p - onehot)
    g[~T["valid"]] = 0.0
    return g


# ------------------------------------------------------------------------------------------------ the bounds, counted
def _depth_row(C):
    """additions behind one term of a row sum: ceil(C / G) in the lane (the first onto 0.0f is exact but counted), log2 G butterfly levels"""
    G = group_lanes(C)
    return (C + G - 1) // G + int(np.log2(G))


def _rel_s(T):
    """relative error of s~ (finite rows), cls_terms_ref._rel_s with this kernel's depth: a term is expf(fl(x - m)): the subtraction's
    rounding U |d| moves exp by a relative |d| U, the call's ULPS ulps (2 U each), FLUSH where the result underflows; then the
    sum's depth on non-negative terms."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.where(np.isfinite(T["x"]), T["x"] - T["m"][:, None], 0.0))
        e = np.where(np.isfinite(T["e"]), T["e"], 0.0)
        per = (e * (1.01 * d * U + _g(2 * ULPS["expf"])) + FLUSH).sum(1) / T["s"]
    return per + _g(_depth_row(T["x"].shape[1]))


def bound_ce(T):
    """|ce~ - ce| on valid rows where ce is finite (an ignored row is exactly 0: bound 0): log(s~) - log(s) <= rel_s (1 + rel_s), +
    logf's ULPS ulps of |log s|; the addition of m: U |lse|; the subtraction of x_label: U |ce|."""
    rs = _rel_s(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        logs = np.abs(np.log(T["s"]))
        b = 1.01 * rs + _g(2 * ULPS["logf"]) * logs + _g(1) * np.abs(T["lse"]) + _g(1) * np.abs(T["ce"]) + TINY
    return np.where(T["valid"], b, 0.0)


def sum_chain(R, C):
    """the longest chain of additions behind one row's term of the batch sums: 4 passes in the group, 6 butterfly levels and 4 wave
    sums in the workgroup; in the closing launch ceil(blocks / 256) partials in a thread, 6 butterfly levels, 4 wave sums."""
    return PASSES + 6 + 4 + (blocks(R, C) + THREADS - 1) // THREADS + 6 + 4


def rel_den(T):
    """relative error of means[2]: with weights the chain on non-negative terms; without, the integer count converted once"""
    R, C = T["x"].shape
    return _g(sum_chain(R, C)) if T["weighted"] else _g(1)


def bound_means(T):
    """(3,) bounds.  means[0] = num / den: num's terms t_r = fl(w ce~) carry w bound_ce and the product's U |t| (none without
    weights, counted anyway), the chain gamma_k sum |t|; den's relative error moves the quotient by |num| / den times it; the division
    U |mean|.  means[1]: two conversions and one division of exact integers.  means[2]: rel_den."""
    R, C = T["x"].shape
    fin = T["valid"] & np.isfinite(T["ce"])
    den = T["means"][2]
    with np.errstate(invalid="ignore", divide="ignore"):
        abs_t = np.abs(np.where(fin, T["t"], 0.0)).sum()
        e_num = (T["w"] * np.where(fin, bound_ce(T), 0.0)).sum() + _g(1 + sum_chain(R, C)) * abs_t
        b0 = 1.01 * (e_num + abs_t * rel_den(T)) / den + _g(1) * np.abs(T["means"][0]) + TINY
    return np.array([b0, _g(3) * T["means"][1], rel_den(T) * den])


def bound_backward(T, g_means, g_ce):
    """(R,C) bound on |g~ - g| on finite rows: p = e / s as cls_terms_ref.bound_backward (e's relative error, s's rel_s, the division,
    the subtraction of the one-hot); k: the product g_means[0] w and the division by the kernel's own means[2] (2 U and rel_den on that
    part), the addition (U |k|); the final product U |g|."""
    R, C = T["x"].shape
    k, K, A = upstream_coefficient(T, g_means, g_ce)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.abs(np.where(np.isfinite(T["x"]), T["x"] - T["m"][:, None], 0.0))
        p = T["e"] / T["s"][:, None]
        relp = 1.01 * d * U + _g(2 * ULPS["expf"]) + _rel_s(T)[:, None] + _g(1)
        onehot = (np.arange(C)[None, :] == T["labels"][:, None]).astype(np.float64)
        diff = np.abs(p - onehot)
        ediff = 1.01 * (p * relp + FLUSH) + _g(1) * diff
        ek = (_g(2) + rel_den(T)) * A + _g(1) * K
        b = 1.01 * (K[:, None] * ediff + ek[:, None] * diff + _g(1) * np.abs(k)[:, None] * diff) + TINY
    return np.where(T["valid"][:, None], b, 0.0)


# ------------------------------------------------------------------------------------------------ the cases
# C: one per lane-group width (1, 2, 13 -> 16, 16, 17 -> 32, 50 -> 64, 64) and the two striding cases (65, 130: a lane's second and
# third class; 130 > 128 also takes the counting route without LDS).  (B, N): one row; clouds of 7 rows (boundaries inside a wave,
# the counting route without LDS); 2 x 100 and 5 x 257 (boundaries inside a workgroup and across workgroups, depending on C's rows per
# workgroup: 16 .. 1024); 2 x 1027 (several workgroups per cloud at every C but 1 and 2, a ragged last workgroup).
CLASSES = (1, 2, 13, 16, 17, 50, 64, 65, 130)
CLOUDS = ((1, 1), (3, 7), (2, 100), (5, 257), (2, 1027))
RECIPES = ("random", "ties", "nan_inf", "all_ignored", "cloud_ignored", "mixed_ignored")
WEIGHTS = ("none", "given", "zero_entry")


def seams(C):
    """class indices at the lane-group and 64-class seams of a row of C classes"""
    G = group_lanes(C)
    cand = (0, 1, G // 2 - 1, G // 2, G - 1, 31, 32, 63, 64, 65, 127, 128, 129, C - 2, C - 1)
    return sorted({c for c in cand if 0 <= c < C})


def make_case(recipe, B, N, C, seed=0):
    """-> logits (B * N, C) float32, labels (B * N,) int32."""
    rng = np.random.default_rng([seed, B, N, C, RECIPES.index(recipe)])
    R = B * N
    x = rng.standard_normal((R, C)).astype(np.float32) * 3
    lab = rng.integers(0, C, R).astype(np.int32)
    if recipe == "ties":          # small integers, the maximum planted twice at seam positions: the first must win
        x = rng.integers(-3, 3, (R, C)).astype(np.float32)
        sm = seams(C)
        for r in range(R):
            k = len(sm)
            a, b = sm[r % k], sm[(r % k + 1 + (r // k) % max(k - 1, 1)) % k]  # (two different seams whenever there are two)
            x[r, a] = 3
            x[r, b] = 3
            if r % 3 == 0:
                lab[r] = max(a, b)  # the label on the LATER maximum: not a correct point
    elif recipe == "nan_inf":     # a NaN behind a larger finite value, -inf on other classes, on the label, and a whole row
        for r in range(0, R, 5):
            x[r, (r // 5) % C] = np.nan
        for r in range(1, R, 5):
            x[r, (r // 5) % C] = -np.inf
        for r in range(2, R, 10):
            x[r, lab[r]] = -np.inf
        if R > 3:
            x[3] = -np.inf
    elif recipe == "all_ignored":
        lab[:] = -100
    elif recipe == "cloud_ignored":
        lab[(B - 1) * N:] = -1
    elif recipe == "mixed_ignored":
        bad = np.array([-100, -1, C, 255 if C <= 255 else C + 255, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
        pick = rng.random(R) < 0.4
        lab = np.where(pick, bad[rng.integers(0, len(bad), R)], lab).astype(np.int32)
    elif recipe != "random":
        raise KeyError(recipe)
    return x, lab


def make_weights(kind, C, seed=2):
    if kind == "none":
        return None
    w = np.random.default_rng([seed, C]).uniform(0.25, 4.0, C).astype(np.float32)
    if kind == "zero_entry":
        w[C // 2] = 0
    return w


def upstream_case(R, seed=1):
    """-> g_means (3,), g_ce (R,) float32; g_means[1:] are NaN: they must not be read."""
    rng = np.random.default_rng([seed, R])
    gm = rng.uniform(-2, 2, 3).astype(np.float32)
    gm[1:] = np.nan
    return gm, rng.uniform(-2, 2, R).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the aggregates
def aggregates_loop(pred, labels, num_classes, batch_means, categories=None, parts_of_category=None):
    """The evaluator's figures by a plain loop over clouds and points: pred / labels (clouds, N), batch_means [(loss, _, weight sum)]."""
    L, P, T = ([0] * num_classes for _ in range(3))
    cloud_iou = []
    for b in range(len(labels)):
        l, p, t = ([0] * num_classes for _ in range(3))
        for i in range(len(labels[b])):
            y, q = int(labels[b][i]), int(pred[b][i])
            if 0 <= y < num_classes:
                l[y] += 1
                p[q] += 1
                t[y] += int(q == y)
        for c in range(num_classes):
            L[c] += l[c]
            P[c] += p[c]
            T[c] += t[c]
        if parts_of_category is not None:
            ious = []
            for c in parts_of_category[int(categories[b])]:
                union = l[c] + p[c] - t[c]
                ious.append(1.0 if union == 0 else t[c] / union)
            cloud_iou.append(sum(ious) / len(ious))
    accs, ious = [], []
    for c in range(num_classes):
        if L[c] + P[c] == 0:
            continue
        accs.append(T[c] / L[c] if L[c] else 0.0)
        ious.append(T[c] / (L[c] + P[c] - T[c]))
    num = sum(float(m[0]) * float(m[2]) for m in batch_means if float(m[2]) > 0)
    den = sum(float(m[2]) for m in batch_means)
    out = {"total_valid": sum(L), "overall_accuracy": sum(T) / sum(L) if sum(L) else float("nan"),
           "class_labelled": np.array(L), "class_predicted": np.array(P), "class_correct": np.array(T),
           "mean_class_accuracy": sum(accs) / len(accs) if accs else float("nan"), "miou": sum(ious) / len(ious) if ious else float("nan"),
           "mean_loss": num / den if den > 0 else float("nan")}
    if parts_of_category is not None:
        per_cat = {}
        for b, v in enumerate(cloud_iou):
            per_cat.setdefault(int(categories[b]), []).append(v)
        cat_means = [sum(v) / len(v) for v in per_cat.values()]
        out.update({"cloud_iou": np.array(cloud_iou), "instance_miou": sum(cloud_iou) / len(cloud_iou),
                    "category_miou": sum(cat_means) / len(cat_means)})
    return out

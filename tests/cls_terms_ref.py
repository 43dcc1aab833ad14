"""Test helper for the classification-term tests (tests/test_cls_terms_host.py, tests/test_gpu_cls_terms.py,
tests/test_gpu_task_evaluation.py): the fp64 restatement of sn_classification_terms_forward / _backward as
include/samplenet_hip_internal.h specifies them, the shape table, the input recipes, the aggregates of
classification/evaluate_samplenet.py:156-277 restated, and the error bounds -- every bound COUNTED from the roundings of
samplenet_amd/csrc/cls_terms.hip (compiled without contraction: one rounding per written operation), none fitted to an observed
error.  The observed maxima are recorded beside them in profiles/eval/errors.txt.  Lives in tests/ on purpose: nothing here is a
product route."""
import numpy as np

U = 2.0 ** -24       # unit roundoff of float32
TINY = 2.0 ** -149   # one subnormal step
FLUSH = 2.0 ** -126  # what an exponential that underflows may lose if subnormal results are flushed
# Allowed error of the device's library calls in ulps of the result (1 ulp <= 2 U |result|): the figure HIP's math API documents
# for the fp32 function the kernel calls (expf 1, logf 1), doubled, as tests/batch_ref.py ULPS.  Measured on an MI355X over the
# arguments the kernel can hand them (tools/micro/cls_math_error.hip; profiles/eval/errors.txt): both below the charged figure.
ULPS = {"expf": 2.0, "logf": 2.0}
WAVES = 16           # rows in flight in the one workgroup of the forward: wave w adds rows w, w + 16, ...


def _g(k):
    """a chain of k roundings, with the factor 1.01 for second order"""
    return 1.01 * k * U


# ------------------------------------------------------------------------------------------------ the terms, fp64
def terms(logits, labels):
    """logits (B,C) float32, labels (B,) -> dict of fp64 arrays as the header defines them: ce, pred, correct, means (2,), and the
    intermediates the bounds read (m, s, e = exp(x - m), lse).  Edge cases as the header: bad label -> ce NaN / correct 0; NaN
    logit -> ce NaN and pred = first NaN; label at -inf -> +inf; all -inf -> NaN."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    B, C = x.shape
    nan_row = np.isnan(x).any(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mm = np.max(np.where(np.isnan(x), -np.inf, x), axis=1)
        e = np.exp(x - mm[:, None])
        s = e.sum(1)
        lse = np.log(s) + mm
        inside = (lab >= 0) & (lab < C)
        xl = x[np.arange(B), np.where(inside, lab, 0)]
        ce = np.where(inside & ~nan_row, lse - xl, np.nan)
    pred = np.array([int(np.argmax(np.isnan(r))) if np.isnan(r).any() else int(np.argmax(r)) for r in x], dtype=np.int64).reshape(B)
    correct = (inside & (pred == lab)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        means = np.array([ce.sum() / B, correct.sum() / B]) if B else np.zeros(2)
    return {"ce": ce, "pred": pred, "correct": correct, "means": means, "m": mm, "s": s, "e": e, "lse": lse, "inside": inside,
            "x": x, "labels": lab}


def upstream_weights(B, g_means, g_ce):
    """w_b = g_means[0] / B + g_ce[b] (a missing part left out) and W_b = the sum of the parts' magnitudes, fp64."""
    z = np.zeros(B)
    a = z if g_means is None else z + float(g_means[0]) / B
    c = z if g_ce is None else np.asarray(g_ce, dtype=np.float64)
    return a + c, np.abs(a) + np.abs(c)


def backward(logits, labels, g_means=None, g_ce=None):
    """fp64 g_logits (B,C) = w_b (softmax(x_b)_c - [c == label_b]); a bad label gives a NaN row."""
    T = terms(logits, labels)
    B, C = T["x"].shape
    w, _ = upstream_weights(B, g_means, g_ce)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = T["e"] / T["s"][:, None]
        onehot = (np.arange(C)[None, :] == T["labels"][:, None]).astype(np.float64)
        g = w[:, None] * (p - onehot)
    g[~T["inside"]] = np.nan
    return g


# ------------------------------------------------------------------------------------------------ the bounds, counted
def _depth_row(C):
    """additions behind one term of a row sum: ceil(C / 64) in the lane (the first onto 0.0f is exact but counted), 6 butterfly levels"""
    return (C + 63) // 64 + 6


def _rel_s(T):
    """relative error of s~ (finite rows): a term is expf(fl(x - m)): the subtraction's rounding U |d| moves exp by a relative
    |d| U (d = x - m <= 0; e^d |d| <= 1/e keeps this small where it matters), the call's ULPS ulps (2 U each), FLUSH
    where the result underflows; then the sum's depth on non-negative terms.  -> sum_c e_c (|d_c| U + 2 ULPS U) / s + gamma_depth."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.where(np.isfinite(T["x"]), T["x"] - T["m"][:, None], 0.0))
        e = np.where(np.isfinite(T["e"]), T["e"], 0.0)
        per = (e * (1.01 * d * U + _g(2 * ULPS["expf"])) + FLUSH).sum(1) / T["s"]
    return per + _g(_depth_row(T["x"].shape[1]))


def bound_ce(T):
    """|ce~ - ce| on rows where ce is finite: log(s~) - log(s) <= rel_s (1 + rel_s), + logf's ULPS ulps of |log s|; the addition of
    m: U |lse|; the subtraction of x_label: U |ce|; the inherited error passes both unchanged."""
    rs = _rel_s(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        logs = np.abs(np.log(T["s"]))
        return 1.01 * rs + _g(2 * ULPS["logf"]) * logs + _g(1) * np.abs(T["lse"]) + _g(1) * np.abs(T["ce"]) + TINY


def bound_mean_ce(T):
    """means[0]: the mean of the per-row bounds, + the fixed-order sum: a row's ce passes ceil(B / 16) additions in its wave, 16
    additions of wave sums and the division."""
    B = len(T["ce"])
    k = (B + WAVES - 1) // WAVES + WAVES + 1
    return np.sum(bound_ce(T)) / B + _g(k) * np.sum(np.abs(T["ce"])) / B


def bound_backward(T, g_means, g_ce):
    """(B,C) bound on |g~ - g| on finite rows: p = e / s: e's relative error (|d| U + 2 ULPS U), s's rel_s, the division U; the
    subtraction of the one-hot: U |p - 1h|; w: the division by B and the addition, 2 U W; the product U |g|."""
    B, C = T["x"].shape
    w, W = upstream_weights(B, g_means, g_ce)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.abs(np.where(np.isfinite(T["x"]), T["x"] - T["m"][:, None], 0.0))
        p = T["e"] / T["s"][:, None]
        relp = 1.01 * d * U + _g(2 * ULPS["expf"]) + _rel_s(T)[:, None] + _g(1)
        onehot = (np.arange(C)[None, :] == T["labels"][:, None]).astype(np.float64)
        diff = np.abs(p - onehot)
        ediff = 1.01 * (p * relp + FLUSH) + _g(1) * diff
        return 1.01 * (W[:, None] * ediff + _g(2) * W[:, None] * diff + _g(1) * np.abs(w)[:, None] * diff) + TINY


def means_in_kernel_order(ce):
    """float32 (B,) -> means[0] as the one-workgroup forward adds it: wave w's rows ascending from 0, the 16 wave sums ascending
    from 0, one float32 division."""
    v = np.asarray(ce, dtype=np.float32)
    part = np.zeros(WAVES, dtype=np.float32)
    for b in range(len(v)):
        part[b % WAVES] = part[b % WAVES] + v[b]
    tot = np.float32(0)
    for w in range(WAVES):
        tot = np.float32(tot + part[w])
    return np.float32(tot / np.float32(len(v)))


# ------------------------------------------------------------------------------------------------ the cases
# (B, C).  C: 1 (ce = 0), 2, 40 (ModelNet40: fewer classes than lanes), 63 / 64 / 65 (around the 64 lanes of the class stride), 129
# (a lane's third class), 1024 (16 classes a lane).  B: 1, 2, 3, 5 (fewer rows than the 16 waves), 17 (a wave's second row: the batch
# sum's second trip), 33 (third trip), 257 and 513 (rows >> waves; the wave sums' depth 17 and 33).  With the means the forward is one
# workgroup; without them 16 rows per workgroup: 17 / 33 / 257 / 513 are then 2 / 3 / 17 / 33 workgroups.
SHAPES = ((1, 1), (1, 2), (2, 40), (3, 63), (3, 64), (3, 65), (5, 129), (2, 1024), (17, 40), (33, 40), (257, 40), (513, 3))
RECIPES = ("normal", "large", "ties", "equal", "inf_others", "inf_label", "inf_row", "nan", "bad_label")


def make_case(recipe, B, C, seed=0):
    """-> logits (B,C) float32, labels (B,) int32."""
    rng = np.random.default_rng([seed, B, C, RECIPES.index(recipe)])
    x = rng.standard_normal((B, C)).astype(np.float32) * 3
    lab = rng.integers(0, C, B).astype(np.int32)
    if recipe == "large":        # a sum without the max subtraction overflows
        x = (rng.uniform(-1, 1, (B, C)) * 1e4).astype(np.float32)
    elif recipe == "ties":       # small integers, the maximum repeated (first maximum wins); label on a late maximum in row 0
        x = rng.integers(-3, 3, (B, C)).astype(np.float32)
        x[:, C // 2] = 3
        x[:, C - 1] = 3
        lab[0] = C - 1
    elif recipe == "equal":
        x[:] = np.float32(0.75)
    elif recipe == "inf_others":  # -inf on classes other than the label
        for b in range(B):
            for c in range(C):
                if c != lab[b] and (c + b) % 3 == 0:
                    x[b, c] = -np.inf
    elif recipe == "inf_label":  # -inf on the label (C = 1: the row is all -inf)
        x[np.arange(B), lab] = -np.inf
    elif recipe == "inf_row":
        x[B // 2] = -np.inf
    elif recipe == "nan":        # one NaN in row 0, past a larger finite value when the row allows
        x[0, C - 1] = np.nan
        if B > 1 and C > 2:
            x[B - 1, 1] = np.nan
            x[B - 1, 2] = np.nan
    elif recipe == "bad_label":
        lab[0] = -1
        lab[B - 1] = C if B > 1 else -1
        if B > 2:
            lab[1] = 2 ** 31 - 1
    elif recipe != "normal":
        raise KeyError(recipe)
    return x, lab


def upstream_case(B, seed=1):
    """-> g_means (2,), g_ce (B,) float32; g_means[1] is a NaN: it must not be read."""
    rng = np.random.default_rng([seed, B])
    gm = rng.uniform(-2, 2, 2).astype(np.float32)
    gm[1] = np.nan
    return gm, rng.uniform(-2, 2, B).astype(np.float32)


def same_kind(a, b):
    """non-finite entries of a and b at the same places and of the same kind (NaN / +inf / -inf)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


# ------------------------------------------------------------------------------------------------ the aggregates
def aggregates_restated(batches, num_classes):
    """classification/evaluate_samplenet.py:156-277 restated over `batches` = [(pred_val (B_j,), labels (B_j,), loss_val_j,
    n_unique (B_j,))]: the running totals of lines 158-163, the per-batch updates of 227-228 and 244-257, the figures of 260-275."""
    total_correct = 0
    total_seen = 0
    loss_sum = 0
    num_unique_idx = 0
    total_seen_class = [0 for _ in range(num_classes)]
    total_correct_class = [0 for _ in range(num_classes)]
    for pred_val, labels, loss_val, n_unique in batches:
        cur_batch_size = len(labels)
        for ii in range(cur_batch_size):
            num_unique_idx += int(n_unique[ii])
        batch_loss_sum = float(loss_val) * cur_batch_size
        correct = np.sum(np.asarray(pred_val) == np.asarray(labels))
        total_correct += correct
        total_seen += cur_batch_size
        loss_sum += batch_loss_sum
        for i in range(cur_batch_size):
            l = int(labels[i])
            total_seen_class[l] += 1
            total_correct_class[l] += int(pred_val[i] == l)
    with np.errstate(invalid="ignore", divide="ignore"):
        class_accuracies = np.array(total_correct_class) / np.array(total_seen_class, dtype=np.float64)
    return {"total_seen": total_seen, "mean_loss": loss_sum / float(total_seen), "accuracy": total_correct / float(total_seen),
            "class_seen": np.array(total_seen_class), "class_correct": np.array(total_correct_class),
            "class_accuracies": class_accuracies, "avg_class_accuracy": np.mean(class_accuracies),
            "mean_unique": num_unique_idx / float(total_seen)}

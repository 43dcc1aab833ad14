"""Test helper for tests/test_emd_host.py and tests/test_gpu_emd_direct.py: a plain float64 restatement of the EMD family
(approx_match / match_cost / match_cost_grad, the algorithm documented above orc_approxmatch in oracle/samplenet_oracle.c),
the input recipes, the shape table -- one row per branch of samplenet_amd/csrc/emd.hip, each naming the branch it exists for --
the bars against float64 and the admission rule that decides which (shape, recipe, seed) cases those bars are asserted at.
Nothing here runs on a GPU or calls the library's compute entries.  Lives in tests/ on purpose: nothing here is a product route.

Bars (the ones tests/test_gpu_emd.py holds against the fp32 oracle, here against float64):
    match          5e-4 per entry, mean 1e-7 (the mean is NOT asserted at shapes with n m < 4096: a few dozen entries of ~0.2 each
                   have no small mean error to speak of)
    cost           1e-5 relative
    gradients      5e-3 of the gradient's largest component, 1e-4 of its norm
    recipe `same`  cost and gradients are near zero, so their own magnitude is no scale: cost against S = (sum of the float64
                   match) x (the diameter of the two clouds), gradients against multiL multiR (|grad1_k| <= sum_l match[l,k] <= multiL,
                   |grad2_l| <= multiR), with the same factors
    ratio vectors  the match bar scaled by multiL multiR, element by element against float64:
                   ratioR at all ten levels, absolute (ratioR <= remainR <= multiR, and min(., 1) remainR damps a cancelled residue);
                   ratioL at every level on the elements the float64 run shows WELL-POSED -- those whose point still holds at least
                   HELD = 1/2 of its mass multiL before the level (all of them at level 1) --, relative to the element where it
                   exceeds 1 (an isolated point's exponentials all underflow at level -16384: ratioL = multiL / 1e-9).
                   ratioL = remainL / (1e-9 + sum_l exp(.) remainR[l]) of a SERVED point is ill-posed in float32: its remainL is a
                   difference that has cancelled to rounding noise (1e-8 where float64 has 1e-12), divided by a sum that may be as
                   small -- a plain float32 numpy evaluation of the algorithm is off by factors there, the device by 0.03 .. 30
                   relative to max(1, |element|).  Those elements are held through the match all the vectors define, sum over levels
                   of exp(level d2) ratioL[k] ratioR[l] evaluated in float64 from the device's vectors, under the match bar: the small
                   denominator that amplifies such a ratio's error also bounds what it can add to a match entry.

Admission rule: a case is asserted under these bars only if the REFERENCE ALONE stays within 1/4 of each of them -- for the
compensated-exponential entries (sn_approxmatch, sn_emd_loss) the fp32 oracle against float64, for sn_emd_loss_fast additionally the
float64 computation with the exponential's argument rounded as the kernel's fast form rounds it (fast_exp=True, a CPU model of the
reference op's own __expf) against float64, on the outputs that entry has (cost, gradients).  The kernel performs the oracle's
operations regrouped at segment and tile borders, so it sits at the oracle's own distance from float64 times a small factor; the
auction amplifies last-bit differences through its ten levels, and a case where the oracle itself is near a bar says nothing about a
kernel that misses it.  The oracle hands out no ratio vectors: for them the reference alone is approx_match_fp32, a plain float32
numpy evaluation of the same passes (numpy's own summation order, libm's expf).  CASE_SEEDS holds one admitted seed per (shape, recipe); tests/test_emd_host.py re-checks every one of them."""
import functools

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)  # j = 7 .. -1, then 0 at j == -2
FLOOR = float(np.float32(1e-9))    # the kernels' 1e-9f
CLAMP = float(np.float32(1e-20))   # the gradient's max(d2, 1e-20f)
LOG2E_HI = float(np.float32(1.4426950408889634))  # kLog2eHi of emd.hip: log2(e) rounded to float32

MATCH_ABS, MATCH_MEAN, COST_REL, GRAD_MAX, GRAD_NORM = 5e-4, 1e-7, 1e-5, 5e-3, 1e-4
MEAN_FROM = 4096  # the mean bar is asserted from n m >= 4096
HELD = 0.5        # a point "still holds its mass" while float64 remain >= HELD multi; below, it counts as served
RESIDUE = 64 * U  # what a served point's remain may carry in float32 instead of ~0, per unit of multi: a few dozen roundings


# ------------------------------------------------------------------------------------------------ the shape table
def seg_plan(b, nself, nother):
    """emd_seg_plan of emd.hip: (ranges, points per range) of the other cloud for one level pass."""
    if nother <= 0:
        return 1, 0
    base = b * ((nself + 255) // 256)
    s = (2048 + base - 1) // base if base > 0 else 1
    s = max(1, min(s, nother // 256))
    length = ((nother + s - 1) // s + 63) // 64 * 64
    nseg = (nother + length - 1) // length
    return (1, nother) if nseg <= 1 else (nseg, length)


def seg_ranges(b, nself, nother):
    nseg, length = seg_plan(b, nself, nother)
    return tuple(min(nother, (q + 1) * length) - q * length for q in range(nseg))


# (b, n, m): the branch the row exists for; pass k sweeps xyz2 (m points) per xyz1 point, pass l sweeps xyz1
SHAPES = (
    ((3, 7, 5), "n > m not divisible; everything ragged: the 16-row materialise grid, the 4-row grad2 grid, one 64-tile; P1 unaligned before the fix"),
    ((2, 64, 64), "exact 64-tiles, n = m (the diagonal property of `same`)"),
    ((2, 65, 129), "one element past a 64-tile on both axes; n < m with multiL = 1"),
    ((2, 100, 300), "multiL = 3; crosses the 256-point loss tile; no segments"),
    ((1, 600, 300), "only pass l is segmented (2 ranges, 320 + 280)"),
    ((1, 300, 600), "only pass k is segmented (2 ranges, 320 + 280)"),
    ((1, 520, 600), "both passes segmented, both with a ragged last range (320 + 280, 320 + 200)"),
    ((1, 100, 800), "three ranges (320, 320, 160) in pass k; multiL = 8"),
    ((1, 1030, 70), "segments off: pass l crosses the 1024-point LDS tile by 6 points; segments on: four ranges (320, 320, 320, 70)"),
)
SEGMENTED = ((1, 600, 300), (1, 300, 600), (1, 520, 600), (1, 100, 800), (1, 1030, 70))
RECIPES = ("cube", "sphere", "noisy", "same", "cluster", "apart", "big")


def multis(n, m):
    """multiL, multiR by integer division (tf_approxmatch_g.cu:3-10)."""
    return (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)


# ------------------------------------------------------------------------------------------------ inputs
def cluster_len(n):
    """points of the repeated group of recipe `cluster`: the first quarter of the cloud, at least two."""
    return max(2, (n + 3) // 4)


def make(recipe, b, n, m, seed):
    """-> x1 (b, n, 3), x2 (b, m, 3) float32."""
    rng = np.random.default_rng([seed, b, n, m, RECIPES.index(recipe)])
    x1 = rng.random((b, n, 3), dtype=np.float32)
    x2 = rng.random((b, m, 3), dtype=np.float32)
    if recipe == "sphere":  # centred unit ball: negative coordinates
        def ball(k):
            v = rng.standard_normal((b, k, 3))
            v /= np.linalg.norm(v, axis=2, keepdims=True)
            return (v * rng.random((b, k, 1)) ** (1.0 / 3.0)).astype(np.float32)
        x1, x2 = ball(n), ball(m)
    elif recipe == "noisy":  # the regime a trained autoencoder produces: a near-copy, the transport plan is sharp
        x1 = (x2[:, np.arange(n) % m] + 0.01 * rng.standard_normal((b, n, 3))).astype(np.float32)
    elif recipe == "same":  # bit for bit
        k = min(n, m)
        x1[:, :k] = x2[:, :k]
    elif recipe == "cluster":  # coincident points inside each cloud
        x1[:, :cluster_len(n)] = x1[:, :1]
        x2[:, :cluster_len(m)] = x2[:, :1]
    elif recipe == "apart":  # every high level underflows, the 1e-9 floor governs
        x2 = x2 + np.float32(3.0)
    elif recipe == "big":
        x1, x2 = x1 * np.float32(20.0), x2 * np.float32(20.0)
    return np.ascontiguousarray(x1, dtype=np.float32), np.ascontiguousarray(x2, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ float64 references
def sqdist(x1, x2):
    """(b, n, m) float64 squared distances of float32 clouds (the differences of float32 numbers are formed in float64)."""
    d = np.asarray(x1, np.float64)[:, :, None, :] - np.asarray(x2, np.float64)[:, None, :, :]
    return (d * d).sum(-1)


def approx_match_fp64(x1, x2, fast_exp=False):
    """The auction in float64.  -> match (b, m, n), [(ratioL (b, n), ratioR (b, m), whether ratioL[k] is well-posed (b, n)) for each
    of the ten levels].
    fast_exp: the exponential's argument rounded as emd_exp2<true> rounds it -- y = fl32(fl32(d2) fl32(level log2 e)) --, then 2^y
    exactly; everything else unchanged."""
    b, n, _ = x1.shape
    m = x2.shape[1]
    d2 = sqdist(x1, x2)  # [b, k, l]
    multiL, multiR = multis(n, m)
    remainL, remainR = np.full((b, n), multiL), np.full((b, m), multiR)
    match = np.zeros((b, m, n))
    ratios = []
    d2f = d2.astype(np.float32).astype(np.float64)
    for level in LEVELS:
        if fast_exp:
            y = (d2f * (level * LOG2E_HI)).astype(np.float32).astype(np.float64)  # (level log2e_hi is exact: a power of two)
            E = np.exp2(y)
        else:
            E = np.exp(level * d2)
        den = FLOOR + (E * remainR[:, None, :]).sum(2)
        served = (E * (remainR < HELD * multiR)[:, None, :]).sum(2)  # sum of exp(.) over the right points already served
        held = (remainL >= HELD * multiL) & (RESIDUE * multiR * served <= 0.2 * MATCH_ABS * den)
        ratioL = remainL / den
        sumr = (E * ratioL[:, :, None]).sum(1) * remainR
        ratioR = np.minimum(remainR / (sumr + FLOOR), 1.0) * remainR
        remainR = np.maximum(0.0, remainR - sumr)
        w = E * ratioL[:, :, None] * ratioR[:, None, :]
        match += w.transpose(0, 2, 1)
        remainL = np.maximum(0.0, remainL - w.sum(2))
        ratios.append((ratioL, ratioR, held))
    return match, ratios


def approx_match_fp32(x1, x2):
    """The same passes in float32 numpy (every product, sum and quotient rounded to float32; numpy's summation order, not the
    kernels') -> the ratio vectors in ratio_block()'s layout.  What ANY float32 evaluation leaves in them: the reference-alone side of
    the admission rule for the ratio vectors."""
    f = np.float32
    b, n, _ = x1.shape
    m = x2.shape[1]
    d = x2[:, None, :, :] - x1[:, :, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    multiL, multiR = multis(n, m)
    remainL, remainR = np.full((b, n), multiL, f), np.full((b, m), multiR, f)
    rl, rr = [], []
    for level in LEVELS:
        E = np.exp(f(level) * d2)
        ratioL = remainL / (f(1e-9) + (E * remainR[:, None, :]).sum(2, dtype=f))
        sumr = (E * ratioL[:, :, None]).sum(1, dtype=f) * remainR
        ratioR = np.minimum(remainR / (sumr + f(1e-9)), f(1)) * remainR
        remainR = np.maximum(f(0), remainR - sumr)
        remainL = np.maximum(f(0), remainL - (E * ratioL[:, :, None] * ratioR[:, None, :]).sum(2, dtype=f))
        rl.append(ratioL)
        rr.append(ratioR)
    assert ratioL.dtype == f and ratioR.dtype == f
    return np.concatenate(rl + rr, 1)


def match_cost_fp64(x1, x2, match, absolute=False):
    """cost (b) = sum_{k,l} match[l,k] |x1_k - x2_l|; absolute: the sum of |terms| instead."""
    t = np.asarray(match, np.float64).transpose(0, 2, 1) * np.sqrt(sqdist(x1, x2))
    return (np.abs(t) if absolute else t).sum((1, 2))


def match_cost_grad_fp64(x1, x2, match, absolute=False):
    """grad1 (b, n, 3) = sum_l match[l,k] (x1_k - x2_l) / sqrt(max(d2, 1e-20)), grad2 (b, m, 3) the same from the other side;
    absolute: the sums of |terms| instead."""
    e = np.asarray(x1, np.float64)[:, :, None, :] - np.asarray(x2, np.float64)[:, None, :, :]  # [b, k, l, 3]
    g = np.asarray(match, np.float64).transpose(0, 2, 1) / np.sqrt(np.maximum((e * e).sum(-1), CLAMP))
    t = e * g[..., None]
    if absolute:
        return np.abs(t).sum(2), np.abs(t).sum(1)
    return t.sum(2), -t.sum(1)


def diameter(x1, x2):
    """(b) the largest distance between two points of the two clouds taken together."""
    x = np.concatenate([x1, x2], 1)
    return np.sqrt(sqdist(x, x).max((1, 2)))


class Ref:
    """Inputs and float64 results of one case, computed once and left unchanged."""

    def __init__(self, shape, recipe, seed):
        self.shape, self.recipe, self.seed = shape, recipe, seed
        b, n, m = shape
        self.x1, self.x2 = make(recipe, b, n, m, seed)
        self.match, self.ratios = approx_match_fp64(self.x1, self.x2)
        self.cost = match_cost_fp64(self.x1, self.x2, self.match)
        self.grad1, self.grad2 = match_cost_grad_fp64(self.x1, self.x2, self.match)
        self.mlmr = multis(n, m)[0] * multis(n, m)[1]
        self.S = self.match.sum((1, 2)) * diameter(self.x1, self.x2)
        for a in (self.x1, self.x2, self.match, self.cost, self.grad1, self.grad2):
            a.setflags(write=False)

    @functools.cached_property
    def fast(self):
        """(cost, grad1, grad2) of the fast_exp model."""
        mt, _ = approx_match_fp64(self.x1, self.x2, fast_exp=True)
        return (match_cost_fp64(self.x1, self.x2, mt),) + match_cost_grad_fp64(self.x1, self.x2, mt)

    def ratio_block(self):
        """The ten ratio-vector pairs laid out as the workspace holds them per cloud: ratioL[10][n] then ratioR[10][m] -> (b, 10 (n + m))."""
        return np.concatenate([np.concatenate([r[0] for r in self.ratios], 1), np.concatenate([r[1] for r in self.ratios], 1)], 1)

    def well_posed(self):
        """(b, 10 n) bool: the ratioL elements asserted one by one (see the module docstring)."""
        return np.concatenate([r[2] for r in self.ratios], 1)


def match_from_ratios(x1, x2, block):
    """match (b, m, n) = sum over levels of exp(level d2) ratioL[level][k] ratioR[level][l] in float64, from a ratio_block()-shaped
    array (the device's, read out of the workspace)."""
    b, n, _ = x1.shape
    m = x2.shape[1]
    d2 = sqdist(x1, x2)
    block = np.asarray(block, np.float64)
    rl, rr = block[:, :10 * n].reshape(b, 10, n), block[:, 10 * n:].reshape(b, 10, m)
    match = np.zeros((b, m, n))
    for li, level in enumerate(LEVELS):
        match += (np.exp(level * d2) * rl[:, li, :, None] * rr[:, li, None, :]).transpose(0, 2, 1)
    return match


@functools.lru_cache(maxsize=None)
def reference(shape, recipe, seed):
    return Ref(tuple(shape), recipe, seed)


# ------------------------------------------------------------------------------------------------ figures and bars
def figures(ref, match=None, cost=None, grad1=None, grad2=None, ratios=None):
    """{name: (distance from float64, bar)} for every output given (numpy arrays of the outputs' shapes; ratios: ratio_block()'s)."""
    b, n, m = ref.shape
    same = ref.recipe == "same"
    out = {}
    if match is not None:
        d = np.abs(np.asarray(match, np.float64) - ref.match)
        out["match"] = (float(d.max()), MATCH_ABS)
        if n * m >= MEAN_FROM:
            out["match mean"] = (float(d.mean()), MATCH_MEAN)
    if cost is not None:
        scale = ref.S if same else np.abs(ref.cost)
        out["cost"] = (float((np.abs(np.asarray(cost, np.float64) - ref.cost) / scale).max()), COST_REL)
    for name, g, rg in (("grad1", grad1, ref.grad1), ("grad2", grad2, ref.grad2)):
        if g is None:
            continue
        d = np.asarray(g, np.float64) - rg
        out[name + " max"] = (float(np.abs(d).max() / (ref.mlmr if same else np.abs(rg).max())), GRAD_MAX)
        out[name + " norm"] = (float(np.linalg.norm(d) / (ref.mlmr if same else np.linalg.norm(rg))), GRAD_NORM)
    if ratios is not None:
        want, got = ref.ratio_block(), np.asarray(ratios, np.float64)
        out["ratioR"] = (float(np.abs(got[:, 10 * n:] - want[:, 10 * n:]).max()), MATCH_ABS * ref.mlmr)
        wp = ref.well_posed()
        assert wp[:, :n].all()  # level 1: every point holds multiL
        d = np.abs(got[:, :10 * n] - want[:, :10 * n]) / np.maximum(1.0, np.abs(want[:, :10 * n]))
        out["ratioL held"] = (float(d[wp].max()), MATCH_ABS * ref.mlmr)
        out["ratios as match"] = (float(np.abs(match_from_ratios(ref.x1, ref.x2, got) - ref.match).max()), MATCH_ABS)
    return out


def misses(fig, fraction=1.0):
    """the figures beyond `fraction` of their bar (NaN counts as beyond)."""
    return {k: v for k, v in fig.items() if not v[0] <= fraction * v[1]}


def show(tag, fig):
    return "%-34s " % tag + "  ".join("%s %.1e" % (k, v[0]) for k, v in fig.items())


def oracle_figures(O, ref):
    """The fp32 oracle's own distance from float64: match, and cost / gradients of the oracle's match."""
    om = O.approxmatch(ref.x1, ref.x2)
    g1, g2 = O.matchcost_grad(ref.x1, ref.x2, om)
    return figures(ref, match=om, cost=O.matchcost(ref.x1, ref.x2, om), grad1=g1, grad2=g2)


def fast_figures(ref):
    """The fast_exp model's distance from float64 on what sn_emd_loss_fast hands out."""
    c, g1, g2 = ref.fast
    return figures(ref, cost=c, grad1=g1, grad2=g2)


def fp32_ratio_figures(ref):
    """The plain float32 evaluation's ratio vectors against float64's, on the elements and under the bars the device's are held to."""
    fig = figures(ref, ratios=approx_match_fp32(ref.x1, ref.x2))
    return {k: fig[k] for k in ("ratioR", "ratioL held")}


def admitted(O, ref):
    """-> (bool, oracle figures (+ the float32 evaluation's ratio figures), fast-model figures)."""
    fo, ff = oracle_figures(O, ref), fast_figures(ref)
    fo.update(fp32_ratio_figures(ref))
    return not misses(fo, 0.25) and not misses(ff, 0.25), fo, ff


# ------------------------------------------------------------------------------------------------ the admitted cases
# (shape, recipe) -> seed: the first seed of 0 .. 9 under which the case meets the admission rule (tools-free: admitted() above;
# tests/test_emd_host.py::test_every_case_of_the_table_is_admitted re-checks each).  A pair that no seed of 0 .. 9 admits is absent and
# listed in NOT_ADMITTED with the figure that kept it out.
_OTHER_SEED = {  # seed 0 unless listed: at the seeds before the listed one the ORACLE is beyond 1/4 of a bar (match 1.3e-4 .. 3.2e-4 per entry,
    # or its mean 4.4e-8 .. 1.9e-7 at 64 x 64, or the norm of a `same` gradient 4.4e-5 .. 2.1e-4)
    ((2, 64, 64), "cube"): 1, ((2, 64, 64), "big"): 3, ((2, 65, 129), "big"): 1, ((1, 600, 300), "same"): 1,
    ((1, 300, 600), "cube"): 1, ((1, 300, 600), "noisy"): 1, ((1, 300, 600), "same"): 1, ((1, 520, 600), "cube"): 1,
    ((1, 520, 600), "big"): 9,  # (seeds 1, 2, 6 pass on match; the float32 evaluation's ratioR / held ratioL sit at 2.9e-4 / 1.4e-4 / 1.7e-4)
}
NOT_ADMITTED = {}  # every (shape, recipe) pair of the table has an admitted seed
CASE_SEEDS = {(s, r): _OTHER_SEED.get((s, r), 0) for s, _ in SHAPES for r in RECIPES if (s, r) not in NOT_ADMITTED}


def cases(shapes=None, recipes=None):
    """[(shape, recipe, seed)] of the admitted cases, in table order."""
    return [(s, r, CASE_SEEDS[(s, r)]) for s, _ in SHAPES for r in RECIPES
            if (s, r) in CASE_SEEDS and (shapes is None or s in shapes) and (recipes is None or r in recipes)]


def case_id(c):
    return "%dx%dx%d-%s-s%d" % (c[0] + (c[1], c[2]))

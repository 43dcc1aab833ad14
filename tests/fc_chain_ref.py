"""Plain fp64 restatement of the FC-chain entries (sn_fc_chain_forward, _forward_pool, _forward_pool_out, sn_fc_chain_backward, _backward_obn:
csrc/fc_chain.hip),
the data the tests feed them, the shape tables (one row per branch of the two kernels) and drivers that call the raw entries through
samplenet_amd._lib with every output, the exchange slabs and the `sync` state as views into sentinel-filled buffers (tests/skinny_ref.py:
Guarded, Launch).  Imported by tests/test_fc_chain_host.py (no GPU: the recipes and tables) and tests/test_gpu_fc_chain.py (the calls).
The references are torch in fp64 and call nothing of the library; every generator takes the device, so the host test runs them on the CPU.

Error bounds are first order and component-wise, counted from the kernels' operations (the count stands next to the line it bounds):
U = 2^-24 is one fp32 rounding; a GEMM of K terms costs (K + 8) U times the magnitude product (the project's figure, profiles/skinny);
a col_sum_seq over R rows costs (R + 3) U times the sum of magnitudes (at most R - 1 adds along the rows' lane chain + 3 DPP adds);
what the kernels compute in double costs nothing until it is stored as fp32 (one U)."""
import ctypes
import os
import re

import torch

from skinny_ref import SENTINEL, Guarded, Launch

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNC_WORDS, SYNC_STRIDE = 16, 32  # 16 words of state, 128 bytes apart (csrc/sn_common.h: kFcSyncStride)
H = 256
EPS, MOMENTUM = float(torch.tensor(1e-5).item()), float(torch.tensor(0.1).item())  # the fp32 values the entries receive, as doubles

# ---- shape tables ----------------------------------------------------------------------------------------------------------------
# forward (C0, nl) -> (branch it reaches, supported).  nl = 4 never fits: the LDS formula (fwd_lds_bytes below) needs 171 520 bytes at
# C0 = 64 already, more than the 160 KB - 64 the entry grants -- so the run-time-loop instantiation is reached at nl = 2 (any C0) and
# at (64, 3) only, and seam counter 3 / a fourth weight slice by nothing.  The rows stay: an edit of the formula shows up here.
FWD_TABLE = {
    (128, 3): ("<128, 3>: one batch of operand loads", True),
    (256, 3): ("<256, 3>: LDA = C0 + 4, 162 816 bytes of LDS (the largest that fits)", True),
    (64, 3): ("<0, 0>: run-time loops, two rows of a0 per pass, seams 1 and 2", True),
    (64, 2): ("<0, 0>: one seam, slab 0 only", True),
    (128, 2): ("<0, 0>: one seam, C0 = 128", True),
    (256, 2): ("<0, 0>: one seam, C0 = H", True),
    (64, 4): ("refused: 171 520 bytes of LDS", False),
    (128, 4): ("refused: 179 712 bytes of LDS", False),
    (256, 4): ("refused: 196 096 bytes of LDS", False),
}
FWD_FULL_ROWS = ((128, 3), (256, 3), (64, 2))  # one shape per kernel instantiation
ROWS_FULL, ROWS_FEW = (1, 2, 5, 16, 17, 31, 32), (5, 32)

# backward (Co[], Ci[]), top stage first -> the branch
BWD_TABLE = [
    ((192, 256, 256), (256, 256, 128), "the sampler's head: Co[0] = 192 (weight-gradient workgroups 6, 7 skip stage 0), last Ci = 128"),
    ((64, 256), (256, 32), "ns = 2; Co[0] = 64: weight-gradient workgroups 2..7 skip stage 0; last Ci = 32: one chain workgroup owns a tile"),
    ((256,) * 5, (256,) * 5, "ns = 5: five slabs, counters 1..4"),
    ((128, 256, 256, 256), (256, 256, 256, 96), "ns = 4; last Ci = 96: three chain workgroups own a tile, q4 = 24"),
    ((256, 256, 256), (256, 256, 160), "last Ci = 160: five tiles, q4 = 40"),
    ((192, 256), (256, 224), "ns = 2; last Ci = 224: seven tiles, q4 = 56"),
]
BWD_FULL_ROWS = (0,)  # (one kernel: one shape carries every row count)
# `integer` backward cases (shape index -> row counts): every R is a power of two (1 / R exact).  A chain divides its unit by R at every
# stage (k3 holds s0 / R) and the values grow on top of that, so the deeper chains take fewer rows, and fewer still with the output
# BatchNorm in front (one more division): tests/test_fc_chain_host.py proves for each case listed here that every intermediate is exact
# in fp32 whatever the summation order, and that no case is listed that is not.  The rows left out are covered by `real` data.
INT_BWD_ROWS = {0: (1, 2, 4, 8, 16, 32), 1: (1, 2, 4, 8, 16, 32), 2: (1, 2, 4, 8), 3: (1, 2, 4, 8, 16), 4: (1, 2, 4, 8, 16, 32),
                5: (1, 2, 4, 8, 16, 32)}
INT_OBN_ROWS = {0: (1, 2, 4, 8), 1: (1, 2, 4, 8, 16), 2: (1, 2, 4), 3: (1, 2, 4), 4: (1, 2, 4, 8, 16), 5: (1, 2, 4, 8, 16)}


def fwd_rows(shape):
    return ROWS_FULL if shape in FWD_FULL_ROWS else ROWS_FEW


def bwd_rows(i):
    return ROWS_FULL if i in BWD_FULL_ROWS else ROWS_FEW


# ---- the `_supported` answers restated (constants read from the sources) -----------------------------------------------------------
def source_constants():
    out = {}
    for fn in ("mlp_device.h", "fc_chain.hip", "sn_common.h"):
        text = open(os.path.join(ROOT, "samplenet_amd", "csrc", fn)).read()
        for name in ("kRsPitch", "kFcChainMaxLayers", "kFcBwdMaxStages", "kFcSyncStride"):
            m = re.search(r"constexpr int %s = (\d+);" % name, text)
            if m:
                out[name] = int(m.group(1))
        m = re.search(r"constexpr int kRsFloats = ([^;]+);", text)
        if m:
            out["kRsFloats"] = eval(m.group(1), {"__builtins__": {}}, dict(out))  # "4 * 64 * kRsPitch"
    return out


def fwd_lds_bytes(C0, Hh, nl, k):
    lda = max(C0, Hh) + 4
    return 4 * (32 * lda + 32 * (C0 + 4) + (nl - 1) * 32 * (Hh + 4) + k["kRsFloats"] + 2 * 32 * 36)


def fwd_supported(R, C0, Hh, nl, k):
    return int(1 <= R <= 32 and 2 <= nl <= k["kFcChainMaxLayers"] and Hh == 256 and C0 in (64, 128, 256) and
               fwd_lds_bytes(C0, Hh, nl, k) <= 160 * 1024 - 64)


def pool_supported(B, N, C0, Hh, nl):
    return int(1 <= B <= 32 and N >= 64 and N % 64 == 0 and C0 == 128 and Hh == 256 and nl == 3)


def pool_out_supported(B, N, C0, Hh, nl, Co):
    return int(pool_supported(B, N, C0, Hh, nl) and 32 <= Co <= Hh and Co % 32 == 0)


def bwd_supported(R, ns, Co, Ci, k):
    if not (1 <= R <= 32 and 2 <= ns <= k["kFcBwdMaxStages"]):
        return 0
    for s in range(ns):
        if Co[s] < 64 or Co[s] > 256 or Co[s] % 64 or Ci[s] < 32 or Ci[s] > 256 or Ci[s] % 32:
            return 0
        if s > 0 and Co[s] != Ci[s - 1]:
            return 0
        if s + 1 < ns and Ci[s] != 256:
            return 0
    return 1


# ---- data ------------------------------------------------------------------------------------------------------------------------
def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, device=g.device, generator=g).float()


def randn(g, *shape):
    return torch.randn(*shape, device=g.device, generator=g)


def signed_pow2(g, *shape):
    """values from {-2, -1, 1, 2}"""
    return (torch.randint(1, 3, shape, device=g.device, generator=g) * (torch.randint(0, 2, shape, device=g.device, generator=g) * 2 - 1)).float()


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def fwd_case(recipe, shape, R, dev, seed=0):
    """a0 (R, C0), per layer W (H, K), bias, gamma, beta, running statistics.  integer: a0, W, bias in [-4, 4] -- every sum of layer 0
    stays below 256 * 16 + 4 < 2^13, exact in any order.  real / few: standard normal a0, W ~ K^-1/2, gamma of both signs with one zero."""
    C0, nl = shape
    g = gen(seed * 7919 + C0 * 31 + nl * 7 + R + (0 if recipe == "integer" else 100003), dev)
    c = Case(recipe=recipe, R=R, C0=C0, nl=nl, W=[], bias=[], gamma=[], beta=[], rm=[], rv=[])
    c.a0 = ints(g, -4, 4, R, C0) if recipe == "integer" else randn(g, R, C0)
    for l in range(nl):
        K = C0 if l == 0 else H
        if recipe == "integer":
            c.W.append(ints(g, -4, 4, H, K)), c.bias.append(ints(g, -4, 4, H))
        else:
            c.W.append(randn(g, H, K) * K ** -0.5), c.bias.append(randn(g, H) * 0.5)
        gamma = randn(g, H)
        gamma[5 + l] = 0.0
        assert bool((gamma < 0).any()) and bool((gamma > 0).any())
        c.gamma.append(gamma), c.beta.append(randn(g, H) * 0.5)
        c.rm.append(randn(g, H)), c.rv.append(torch.rand(H, device=dev, generator=g) + 0.5)
    return c


# ---- forward reference, teacher-forced per layer ---------------------------------------------------------------------------------
def fwd_layer_z_ref(a_in, zprev, coefprev, W, bias):
    """z_ref (fp64) of one layer and its bound, from the KERNEL's own z / coef of the layer below (None: a_in = a0 as is)."""
    K = W.shape[1]
    if zprev is None:
        a, extra = a_in.double(), 0.0
    else:
        Hc = zprev.shape[1]
        a = (zprev.double() * coefprev[0].double() + coefprev[1].double()).clamp_min(0)
        extra = 1.0  # the activation relu(fmaf(z, scale, shift)) is rounded once before the GEMM reads it: U |a|, through |W|
    z = a @ W.double().t() + bias.double()
    A = a.abs() @ W.double().abs().t() + bias.double().abs()
    return z, ((K + 8) + extra) * U * A  # GEMM over K split into 8 partials + their tree + the bias add: (K + 8) U


def bn_ref(z, gamma, beta, eps, momentum, rm, rv, R):
    """From the kernel's own z (R, C) fp32: mean, biased variance, coefficients (4, C) and the running-statistics update, with bounds.
    -> dict name -> (value, bound)"""
    zd = z.double()
    mean, sabs = zd.mean(0), zd.abs().sum(0)
    var = ((zd - mean) ** 2).mean(0)
    E_mean = (R + 3) * U * sabs / R          # s0 = col_sum_seq(z); mean = s0 / R in double
    # s2 = col_sum_seq((z - meanf)^2): per term the subtraction (counts twice in the square) and the product, 3 U; the sum (R + 3) U;
    # var = s2 / R - (mean - meanf)^2 in double is the variance identity for any meanf
    E_var = (R + 6) * U * var
    return bn_coef_ref(mean, var, E_mean, E_var, gamma, beta, eps, momentum, rm, rv, R / (R - 1.0) if R > 1 else 1.0)


def bn_coef_ref(mean, var, E_mean, E_var, gamma, beta, eps, momentum, rm, rv, unbias):
    """Coefficients (scale, shift, mean, invstd) and the running-statistics update from a batch mean and biased variance known to
    E_mean / E_var (the expressions of fc_chain.hip's epilogue and of bn_finalize_channel_mv: the same).  -> dict name -> (value, bound)"""
    inv = (var + eps) ** -0.5
    E_inv = 0.5 * inv * E_var / (var + eps) + U * inv       # fast_rsqrt is double-accurate after two Newton steps; stored as fp32: U
    g, b = gamma.double(), beta.double()
    sc = g * inv
    E_sc = g.abs() * E_inv + U * sc.abs()                   # eg * invstd: one product
    sh = b - mean * sc
    E_meanf = E_mean + U * mean.abs()                       # (float)mean
    E_sh = mean.abs() * E_sc + sc.abs() * E_meanf + U * (mean * sc).abs() + U * (b.abs() + (mean * sc).abs())  # product, subtraction
    unb = var * unbias
    m = momentum
    nrm = (1 - m) * rm.double() + m * mean
    # (1.f - m): one rounding, times rm: one; m * mean: one; the sum: one (on at most the sum of the magnitudes)
    E_rm = 2 * U * ((1 - m) * rm.double()).abs() + U * (m * mean).abs() + U * (((1 - m) * rm.double()).abs() + (m * mean).abs()) + m * E_meanf
    nrv = (1 - m) * rv.double() + m * unb
    E_unb = E_var * unbias + U * unb
    E_rv = 2 * U * ((1 - m) * rv.double()).abs() + U * (m * unb) + U * (((1 - m) * rv.double()).abs() + m * unb) + m * E_unb
    return {"scale": (sc, E_sc), "shift": (sh, E_sh), "mean": (mean, E_meanf), "invstd": (inv, E_inv), "running_mean": (nrm, E_rm),
            "running_var": (nrv, E_rv)}


def conv_stats_ref(z, rows):
    """Mean and biased variance over the `rows` rows of the last conv layer's z (fp32), as its producer accumulates them: fp32 sums of z
    and z z over blocks of rows, the block sums added exactly in 64-bit fixed point (2^-kFxShiftFwd = 2^-32 per unit, each contribution
    rounded to it: 2^-33), mean = s / R and var = ss / R - mean^2 in double.  The bound does not depend on how the rows are blocked:
    fp32 sums of `rows` terms in any order cost at most (rows - 1) U of the sum of magnitudes (+ U for the product z z), and there are
    at most rows / 64 contributions.  -> mean, var, E_mean, E_var"""
    zd = z.double()
    mean, ms = zd.mean(0), (zd * zd).mean(0)
    var = (ms - mean * mean).clamp_min(0)
    q = (rows / 64.0) * 2.0 ** -33 / rows
    E_mean = (rows - 1) * U * zd.abs().mean(0) + q
    E_ms = rows * U * ms + q
    return mean, var, E_mean, E_ms + 2 * mean.abs() * E_mean


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _coef_from(g, zprev, R, dev, stats_rows):
    """(4, C) coefficients of a BatchNorm over zprev: gamma of both signs with one zero; statistics of zprev itself when the BatchNorm
    averaged over these R rows, arbitrary ones behind the max-pool (the rows it averaged over are not here)."""
    C = zprev.shape[1]
    gamma, beta = randn(g, C), randn(g, C) * 0.5
    gamma[3] = 0.0
    if stats_rows == R:
        mean = zprev.double().mean(0)
        var = ((zprev.double() - mean) ** 2).mean(0)
    else:
        mean, var = randn(g, C).double() * 0.3, torch.rand(C, device=dev, generator=g).double() + 0.5
    mean32, inv32 = mean.float(), ((var + EPS) ** -0.5).float()
    sc = gamma * inv32
    return torch.stack([sc, beta - mean32 * sc, mean32, inv32]).contiguous()


def int_invstd(R):
    """the power of two whose square is R or 2 R: k2 = -scale invstd^2 s1 / R then keeps the unit of s1"""
    a = 0
    while 4 ** a < R:
        a += 1
    return float(2 ** a)


def bwd_case(recipe, idx, R, dev, form="R", obn=None, seed=0):
    """form: "R" (bn_rows = R), "fixed" (bn_rows = -1: k2 = k3 = 0), "pool" (last stage: bn_rows = R * 1024, araw = 1, a raw operand).
    obn: None | 0 | 1 -- the output BatchNorm in front with that `fixed`.
    integer: gy in [-2, 2]; W sparse (about three non-zeros from {+-1, +-2} per column); scale from {+-1, +-2}; mean an integer in
    [-2, 2]; zprev = mean + d with d non-zero in a quarter of the elements; shift such that mean scale + shift is -1, 0 or 1 (the
    pre-activation (mean + d) scale + shift then crosses zero all over, exact zeros included); invstd a power of two (int_invstd)."""
    Co, Ci, _ = BWD_TABLE[idx]
    ns = len(Co)
    g = gen(seed * 104729 + idx * 1009 + R * 17 + {"R": 0, "fixed": 1, "pool": 2}[form] + (0 if obn is None else 5 + obn) +
            {"integer": 0, "real": 300007, "few": 600011}[recipe], dev)
    exact = recipe == "integer"
    assert not exact or (form == "R" and R in (1, 2, 4, 8, 16, 32))
    c = Case(recipe=recipe, idx=idx, R=R, ns=ns, Co=list(Co), Ci=list(Ci), W=[], zprev=[], coef=[], aprev=[], araw=[], bn_rows=[], obn=None,
             form=form)
    c.gy = ints(g, -1, 1, R, Co[0]) if exact else randn(g, R, Co[0])
    for s in range(ns):
        co, ci = Co[s], Ci[s]
        pooled = form == "pool" and s == ns - 1
        if exact:
            W = (ints(g, 0, 1, co, ci) * 2 - 1) * (torch.rand(co, ci, device=dev, generator=g) < 2.0 / co).float()
            sc, mean = signed_pow2(g, ci), ints(g, -1, 1, ci)
            base = ints(g, -1, 1, ci)
            d = (ints(g, 0, 1, R, ci) * 2 - 1) * (torch.rand(R, ci, device=dev, generator=g) < max(2.0 / R, 0.125)).float()
            sc[0], base[0], d[0, 0] = 1.0, 0.0, 0.0    # an exact zero on a live row ...
            sc[1], base[1], d[0, 1] = 1.0, -1.0, 0.0   # ... and a negative one
            if s == 0:  # the gradient that reaches the exact zero is not zero: `> 0` and `>= 0` give different results
                W[:, 0] = 0.0
                W[0, 0], c.gy[0, 0] = 1.0, 1.0
            zp = mean + d
            coef = torch.stack([sc, base - mean * sc, mean, torch.full((ci,), int_invstd(R), device=dev)]).contiguous()
        else:
            W = randn(g, co, ci) * ci ** -0.5
            zp = randn(g, R, ci) * 1.5 + 0.5
            coef = _coef_from(g, zp, R, dev, -1 if pooled else R)
        c.W.append(W.contiguous()), c.zprev.append(zp.contiguous()), c.coef.append(coef)
        if pooled:
            c.aprev.append(ints(g, -2, 2, R, ci) if exact else randn(g, R, ci)), c.araw.append(1), c.bn_rows.append(R * 1024)
        else:
            c.aprev.append(c.zprev[-1]), c.araw.append(0), c.bn_rows.append(-1 if form == "fixed" else R)
    if obn is not None:
        co = Co[0]
        if exact:
            z = ints(g, -1, 1, R, co)
            coef = torch.stack([signed_pow2(g, co), ints(g, -2, 2, co), ints(g, -1, 1, co), torch.full((co,), int_invstd(R), device=dev)])
        else:
            z = randn(g, R, co)
            coef = _coef_from(g, z, R, dev, R)
        c.obn = Case(z=z.contiguous(), coef=coef.contiguous(), fixed=int(obn))
    return c


def _bn_backward_coefs(sc, mean, inv, s0, s1, E_s0, E_s1, rows):
    """dgamma, k2, k3 of a BatchNorm backward from its two sums (the kernels' double expressions, stored as fp32) with bounds."""
    rinv = 1.0 / rows if rows > 0 else 0.0
    dg = inv * s1
    E_dg = inv.abs() * E_s1                                                  # double product
    k2 = -sc * inv * dg * rinv
    E_k2 = (sc * inv).abs() * rinv * E_dg + U * k2.abs()                     # stored as fp32: U
    k3 = sc * (inv * mean * dg * rinv - s0 * rinv)
    E_k3 = sc.abs() * rinv * ((inv * mean).abs() * E_dg + E_s0) + U * (sc * inv * mean * dg * rinv).abs() + U * (sc * s0 * rinv).abs()
    return dg, E_dg, k2, E_k2, k3, E_k3


def bwd_ref(c, mask_ge=False, trace=None):
    """The whole chain in fp64 from the inputs.  -> {name: (value, bound)}.  mask_ge: the WRONG mask `>= 0` (the host test shows that
    the integer recipes tell it from `> 0`).  trace: a list that receives ("value", name, tensor) for every intermediate the kernel
    holds in fp32 and ("sum", name, sum of |terms|, [factor tensors]) for every fp32 sum."""
    R, out = c.R, {}
    tv = (lambda n, t: trace.append(("value", n, t))) if trace is not None else (lambda n, t: None)
    ts = (lambda n, m, f: trace.append(("sum", n, m, f))) if trace is not None else (lambda n, m, f: None)
    dZ = c.gy.double()
    E = torch.zeros_like(dZ)
    if c.obn is not None:  # fc_out_bn_backward: sums in double over the rows in order
        z, sc, mean, inv = c.obn.z.double(), c.obn.coef[0].double(), c.obn.coef[2].double(), c.obn.coef[3].double()
        zm = z - mean
        tv("obn z - mean", zm)
        s0, s1 = dZ.sum(0), (dZ * zm).sum(0)
        D = R * 2.0 ** -53                                                   # the two double sums over R rows
        E_s0 = D * dZ.abs().sum(0)
        E_s1 = (dZ.abs() * U * zm.abs()).sum(0) + D * (dZ * zm).abs().sum(0) # zv - mean in fp32: U; products and sums in double
        dg, E_dg, k2, E_k2, k3, E_k3 = _bn_backward_coefs(sc, mean, inv, s0, s1, E_s0, E_s1, -1 if c.obn.fixed else R)
        out["odgamma"], out["odbeta"] = (dg, E_dg + U * dg.abs()), (s0, E_s0 + U * s0.abs())  # stored as fp32
        inner = k2 * z + k3
        E_in = z.abs() * E_k2 + E_k3 + U * ((k2 * z).abs() + k3.abs())       # fmaf(k2, z, k3): one rounding
        tv("obn k2", k2), tv("obn k3", k3), tv("obn dgamma", dg), tv("obn dbeta", s0), tv("obn k2 z + k3", inner)
        E = E_in + U * ((sc * dZ).abs() + inner.abs())                       # fmaf(k1, g, .): one rounding
        dZ = sc * dZ + inner
    for s in range(c.ns):
        W, zp, coef = c.W[s].double(), c.zprev[s].double(), c.coef[s].double()
        sc, sh, mean, inv = coef[0], coef[1], coef[2], coef[3]
        Co = c.Co[s]
        tv("dZ%d" % s, dZ)
        # ---- weight gradient (its own workgroups): dW = dZ^T A over the R rows, one MFMA chain
        if c.araw[s]:
            a, E_a = c.aprev[s].double(), 0.0
        else:
            a = (c.aprev[s].double() * sc + sh).clamp_min(0)
            E_a = U * a                                                      # relu(fmaf(v, sc, sh)): one rounding
            tv("a%d" % s, a)
        mag = dZ.abs().t() @ a.abs()
        out["dW%d" % s] = (dZ.t() @ a, (R + 8) * U * mag + E.t() @ a.abs() + dZ.abs().t() @ (E_a * torch.ones_like(a)))  # GEMM of R terms
        ts("dW%d" % s, mag, [dZ, a])
        if s == 0:
            out["db_top"] = (dZ.sum(0), (R + 8) * U * dZ.abs().sum(0) + E.sum(0))  # the ones-column MFMA: a GEMM of R terms
            ts("db_top", dZ.abs().sum(0), [dZ])
        # ---- data gradient: dv = dZ W, a GEMM of Co terms
        magv = dZ.abs() @ W.abs()
        dv, E_dv = dZ @ W, (Co + 8) * U * magv + E @ W.abs()
        ts("dv%d" % s, magv, [dZ, W])
        pre = zp * sc + sh  # (the kernel's single fmaf has the same sign)
        live = ((pre >= 0) if mask_ge else (pre > 0)).double()
        gv, E_gv = dv * live, E_dv * live
        zm = zp - mean
        t1 = gv * zm
        E_t1 = E_gv * zm.abs() + 2 * U * t1.abs()                            # zpv - pmean: U; the product: U
        tv("zm%d" % s, zm), tv("gv%d" % s, gv), tv("t1_%d" % s, t1)
        s0, s1 = gv.sum(0), t1.sum(0)
        E_s0 = (R + 3) * U * gv.abs().sum(0) + E_gv.sum(0)                   # col_sum_seq
        E_s1 = (R + 3) * U * t1.abs().sum(0) + E_t1.sum(0)                   # col_sum_seq
        ts("s0_%d" % s, gv.abs().sum(0), [gv]), ts("s1_%d" % s, t1.abs().sum(0), [t1])
        rows = c.bn_rows[s]
        dg, E_dg, k2, E_k2, k3, E_k3 = _bn_backward_coefs(sc, mean, inv, s0, s1, E_s0, E_s1, rows)
        out["dgamma%d" % s], out["dbeta%d" % s] = (dg, E_dg + U * dg.abs()), (s0, E_s0)  # (float)dg: U; (float)sd: exact
        parts = (sc * s0, k2 * rows * mean, rows * k3)
        dbias = parts[0] + parts[1] + parts[2]                               # double, from the fp32 k1, k2, k3; stored as fp32: U
        out["dbias%d" % s] = (dbias, sc.abs() * E_s0 + abs(rows) * mean.abs() * E_k2 + abs(rows) * E_k3 + U * sum(p.abs() for p in parts))
        tv("dgamma%d" % s, dg), tv("dbeta%d" % s, s0), tv("k2_%d" % s, k2), tv("k3_%d" % s, k3), tv("dbias%d" % s, dbias)
        if s == c.ns - 1:
            out["gout"] = (gv, E_gv)
            out["kout"] = (torch.stack([sc, k2, k3]), torch.stack([torch.zeros_like(sc), E_k2, E_k3]))
        inner = k2 * zp + k3
        E_in = zp.abs() * E_k2 + E_k3 + U * ((k2 * zp).abs() + k3.abs())     # fmaf(k2, zpv, k3): one rounding
        tv("inner%d" % s, inner)
        E = sc.abs() * E_gv + E_in + U * ((sc * gv).abs() + inner.abs())     # fmaf(k1, gv, .): one rounding
        dZ = sc * gv + inner
    return out


# ---- exactness of a recipe (host) ------------------------------------------------------------------------------------------------
def fp32_exact(t):
    return bool((t.float().double() == t).all()) and bool(torch.isfinite(t).all())


def unit_of(t):
    """The largest power of two that divides every element of t (fp64, dyadic); 1.0 for an all-zero tensor."""
    nz = t[t != 0]
    if nz.numel() == 0:
        return 1.0
    _, e = torch.frexp(nz)                         # nz = m 2^e, 0.5 <= |m| < 1
    k = torch.round(nz * torch.exp2(60.0 - e.double())).long()  # m 2^60: an integer below 2^60, the 53 significant bits kept
    low = (k & -k).double() * torch.exp2(e.double() - 60.0)
    return float(low.min())


# ---- sync state ------------------------------------------------------------------------------------------------------------------
def sync_block(limit=0):
    """16 x 32 words, zeroed at the 16 words the kernels use, the sentinel everywhere else; between guard words."""
    gb = Guarded(SYNC_WORDS * SYNC_STRIDE, torch.int32, zero=False)
    gb.view.view(SYNC_WORDS, SYNC_STRIDE)[:, 0] = 0
    gb.view[13 * SYNC_STRIDE] = limit
    return gb


def sync_words(gb):
    """the 16 words as Python ints modulo 2^32 (synchronises)"""
    return [int(v) & 0xFFFFFFFF for v in gb.view.view(SYNC_WORDS, SYNC_STRIDE)[:, 0].tolist()]


def sync_set(gb, words):
    w = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in words], dtype=torch.int32, device=gb.view.device)
    gb.view.view(SYNC_WORDS, SYNC_STRIDE)[:, 0] = w


def sync_intact(gb):
    return gb.intact() and bool((gb.view.view(SYNC_WORDS, SYNC_STRIDE)[:, 1:] == SENTINEL).all())


def fwd_sync_closed_form(E, nl, limit=0):
    w = [0] * SYNC_WORDS
    w[0] = E & 0xFFFFFFFF
    for l in range(nl - 1):
        w[1 + l] = (8 * E) & 0xFFFFFFFF
    w[13] = limit
    return w


def bwd_sync_closed_form(E, ns, limit=0):
    w = [0] * SYNC_WORDS
    w[0] = E & 0xFFFFFFFF
    for s in range(ns - 1):
        w[1 + s] = (8 * E) & 0xFFFFFFFF
    w[13], w[14] = limit, (16 * E) & 0xFFFFFFFF
    return w


# ---- launch drivers --------------------------------------------------------------------------------------------------------------
def _lib():
    from samplenet_amd import _lib as L

    return L


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class ChainLaunch(Launch):
    def __init__(self, what, sync):
        super().__init__(what)
        self.sync = sync

    def check(self):
        super().check()
        assert sync_intact(self.sync), "write between the sync words: %s" % (self.what,)
        return self

    def filled(self, t):
        """every element of an output was written (none still holds the sentinel's NaN pattern)"""
        return not bool((t.view(torch.int32) == SENTINEL).any())


def launch_forward(c, sync, stats="all"):
    """One sn_fc_chain_forward on the current stream.  stats: "all" | "none" (the three arrays NULL).
    -> ChainLaunch with .z[l] (R, H), .coef[l] (4, H), .rm[l], .rv[l], .nbt[l] (copies of the case's, updated in place), .xbuf"""
    L = _lib()
    call = ChainLaunch(("fc_chain_forward", c.recipe, c.R, c.C0, c.nl, stats), sync)
    call.z = [call.add((c.R, H)) for _ in range(c.nl)]
    call.coef = [call.add((4, H)) for _ in range(c.nl)]
    call.xbuf = call.add((2 * 32 * H,))
    call.rm, call.rv, call.nbt = [], [], []
    for l in range(c.nl):
        rm, rv = call.add((H,)), call.add((H,))
        rm.copy_(c.rm[l]), rv.copy_(c.rv[l])
        gb = Guarded(4, torch.int64, zero=True)  # num_batches_tracked and one more word pair, which stays 0
        call.outs.append(gb)
        gb.view[0] = 7 + l
        call.rm.append(rm), call.rv.append(rv), call.nbt.append(gb.view)
    eps, mom = (ctypes.c_float * c.nl)(*[EPS] * c.nl), (ctypes.c_float * c.nl)(*[MOMENTUM] * c.nl)
    st = (_arr(call.rm), _arr(call.rv), _arr(call.nbt)) if stats == "all" else (None, None, None)
    rc = L.lib.sn_fc_chain_forward(c.R, c.C0, H, c.nl, c.a0.data_ptr(), _arr(c.W), _arr(c.bias), _arr(c.gamma), _arr(c.beta), st[0], st[1],
                                   st[2], eps, mom, _arr(call.z), _arr(call.coef), call.xbuf.data_ptr(), sync.view.data_ptr(),
                                   L.stream_of(c.a0))
    L.check(rc, str(call.what))
    return call


def launch_layer_forward(c, l, ain, coef_prev):
    """sn_layer_forward_bn of layer l alone (the per-layer launch the chain replaces), fed with `ain` / `coef_prev`."""
    L = _lib()
    K = c.C0 if l == 0 else H
    call = Launch(("layer_forward_bn", c.R, K, H))
    call.z, call.coef = call.add((c.R, H)), call.add((4, H))
    stats = call.add((L.lib.sn_linear_stats_blocks(c.R), 2, H))
    call.rm, call.rv = call.add((H,)), call.add((H,))
    call.rm.copy_(c.rm[l]), call.rv.copy_(c.rv[l])
    nbt = torch.zeros(1, dtype=torch.int64, device=ain.device)
    p = L.ptr
    L.check(L.lib.sn_layer_forward_bn(c.R, K, H, p(ain), p(coef_prev), p(c.W[l]), p(c.bias[l]), p(call.z), p(stats), p(c.gamma[l]), p(c.beta[l]),
                                      EPS, MOMENTUM, p(call.rm), p(call.rv), p(nbt), p(call.coef), L.stream_of(ain)), str(call.what))
    return call


BWD_OPTIONAL = ("db_top", "dbias", "gout", "kout")


def launch_backward(c, sync, without=()):
    """One sn_fc_chain_backward (or _obn when the case has an output BatchNorm).  without: names from BWD_OPTIONAL passed as NULL.
    -> ChainLaunch with .out {name: tensor} named as bwd_ref names them, .xbuf"""
    L = _lib()
    ns, R = c.ns, c.R
    call = ChainLaunch(("fc_chain_backward", c.recipe, c.idx, R, c.form, None if c.obn is None else c.obn.fixed, tuple(without)), sync)
    o = call.out = {}
    for s in range(ns):
        o["dW%d" % s] = call.add((c.Co[s], c.Ci[s]))
        o["dgamma%d" % s], o["dbeta%d" % s] = call.add((c.Ci[s],)), call.add((c.Ci[s],))
        if "dbias" not in without:
            o["dbias%d" % s] = call.add((c.Ci[s],))
    if "db_top" not in without:
        o["db_top"] = call.add((c.Co[0],))
    if "gout" not in without:
        o["gout"] = call.add((R, c.Ci[-1]))
    if "kout" not in without:
        o["kout"] = call.add((3, c.Ci[-1]))
    call.xbuf = call.add((ns * 32 * 256,))
    Co, Ci = (ctypes.c_int * ns)(*c.Co), (ctypes.c_int * ns)(*c.Ci)
    rows, araw = (ctypes.c_longlong * ns)(*c.bn_rows), (ctypes.c_int * ns)(*c.araw)
    p = lambda t: None if t is None else t.data_ptr()
    tail = (_arr(c.W), _arr(c.zprev), _arr(c.coef), rows, _arr([o["dgamma%d" % s] for s in range(ns)]), _arr([o["dbeta%d" % s] for s in range(ns)]),
            _arr([o.get("dbias%d" % s) for s in range(ns)]), _arr([o["dW%d" % s] for s in range(ns)]), p(o.get("db_top")), _arr(c.aprev), araw,
            p(o.get("gout")), p(o.get("kout")), p(call.xbuf), p(sync.view), L.stream_of(c.gy))
    if c.obn is None:
        rc = L.lib.sn_fc_chain_backward(R, ns, Co, Ci, p(c.gy), *tail)
    else:
        o["odgamma"], o["odbeta"] = call.add((c.Co[0],)), call.add((c.Co[0],))
        rc = L.lib.sn_fc_chain_backward_obn(R, ns, Co, Ci, p(c.gy), p(c.obn.z), p(c.obn.coef), c.obn.fixed, p(o["odgamma"]), p(o["odbeta"]), *tail)
    L.check(rc, str(call.what))
    return call


def launch_bn_output_backward(c):
    """sn_bn_output_backward on the case's output BatchNorm alone.  -> Launch with .dz (R, Co[0]), .dgamma, .dbeta"""
    L = _lib()
    co = c.Co[0]
    call = Launch(("bn_output_backward", c.R, co, c.obn.fixed))
    call.dz, call.dgamma, call.dbeta = call.add((c.R, co)), call.add((co,)), call.add((co,))
    p = L.ptr
    L.check(L.lib.sn_bn_output_backward(c.R, co, c.obn.fixed, p(c.gy), p(c.obn.z), p(c.obn.coef), p(call.dz), p(call.dgamma), p(call.dbeta),
                                        L.stream_of(c.gy)), str(call.what))
    return call


# ---- the pool variants: sn_conv_stack_forward_bn (pooled = argsel = zsel = NULL) as producer ------------------------------------------
POOL_STACKS = ((3, 64, 128), (3, 64, 64, 64, 128, 128))  # the smallest stack that ends in 128 channels first, else the sampler's five layers
POOL_SHAPES = ((5, 64), (32, 64), (3, 1024), (1, 128))   # (B, N); (1, 128) stands for (1, 64), which no conv stack admits (B N > 64)
POOL_OUT_WIDTHS = (32, 96, 256)


def pool_stack(B, N):
    L = _lib()
    for ch in POOL_STACKS:
        if L.lib.sn_conv_stack_forward_supported(B, N, len(ch) - 1, (ctypes.c_int * len(ch))(*ch)):
            return ch
    return None


def pool_case(B, N, dev, Co=None, seed=0):
    """A cloud, the conv stack's parameters, the FC head 128 -> 256 x 3 (fwd_case's `real` recipe) and, with Co, an output layer
    (Co, 256) + BatchNorm.  Some bn5 scales negative (those channels pick the minima) and one zero."""
    ch = pool_stack(B, N)
    g = gen(seed * 31 + B * 1031 + N + (Co or 0) * 7, dev)
    c = fwd_case("real", (128, 3), B, dev, seed=seed + N)
    c.B, c.N, c.ch, c.Co = B, N, ch, Co
    c.x = (torch.rand(B, N, 3, device=dev, generator=g) - 0.5).contiguous()
    c.cW, c.cb, c.cg, c.cbeta, c.crm, c.crv = [], [], [], [], [], []
    for ci, co in zip(ch[:-1], ch[1:]):
        c.cW.append(randn(g, co, ci) * ci ** -0.5), c.cb.append(randn(g, co) * 0.1)
        c.cg.append(randn(g, co).abs() + 0.5), c.cbeta.append(randn(g, co) * 0.1)
        c.crm.append(randn(g, co) * 0.1), c.crv.append(torch.rand(co, device=dev, generator=g) + 0.5)
    c.cg[-1][::5] *= -1.0
    c.cg[-1][3] = 0.0
    if Co is not None:
        c.oW, c.ob = randn(g, Co, H) * H ** -0.5, randn(g, Co) * 0.5
        c.og, c.obeta = randn(g, Co), randn(g, Co) * 0.5
        c.og[1] = 0.0
        c.orm, c.orv = randn(g, Co), torch.rand(Co, device=dev, generator=g) + 0.5
    return c


def launch_pool(c, sync):
    """sn_conv_stack_forward_bn with pooled = argsel = zsel = NULL, then sn_fc_chain_forward_pool (or _pool_out when the case has an output
    layer) on the current stream.  -> ChainLaunch with .z5 (B N, 128) the producer's last z, .coef5 (4, 128), .rm5 / .rv5 / .nbt5,
    .pooled / .zsel (B, 128), .argsel, .acc (the whole accumulator scratch), .nsum (its leading statistics part), the chain's .z / .coef /
    .rm / .rv / .nbt, and .zo / .coef_o / .y / .orm / .orv / .onbt"""
    L = _lib()
    B, N, ch = c.B, c.N, c.ch
    n, R, dev = len(ch) - 1, B * N, c.x.device
    chans = (ctypes.c_int * (n + 1))(*ch)
    call = ChainLaunch(("fc_chain_forward_pool", B, N, ch, c.Co), sync)
    acc_gb = Guarded(2 * L.lib.sn_conv_stack_acc_elems(n), torch.int64, zero=True)
    call.outs.append(acc_gb)
    call.acc, call.nsum = acc_gb.view, L.lib.sn_conv_stack_acc_sum_elems(n, chans)
    zc = [torch.empty(R, co, device=dev) for co in ch[1:]]
    cc = [call.add((4, co)) for co in ch[1:]]
    nblk = L.lib.sn_linear_stats_blocks(R)
    pool_val = torch.zeros(max(nblk, 2 * B) * 2 * 128, device=dev)
    pool_idx = torch.zeros(nblk * 2 * 128, device=dev, dtype=torch.int32)
    crm, crv = [t.clone() for t in c.crm], [t.clone() for t in c.crv]
    cnbt = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(n)]
    eps, mom = (ctypes.c_float * n)(*[EPS] * n), (ctypes.c_float * n)(*[MOMENTUM] * n)
    st = L.stream_of(c.x)
    L.check(L.lib.sn_conv_stack_forward_bn(B, N, n, chans, c.x.data_ptr(), _arr(c.cW), _arr(c.cb), _arr(c.cg), _arr(c.cbeta), _arr(crm), _arr(crv),
                                           _arr(cnbt), eps, mom, _arr(zc), _arr(cc), call.acc.data_ptr(), pool_val.data_ptr(), pool_idx.data_ptr(),
                                           None, None, None, st), "sn_conv_stack_forward_bn")
    call.z5, call.coef5 = zc[-1], cc[-1]
    call.rm5, call.rv5 = call.add((128,)), call.add((128,))
    call.rm5.copy_(c.crm[-1]), call.rv5.copy_(c.crv[-1])
    nb5 = Guarded(4, torch.int64, zero=True)
    call.outs.append(nb5)
    call.nbt5 = nb5.view
    call.pooled, call.zsel = call.add((B, 128)), call.add((B, 128))
    ag = Guarded(B * 128, torch.int32)
    call.outs.append(ag)
    call.argsel = ag.view.view(B, 128)
    call.z = [call.add((B, H)) for _ in range(3)]
    call.coef = [call.add((4, H)) for _ in range(3)]
    call.xbuf = call.add((2 * 32 * H,))
    call.rm, call.rv, call.nbt = [], [], []
    for l in range(3):
        rm, rv = call.add((H,)), call.add((H,))
        rm.copy_(c.rm[l]), rv.copy_(c.rv[l])
        gb = Guarded(4, torch.int64, zero=True)
        call.outs.append(gb)
        call.rm.append(rm), call.rv.append(rv), call.nbt.append(gb.view)
    e3, m3 = (ctypes.c_float * 3)(*[EPS] * 3), (ctypes.c_float * 3)(*[MOMENTUM] * 3)
    p = lambda t: t.data_ptr()
    args = [B, N, n, p(call.acc), p(pool_val), p(pool_idx), p(c.cg[-1]), p(c.cbeta[-1]), p(call.rm5), p(call.rv5), p(call.nbt5), EPS, MOMENTUM,
            p(call.coef5), p(call.pooled), p(call.argsel), p(call.zsel), H, 3, _arr(c.W), _arr(c.bias), _arr(c.gamma), _arr(c.beta), _arr(call.rm),
            _arr(call.rv), _arr(call.nbt), e3, m3, _arr(call.z), _arr(call.coef), p(call.xbuf), p(sync.view)]
    if c.Co is None:
        rc = L.lib.sn_fc_chain_forward_pool(*args, st)
    else:
        call.zo, call.coef_o, call.y = call.add((B, c.Co)), call.add((4, c.Co)), call.add((B, c.Co))
        call.orm, call.orv = call.add((c.Co,)), call.add((c.Co,))
        call.orm.copy_(c.orm), call.orv.copy_(c.orv)
        gb = Guarded(4, torch.int64, zero=True)
        call.outs.append(gb)
        call.onbt = gb.view
        rc = L.lib.sn_fc_chain_forward_pool_out(*args, c.Co, p(c.oW), p(c.ob), p(c.og), p(c.obeta), p(call.orm), p(call.orv), p(call.onbt), EPS,
                                                MOMENTUM, p(call.zo), p(call.coef_o), p(call.y), st)
    L.check(rc, str(call.what))
    call.keep = (zc, pool_val, pool_idx, crm, crv, cnbt)
    return call

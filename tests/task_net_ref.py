"""Plain fp64 restatement of the registration task network's extractor entries (csrc/task_network.hip and the pooled epilogue of
linear_fwd_kernel in csrc/pointnet_mlp.hip) -- sn_linear_forward_maxpool, sn_linear_forward_maxpool_wide (with _supported and
_scratch_bytes), sn_pool_dgrad_sparse, sn_pointnet_narrow_forward, sn_pointnet_narrow_backward --, the data the tests feed them, the
shape tables (one sentence per row: the branch it reaches) and drivers that call the raw entries through samplenet_amd._lib.
Imported by tests/test_task_net_host.py (no GPU: the references against torch, the generators' conditions, the tables against the
sources) and tests/test_gpu_task_net_direct.py (the calls).  The references are torch in fp64 and call nothing of the library; every
generator draws on the CPU from a seeded generator and moves the data, so the host test's proofs are about the very numbers the GPU sees.

Yardsticks (all counted, none measured).  U = 2^-24.  A product of K split-bf16 terms costs (K + 8) U times |a| . |w| (the project's
GEMM figure), element by element, the magnitude product in fp64 (the bias add is one of the 8).  Integer recipes (small integers,
weights sparse in {-1, 0, 1}, and in the pooled layer one input channel of 9-bit integers on both sides: no operand has a third
bf16 plane, so the six products of a k-step hold every non-zero one; every partial sum below 2^24) are compared bit for bit.
Picks and masks are exact: a call that stores z is held to its own
z (first argmax, zsel = z[argsel], pooled = relu(zsel)), one that does not to the bits of the storing call; ReLU masks of the two
backward entries are made exact by the generators (every argument further from 0 than its rounding, planted exact zeros mask).
The operand of the pooled layer, relu(fmaf(z, scale, shift)), is restated as the fp64 sum rounded once to fp32: the same number unless
the fp64 sum is an exact fp32 midpoint, which the host test rules out for every case."""
import os
import re

import torch

from skinny_ref import SENTINEL, Guarded, Launch

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
TIE_DISTANCES = (4, 8, 32, 64, 128)  # other half-wave, same lane, other wave, other tile / key group, other partial / workgroup
TIE_SCALE = 6.0

# ---- shape tables ------------------------------------------------------------------------------------------------------------------
# sn_linear_forward_maxpool (64 x 64 tiles, keys by atomicMax): (B, npts, Ci, Co) -> branch
TILE_TABLE = {
    (2, 64, 64, 64): "one tile per cloud, one K chunk, one column block",
    (1, 128, 128, 128): "two tiles meet in one key by atomicMax",
    (3, 192, 192, 64): "three tiles per cloud, Ci not a power of two",
    (2, 64, 128, 1024): "PCRNet's last-layer width at small R",
}
# sn_linear_forward_maxpool_wide: (R, npts, Ci, Co) -> (branch, key group rows, partials per cloud, column split, column blocks per
# workgroup, coef_prev == NULL also run on this row)
WIDE_TABLE = {
    (16384, 128, 128, 512): ("group 128, one partial per cloud, columns split in two", 128, 1, 2, 4, True),
    (16384, 64, 64, 512): ("group 64, two waves per group, K = 64", 64, 1, 2, 4, True),
    (16384, 32, 128, 512): ("group 32, four clouds per workgroup", 32, 1, 2, 4, False),
    (16512, 96, 64, 512): ("group 32, three partials, clouds straddle workgroups", 32, 3, 2, 4, False),
    (16512, 192, 128, 512): ("group 64, three partials, straddling", 64, 3, 2, 4, False),
    (16384, 128, 64, 576): ("nine column blocks: no split, odd nblk, the rotation wraps", 128, 1, 1, 9, False),
    (32768, 1024, 128, 512): ("256 row blocks: no split, eight partials per cloud", 128, 8, 1, 8, False),
}
WIDE_AGAINST_TILE = ((16384, 128, 128, 512), (16384, 64, 64, 512))  # one row per Ci
# sn_pointnet_narrow_forward: R -> branch
NARROW_FWD_TABLE = {
    64: "supported: one workgroup, two idle waves",
    128: "supported: one full workgroup",
    192: "supported: a second workgroup half full",
    4160: "supported: 33 workgroups, the last half full",
    1: "ragged: one live lane",
    33: "ragged: a second wave with one live lane",
    150: "ragged: a second workgroup whose first wave ends at lane 21",
}
NARROW_RIDER_N = (0, 1, 255, 1000)  # words to clear at R = 64: one workgroup of 256 threads grid-strides four times at 1000
NARROW_BWD_ROWS = (1, 31, 32, 33, 64, 129, 150, 4160)
# sn_pool_dgrad_sparse: (B, npts, Ci, Co) -> (branch, pick recipes)
PICKS = ("one row", "uniform", "outside")
PICKS_ALL = PICKS + ("early",)
SPARSE_TABLE = {
    (1, 1, 1, 1): ("single element", PICKS),
    (3, 64, 32, 16): ("one channel per group", PICKS),
    (2, 63, 33, 17): ("ragged everywhere: a second Ci block with one live lane, group 0 with two channels", PICKS),
    (2, 65, 128, 512): ("second row chunk of one row, one full pass", PICKS),
    (2, 256, 128, 513): ("four chunks, second pass of one channel", PICKS),
    (4, 256, 128, 1024): ("every pick below 64 except one channel of one cloud in chunk 3: early-exit chunks write zeros, that chunk does not",
                          ("early",)),
    (32, 64, 128, 1024): ("the registration step's own shape", PICKS),
}
EARLY_HIT = (2, 77, 255)  # (cloud, channel, row): the one pick outside the first chunk -- the LAST row of chunk 3
MASKS = ("zprev+coef", "zprev", "none")


# ---- the host functions and constants, restated and read ---------------------------------------------------------------------------
def source_constants():
    out = {}
    tn = open(os.path.join(ROOT, "samplenet_amd", "csrc", "task_network.hip")).read()
    for name in ("kWideRows", "kWideBN", "kNarrowRows", "kPdsThreads", "kPdsGroups", "kPdsCi", "kPdsPts", "kPdsCh"):
        out[name] = int(re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, tn).group(1))
    host = open(os.path.join(ROOT, "samplenet_amd", "csrc", "mlp_host.h")).read()
    out["TileBig::BM"], out["TileBig::BN"] = map(int, re.search(r"using TileBig = Tile<(\d+), (\d+),", host).groups())
    out["BK"] = int(re.search(r"constexpr int BK = (\d+);", open(os.path.join(ROOT, "samplenet_amd", "csrc", "mlp_device.h")).read()).group(1))
    return out


# the predicates and index expressions the restatements below and the tables' sentences were read from, as they stand in the sources
ROUTE_LINES = {
    "tile supported": ("pointnet_mlp.hip", "return R > 64 && npts >= 64 && npts % 64 == 0 && R % npts == 0 && R % TileBig::BM == 0 && Co % TileBig::BN == 0 && Ci % BK == 0;"),
    "tile keys cleared": ("pointnet_mlp.hip", "if (!keys_cleared) {"),
    "wide supported": ("task_network.hip", "return R >= 128 * kWideRows && R % kWideRows == 0 && npts >= 32 && npts % 32 == 0 && R % npts == 0 && (Ci == 64 || Ci == 128) && "
                                           "Co >= 8 * kWideBN && Co % kWideBN == 0;"),
    "wide group rows": ("task_network.hip", "static int wide_group_rows(int npts) { return npts % 128 == 0 ? 128 : npts % 64 == 0 ? 64 : 32; }"),
    "wide scratch": ("task_network.hip", "return (long long)(R / wide_group_rows(npts)) * Co * (long long)sizeof(unsigned long long);"),
    "wide column split": ("task_network.hip", "while (rb * cs < 256 && Co / (cs * 2) >= kWideBN && (Co / kWideBN) % (cs * 2) == 0) cs *= 2;"),
    "wide rotation": ("task_network.hip", "const int rot = (blockIdx.x / 8) % nblk;"),
    "wide row in cloud": ("task_network.hip", "const int rin0 = row0 % g.npts;"),
    "wide no activation": ("task_network.hip", "if (g.scale) {"),
    "narrow forward supported": ("task_network.hip", "return R >= 64 && R % 64 == 0 && c1 == 64 && c2 == 64 && c3 == 64 && c4 == 128;"),
    "narrow forward any R": ("task_network.hip", 'SN_REQUIRE(R >= 1 && x && W1 && W2 && W3 && W4 && wplanes && z4, "bad argument");'),
    "narrow grid": ("task_network.hip", "const dim3 grid((R + kNarrowRows - 1) / kNarrowRows);"),
    "narrow rider": ("task_network.hip", "for (int i = blockIdx.x * 256 + tid; i < g.zero_n; i += gridDim.x * 256) g.zero_keys[i] = 0ull;"),
    "sparse supported": ("task_network.hip", "return B >= 1 && npts >= 1 && npts <= 4 * kPdsPts && Ci >= 1 && Co >= 1;"),
    "sparse grid": ("task_network.hip", "dim3(B, (Ci + kPdsCi - 1) / kPdsCi, (npts + kPdsPts - 1) / kPdsPts)"),
    "sparse early exit": ("task_network.hip", "if (gridDim.z > 1) {"),
}


def source_routes():
    """name -> number of occurrences of its line in its source file (white space apart)"""
    out, texts = {}, {}
    for name, (fn, line) in ROUTE_LINES.items():
        if fn not in texts:
            texts[fn] = open(os.path.join(ROOT, "samplenet_amd", "csrc", fn)).read()
        out[name] = len(re.findall(r"\s+".join(re.escape(tok) for tok in line.split()), texts[fn]))
    return out


def tile_supported(R, Ci, Co, npts):
    return R > 64 and npts >= 64 and npts % 64 == 0 and R % npts == 0 and R % 64 == 0 and Co % 64 == 0 and Ci % 64 == 0


def wide_supported(R, Ci, Co, npts):
    return (R >= 128 * 128 and R % 128 == 0 and npts >= 32 and npts % 32 == 0 and R % npts == 0 and Ci in (64, 128) and Co >= 512
            and Co % 64 == 0)


def wide_group_rows(npts):
    return 128 if npts % 128 == 0 else 64 if npts % 64 == 0 else 32


def wide_column_split(R, Co):
    rb, cs = R // 128, 1
    while rb * cs < 256 and Co // (cs * 2) >= 64 and (Co // 64) % (cs * 2) == 0:
        cs *= 2
    return cs


def wide_scratch_bytes(R, Co, npts):
    return (R // wide_group_rows(npts)) * Co * 8


def sparse_supported(B, npts, Ci, Co):
    return B >= 1 and 1 <= npts <= 256 and Ci >= 1 and Co >= 1


# ---- references (fp64, torch only) ---------------------------------------------------------------------------------------------------
def operand(ain, coef):
    """The pooled layer's operand as an exact fp64 image of the fp32 number the kernels form: relu(fmaf(z, scale, shift)) with
    coef = [scale | shift]; coef None: z as is (no ReLU -- sn_linear_forward_maxpool_wide's pinned behaviour)."""
    if coef is None:
        return ain.double()
    Ci = ain.shape[1]
    return (ain.double() * coef[:Ci].double() + coef[Ci:].double()).float().clamp_min(0).double()


def operand_midpoints(ain, coef):
    """number of elements whose fp64 sum z scale + shift was ROUNDED onto an fp32 midpoint (the only place where rounding it once
    more to fp32 could differ from fmaf's single rounding; the product of two fp32 numbers is exact in fp64, and the sum's own
    rounding error is the TwoSum residual: zero means the midpoint is the exact value, which both roundings treat alike)"""
    Ci = ain.shape[1]
    p, t = ain.double() * coef[:Ci].double(), coef[Ci:].double().expand(ain.shape)
    s = p + t
    bp = s - p
    residual = (p - (s - bp)) + (t - bp)
    return int((((s.view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)) & (residual != 0)).sum())


def linear_ref(a, W, bias, K=None):
    """z = a W^T + b in fp64 and the bound (K + 8) U (|a| |W|^T + |b|).  a is fp64 already.  -> (z, bound)"""
    K = a.shape[1] if K is None else K
    Wd = W.double()
    z, A = a @ Wd.t(), a.abs() @ Wd.abs().t()
    if bias is not None:
        z, A = z + bias.double(), A + bias.double().abs()
    return z, (K + 8) * U * A


def first_argmax(z, B, npts):
    """per cloud and column: the maximum and the FIRST row that holds it (torch's own argmax promises no order among ties)"""
    zc = z.view(B, npts, -1)
    m = zc.amax(1)
    rows = torch.arange(npts, device=z.device).view(1, npts, 1)
    first = torch.where(zc == m[:, None, :], rows, npts).amin(1)
    return m, first.int()


def pooled_ref(c, with_bias=True, with_coef=True):
    """-> z64 (R, Co), bound (R, Co), relu(max64) (B, Co), its bound (the max is 1-Lipschitz: the largest bound among the cloud's rows)"""
    z, bnd = linear_ref(operand(c.ain, c.coef if with_coef else None), c.W, c.bias if with_bias else None)
    return z, bnd, z.view(c.B, c.npts, -1).amax(1).clamp_min(0), bnd.view(c.B, c.npts, -1).amax(1)


def narrow_layer1_ref(x, W1, b1):
    """z1 = x W1^T + b1 in fp64; bound 4 U (sum |w| |x| + |b|): a product, two fmas and an add"""
    z, A = x.double() @ W1.double().t(), x.double().abs() @ W1.double().abs().t()
    if b1 is not None:
        z, A = z + b1.double(), A + b1.double().abs()
    return z, 4 * U * A


def narrow_forward_ref(c, with_bias=True):
    """the whole front in fp64, free-running (the host test holds it to torch's Linear / relu) -> [z1, z2, z3, z4]"""
    b = c.b if with_bias else [None] * 4
    out = [narrow_layer1_ref(c.x, c.W[0], b[0])[0]]
    for l in (1, 2, 3):
        out.append(linear_ref(out[-1].clamp_min(0), c.W[l], b[l])[0])
    return out


def narrow_backward_ref(c):
    """dx = (((dz4 W4 . [z3 > 0]) W3 . [z2 > 0]) W2 . [z1 > 0]) W1 in fp64 and its first-order bound: each of the three products costs
    (K + 8) U of its magnitude product (K = 128, 64, 64) and hands the error it received on through |W|; the last is a 64-term fma
    chain (32 per half-wave and the add across): 64 U of its magnitude product.  -> (dx, bound)"""
    d, e = c.dz4.double(), torch.zeros_like(c.dz4, dtype=torch.float64)
    for W, zmask in ((c.W[3], c.z[2]), (c.W[2], c.z[1]), (c.W[1], c.z[0])):
        Wd, m = W.double(), (zmask > 0).double()
        e = ((d.shape[1] + 8) * U * (d.abs() @ Wd.abs()) + e @ Wd.abs()) * m
        d = (d @ Wd) * m
    W1 = c.W[0].double()
    return d @ W1, 64 * U * (d.abs() @ W1.abs()) + e @ W1.abs()


def sparse_ref(c, mask):
    """dyprev (B npts, Ci) = relu'_prev . sum_c [argsel[b][c] == n] (pooled > 0 ? g : 0)[b][c] W[c][:] in fp64; bound
    (cnt + 16) U sum |g W| with cnt the number of channels whose pick is row n (the fma chain of a group's copy, then the add across the
    sixteen copies).  A pick outside [0, npts) contributes nothing.  -> (dyprev, bound)"""
    B, npts, Ci, Co = c.shape
    gsel = torch.where(c.pooled > 0, c.g, torch.zeros_like(c.g)).double()
    arg = c.argsel.long()
    inside = (arg >= 0) & (arg < npts)
    dz = torch.zeros(B, npts + 1, Co, dtype=torch.float64, device=c.g.device)
    dz.scatter_(1, torch.where(inside, arg, npts)[:, None, :], gsel[:, None, :])
    dz = dz[:, :npts].reshape(B * npts, Co)
    cnt = torch.zeros(B, npts + 1, dtype=torch.float64, device=c.g.device)
    cnt.scatter_add_(1, torch.where(inside, arg, npts), torch.ones_like(gsel))
    Wd = c.W.double()
    out, A = dz @ Wd, dz.abs() @ Wd.abs()
    m = sparse_mask(c, mask)
    if m is not None:
        out, A = out * m, A * m
    return out, (cnt[:, :npts].reshape(-1, 1) + 16) * U * A


def sparse_mask_argument(c, mask):
    """fp64 z scale + shift of the previous layer (the sign the kernel's fmaf must reproduce) and the magnitude of its two terms"""
    Ci = c.shape[2]
    z = c.zprev.double()
    if mask == "zprev+coef":
        return z * c.coef[:Ci].double() + c.coef[Ci:].double(), (z * c.coef[:Ci].double()).abs() + c.coef[Ci:].double().abs()
    return z, z.abs()


def sparse_mask(c, mask):
    return None if mask == "none" else (sparse_mask_argument(c, mask)[0] > 0).double()


# ---- data --------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, dev):
        move = lambda v: v.to(dev) if torch.is_tensor(v) else [move(t) for t in v] if isinstance(v, list) else v
        return Case(**{k: move(v) for k, v in self.__dict__.items()})


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def sparse_pm1(g, density_inv, *shape):
    """{-1, 0, 1} with a non-zero at one place in density_inv"""
    return ints(g, -1, 1, *shape) * (torch.randint(0, density_inv, shape, generator=g) == 0).float()


def tie_plan(B, npts):
    """[(cloud, first row, distance)]: in every cloud one pair of duplicate rows per distance that fits, no row used twice; the first
    cloud's first pair starts at row 0"""
    plan = []
    for b in range(B):
        used = set()
        for k, d in enumerate(TIE_DISTANCES):
            if d >= npts:
                continue
            p = (3 * b + 11 * k) % (npts - d)
            while p in used or p + d in used:
                p = (p + 1) % (npts - d)
            used |= {p, p + d}
            plan.append((b, p, d))
    return plan


def plant_ties(g, ain, B, npts):
    """rows p and p + d of cloud b := TIE_SCALE x one random row of the call: the same operand, hence the same bits in every column, and
    the column's maximum in a good share of the columns (the host test counts them)"""
    plan = tie_plan(B, npts)
    src = torch.randperm(ain.shape[0], generator=g)[:len(plan)]  # (distinct: two pairs with one source would tie with each other)
    rows = ain[src] * TIE_SCALE  # (taken before any row is overwritten)
    for (b, p, d), row in zip(plan, rows):
        ain[b * npts + p] = row
        ain[b * npts + p + d] = row
    return plan


def pooled_case(recipe, B, npts, Ci, Co):
    """ain (R, Ci), coef [scale | shift] (non-identity, scales of both signs), W (Co, Ci), bias (Co), ties"""
    g = gen(1000 * B + npts + 7 * Ci + Co + (0 if recipe == "integer" else 1))
    R = B * npts
    if recipe == "integer":
        ain, W, bias = ints(g, -4, 4, R, Ci), sparse_pm1(g, 2, Co, Ci), ints(g, -4, 4, Co)
        scale, shift = torch.tensor([1.0, -1.0, 2.0])[torch.randint(0, 3, (Ci,), generator=g)], ints(g, -2, 2, Ci)
        # input channel 2 carries 9-bit integers on both sides (257 = 256 + 1: two bf16 planes each, and 6 x 257 in a planted row): the
        # second planes of BOTH operands must meet for the exact product, so a swapped or dropped plane shows bit for bit
        scale[2], shift[2] = 1.0, 0.0
        ain[::3, 2], W[::4, 2] = 257.0, 257.0
    else:
        ain, W, bias = randn(g, R, Ci), randn(g, Co, Ci) * Ci ** -0.5, randn(g, Co) * 0.5
        scale, shift = torch.rand(Ci, generator=g) * 1.5 + 0.25, randn(g, Ci) * 0.3
        scale[1::5] *= -1.0
    ties = plant_ties(g, ain, B, npts)
    return Case(recipe=recipe, B=B, npts=npts, Ci=Ci, Co=Co, R=R, ain=ain, coef=torch.cat([scale, shift]), W=W, bias=bias, ties=ties)


def other_weights(c):
    """a second W of the same kind (the planes_ready checks overwrite W with it)"""
    g = gen(77 + c.Co + c.Ci)
    return sparse_pm1(g, 2, c.Co, c.Ci) if c.recipe == "integer" else randn(g, c.Co, c.Ci) * c.Ci ** -0.5


NARROW_DIMS = ((64, 3), (64, 64), (64, 64), (128, 64))


def narrow_weights(g, recipe):
    if recipe == "integer":
        W = [ints(g, -1, 1, 64, 3)] + [sparse_pm1(g, 4, co, ci) for co, ci in NARROW_DIMS[1:]]
        return W, [ints(g, -2, 2, co) for co, _ in NARROW_DIMS]
    W = [randn(g, 64, 3)] + [randn(g, co, ci) * (2.0 / ci) ** 0.5 for co, ci in NARROW_DIMS[1:]]
    return W, [randn(g, co) * 0.1 for co, _ in NARROW_DIMS]


def narrow_forward_case(recipe, R, seed=0):
    g = gen(31 * R + seed + (0 if recipe == "integer" else 1))
    x = ints(g, -3, 3, R, 3) if recipe == "integer" else torch.rand(R, 3, generator=g) - 0.5
    W, b = narrow_weights(g, recipe)
    return Case(recipe=recipe, R=R, x=x, W=W, b=b)


def narrow_backward_case(recipe, R):
    """dz4 (R, 128); z1..z3 (R, 64) used only as masks: signs drawn freely, exact zeros and negative zeros planted (both must mask)"""
    g = gen(57 * R + (0 if recipe == "integer" else 1))
    W, _ = narrow_weights(g, recipe)
    if recipe == "integer":
        dz4, z = ints(g, -2, 2, R, 128), [ints(g, -2, 2, R, 64) for _ in range(3)]
    else:
        dz4, z = randn(g, R, 128), [randn(g, R, 64) for _ in range(3)]
    for l, t in enumerate(z):
        if recipe == "real":
            t[t == 0] = 1.0
        t.view(-1)[l::7][:40] = 0.0
        t.view(-1)[l + 3::11][:40] = -0.0
    return Case(recipe=recipe, R=R, dz4=dz4, z=z, W=W)


def sparse_picks(g, pick, B, npts, Co):
    if pick == "one row":
        return ((torch.arange(B) * 7 + 5) % npts).view(B, 1).expand(B, Co).contiguous().int()
    if pick == "early":
        arg = torch.randint(0, 64, (B, Co), generator=g).int()
        arg[EARLY_HIT[0], EARLY_HIT[1]] = EARLY_HIT[2]
        return arg
    arg = torch.randint(0, npts, (B, Co), generator=g).int()
    if pick == "outside":
        flat = arg.view(-1)
        for i, v in enumerate((-1, npts, npts + 5, 1 << 30, -(1 << 31), 256, 64)):
            flat[i::13][:3] = v if (v < 0 or v >= npts) else npts
    return arg


def sparse_case(recipe, shape, pick):
    """g, pooled (positive / negative / exactly 0 by thirds), argsel, W, zprev, coef [scale | shift] (non-identity).  Real data: every
    mask argument (z scale + shift, and z alone) further from 0 than 4 roundings of its terms, except the planted exact zeros."""
    B, npts, Ci, Co = shape
    g0 = gen(B + 3 * npts + 5 * Ci + 7 * Co + 11 * PICKS_ALL.index(pick) + (0 if recipe == "integer" else 1))
    arg = sparse_picks(g0, pick, B, npts, Co)
    third = torch.randint(0, 3, (B, Co), generator=g0)
    if recipe == "integer":
        g, W, zprev = ints(g0, -3, 3, B, Co), sparse_pm1(g0, 2, Co, Ci), ints(g0, -2, 2, B * npts, Ci)
        scale, shift = torch.tensor([1.0, -1.0, 2.0])[torch.randint(0, 3, (Ci,), generator=g0)], ints(g0, -1, 1, Ci)
        mag = ints(g0, 1, 4, B, Co)
    else:
        g, W, zprev = randn(g0, B, Co), randn(g0, Co, Ci) * Co ** -0.5, randn(g0, B * npts, Ci)
        scale, shift = torch.rand(Ci, generator=g0) + 0.5, randn(g0, Ci) * 0.3
        scale[::3] *= -1.0
        mag = torch.rand(B, Co, generator=g0) + 0.1
    scale[0], shift[0] = 0.5, -1.0  # (the planted zeros' coefficients, below)
    shift[1:3] = 0.0
    if recipe == "real":
        for _ in range(2):  # push every mask argument away from 0
            t = zprev.double() * scale.double() + shift.double()
            near = (t.abs() <= 1e-3) | (zprev.abs() <= 1e-3)
            zprev[near] = 1.0 + zprev[near].abs()
    pooled = torch.where(third == 0, mag, torch.where(third == 1, -mag, torch.zeros_like(mag)))
    if pick == "early":
        b, ch, _ = EARLY_HIT
        pooled[b, ch], g[b, ch] = 1.0, 2.0
    # exact zeros of the mask argument, on the row that holds cloud 0's first inside pick: scale 0.5, shift -1, z 2 (0.5 * 2 - 1 = 0) in
    # input channel 0; z = +0.0 / -0.0 with shift 0 in the next two
    n0 = int(arg[0][(arg[0] >= 0) & (arg[0] < npts)][0]) if bool(((arg[0] >= 0) & (arg[0] < npts)).any()) else 0
    zprev[n0, 0] = 2.0
    for j, v in ((1, 0.0), (2, -0.0)):
        if j < Ci:
            zprev[n0, j] = v
    return Case(recipe=recipe, shape=shape, pick=pick, g=g, pooled=pooled, argsel=arg, W=W, zprev=zprev, coef=torch.cat([scale, shift]), row0=n0)


# ---- launch drivers ------------------------------------------------------------------------------------------------------------------
def _lib():
    from samplenet_amd import _lib as L

    return L


class NetLaunch(Launch):
    """Outputs and scratches of one raw call, every one a view into a sentinel-filled buffer of exactly the documented size."""

    def buf(self, shape, dtype=torch.float32, zero=False):
        n = 1
        for s in shape:
            n *= s
        gb = Guarded(n, dtype, zero=zero)
        self.outs.append(gb)
        return gb.view.view(shape)

    def words64(self, n, zero=False):
        """n 64-bit words as a view of a guarded int32 buffer (8-byte aligned: the guard is a multiple of 4 words) -> (Guarded, int64 view)"""
        gb = Guarded(2 * n, torch.int32, zero=zero)
        self.outs.append(gb)
        return gb, gb.view.view(torch.int64)

    def share(self, gb):
        self.outs.append(gb)
        return gb

    def filled(self, t):
        return not bool((t.reshape(-1).view(torch.int32) == SENTINEL).any())

    def untouched(self, t):
        return bool((t.reshape(-1).view(torch.int32) == SENTINEL).all())


def _pool_outputs(call, c, z, arg):
    call.z = call.buf((c.R, c.Co)) if z else None
    call.pooled = call.buf((c.B, c.Co))
    call.argsel = call.buf((c.B, c.Co), torch.int32) if arg else None
    call.zsel = call.buf((c.B, c.Co)) if arg else None


def launch_tile(c, z=True, arg=True, bias=True, keys="dirty", W=None):
    """One sn_linear_forward_maxpool call.  keys: "dirty" (sentinel garbage, keys_cleared = 0), "zeroed" (zeros, keys_cleared = 1) or
    a (Guarded, view) pair that an earlier launch cleared (keys_cleared = 1)."""
    L = _lib()
    call = NetLaunch(("maxpool", c.recipe, c.B, c.npts, c.Ci, c.Co, "z" if z else "-", "arg" if arg else "-", "bias" if bias else "-",
                      keys if isinstance(keys, str) else "rider"))
    _pool_outputs(call, c, z, arg)
    if isinstance(keys, str):
        call.keys_gb, call.keys = call.words64(c.B * 2 * c.Co, zero=(keys == "zeroed"))
    else:
        call.keys_gb, call.keys = call.share(keys[0]), keys[1]
    p = L.ptr
    rc = L.lib.sn_linear_forward_maxpool(c.R, c.Ci, c.Co, c.npts, p(c.ain), p(c.coef), p(c.W if W is None else W), p(c.bias if bias else None),
                                         p(call.z), p(call.keys), p(call.pooled), p(call.argsel), p(call.zsel), int(keys != "dirty"),
                                         L.stream_of(c.ain))
    L.check(rc, str(call.what))
    return call


def launch_wide(c, z=True, arg=True, bias=True, coef=True, W=None, planes=None, planes_ready=0):
    """One sn_linear_forward_maxpool_wide call: the scratch of exactly _scratch_bytes, the planes of exactly 3 Co Ci bf16 (planes: the
    Guarded of an earlier call, to read it again or over it)."""
    L = _lib()
    call = NetLaunch(("maxpool_wide", c.recipe, c.R, c.npts, c.Ci, c.Co, "z" if z else "-", "arg" if arg else "-", "bias" if bias else "-",
                      "coef" if coef else "-", "planes_ready %d" % planes_ready))
    _pool_outputs(call, c, z, arg)
    nbytes = L.lib.sn_linear_forward_maxpool_wide_scratch_bytes(c.R, c.Ci, c.Co, c.npts)
    assert nbytes == wide_scratch_bytes(c.R, c.Co, c.npts)
    call.scratch_gb = call.share(Guarded(nbytes // 4, torch.int32))
    call.planes_gb = call.share(planes if planes is not None else Guarded(3 * c.Co * c.Ci // 2, torch.int32))
    p = L.ptr
    rc = L.lib.sn_linear_forward_maxpool_wide(c.R, c.Ci, c.Co, c.npts, p(c.ain), p(c.coef if coef else None), p(c.W if W is None else W),
                                              p(c.bias if bias else None), p(call.z), p(call.scratch_gb.view), p(call.pooled), p(call.argsel),
                                              p(call.zsel), p(call.planes_gb.view), planes_ready, L.stream_of(c.ain))
    L.check(rc, str(call.what))
    return call


def pool_bits(call):
    return {n: getattr(call, n) for n in ("z", "pooled", "argsel", "zsel") if getattr(call, n) is not None}


def padded_rows(R):
    return (R + 127) // 128 * 128 + 128  # (the rows a ragged last workgroup could reach, and a workgroup more)


def launch_narrow_forward(c, store=True, bias=True, W=None, planes=None, planes_ready=0, zero=None, zero_n=0):
    """One sn_pointnet_narrow_forward call.  The outputs have padded_rows(R) rows: those at and beyond R must stay sentinel.
    zero: a (Guarded, int64 view) pair for the rider, or None (zero_keys == NULL; zero_n is passed all the same)."""
    L = _lib()
    W = c.W if W is None else W
    call = NetLaunch(("narrow_forward", c.recipe, c.R, "store" if store else "-", "bias" if bias else "-", "planes_ready %d" % planes_ready,
                      "zero_n %d" % zero_n, "keys" if zero is not None else "-"))
    Rp = padded_rows(c.R)
    call.z = [call.buf((Rp, 64)) if store else None for _ in range(3)] + [call.buf((Rp, 128))]
    call.planes_gb = call.share(planes if planes is not None else Guarded(3 * 16384 // 2, torch.int32))
    if zero is not None:
        call.share(zero[0])
    p, b = L.ptr, (c.b if bias else [None] * 4)
    rc = L.lib.sn_pointnet_narrow_forward(c.R, p(c.x), p(W[0]), p(b[0]), p(W[1]), p(b[1]), p(W[2]), p(b[2]), p(W[3]), p(b[3]),
                                          p(call.planes_gb.view), planes_ready, p(call.z[0]), p(call.z[1]), p(call.z[2]), p(call.z[3]),
                                          p(zero[1]) if zero is not None else None, zero_n, L.stream_of(c.x))
    L.check(rc, str(call.what))
    return call


def launch_narrow_backward(c, W=None, planes=None, planes_ready=0):
    L = _lib()
    W = c.W if W is None else W
    call = NetLaunch(("narrow_backward", c.recipe, c.R, "planes_ready %d" % planes_ready))
    call.dx = call.buf((padded_rows(c.R), 3))
    call.planes_gb = call.share(planes if planes is not None else Guarded(3 * 16384 // 2, torch.int32))
    p = L.ptr
    rc = L.lib.sn_pointnet_narrow_backward(c.R, p(c.dz4), p(c.z[0]), p(c.z[1]), p(c.z[2]), p(W[0]), p(W[1]), p(W[2]), p(W[3]),
                                           p(call.planes_gb.view), planes_ready, p(call.dx), L.stream_of(c.dz4))
    L.check(rc, str(call.what))
    return call


def launch_sparse(c, mask):
    L = _lib()
    B, npts, Ci, Co = c.shape
    call = NetLaunch(("pool_dgrad_sparse", c.recipe, B, npts, Ci, Co, c.pick, mask))
    call.dyprev = call.buf((B * npts, Ci))
    p = L.ptr
    rc = L.lib.sn_pool_dgrad_sparse(B, npts, Ci, Co, p(c.g), p(c.pooled), p(c.argsel), p(c.W), p(c.zprev if mask != "none" else None),
                                    p(c.coef if mask == "zprev+coef" else None), p(call.dyprev), L.stream_of(c.g))
    L.check(rc, str(call.what))
    return call

"""Plain fp64 restatement of the layer, BatchNorm and max-pool entries of csrc/pointnet_mlp.hip and csrc/pointnet_mlp_backward.hip --
sn_bn_finalize, sn_bn_eval_coef, sn_bn_batch_stats_twopass (sn_bn_output_forward on top of it), sn_bn_backward_coef, sn_pool_forward,
sn_pool_backward, sn_pool_backward_bn, sn_layer_forward_bn, sn_conv_forward_bn_pool, sn_layer_backward in its five routes,
sn_layer_backward_in3, sn_linear_dgrad / sn_linear_wgrad alone and sn_conv_stack_forward_bn layer by layer -- the data the tests feed them, the shape tables (one row per branch, evaluated by hand from
the loops and the dispatch they name) and drivers that call the raw entries through samplenet_amd._lib with every output and scratch
buffer a view into a sentinel-filled allocation (tests/skinny_ref.py: Guarded, Launch).  Imported by tests/test_mlp_host.py (no GPU:
the references against torch's own fp64 modules, the generators' conditions, the tables against the dispatch restated and the
sources) and tests/test_gpu_mlp_direct.py (the calls).  The references are torch in fp64 and call nothing of the library; every
generator takes the device, so the host test runs them on the CPU.

Error bounds are first order and component-wise, counted from the kernels' operations (the count stands next to the line it bounds):
U = 2^-24 is one fp32 rounding; a GEMM of K terms costs (K + 8) U times the magnitude product (the project's figure); an fp32 sum of
n terms in a fixed order costs (n - 1) U times the sum of magnitudes; what a kernel computes in double costs D = 2^-53 per operation
-- nothing next to U -- until it is stored as fp32 (one U).

Two consequences.  sn_bn_finalize and sn_bn_backward_coef add the fp32 partials THEY ARE GIVEN in double: against fp64 of the same
partials every output is good to a few U, and the cancellations ss / R - mean^2 and sz - mean s, done in double, cost nothing
relative to those partials -- channels with |mean| / std of 0, 3 and 100 and a constant channel stand in every case to show it.
sn_bn_batch_stats_twopass takes its sums in double from z itself, and the layer kernels up to 64 rows sum the squares around the
mean in registers: their bounds carry no conditioning factor either.  Where the sums come out of a GEMM epilogue or pool_bwd_kernel
in fp32 (FWD_STATS_SCHEME / STATS_SCHEME: "partials") the bound on mean, var, dgamma, k2, k3 carries what the cancellation makes of
the sums' error -- E_ss / R + 2 |mean| E_mean, invstd (E_sz + |mean| E_s) -- counted, not chosen.

No element is excluded from any comparison: a mask or pick that depends on a sign is made exact by construction (pool values differ
as fp32 numbers except for planted, identical ties; every ReLU argument of the layer backward stands further from 0 than one fp32
rounding of its two terms, a few nudged deterministically, and one channel holds exact zeros), and the host test proves those
conditions for every table row.

sn_layer_backward_in3 is held on real data with dW_in bounded from its closed form, and sn_conv_stack_forward_bn teacher-forced: every
z[l] against the fp64 layer of the GPU's own z[l-1] / coef[l-1], every coef[l] and running statistic against fp64 statistics of the GPU's
own z[l] with the fixed-point quantum in the bound.  sn_conv_stack_backward exposes no intermediate to teacher-force and stays held to
the per-layer walk by the existing test_conv_stack_one_call_backward."""
import os
import re

import torch

from skinny_ref import SENTINEL, Guarded, Launch

U = 2.0 ** -24
D = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MOMENTUM = float(torch.tensor(1e-5).item()), float(torch.tensor(0.1).item())  # the fp32 values the entries receive, as doubles

# ---- shape tables ----------------------------------------------------------------------------------------------------------------
def trips(total, first, lanes, unroll):
    """(unrolled trips, tail trips) of the worker that starts at `first` in the kernels' common loop pair
    `for (; i + (unroll - 1) * lanes < total; i += unroll * lanes)` / `for (; i < total; i += lanes)`"""
    i, wide, tail = first, 0, 0
    while i + (unroll - 1) * lanes < total:
        i, wide = i + unroll * lanes, wide + 1
    while i < total:
        i, tail = i + lanes, tail + 1
    return wide, tail


# Each row: size -> (the branch, (unrolled, tail) trips of the FIRST worker, of the LAST worker), evaluated by hand from the two loops;
# tests/test_mlp_host.py holds them against trips() and asserts that no two rows of a table agree in both pairs AND in the number of
# workers that have anything to do (min(size, workers)).
# partial_sums (mlp_device.h): 1024 threads = 8 channels x 128 slices; slice sl takes blocks sl, sl + 128, ...: four at a time while
# b + 384 < nblk, then one at a time.
PARTIAL_SUMS_TABLE = {
    1: ("tail loop only: slice 0 one load, slices 1..127 none", (0, 1), (0, 0)),
    7: ("tail loop only: slices 0..6 one load (a second row of this kind: fewer blocks than slices, more than one)", (0, 1), (0, 0)),
    128: ("tail loop only: a full slice round, every slice one load", (0, 1), (0, 1)),
    129: ("tail loop only: slice 0 a second trip", (0, 2), (0, 1)),
    385: ("four-way loop on slice 0 alone (0 + 384 < 385) and nothing behind it; slices 1..127 three tail trips", (1, 0), (0, 3)),
    1000: ("four-way loop: slices 0..103 two trips (sl + 896 < 1000), slices 104..127 one trip and three tail trips", (2, 0), (1, 3)),
}
PARTIAL_SUMS_C = {8: "one whole channel block", 5: "one ragged channel block", 72: "nine whole channel blocks"}

# pool_fwd_kernel: 16 waves, wave w takes rows w, w + 16, ...: four at a time while n + 48 < N, then one at a time; wave 0 then
# picks across the waves.
POOL_FWD_TABLE = {
    1: ("fewer rows than waves: waves 1..15 carry (-inf, +inf, row 0) into the cross-wave pick", (0, 1), (0, 0)),
    15: ("fewer rows than waves: wave 15 alone empty (a second row of this kind: ties n, n + 5 fit)", (0, 1), (0, 0)),
    16: ("tail loop, one row per wave", (0, 1), (0, 1)),
    17: ("tail loop, wave 0 a second row: ties n, n + 16 fit", (0, 2), (0, 1)),
    63: ("four-way loop on waves 0..14 (w + 48 < 63) with no tail, wave 15 three tail rows", (1, 0), (0, 3)),
    65: ("four-way loop on every wave, wave 0 one tail row", (1, 1), (1, 0)),
    200: ("four-way loop three times on every wave, waves 0..7 one tail row; ties across 64-row blocks fit", (3, 1), (3, 0)),
}
POOL_FWD_C = {64: "one whole channel block", 40: "one ragged channel block", 100: "two channel blocks, the second ragged"}
POOL_FWD_B = 3

# pool_bwd_kernel: 64 channels x 16 batch slices; slice sl takes clouds sl, sl + 16, ...: four at a time while b + 48 < B
POOL_BWD_TABLE = {
    1: ("tail loop: slice 0 one cloud, slices 1..15 none", (0, 1), (0, 0)),
    16: ("tail loop: every slice one cloud", (0, 1), (0, 1)),
    17: ("tail loop: slice 0 a second cloud", (0, 2), (0, 1)),
    63: ("four-way loop on slices 0..14 (sl + 48 < 63) with no tail, slice 15 three tail trips", (1, 0), (0, 3)),
    65: ("four-way loop on every slice, slice 0 one tail trip", (1, 1), (1, 0)),
    100: ("four-way loop once on every slice, then three (slices 0..3) or two tail trips", (1, 3), (1, 2)),
}
POOL_BWD_C = {64: "one whole channel block", 40: "one ragged channel block"}
POOL_BWD_N = 64  # the rows per cloud the BatchNorm under the pool saw: R = B * 64
# sn_bn_finalize / sn_bn_backward_coef: the row count whose forward leaves that many partial blocks (sn_linear_stats_blocks: 32-row
# blocks up to 64 rows, 64-row blocks above), ragged where the count allows
ROWS_OF_NBLK = {1: 29, 7: 64 * 7 - 3, 128: 64 * 128 - 3, 129: 64 * 129 - 3, 385: 64 * 385 - 3, 1000: 64 * 1000 - 3}

# bn_twopass_kernel: 64 channels x 16 row stripes; stripe st takes rows st, st + 16, ...: eight at a time while r + 112 < R
TWOPASS_TABLE = {
    33: ("tail loop only: three rows on stripe 0, two on stripe 15", (0, 3), (0, 2)),
    127: ("eight-loads loop on stripes 0..14 (st + 112 < 127) with no tail, stripe 15 seven tail rows", (1, 0), (0, 7)),
    128: ("eight-loads loop on every stripe, no tail", (1, 0), (1, 0)),
    129: ("eight-loads loop on every stripe, stripe 0 one tail row", (1, 1), (1, 0)),
    300: ("eight-loads loop twice on every stripe, then three (stripes 0..11) or two tail rows", (2, 3), (2, 2)),
}
TWOPASS_C = {64: "one whole block; C % 4 == 0: sn_bn_output_forward's float4 kernel", 36: "one ragged block; C % 4 == 0",
             5: "one ragged block; C % 4 != 0: sn_bn_output_forward's scalar kernel"}
LOOPS = {"partial_sums": (PARTIAL_SUMS_TABLE, 128, 4), "pool_fwd": (POOL_FWD_TABLE, 16, 4), "pool_bwd": (POOL_BWD_TABLE, 16, 4),
         "twopass": (TWOPASS_TABLE, 16, 8)}

# sn_layer_backward, R <= 32 (small_bwd_kernel).  (R, Ci, Co, dz_mode, npts) -> the branch.  VEC = (Co % 64 == 0); the weight
# gradient stores whole tiles when no bias column is asked for, Ci % 32 == 0 and the tile lies inside Co.
SMALL_BWD_TABLE = [
    ((32, 64, 64, 0, 0), "DZ_PLAIN, VEC, whole dW tiles"),
    ((17, 40, 72, 0, 0), "DZ_PLAIN, scalar loads (Co % 64 != 0), ragged column block, ragged dW tiles"),
    ((5, 64, 128, 1, 0), "DZ_BN, VEC: two K passes per wave pair"),
    ((32, 96, 40, 1, 0), "DZ_BN, scalar loads, three column blocks"),
    ((32, 64, 64, 2, 16), "DZ_POOL, VEC: two clouds of 16 rows"),
    ((24, 40, 72, 2, 8), "DZ_POOL, scalar loads: three clouds of 8 rows"),
]
SMALL_BWD_FORMS = ("rows", "pool", "fixed")  # prev_bn_rows = 0 (R), R * 64 (> 0), -1 (< 0)

# sn_layer_backward above 32 rows, always over a BatchNorm + ReLU layer (coef_prev given).  ((R, Ci, Co, dz_mode, npts), db wanted) ->
# (route, why), each evaluated by hand from the entry's dispatch (layer_backward_route below restates it; the host test holds the two
# together).  Every route in every dz_mode it serves; prev_bn_rows = 0 and < 0 on each (> 0 is refused above 32 rows).
LAYER_BWD_TABLE = [
    (((256, 64, 64, 1, 0), False), ("fused", "conv_bwd_fused_ok: R >= 256, (64, 64), DZ_BN: four whole 64-row tiles, one per workgroup")),
    (((256, 64, 64, 2, 64), False), ("fused", "(64, 64), DZ_POOL, npts % 64 == 0")),
    (((300, 64, 128, 1, 0), False), ("fused", "(64, 128), DZ_BN, a ragged last tile (300 % 64 != 0)")),
    (((320, 64, 128, 2, 64), False), ("fused", "(64, 128), DZ_POOL")),
    (((288, 128, 128, 1, 0), False), ("fused", "(128, 128): 32-row tiles, nine of them on five workgroups")),
    (((320, 128, 128, 2, 64), False), ("fused", "(128, 128), DZ_POOL: two tiles per cloud")),
    (((256, 128, 256, 1, 0), False), ("fused", "256 output channels: two passes over halves of dZ's columns, dYprev summed in place (DZ_BN only)")),
    (((256, 256, 128, 1, 0), False), ("fused", "256 input channels: two independent passes over halves of W's columns")),
    (((256, 256, 128, 2, 64), False), ("fused", "256 input channels, DZ_POOL")),
    (((33, 40, 72, 0, 0), True), ("rows<=64", "rows_bwd_shape, R <= 64: coefficients inside the launch; scalar loads, one half-filled second 32-row half")),
    (((64, 64, 128, 1, 0), False), ("rows<=64", "R = 64 exactly, DZ_BN, VEC")),
    (((70, 40, 72, 1, 0), True), ("rows>64", "rows_bwd_shape, R > 64: two row blocks, bn_bwd_coef_kernel behind; DZ_BN with db (the fused / fast routes refuse db)")),
    (((192, 64, 128, 0, 0), False), ("rows>64", "the largest multiple of 64 on this route; DZ_PLAIN, VEC")),
    (((300, 64, 64, 1, 0), True), ("rows>64", "a fused shape with db wanted: conv_bwd_fused_ok refuses, 300 % 64 != 0 and <= 512")),
    (((256, 128, 64, 1, 0), False), ("fast", "the combined launch: whole tiles, (128, 64) is no fused shape, DZ_BN")),
    (((256, 128, 64, 2, 64), False), ("fast", "the combined launch, DZ_POOL")),
    (((256, 64, 64, 0, 0), True), ("fast", "plain_top: DZ_PLAIN with db, the bias gradient by extra workgroups of the closing launch")),
    (((256, 40, 72, 1, 0), False), ("fallback", "sn_linear_wgrad + sn_linear_dgrad: unaligned widths")),
    (((256, 64, 64, 1, 0), True), ("fallback", "db wanted with dz_mode != 0 at 256 rows (a multiple of 64 above 192: not the rows route)")),
    (((264, 64, 64, 2, 88), False), ("fallback", "DZ_POOL on rows that are no multiple of 64 (never the rows route), npts % 64 != 0 (not fused)")),
    (((576, 40, 72, 0, 0), True), ("fallback", "DZ_PLAIN, unaligned widths, R a multiple of 64 above 192")),
]
LAYER_BWD_FORMS = ("rows", "fixed")
# sn_linear_dgrad / sn_linear_wgrad alone in dz_mode 1 and 2: one tile-path shape, one R <= 32 shape
ALONE_TABLE = [(256, 128, 64, 1, 0), (256, 128, 64, 2, 64), (32, 64, 64, 1, 0), (32, 64, 64, 2, 16)]
FUSED_SHAPES = ((64, 64), (64, 128), (128, 128), (128, 256), (256, 128))


def wgrad_splits(R, Ci, Co, with_bias, cus=256):
    """sn_linear_wgrad_splits restated (cus: the device's compute units; every fused row of the table has fewer tiles)"""
    if R <= 32:
        return 1
    if not with_bias and R >= 256 and (Ci, Co) in FUSED_SHAPES:
        return min((R + 63) // 64, cus)
    tiles = ((Co + 63) // 64) * ((Ci + (1 if with_bias else 0) + 63) // 64)
    return max(1, min(max(1, 512 // tiles), max(1, (R + 127) // 128)))


def layer_backward_route(R, Ci, Co, mode, npts, db):
    """sn_layer_backward's dispatch (coef_prev and kcoef given), predicate by predicate, in its order"""
    if R <= 32:
        return "small"
    if not db and R >= 256 and (Ci, Co) in FUSED_SHAPES and (mode == 1 or (mode == 2 and npts > 0 and npts % 64 == 0 and Co != 256)):
        return "fused"
    if mode != 2 and (R <= 512 if R % 64 else R <= 192):
        return "rows<=64" if R <= 64 else "rows>64"
    nsplit = wgrad_splits(R, Ci, Co, db)
    rps = -(-(-(-R // nsplit)) // 64) * 64
    plain_top = mode == 0
    if (plain_top or (not db and mode != 0)) and R % 64 == 0 and Ci % 64 == 0 and Co % 64 == 0 and R % rps == 0:
        return "fast"
    return "fallback"


# sn_layer_backward_in3: (R, Ci, Co) -> (supported, why); in3_stats_floats restates sn_layer_backward_in3_stats_floats
IN3_TABLE = [
    ((300, 64, 64), True, "64 -> 64 on the xyz layer, five workgroups of one 64-row tile, the last ragged"),
    ((256, 64, 128), False, "a fused shape, but not (64, 64): 0 floats"),
    ((192, 64, 64), False, "(64, 64) below 256 rows: no fused shape, 0 floats"),
]


def in3_stats_floats(R, Ci, Co, cus=256):
    if R < 1 or (Ci, Co) != (64, 64) or R < 256:
        return 0
    return min((R + 63) // 64, cus) * 6 * Ci


# sn_conv_stack_forward_bn, teacher-forced: ((B, N), channels) -> (z[0] == NULL admitted, why)
CONV_STACK_TABLE = [
    (((2, 64), (3, 64, 64, 64, 128, 128)), (False, "the sampler's five layers on two 64-row blocks: too few blocks to carry the weight split (32 > 2)")),
    (((12, 64), (3, 64, 64, 128)), (True, "three layers on twelve blocks: the split of 64 x 64 + 64 x 128 weights takes exactly 12")),
]


def conv_stack_supported(B, N, ch):
    n = len(ch) - 1
    if B < 1 or N < 1 or n < 2 or ch[0] != 3 or B * N <= 64 or N % 64:
        return 0
    if any(c % 64 or c > 256 for c in ch[1:]):
        return 0
    nb = sum((ch[l] * ch[l + 1] + 1023) // 1024 for l in range(1, n))
    if any(c > 128 for c in ch[1:]) and (n - 1 > 4 or nb > B * N // 64 or ch[n] > 128 or ch[1] > 128):
        return 0
    return 1


def conv_stack_z1_free(B, N, ch):
    n = len(ch) - 1
    if not conv_stack_supported(B, N, ch) or n < 3 or n - 1 > 4 or ch[1] != 64 or ch[2] != 64:
        return 0
    return int(sum((ch[l] * ch[l + 1] + 1023) // 1024 for l in range(1, n)) <= B * N // 64)


# sn_layer_forward_bn.  ((R, Ci, Co), coef_prev given, running statistics given) -> (route, why); layer_forward_route restates the dispatch.
LAYER_FWD_TABLE = [
    (((5, 64, 40), True, True), ("small lds", "R <= 32, Ci a power of two in 64..512: small_fwd_lds_kernel, finalised in the epilogue")),
    (((32, 192, 72), False, True), ("small vec", "R <= 32, Ci % 64 == 0 but no power of two: small_fwd_kernel<VEC>; raw input")),
    (((17, 40, 64), True, False), ("small scalar", "R <= 32, Ci % 64 != 0: small_fwd_kernel scalar loads; no running statistics")),
    (((33, 64, 72), True, True), ("rows64", "33..64 rows, Ci = 64: rows64_fwd_kernel, second half one row")),
    (((48, 128, 40), False, False), ("rows64", "Ci = 128, raw input, no running statistics")),
    (((64, 256, 64), True, True), ("rows64", "Ci = 256, both halves full")),
    (((40, 96, 72), True, True), ("tile small", "33..64 rows with another Ci: 32-row tiles (two partial blocks) + bn_finalize_kernel")),
    (((128, 64, 64), True, True), ("tile big", "R > 64, aligned: whole 64 x 64 tiles + bn_finalize_kernel")),
    (((200, 40, 72), True, False), ("tile big", "R > 64, ragged rows, ragged widths, no running statistics")),
    (((130, 128, 128), False, True), ("tile big", "R > 64, ragged rows only, raw input")),
    (((128, 3, 64), False, True), ("in3", "the xyz layer above 64 rows: conv_in3_fwd_kernel, raw input")),
]
# sn_conv_forward_bn_pool: (R, npts, Ci, Co) -> why
CONV_POOL_TABLE = [
    ((128, 64, 64, 128), "two clouds, one 64-row block each"),
    ((320, 64, 128, 64), "five clouds, one block each"),
    ((384, 192, 64, 64), "two clouds, three blocks per cloud: the pick runs over a cloud's blocks, one per quarter of its threads"),
    ((640, 320, 64, 64), "two clouds, five blocks per cloud: a quarter walks TWO blocks in order (rows 7 and 77 tie inside quarter 0)"),
]


def layer_forward_route(R, Ci, Co, coef_prev):
    """sn_layer_forward_bn's dispatch and launch_fwd's behind it, predicate by predicate"""
    if 32 < R <= 64 and Ci in (64, 128, 256):
        return "rows64"
    if not coef_prev and Ci == 3 and R > 64:
        return "in3"
    if R <= 32:
        if 64 <= Ci <= 512 and Ci & (Ci - 1) == 0:
            return "small lds"
        return "small vec" if Ci % 64 == 0 else "small scalar"
    return "tile big" if R > 64 else "tile small"


# how each forward route takes the batch statistics: ("registers", n): mean from an fp32 sum of at most n additions, then the squares
# around its fp32 rounding (two-pass, in the lane's registers, corrected in double); ("partials", n): fp32 sums of z and z z over
# blocks of n rows, added in double -- var = ss / R - mean^2 then carries the conditioning of that difference
FWD_STATS_SCHEME = {"small lds": ("registers", 17), "small vec": ("registers", 17), "small scalar": ("registers", 17), "rows64": ("registers", 33),
                    "tile small": ("partials", 32), "tile big": ("partials", 64), "in3": ("partials", 64)}


# ---- the route predicates of the dispatch, read from the sources --------------------------------------------------------------------
ROUTE_PATTERNS = {
    # name -> (file, regular expression that must match exactly once)
    "partial_sums four-way": ("mlp_device.h", r"for \(; b \+ 3 \* kSlices < nblk; b \+= 4 \* kSlices\)"),
    "partial_sums tail": ("mlp_device.h", r"for \(; b < nblk; b \+= kSlices\)"),
    "partial_sums geometry": ("mlp_device.h", r"constexpr int kSlices = 128, kChan = 8;"),
    "pool_fwd waves": ("pointnet_mlp.hip", r"constexpr int NW = 16;"),
    "pool_fwd four-way": ("pointnet_mlp.hip", r"for \(; n \+ 3 \* NW < N; n \+= 4 \* NW\)"),
    "pool_fwd tail": ("pointnet_mlp.hip", r"for \(; n < N; n \+= NW\)"),
    "pool_fwd pick": ("pointnet_mlp.hip", r"const bool up = sc >= 0\.f;"),
    "pool_bwd four-way": ("pointnet_mlp_backward.hip", r"for \(; b \+ 3 \* 16 < B; b \+= 4 \* 16\)"),
    "pool_bwd tail": ("pointnet_mlp_backward.hip", r"for \(; b < B; b \+= 16\)"),
    "twopass eight loads": ("pointnet_mlp.hip", r"for \(; r \+ 7 \* 16 < R; r \+= 8 \* 16\)"),
    "twopass tail": ("pointnet_mlp.hip", r"for \(; r < R; r \+= 16\)"),
    "bn_output float4": ("pointnet_mlp.hip", r"if \(C % 4 == 0\) \{"),
    "layer_backward small": ("pointnet_mlp_backward.hip", r"if \(R <= 32\) \{\n        DgradArgs g = make_dgrad"),
    "layer_backward small VEC": ("pointnet_mlp_backward.hip", r"dz_mode, coef_prev != nullptr, Co % 64 == 0,"),
    "layer_backward bn rows": ("pointnet_mlp_backward.hip", r"prev_bn_rows > 0 \? prev_bn_rows : \(prev_bn_rows < 0 \? -1ll : \(long long\)R\)"),
    "layer_backward fused": ("pointnet_mlp_backward.hip", r"return !db && coef_prev && kcoef && conv_bwd_fused_shape\(R, Ci, Co\) &&\n\s+\(dz_mode == DZ_BN \|\| "
                             r"\(dz_mode == DZ_POOL && npts > 0 && npts % 64 == 0 && Co != 256\)\);"),
    "layer_backward fused rows": ("pointnet_mlp_backward.hip", r"if \(R < 256\) return false;\n    if \(\(Ci == 64 && \(Co == 64 \|\| Co == 128\)\) \|\| "
                                  r"\(Ci == 128 && Co == 128\)\) return true;"),
    "layer_backward fused 256": ("pointnet_mlp_backward.hip", r"if \(\(Ci == 128 && Co == 256\) \|\| \(Ci == 256 && Co == 128\)\) return true;"),
    "layer_backward rows": ("pointnet_mlp_backward.hip", r"if \(R <= 32 \|\| dz_mode == DZ_POOL\) return false;\n    return R % 64 != 0 \? R <= 512 : R <= 192;"),
    "layer_backward rows fin": ("pointnet_mlp_backward.hip", r"const bool fin = coef_prev && R <= 64;"),
    "layer_backward fast": ("pointnet_mlp_backward.hip", r"const bool fast = \(plain_top \|\| \(!db && dz_mode != DZ_PLAIN\)\) && coef_prev && R % TileBig::BM == 0 && "
                            r"Ci % TileBig::BN == 0 &&\n\s+Co % BK == 0 && Co % TileW::BM == 0 && Ci % TileW::BN == 0 && R % rps == 0;"),
    "layer_backward plain_top": ("pointnet_mlp_backward.hip", r"const bool plain_top = dz_mode == DZ_PLAIN && dy != nullptr;"),
    "layer_backward pool rows": ("pointnet_mlp_backward.hip", r'SN_REQUIRE\(prev_bn_rows <= 0 \|\| R <= 32,'),
    "wgrad splits": ("pointnet_mlp_backward.hip", r"const int want = std::max\(1, 512 / tiles\);\s+// [^\n]*\n    const int maxsplit = std::max\(1, \(R \+ 2 \* BK - 1\) / \(2 \* BK\)\);"),
    "layer_forward rows64": ("pointnet_mlp.hip", r"if \(R > 32 && R <= 64 && \(Ci == 64 \|\| Ci == 128 \|\| Ci == 256\)\) \{"),
    "layer_forward in3": ("pointnet_mlp.hip", r"if \(AMODE == ACT_NONE && Ci == 3 && R > 64\) \{"),
    "layer_forward lds_ci": ("pointnet_mlp.hip", r"const bool lds_ci = Ci >= 64 && Ci <= 512 && \(Ci & \(Ci - 1\)\) == 0;"),
    "layer_forward small": ("pointnet_mlp.hip", r"if \(R <= 32 \|\| row_tiled\) \{"),
    "layer_forward small vec": ("pointnet_mlp.hip", r"\} else if \(Ci % 64 == 0\)\n\s+hipLaunchKernelGGL\(\(small_fwd_kernel<AMODE, true>\)"),
    "layer_forward tile big": ("pointnet_mlp.hip", r"\} else if \(R > 64\) \{\n\s+dim3 grid\(\(R \+ TileBig::BM - 1\) / TileBig::BM"),
    "layer_forward finalize": ("pointnet_mlp.hip", r"if \(R > 32\)\n\s+hipLaunchKernelGGL\(bn_finalize_kernel,"),
    "conv_pool shapes": ("pointnet_mlp.hip", r"if \(R <= 64 \|\| R % 64 \|\| npts % 64 \|\| R % npts \|\| Co % 64 \|\| Ci % 64\)"),
    "in3 stats floats": ("pointnet_mlp_backward.hip", r"if \(R < 1 \|\| !\(Ci == 64 && Co == 64\) \|\| !conv_bwd_fused_shape\(R, Ci, Co\)\) return 0;\n    return \(long long\)conv_bwd_fused_groups\(R\) \* 6 \* Ci;"),
    "conv stack supported": ("pointnet_mlp.hip", r"if \(R <= 64 \|\| R > \(1ll << 30\) \|\| N % 64\) return 0;"),
    "conv stack z1 free": ("pointnet_mlp.hip", r"if \(channels\[1\] != 64 \|\| channels\[2\] != 64\) return 0;\n    long long nb = 0;\n    for \(int l = 1; l < nlayers; \+\+l\) nb \+= "
                           r"\(\(long long\)channels\[l\] \* channels\[l \+ 1\] \+ 1023\) / 1024;\n    return nb <= \(long long\)B \* N / 64 \? 1 : 0;"),
    "fixed point shift": ("mlp_device.h", r"constexpr int kFxShiftFwd = 32, kFxShiftBwd = 60;"),
    "fixed point rounding": ("mlp_device.h", r"\(unsigned long long\)__double2ll_rn\(d\)\);"),
    "stats blocks": ("pointnet_mlp.hip", r"return R > 64 \? \(R \+ TileBig::BM - 1\) / TileBig::BM : \(R \+ TileSmall::BM - 1\) / TileSmall::BM;"),
}
# the loops with one occurrence per pass over the data (two-pass kernel: mean pass and squares pass)
# (and the VEC predicate once in sn_linear_dgrad's R <= 32 launch, once in sn_layer_backward's)
ROUTE_COUNTS = {"twopass eight loads": 2, "twopass tail": 2, "layer_backward small VEC": 2}


def source_routes():
    """name -> number of matches of its pattern in its source file"""
    out, texts = {}, {}
    for name, (fn, pat) in ROUTE_PATTERNS.items():
        if fn not in texts:
            texts[fn] = open(os.path.join(ROOT, "samplenet_amd", "csrc", fn)).read()
        out[name] = len(re.findall(pat, texts[fn]))
    return out


def source_constants():
    out = {}
    text = open(os.path.join(ROOT, "samplenet_amd", "csrc", "mlp_host.h")).read()
    for name in ("TileBig", "TileSmall"):
        out[name + "::BM"] = int(re.search(r"using %s = Tile<(\d+)," % name, text).group(1))
    return out


def stats_blocks(R, k):
    return (R + k["TileBig::BM"] - 1) // k["TileBig::BM"] if R > 64 else (R + k["TileSmall::BM"] - 1) // k["TileSmall::BM"]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=g.device, generator=g)


def rand(g, *shape):
    return torch.rand(*shape, device=g.device, generator=g)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, device=g.device, generator=g).float()


def signed_pow2(g, *shape):
    """values from {-2, -1, 1, 2}"""
    return (torch.randint(1, 3, shape, device=g.device, generator=g) * (torch.randint(0, 2, shape, device=g.device, generator=g) * 2 - 1)).float()


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


RATIOS = (0.0, 3.0, 100.0)  # |mean| / std of channels 0, 1, 2; channel 3 is constant (C >= 5 in every table)


def bn_params(g, C):
    """gamma of both signs with one zero, beta, running statistics"""
    gamma = randn(g, C)
    gamma[4 % C] = 0.0
    gamma[0], gamma[1] = 1.25, -0.75
    return gamma, randn(g, C) * 0.5, randn(g, C), rand(g, C) + 0.5


def finalize_case(nblk, C, R, dev, seed=0):
    """Synthetic partials (nblk, 2, C) fp32 -- no GEMM in front: block b holds the sum and the sum of squares of R / nblk values of
    mean mu_c and deviation sd_c, drawn directly.  Channels 0..2: |mu| / sd = 0, 3, 100; channel 3 constant (2.0: every partial exact,
    variance 0 before the clamp up to the double rounding of 1 / R)."""
    g = gen(seed * 7919 + nblk * 131 + C * 17 + 1, dev)
    n = R / float(nblk)
    sd = rand(g, C).double() + 0.5
    mu = randn(g, C).double()
    for c, ratio in enumerate(RATIOS):
        mu[c] = ratio * sd[c] * (-1.0 if c == 1 else 1.0)
    m_b = mu + sd * randn(g, nblk, C).double() * n ** -0.5          # block means
    v_b = sd * sd * (1.0 + 0.2 * (rand(g, nblk, C).double() - 0.5))   # block variances
    s, ss = n * m_b, n * (v_b + m_b * m_b)
    rows_b = torch.full((nblk,), 64.0 if nblk > 1 else float(R), dtype=torch.float64, device=dev)
    rows_b[-1] = R - 64.0 * (nblk - 1) if nblk > 1 else float(R)                  # (whole numbers of rows: the constant channel's partials are exact)
    s[:, 3], ss[:, 3] = 2.0 * rows_b, 4.0 * rows_b
    stats = torch.stack([s, ss], 1).float().contiguous()
    if R == 1:  # one row: s = z, ss = z z rounded to fp32
        z = randn(g, C)
        stats = torch.stack([z, z * z]).view(1, 2, C).contiguous()
    gamma, beta, rm, rv = bn_params(g, C)
    return Case(nblk=nblk, C=C, R=R, stats=stats, gamma=gamma, beta=beta, rm=rm, rv=rv)


def twopass_case(R, C, dev, seed=0):
    """z (R, C) fp32: channels 0..2 with |mean| / std = 0, 3, 100, channel 3 constant, the rest standard normal around a random mean"""
    g = gen(seed * 104729 + R * 31 + C + 2, dev)
    sd = rand(g, C) + 0.5
    mu = randn(g, C)
    z = randn(g, R, C)
    z = (z - z.mean(0)) / z.std(0, unbiased=False) if R > 1 else z
    for c, ratio in enumerate(RATIOS):
        mu[c] = ratio * sd[c] * (-1.0 if c == 1 else 1.0)
    z = (z * sd + mu).contiguous()
    z[:, 3] = 2.0
    gamma, beta, rm, rv = bn_params(g, C)
    return Case(R=R, C=C, z=z, gamma=gamma, beta=beta, rm=rm, rv=rv)


def eval_case(C, dev, seed=0):
    g = gen(seed * 31 + C + 3, dev)
    gamma, beta, rm, rv = bn_params(g, C)
    rv[2 % C] = 1e-4  # a small running variance: eps is a tenth of it
    return Case(C=C, gamma=gamma, beta=beta, rm=rm, rv=rv)


# ---- BatchNorm forward references ----------------------------------------------------------------------------------------------------
def bn_coef_ref(mean, var, E_mean, E_var, gamma, beta, eps, momentum, rm, rv, R):
    """bn_finalize_channel_mv from a batch mean and BIASED variance known to E_mean / E_var: coefficients (scale, shift, mean, invstd)
    and torch.nn.BatchNorm1d's running-statistics update (the unbiased variance var R / (R - 1); R == 1 keeps the biased one: THE
    CONTRACT, torch itself refuses one row in training mode).  rm None: no update.  -> dict name -> (value, bound)"""
    inv = (var + eps) ** -0.5
    E_inv = 0.5 * inv * E_var / (var + eps) + U * inv       # fast_rsqrt: double-accurate after two Newton steps; stored as fp32: U
    gm, b = gamma.double(), beta.double()
    sc = gm * inv
    E_sc = gm.abs() * E_inv + U * sc.abs()                  # gamma * invstd: one product
    sh = b - mean * sc
    E_meanf = E_mean + U * mean.abs()                       # (float)mean
    E_sh = mean.abs() * E_sc + sc.abs() * E_meanf + U * (mean * sc).abs() + U * (b.abs() + (mean * sc).abs())  # product, subtraction
    out = {"scale": (sc, E_sc), "shift": (sh, E_sh), "mean": (mean, E_meanf), "invstd": (inv, E_inv)}
    if rm is not None:
        unbias = R / (R - 1.0) if R > 1 else 1.0
        unb = var * unbias
        m = momentum
        a, bb = (1 - m) * rm.double(), (1 - m) * rv.double()
        # (1.f - m): one rounding, times the old value: one; m * new: one; the sum: one (on at most the sum of the magnitudes)
        out["running_mean"] = (a + m * mean, 2 * U * a.abs() + U * (m * mean).abs() + U * (a.abs() + (m * mean).abs()) + m * E_meanf)
        E_unb = E_var * unbias + U * unb                    # (float)unbiased
        out["running_var"] = (bb + m * unb, 2 * U * bb.abs() + U * (m * unb) + U * (bb.abs() + m * unb) + m * E_unb)
    return out


def finalize_ref(c, with_running=True):
    """sn_bn_finalize against fp64 OF THE SAME PARTIALS: s, ss summed in double (nblk terms, any order: nblk D), mean = s rR with
    rR = 1 / R to one double ulp, var = max(ss rR - mean^2, 0) in double: (nblk + 4) D on each of the two terms, NOT U -- the
    cancellation costs nothing relative to the partials."""
    st = c.stats.double()
    s, ss = st[:, 0].sum(0), st[:, 1].sum(0)
    sa, ssa = st[:, 0].abs().sum(0), st[:, 1].abs().sum(0)
    mean = s / c.R
    var = (ss / c.R - mean * mean).clamp_min(0)
    E_mean = (c.nblk + 2) * D * sa / c.R
    E_var = (c.nblk + 4) * D * (ssa / c.R + mean * mean) + 2 * mean.abs() * E_mean
    return bn_coef_ref(mean, var, E_mean, E_var, c.gamma, c.beta, EPS, MOMENTUM, c.rm if with_running else None, c.rv, c.R)


def twopass_ref(c, with_running=True):
    """sn_bn_batch_stats_twopass: the mean and the squares around it summed in double from z itself: (R + 2) D each.  No conditioning
    factor: a channel with |mean| / std = 100 is held to the same few U as one with mean 0."""
    zd = c.z.double()
    mean = zd.mean(0)
    var = ((zd - mean) ** 2).mean(0)
    E_mean = (c.R + 2) * D * zd.abs().mean(0)
    E_var = (c.R + 4) * D * var + 2 * E_mean * (zd - mean).abs().mean(0)
    return bn_coef_ref(mean, var, E_mean, E_var, c.gamma, c.beta, EPS, MOMENTUM, c.rm if with_running else None, c.rv, c.R)


def eval_coef_ref(c):
    """sn_bn_eval_coef, all in fp32: invstd = 1 / sqrtf(rv + eps): the sum one U (half of it behind the root), the root one, the
    quotient one: 2.5 U; scale one product; shift a product and a subtraction; mean a copy."""
    rm, rv = c.rm.double(), c.rv.double()
    inv = (rv + EPS) ** -0.5
    E_inv = 2.5 * U * inv
    sc = c.gamma.double() * inv
    E_sc = c.gamma.double().abs() * E_inv + U * sc.abs()
    sh = c.beta.double() - rm * sc
    E_sh = rm.abs() * E_sc + U * (rm * sc).abs() + U * (c.beta.double().abs() + (rm * sc).abs())
    return {"scale": (sc, E_sc), "shift": (sh, E_sh), "mean": (rm, torch.zeros_like(rm)), "invstd": (inv, E_inv)}


def layer_forward_case(shape, with_prev, dev, seed=0):
    """ain (R, Ci), W ~ Ci^-1/2, bias, BatchNorm parameters; with_prev: ain is a pre-BN tensor seen through coef_prev (4, Ci) with
    real-valued scale / shift (the activation is max(x, 0) of a value rounded once: no decision to protect -- a rounding keeps the sign)"""
    R, Ci, Co = shape
    g = gen(seed * 7919 + R * 131 + Ci * 17 + Co + 7, dev)
    c = Case(R=R, Ci=Ci, C=Co, Co=Co, ain=(randn(g, R, Ci) * 1.5 + 0.5).contiguous(), W=(randn(g, Co, Ci) * Ci ** -0.5).contiguous(),
             bias=randn(g, Co) * 0.5, coef_prev=coef_of(g, Ci) if with_prev else None)
    c.gamma, c.beta, c.rm, c.rv = bn_params(g, Co)
    return c


def layer_z_ref(c):
    """Z = act(A) W^T + b in fp64 with its bound: the GEMM of Ci terms in 8 partials, their tree and the bias add: (Ci + 8) U; the
    activation relu(fmaf(x, scale, shift)) rounded once before the GEMM reads it: one more U"""
    if c.coef_prev is None:
        a, extra = c.ain.double(), 0.0
    else:
        a, extra = (c.ain.double() * c.coef_prev[0].double() + c.coef_prev[1].double()).clamp_min(0), 1.0
    W, b = c.W.double(), c.bias.double()
    return a @ W.t() + b, (c.Ci + 8 + extra) * U * (a.abs() @ W.abs().t() + b.abs())


def layer_stats_ref(z, c, route, with_running=True):
    """Coefficients and running statistics from fp64 statistics of THE GPU'S OWN z (R, Co), bounds by FWD_STATS_SCHEME[route]."""
    scheme, n = FWD_STATS_SCHEME[route]
    R = z.shape[0]
    zd = z.double()
    mean = zd.mean(0)
    var = ((zd - mean) ** 2).mean(0)
    if scheme == "registers":
        E_mean = n * U * zd.abs().mean(0)                 # s0: at most n additions; mean = s0 / R in double
        E_var = (n + 3) * U * var                         # per term the subtraction (twice in the square) and the product; n additions
    else:
        ms = (zd * zd).mean(0)
        E_mean = (n - 1) * U * zd.abs().mean(0)           # a block's n rows in any order: n - 1 additions; blocks added in double
        E_var = n * U * ms + 2 * mean.abs() * E_mean      # the product and n - 1 additions; ss / R - mean^2 in double: the conditioning
    return bn_coef_ref(mean, var, E_mean, E_var, c.gamma, c.beta, EPS, MOMENTUM, c.rm if with_running else None, c.rv, R)


# ---- BatchNorm backward --------------------------------------------------------------------------------------------------------------
def bn_backward_ref(coef, dg, E_dg, s, E_s, rows, fixed=False):
    """bn_backward_coefs from dgamma = invstd sum dY (Z - mean) and s = sum dY (doubles in the kernel, known to E_dg / E_s), with
    dZ = k1 dY + k2 Z + k3 over `rows` rows the BatchNorm averaged over.  fixed (the entries' R <= 0 / prev_bn_rows < 0): k2 = k3 = 0;
    dgamma / dbeta unchanged.  dbias = sum_r dZ = k1 s + k2 rows mean + rows k3 from the fp32 k1, k2, k3, in double: identically 0 in
    exact arithmetic for batch statistics (what is left is the rounding of k2 and k3), k1 s for fixed ones.
    -> dict name -> (value, bound)"""
    sc, mean, inv = coef[0].double(), coef[2].double(), coef[3].double()
    rinv = 0.0 if fixed else 1.0 / rows
    k2 = -sc * inv * dg * rinv
    E_k2 = (sc * inv).abs() * rinv * E_dg + U * k2.abs()                     # stored as fp32: U
    t1, t2 = sc * inv * mean * dg * rinv, sc * s * rinv
    k3 = t1 - t2
    E_k3 = sc.abs() * rinv * ((inv * mean).abs() * E_dg + E_s) + 8 * D * (t1.abs() + t2.abs()) + U * k3.abs()  # the difference in double
    rr = 0.0 if fixed else float(rows)
    parts = (sc * s, k2 * rr * mean, rr * k3)
    dbias = parts[0] + parts[1] + parts[2]
    # batch statistics: the expression vanishes identically for ANY s and dg the kernel holds, so their errors do not reach it: what is
    # left is the fp32 rounding of k2 and k3 (times rows), the double arithmetic, and the store.  Fixed statistics: k1 s.
    E_db = (sc.abs() * E_s if fixed else rr * (U * ((k2 * mean).abs() + k3.abs()) + 8 * D * (t1.abs() + t2.abs()))) + \
        4 * D * sum(p.abs() for p in parts) + U * dbias.abs()
    return {"dgamma": (dg, E_dg + U * dg.abs()), "dbeta": (s, E_s + U * s.abs()), "dbias": (dbias, E_db),
            "kcoef": (torch.stack([sc, k2, k3]), torch.stack([torch.zeros_like(sc), E_k2, E_k3]))}


def coef_of(g, C, mean=None, var=None):
    """(4, C) fp32 coefficients of a BatchNorm with the given (or drawn) statistics: gamma of both signs, one zero"""
    dev = g.device
    gamma, beta = randn(g, C), randn(g, C) * 0.5
    gamma[4 % C] = 0.0
    gamma[0], gamma[1] = 1.25, -0.75
    mean = randn(g, C).double() * 0.5 if mean is None else mean
    var = rand(g, C).double() + 0.5 if var is None else var
    mean32, inv32 = mean.float(), ((var + EPS) ** -0.5).float()
    sc = gamma * inv32
    return torch.stack([sc, beta - mean32 * sc, mean32, inv32]).contiguous().to(dev)


def backward_coef_case(recipe, nblk, C, R, dev, seed=0):
    """Synthetic partials (nblk, 2, C) = (sum dY, sum dY Z) per block and coefficients.  real: block sums of R / nblk products of a
    gradient of unit size with Z of mean mu_c and deviation sd_c, |mu| / sd = 0, 3, 100 on channels 0..2 -- sz - mean s then cancels
    two to four digits, in double.  integer: sums in [-64, 64], scale from {+-1, +-2}, mean an integer, invstd and R powers of two:
    every output exact in fp32 whatever the order."""
    g = gen(seed * 7919 + nblk * 131 + C * 17 + R + (0 if recipe == "integer" else 50021), dev)
    if recipe == "integer":
        assert R & (R - 1) == 0
        stats = ints(g, -64, 64, nblk, 2, C)
        coef = torch.stack([signed_pow2(g, C), ints(g, -2, 2, C), ints(g, -2, 2, C), torch.full((C,), 0.5, device=dev)]).contiguous()
        return Case(recipe=recipe, nblk=nblk, C=C, R=R, stats=stats, coef=coef)
    n = R / float(nblk)
    sd = rand(g, C).double() + 0.5
    mu = randn(g, C).double()
    for c, ratio in enumerate(RATIOS):
        mu[c] = ratio * sd[c] * (-1.0 if c == 1 else 1.0)
    s = randn(g, nblk, C).double() * n ** 0.5
    sz = mu * s + sd * randn(g, nblk, C).double() * n ** 0.5
    stats = torch.stack([s, sz], 1).float().contiguous()
    return Case(recipe=recipe, nblk=nblk, C=C, R=R, stats=stats, coef=coef_of(g, C, mu, sd * sd))


def int_rows(nblk):
    """a power of two of rows for the integer recipe (1 / R exact): 64 times the next power of two at or above nblk"""
    return 64 * (1 << (nblk - 1).bit_length())


def backward_coef_ref(c):
    """sn_bn_backward_coef against fp64 of the same partials: both sums in double (nblk D), dg = invstd (sz - mean s) in double:
    4 D on each of its two terms."""
    st = c.stats.double()
    s, sz = st[:, 0].sum(0), st[:, 1].sum(0)
    sa, sza = st[:, 0].abs().sum(0), st[:, 1].abs().sum(0)
    mean, inv = c.coef[2].double(), c.coef[3].double()
    dg = inv * (sz - mean * s)
    E_s = (c.nblk + 2) * D * sa
    E_dg = inv * ((c.nblk + 4) * D * (sza + mean.abs() * sa))
    return bn_backward_ref(c.coef, dg, E_dg, s, E_s, c.R)


# ---- max-pool ------------------------------------------------------------------------------------------------------------------------
TIE_ARRANGEMENTS = (("one wave's row stride", 16), ("across waves", 5), ("across 64-row blocks", 67))


def pool_case(N, C, dev, B=POOL_FWD_B, seed=0):
    """z (B, N, C) fp32 whose values along the points differ pairwise AS FP32 NUMBERS (a random permutation of the multiples of 1/64
    plus one offset per cloud and channel), and (4, C) coefficients: scales of both signs, channel 2 exactly 0, channel 3 exactly
    -0.0 (both pick the maximum: -0.0 >= 0).  Ties, planted as identical fp32 values that are the extreme the channel selects: on
    channels 5, 6, 7 (positive scale: two maxima) and 8, 9, 10 (negative: two minima) rows n and n + 16 (within one wave's row
    stride), n and n + 5 (across waves), n and n + 67 (across 64-row blocks), where N holds both rows; the LATER row comes first in
    a wave's own order for no arrangement, so only `first row` tells the answer."""
    g = gen(seed * 7919 + N * 131 + C * 17 + B + 4, dev)
    rank = rand(g, B, N, C).argsort(1).argsort(1).float()                   # a permutation of 0..N-1 along the points
    z = ((rank - N // 2) / 64.0 + rand(g, B, 1, C) / 128.0).contiguous()
    coef = coef_of(g, C)
    coef[0, 2], coef[0, 3] = 0.0, -0.0
    coef[0, 5:8] = coef[0, 5:8].abs() + 0.25
    coef[0, 8:11] = -coef[0, 8:11].abs() - 0.25
    coef[1] = randn(g, C) * 0.5 - coef[0] * 0.5                              # shift: the selected pre-activations of both signs
    ties = []
    for k, (name, step) in enumerate(TIE_ARRANGEMENTS):
        for c, sign in ((5 + k, 1.0), (8 + k, -1.0)):
            for b in range(B):
                n0 = (3 + 7 * b + k) % N
                if n0 + step >= N or c >= C:
                    continue
                v = sign * (float(z[b, :, c].abs().max()) + 1.0 + b / 4.0)
                z[b, n0, c] = v
                z[b, n0 + step, c] = v
                ties.append((name, b, n0, n0 + step, c))
    return Case(B=B, N=N, C=C, z=z, coef=coef, ties=ties)


def pool_forward_ref(z, coef):
    """pooled = relu(scale (scale >= 0 ? max_n z : min_n z) + shift), argsel = the FIRST row that holds the selected value, zsel = the
    selected pre-BN value.  A scale of exactly 0 (and -0.0) selects the maximum.  The kernel rounds once, in relu(fmaf(zs, sc, sh)):
    U |zs sc + sh|; a single rounding keeps the sign, so the ReLU decides as the exact value does.
    -> argsel (int32), zsel (fp32, exact), pooled (fp64), bound"""
    sc, sh = coef[0], coef[1]
    zmax, zmin = z.max(1).values, z.min(1).values
    first = lambda hit: hit.int().argmax(1).int()
    up = sc >= 0
    arg = torch.where(up, first(z == zmax[:, None, :]), first(z == zmin[:, None, :]))
    zs = torch.where(up, zmax, zmin)
    pre = zs.double() * sc.double() + sh.double()
    return arg, zs, pre.clamp_min(0), U * pre.abs()


def pool_backward_case(recipe, B, C, dev, seed=0):
    """g, pooled, zsel (B, C) and the last conv layer's coefficients.  pooled: a third exactly 0 (the ReLU was dead there; g is NOT
    zero there, so the mask `> 0` differs from `>= 0`), the rest positive.  integer: g in [-2, 2], zsel in [-3, 3], scale from
    {+-1, +-2}, mean an integer, invstd a power of two; B and B * 64 powers of two -> every output exact."""
    g_ = gen(seed * 7919 + B * 131 + C * 17 + (5 if recipe == "integer" else 60013), dev)
    dead = rand(g_, B, C) < 1.0 / 3.0
    dead[0, 0], dead[0, 1] = True, False
    if recipe == "integer":
        assert B & (B - 1) == 0
        g = ints(g_, 1, 2, B, C) * (ints(g_, 0, 1, B, C) * 2 - 1)
        zsel = ints(g_, -3, 3, B, C)
        pooled = torch.where(dead, torch.zeros_like(g), ints(g_, 1, 4, B, C))
        coef = torch.stack([signed_pow2(g_, C), ints(g_, -2, 2, C), ints(g_, -2, 2, C), torch.full((C,), 0.5, device=dev)]).contiguous()
    else:
        g = randn(g_, B, C)
        g[0, 0] = 1.5
        coef = coef_of(g_, C)
        zsel = (coef[2] + randn(g_, B, C) * 2.0).contiguous()
        pooled = torch.where(dead, torch.zeros_like(g), rand(g_, B, C) + 2.0 ** -20)
    return Case(recipe=recipe, B=B, C=C, g=g.contiguous(), pooled=pooled.contiguous(), zsel=zsel.contiguous(), coef=coef)


def pool_backward_ref(c, rows=None, fixed=False):
    """gsel = g [pooled > 0] (exact), the two sums, and -- with rows / fixed -- the BatchNorm backward of the layer under the pool,
    which averaged over `rows` = B N rows while only B carry a gradient.  pool_bwd_kernel sums in fp32: slice sl adds its
    ceil(B / 16) clouds in ascending order, then 16 slice sums are added: every term passes at most ceil(B / 16) + 15 additions;
    the product gsel zsel one more.  dgamma = invstd (sz - mean s) from those fp32 sums: the conditioning of that difference is in
    E_dg = invstd (E_sz + |mean| E_s)."""
    gsel = torch.where(c.pooled > 0, c.g, torch.zeros_like(c.g))
    gd, zd = gsel.double(), c.zsel.double()
    s, sz = gd.sum(0), (gd * zd).sum(0)
    n = (c.B + 15) // 16 + 15
    E_s = n * U * gd.abs().sum(0)
    E_sz = (n + 1) * U * (gd * zd).abs().sum(0)
    out = {"gsel": (gsel, None), "stats": (torch.stack([s, sz]), torch.stack([E_s, E_sz]))}
    if rows is not None or fixed:
        mean, inv = c.coef[2].double(), c.coef[3].double()
        dg = inv * (sz - mean * s)
        E_dg = inv * (E_sz + mean.abs() * E_s + 4 * D * (sz.abs() + (mean * s).abs()))
        out.update(bn_backward_ref(c.coef, dg, E_dg, s, E_s, rows, fixed))
    return out


# ---- a layer's backward, R <= 32 -----------------------------------------------------------------------------------------------------
def layer_backward_case(shape, form, dev, seed=0, zprev=None):
    """One layer (Co x Ci) on R rows over a BatchNorm + ReLU layer: dy / z / kcoef (or gsel / argsel per cloud of npts rows), W, zprev,
    coef_prev -- all real-valued.  form: "rows" (prev_bn_rows = 0: the BatchNorm below saw these R rows: its statistics are zprev's),
    "pool" (prev_bn_rows = 64 R: zprev are pooled pre-BN values, statistics drawn), "fixed" (prev_bn_rows = -1).
    Every ReLU argument fmaf(zprev, scale, shift) is kept further from 0 than U (|zprev scale| + |shift|) -- the kernel's single
    rounding cannot change its sign -- by moving the few elements that are not (zprev += 1/8 there), and a dozen are planted where
    the argument is exactly 0 with a non-zero gradient above: channel 4 has scale 0 and shift 0, so `> 0` masks all of it and `>= 0` none."""
    R, Ci, Co, mode, npts = shape
    g = gen(seed * 104729 + R * 1009 + Ci * 31 + Co * 7 + mode * 3 + SMALL_BWD_FORMS.index(form) + 6, dev)
    c = Case(R=R, Ci=Ci, Co=Co, mode=mode, npts=npts, form=form, dy=None, z=None, kcoef=None, gsel=None, argsel=None)
    if mode == 0:
        c.dy = randn(g, R, Co)
    elif mode == 1:
        c.dy, c.z, c.kcoef = randn(g, R, Co), randn(g, R, Co) * 1.5 + 0.5, (randn(g, 3, Co) * torch.tensor([[1.0], [0.1], [0.1]], device=dev)).contiguous()
    else:
        nc = R // npts
        assert nc * npts == R
        c.z, c.kcoef = randn(g, R, Co) * 1.5 + 0.5, (randn(g, 3, Co) * torch.tensor([[1.0], [0.1], [0.1]], device=dev)).contiguous()
        c.gsel = randn(g, nc, Co) * (rand(g, nc, Co) < 0.75).float()
        c.argsel = torch.randint(0, npts, (nc, Co), device=dev, generator=g).int()
    c.W = (randn(g, Co, Ci) * Co ** -0.5).contiguous()
    zp = randn(g, R, Ci) * 1.5 + 0.5 if zprev is None else zprev.clone()
    if form == "rows":
        mean = zp.double().mean(0)
        coef = coef_of(g, Ci, mean, ((zp.double() - mean) ** 2).mean(0))
    else:
        coef = coef_of(g, Ci)
    coef[1, 4] = 0.0
    sc, sh = coef[0].double(), coef[1].double()
    for _ in range(4):  # the nudge: deterministic, a handful of elements
        pre = zp.double() * sc + sh
        near = (pre.abs() <= 4 * U * ((zp.double() * sc).abs() + sh.abs())) & (sc != 0)
        if not bool(near.any()):
            break
        zp = torch.where(near, zp + 0.125, zp)
    c.zprev, c.coef_prev = zp.contiguous(), coef
    assert relu_margin(c) < 0.5, ("the nudge left a ReLU argument within two roundings of 0", shape, form, relu_margin(c))
    assert form != "pool" or R <= 32
    c.prev_bn_rows = {"rows": 0, "pool": 64 * R, "fixed": -1}[form]
    return c


def relu_margin(c):
    """worst U (|zprev scale| + |shift|) / |zprev scale + shift| over the elements with a non-zero scale: below 1 means that the
    kernel's fmaf has the sign of the exact value everywhere (scale 0: the argument is `shift` itself, exact)."""
    sc, sh = c.coef_prev[0].double(), c.coef_prev[1].double()
    pre = c.zprev.double() * sc + sh
    live = (sc != 0).expand_as(pre)
    return float((U * ((c.zprev.double() * sc).abs() + sh.abs()) / pre.abs())[live].max())


def dz_ref(c):
    """dZ (R, Co) fp64 and its bound in the three dz_modes: 0: dy as given; 1: fmaf(k1, dy, fmaf(k2, z, k3)): two roundings;
    2: the same with dy = gsel[b] at row argsel[b] of cloud b and 0 elsewhere."""
    if c.mode == 0:
        return c.dy.double(), torch.zeros_like(c.dy.double())
    k1, k2, k3 = c.kcoef[0].double(), c.kcoef[1].double(), c.kcoef[2].double()
    if c.mode == 1:
        dy = c.dy.double()
    else:
        nc = c.R // c.npts
        dy = torch.zeros(nc, c.npts, c.Co, dtype=torch.float64, device=c.z.device)
        dy.scatter_(1, c.argsel.long()[:, None, :], c.gsel.double()[:, None, :])
        dy = dy.view(c.R, c.Co)
    inner = k2 * c.z.double() + k3
    dz = k1 * dy + inner
    return dz, U * ((k2 * c.z.double()).abs() + k3.abs()) + U * ((k1 * dy).abs() + inner.abs())


STATS_SCHEME = {
    # route -> how the two BatchNorm-backward sums of the layer below are taken (read from the kernels' epilogues)
    "small": ("centred", 16),     # small_dgrad_body: 16 rows per lane in order + one cross-lane add; s1c = sum g (z - mean)
    "rows<=64": ("centred", 32),  # rows_dgrad_body with the coefficients inside the launch: both 32-row halves on the lane, the same
    # every other route: fp32 partials (sum g, sum g z) over at most 64 rows each -- a 64-row block (rows_dgrad_body, TileBig) or a
    # fused workgroup's tiles (R <= 320 here: at most two 32-row or one 64-row tile) -- then partial_sums and bn_backward_coefs in double
    "rows>64": ("partials", 64), "fused": ("partials", 64), "fast": ("partials", 64), "fallback": ("partials", 64),
}


def layer_backward_ref(c, route="small", nsplit=0):
    """dYprev = mask (dZ W), a GEMM of Co terms; dW = dZ^T act(zprev), a GEMM of R terms on the activation rounded once (split over
    nsplit partials added in fp32: nsplit more); db = its ones column, or column sums of dy.  The BatchNorm backward of the layer below
    from fp32 sums over the rows (STATS_SCHEME): centred, dgamma = invstd s1c; or partials, dgamma = invstd (sz - mean s) in double
    from the fp32 partial sums -- the bound then carries the conditioning of that difference: invstd (E_sz + |mean| E_s).
    -> dict name -> (value, bound)"""
    dz, E_dz = dz_ref(c)
    W, zp = c.W.double(), c.zprev.double()
    sc, sh, mean, inv = (c.coef_prev[i].double() for i in range(4))
    pre = zp * sc + sh
    live = (pre > 0).double()
    dv = dz @ W
    E_dv = (c.Co + 8) * U * (dz.abs() @ W.abs()) + E_dz @ W.abs()
    gv, E_gv = dv * live, E_dv * live
    a = pre.clamp_min(0)
    mag = dz.abs().t() @ a
    out = {"dyprev": (gv, E_gv),
           "dW": (dz.t() @ a, (c.R + 8 + nsplit) * U * mag + E_dz.t() @ a + dz.abs().t() @ (U * a)),
           "db": (dz.sum(0), (c.R + 8 + nsplit) * U * dz.abs().sum(0) + E_dz.sum(0))}
    scheme, n = STATS_SCHEME[route]
    s0 = gv.sum(0)
    E_s0 = n * U * gv.abs().sum(0) + E_gv.sum(0)
    if scheme == "centred":
        zm = zp - mean
        t1 = gv * zm
        dg = inv * t1.sum(0)
        E_dg = inv * ((n + 2) * U * t1.abs().sum(0) + (E_gv * zm.abs()).sum(0))      # the difference and the product: one U each
        E_dbeta = E_s0                                                                # (float)(double)s0: exact
    else:
        t1 = gv * zp
        s1 = t1.sum(0)
        E_s1 = (n + 1) * U * t1.abs().sum(0) + (E_gv * zp.abs()).sum(0)                # the product: one U
        dg = inv * (s1 - mean * s0)
        E_dg = inv * (E_s1 + mean.abs() * E_s0 + 4 * D * (s1.abs() + (mean * s0).abs()))
        E_dbeta = E_s0 + U * s0.abs()                                                 # a double sum of partials, stored as fp32
    rows = {"rows": c.R, "pool": c.prev_bn_rows, "fixed": None}[c.form]
    bn = bn_backward_ref(c.coef_prev, dg, E_dg, s0, E_s0, rows, fixed=c.form == "fixed")
    bn["dbeta"] = (s0, E_dbeta)
    out.update({"prev_" + k: v for k, v in bn.items()})
    return out


def linear_dgrad_ref(c):
    """sn_linear_dgrad alone: dYprev as above and the BatchNorm-backward partials [blocks][2][Ci] summed over the blocks (fp32 sums of
    at most 64 rows each; the test adds the blocks in double) -> dict name -> (value, bound)"""
    full = layer_backward_ref(c, "fallback")
    gv, E_gv = full["dyprev"]
    zp = c.zprev.double()
    t1 = gv * zp
    return {"dyprev": (gv, E_gv),
            "stats": (torch.stack([gv.sum(0), t1.sum(0)]),
                      torch.stack([64 * U * gv.abs().sum(0) + E_gv.sum(0), 65 * U * t1.abs().sum(0) + (E_gv * zp.abs()).sum(0)]))}


# ---- sn_layer_backward_in3 -----------------------------------------------------------------------------------------------------------
def in3_case(R, dev, seed=0):
    """The 64 -> 64 layer on top of the xyz layer: x (R, 3), W_in (64, 3), b_in, zprev = x W_in^T + b_in rounded to fp32 (then nudged
    as layer_backward_case does: the kernel takes mask and sums from the zprev it is given and dW_in from the cloud), DZ_BN above."""
    g = gen(seed * 31 + R + 8, dev)
    x = (rand(g, R, 3) - 0.5).contiguous()
    W_in, b_in = randn(g, 64, 3).contiguous(), randn(g, 64) * 0.2
    c = layer_backward_case((R, 64, 64, 1, 0), "rows", dev, seed=seed + 5, zprev=(x.double() @ W_in.double().t() + b_in.double()).float())
    c.x, c.W_in, c.b_in = x, W_in, b_in
    return c


def in3_ref(c, nsplit):
    """sn_layer_backward_in3: dW and the BatchNorm backward of the xyz layer as the fused route gives them (no dYprev), and
        dW_in[c][d] = k1 Gx[c][d] + k2 (sum_e W_in[c][e] Sxx[e][d] + b_in[c] Sx[d]) + k3 Sx[d]
    -- its closed form, evaluated by the kernel in double from fp32 partials over at most 64 rows: Gx = sum_r dYprev x (the product
    and 63 additions: 64 U, on top of dYprev's own bound), Sx = sum_r x (63 U), Sxx = sum_r x x^T (64 U), and the fp32 k1, k2, k3."""
    full = layer_backward_ref(c, "fused", nsplit)
    gv, E_gv = full.pop("dyprev")
    full.pop("db")
    x, Wi, bi = c.x.double(), c.W_in.double(), c.b_in.double()
    Gx, E_Gx = gv.t() @ x, 64 * U * (gv.abs().t() @ x.abs()) + E_gv.t() @ x.abs()
    Sx, E_Sx = x.sum(0), 63 * U * x.abs().sum(0)
    Sxx, E_Sxx = x.t() @ x, 64 * U * (x.abs().t() @ x.abs())
    zx = Wi @ Sxx + bi[:, None] * Sx
    E_zx = Wi.abs() @ E_Sxx + bi.abs()[:, None] * E_Sx
    k, E_k = full["prev_kcoef"]
    terms = (k[0][:, None] * Gx, k[1][:, None] * zx, k[2][:, None] * Sx)
    val = terms[0] + terms[1] + terms[2]
    E = k[0].abs()[:, None] * E_Gx + E_k[1][:, None] * zx.abs() + k[1].abs()[:, None] * E_zx + E_k[2][:, None] * Sx.abs() + \
        k[2].abs()[:, None] * E_Sx + 8 * D * sum(t.abs() for t in terms) + U * val.abs()   # the three terms in double; stored as fp32
    full["dW_in"] = (val, E)
    return full


# ---- sn_conv_stack_forward_bn, teacher-forced ----------------------------------------------------------------------------------------
def conv_stack_case(B, N, ch, dev, seed=0):
    """A cloud and the stack's parameters; gammas of both signs on the last layer (those channels pool their minima) and one zero"""
    g = gen(seed * 31 + B * 1031 + N + len(ch) + 9, dev)
    c = Case(B=B, N=N, R=B * N, ch=tuple(ch), n=len(ch) - 1, x=(rand(g, B, N, 3) - 0.5).contiguous(), W=[], bias=[], gamma=[], beta=[], rm=[], rv=[])
    for ci, co in zip(ch[:-1], ch[1:]):
        c.W.append((randn(g, co, ci) * ci ** -0.5).contiguous()), c.bias.append(randn(g, co) * 0.1)
        c.gamma.append(randn(g, co).abs() + 0.5), c.beta.append(randn(g, co) * 0.1)
        c.rm.append(randn(g, co) * 0.1), c.rv.append(rand(g, co) + 0.5)
    c.gamma[-1][::5] *= -1.0
    c.gamma[-1][3] = 0.0
    return c


def conv_stack_layer(c, l, zprev, coefprev):
    """the Case layer_z_ref / layer_stats_ref take for layer l, fed with the GPU's own z[l - 1] / coef[l - 1] (layer 0: the cloud)"""
    return Case(R=c.R, Ci=c.ch[l], Co=c.ch[l + 1], C=c.ch[l + 1], ain=c.x.view(c.R, 3) if l == 0 else zprev, coef_prev=None if l == 0 else coefprev,
                W=c.W[l], bias=c.bias[l], gamma=c.gamma[l], beta=c.beta[l], rm=c.rm[l], rv=c.rv[l])


def conv_fx_stats_ref(z, lc):
    """Coefficients and running statistics of one stack layer from fp64 statistics of the GPU's own z (R, C).  The producer adds fp32
    sums of z and z z over ONE 64-row tile each into 64-bit fixed point -- at the table's sizes: the xyz pass takes one block per
    workgroup and the persistent kernels, which walk several tiles, start at four tiles per workgroup on every compute unit -- where
    one unit is 2^-kFxShiftFwd = 2^-32, each contribution is rounded to nearest (__double2ll_rn: 2^-33) and the integer additions are
    exact; mean = s / R and var = ss / R - mean^2 in double.  So: 63 U on the sum of magnitudes (64 U with the product z z), and R / 64
    contributions: q = (R / 64) 2^-33 / R on mean and on ss / R.  The difference carries its conditioning: E_var = E_ms + 2 |mean| E_mean."""
    R = z.shape[0]
    zd = z.double()
    mean, ms = zd.mean(0), (zd * zd).mean(0)
    var = (ms - mean * mean).clamp_min(0)
    q = (R / 64.0) * 2.0 ** -33 / R
    E_mean = 63 * U * zd.abs().mean(0) + q
    E_var = 64 * U * ms + q + 2 * mean.abs() * E_mean
    return bn_coef_ref(mean, var, E_mean, E_var, lc.gamma, lc.beta, EPS, MOMENTUM, lc.rm, lc.rv, R)


# ---- launch drivers --------------------------------------------------------------------------------------------------------------
def _lib():
    from samplenet_amd import _lib as L

    return L


class MlpLaunch(Launch):
    def filled(self, t):
        """every element of an output was written (none still holds the sentinel's NaN pattern)"""
        return not bool((t.view(torch.int32) == SENTINEL).any())

    def counter(self, start):
        """num_batches_tracked and one more 64-bit word, which stays 0"""
        gb = Guarded(4, torch.int64, zero=True)
        self.outs.append(gb)
        gb.view[0] = start
        return gb.view


def _running(call, c, running):
    """running: "both" | "none" (both NULL) | "var only" (running_mean NULL, running_var given: both stay untouched)"""
    call.rm, call.rv = call.add((c.C,)), call.add((c.C,))
    call.rm.copy_(c.rm), call.rv.copy_(c.rv)
    call.nbt = call.counter(7)
    return {"both": (call.rm, call.rv), "none": (None, None), "var only": (None, call.rv)}[running]


def launch_finalize(c, running="both"):
    """-> MlpLaunch with .coef (4, C), .rm, .rv (copies of the case's, updated in place), .nbt"""
    L = _lib()
    call = MlpLaunch(("bn_finalize", c.nblk, c.C, c.R, running))
    call.coef = call.add((4, c.C))
    rm, rv = _running(call, c, running)
    p = L.ptr
    L.check(L.lib.sn_bn_finalize(c.nblk, c.C, c.R, p(c.stats), p(c.gamma), p(c.beta), EPS, MOMENTUM, p(rm), p(rv), p(call.nbt), p(call.coef),
                                 L.stream_of(c.stats)), str(call.what))
    return call


def launch_twopass(c, running="both", output=False):
    """sn_bn_batch_stats_twopass, or sn_bn_output_forward(training = 1) with .y (R, C) when `output`"""
    L = _lib()
    call = MlpLaunch(("bn_output_forward" if output else "bn_batch_stats_twopass", c.R, c.C, running))
    call.coef = call.add((4, c.C))
    rm, rv = _running(call, c, running)
    p = L.ptr
    if output:
        call.y = call.add((c.R, c.C))
        rc = L.lib.sn_bn_output_forward(c.R, c.C, 1, p(c.z), p(c.gamma), p(c.beta), EPS, MOMENTUM, p(rm), p(rv), p(call.nbt), p(call.coef),
                                        p(call.y), L.stream_of(c.z))
    else:
        rc = L.lib.sn_bn_batch_stats_twopass(c.R, c.C, p(c.z), p(c.gamma), p(c.beta), EPS, MOMENTUM, p(rm), p(rv), p(call.nbt), p(call.coef),
                                             L.stream_of(c.z))
    L.check(rc, str(call.what))
    return call


def launch_eval_coef(c):
    L = _lib()
    call = MlpLaunch(("bn_eval_coef", c.C))
    call.coef = call.add((4, c.C))
    p = L.ptr
    L.check(L.lib.sn_bn_eval_coef(c.C, p(c.gamma), p(c.beta), EPS, p(c.rm), p(c.rv), p(call.coef), L.stream_of(c.rm)), str(call.what))
    return call


def _bn_outs(call, C, with_dbias=True):
    o = call.out
    o["dgamma"], o["dbeta"], o["kcoef"] = call.add((C,)), call.add((C,)), call.add((3, C))
    if with_dbias:
        o["dbias"] = call.add((C,))


def launch_backward_coef(c, with_dbias=True):
    L = _lib()
    call = MlpLaunch(("bn_backward_coef", c.recipe, c.nblk, c.C, c.R, with_dbias))
    call.out = {}
    _bn_outs(call, c.C, with_dbias)
    o, p = call.out, L.ptr
    L.check(L.lib.sn_bn_backward_coef(c.nblk, c.C, c.R, p(c.stats), p(c.coef), p(o["dgamma"]), p(o["dbeta"]), p(o.get("dbias")), p(o["kcoef"]),
                                      L.stream_of(c.stats)), str(call.what))
    return call


def launch_pool_forward(c):
    L = _lib()
    call = MlpLaunch(("pool_forward", c.B, c.N, c.C))
    call.pooled, call.zsel = call.add((c.B, c.C)), call.add((c.B, c.C))
    ag = Guarded(c.B * c.C, torch.int32)
    call.outs.append(ag)
    call.argsel = ag.view.view(c.B, c.C)
    p = L.ptr
    L.check(L.lib.sn_pool_forward(c.B, c.N, c.C, p(c.z), p(c.coef), p(call.pooled), p(call.argsel), p(call.zsel), L.stream_of(c.z)), str(call.what))
    return call


def launch_pool_backward(c, way, with_dbias=True):
    """way: "alone" (sn_pool_backward: gsel + stats (2, C)), "bn" (sn_pool_backward_bn, R = B * POOL_BWD_N), "fixed" (R = -1)"""
    L = _lib()
    call = MlpLaunch(("pool_backward", way, c.recipe, c.B, c.C, with_dbias))
    o = call.out = {"gsel": call.add((c.B, c.C))}
    p = L.ptr
    if way == "alone":
        o["stats"] = call.add((2, c.C))
        rc = L.lib.sn_pool_backward(c.B, c.C, p(c.g), p(c.pooled), p(c.zsel), p(o["gsel"]), p(o["stats"]), L.stream_of(c.g))
    else:
        _bn_outs(call, c.C, with_dbias)
        rc = L.lib.sn_pool_backward_bn(c.B, c.C, c.B * POOL_BWD_N if way == "bn" else -1, p(c.g), p(c.pooled), p(c.zsel), p(o["gsel"]), p(c.coef),
                                       p(o["dgamma"]), p(o["dbeta"]), p(o.get("dbias")), p(o["kcoef"]), L.stream_of(c.g))
    L.check(rc, str(call.what))
    return call


def launch_layer_backward(c, want_db=True, want_dbias=True):
    """sn_layer_backward.  R <= 32: no stats, no part (the route needs neither: both NULL); above: stats of sn_linear_stats_blocks(R)
    x 2 x Ci floats and part of sn_linear_wgrad_splits(R, Ci, Co, db != NULL) x Co x (Ci + (db != NULL)) floats, both guarded.
    -> MlpLaunch with .out, .nsplit"""
    L = _lib()
    call = MlpLaunch(("layer_backward", c.R, c.Ci, c.Co, c.mode, c.npts, c.form, want_db, want_dbias))
    o = call.out = {"dyprev": call.add((c.R, c.Ci)), "dW": call.add((c.Co, c.Ci))}
    if want_db:
        o["db"] = call.add((c.Co,))
    o["prev_dgamma"], o["prev_dbeta"], o["prev_kcoef"] = call.add((c.Ci,)), call.add((c.Ci,)), call.add((3, c.Ci))
    if want_dbias:
        o["prev_dbias"] = call.add((c.Ci,))
    stats = part = None
    call.nsplit = 0
    if c.R > 32:
        call.nsplit = L.lib.sn_linear_wgrad_splits(c.R, c.Ci, c.Co, int(want_db))
        stats = call.add((L.lib.sn_linear_stats_blocks(c.R), 2, c.Ci))
        part = call.add((call.nsplit, c.Co, c.Ci + int(want_db)))
    p = L.ptr
    L.check(L.lib.sn_layer_backward(c.R, c.Ci, c.Co, c.mode, p(c.dy), p(c.z), p(c.kcoef), p(c.gsel), p(c.argsel), c.npts, p(c.W), p(c.zprev),
                                    p(c.coef_prev), p(o["dyprev"]), p(stats), p(part), p(o["dW"]), p(o.get("db")), p(o["prev_dgamma"]),
                                    p(o["prev_dbeta"]), p(o.get("prev_dbias")), p(o["prev_kcoef"]), c.prev_bn_rows, L.stream_of(c.W)),
            str(call.what))
    return call


def launch_linear_dgrad(c):
    """sn_linear_dgrad alone -> MlpLaunch with .out {dyprev, stats (blocks, 2, Ci)}"""
    L = _lib()
    call = MlpLaunch(("linear_dgrad", c.R, c.Ci, c.Co, c.mode, c.npts))
    nblk = L.lib.sn_linear_stats_blocks(c.R)
    call.out = {"dyprev": call.add((c.R, c.Ci)), "stats": call.add((nblk, 2, c.Ci))}
    p = L.ptr
    L.check(L.lib.sn_linear_dgrad(c.R, c.Ci, c.Co, c.mode, p(c.dy), p(c.z), p(c.kcoef), p(c.gsel), p(c.argsel), c.npts, p(c.W), p(c.zprev),
                                  p(c.coef_prev), p(call.out["dyprev"]), p(call.out["stats"]), L.stream_of(c.W)), str(call.what))
    return call


def launch_linear_wgrad(c, want_db=True):
    """sn_linear_wgrad alone -> MlpLaunch with .out {dW, db}, .nsplit"""
    L = _lib()
    call = MlpLaunch(("linear_wgrad", c.R, c.Ci, c.Co, c.mode, c.npts, want_db))
    call.nsplit = L.lib.sn_linear_wgrad_splits(c.R, c.Ci, c.Co, int(want_db))
    part = call.add((call.nsplit, c.Co, c.Ci + int(want_db)))
    call.out = {"dW": call.add((c.Co, c.Ci))}
    if want_db:
        call.out["db"] = call.add((c.Co,))
    p = L.ptr
    L.check(L.lib.sn_linear_wgrad(c.R, c.Ci, c.Co, c.mode, p(c.dy), p(c.z), p(c.kcoef), p(c.gsel), p(c.argsel), c.npts, p(c.zprev), p(c.coef_prev),
                                  p(part), p(call.out["dW"]), p(call.out.get("db")), L.stream_of(c.W)), str(call.what))
    return call


def launch_layer_forward(c, running=True, npts=0):
    """sn_layer_forward_bn, or (npts > 0) sn_conv_forward_bn_pool with .pooled / .zsel / .argsel (B, Co).  stats (and pool_val / pool_idx):
    sn_linear_stats_blocks(R) x 2 x Co, guarded.  -> MlpLaunch with .z (R, Co), .coef (4, Co), .rm, .rv, .nbt"""
    L = _lib()
    call = MlpLaunch(("conv_forward_bn_pool" if npts else "layer_forward_bn", c.R, c.Ci, c.Co, c.coef_prev is not None, running, npts))
    call.z, call.coef = call.add((c.R, c.Co)), call.add((4, c.Co))
    nblk = L.lib.sn_linear_stats_blocks(c.R)
    stats = call.add((nblk, 2, c.Co))
    rm, rv = _running(call, c, "both" if running else "none")
    p = L.ptr
    head = (p(c.ain), p(c.coef_prev), p(c.W), p(c.bias), p(call.z), p(stats), p(c.gamma), p(c.beta), EPS, MOMENTUM, p(rm), p(rv), p(call.nbt), p(call.coef))
    if npts:
        B = c.R // npts
        pool_val = call.add((nblk, 2, c.Co))
        pi = Guarded(nblk * 2 * c.Co, torch.int32)
        call.outs.append(pi)
        call.pooled, call.zsel = call.add((B, c.Co)), call.add((B, c.Co))
        ag = Guarded(B * c.Co, torch.int32)
        call.outs.append(ag)
        call.argsel = ag.view.view(B, c.Co)
        rc = L.lib.sn_conv_forward_bn_pool(c.R, c.Ci, c.Co, npts, *head, p(pool_val), p(pi.view), p(call.pooled), p(call.argsel), p(call.zsel),
                                           L.stream_of(c.ain))
    else:
        rc = L.lib.sn_layer_forward_bn(c.R, c.Ci, c.Co, *head, L.stream_of(c.ain))
    L.check(rc, str(call.what))
    return call


def launch_layer_backward_in3(c, want_dbias=True):
    """sn_layer_backward_in3 -> MlpLaunch with .out {dW, prev_*, dW_in}, .nsplit"""
    L = _lib()
    call = MlpLaunch(("layer_backward_in3", c.R, c.Ci, c.Co, want_dbias))
    nf = L.lib.sn_layer_backward_in3_stats_floats(c.R, c.Ci, c.Co)
    call.nsplit = L.lib.sn_linear_wgrad_splits(c.R, c.Ci, c.Co, 0)
    stats, part = call.add((max(nf, 1),)), call.add((call.nsplit, c.Co, c.Ci))
    o = call.out = {"dW": call.add((c.Co, c.Ci)), "prev_dgamma": call.add((c.Ci,)), "prev_dbeta": call.add((c.Ci,)), "prev_kcoef": call.add((3, c.Ci)),
                    "dW_in": call.add((c.Ci, 3))}
    if want_dbias:
        o["prev_dbias"] = call.add((c.Ci,))
    p = L.ptr
    L.check(L.lib.sn_layer_backward_in3(c.R, c.Ci, c.Co, p(c.dy), p(c.z), p(c.kcoef), p(c.W), p(c.zprev), p(c.coef_prev), p(stats), p(part), p(o["dW"]),
                                        p(o["prev_dgamma"]), p(o["prev_dbeta"]), p(o.get("prev_dbias")), p(o["prev_kcoef"]), p(c.x), p(c.W_in), p(c.b_in),
                                        p(o["dW_in"]), L.stream_of(c.W)), str(call.what))
    return call


def launch_conv_stack(c, with_z0=True):
    """sn_conv_stack_forward_bn with its own pool.  -> MlpLaunch with .z[l] (R, C) (z[0] None without it), .coef[l], .rm / .rv / .nbt per
    layer, .pooled / .zsel / .argsel (B, Cn), .acc (the whole scratch, zeroed before), .nsum (its statistics part)"""
    import ctypes

    L = _lib()
    n, R, Cn = c.n, c.R, c.ch[-1]
    chans = (ctypes.c_int * (n + 1))(*c.ch)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    call = MlpLaunch(("conv_stack_forward_bn", c.B, c.N, c.ch, with_z0))
    acc = Guarded(2 * L.lib.sn_conv_stack_acc_elems(n), torch.int64, zero=True)
    call.outs.append(acc)
    call.acc, call.nsum = acc.view, L.lib.sn_conv_stack_acc_sum_elems(n, ctypes.cast(chans, ctypes.c_void_p))
    call.z = [call.add((R, co)) if (l or with_z0) else None for l, co in enumerate(c.ch[1:])]
    call.coef = [call.add((4, co)) for co in c.ch[1:]]
    call.rm, call.rv, call.nbt = [], [], []
    for l, co in enumerate(c.ch[1:]):
        rm, rv = call.add((co,)), call.add((co,))
        rm.copy_(c.rm[l]), rv.copy_(c.rv[l])
        call.rm.append(rm), call.rv.append(rv), call.nbt.append(call.counter(7))
    nblk = R // 64
    pool_val = call.add((max(nblk, 2 * c.B), 2, Cn))
    pi = Guarded(nblk * 2 * Cn, torch.int32)
    call.outs.append(pi)
    call.pooled, call.zsel = call.add((c.B, Cn)), call.add((c.B, Cn))
    ag = Guarded(c.B * Cn, torch.int32)
    call.outs.append(ag)
    call.argsel = ag.view.view(c.B, Cn)
    eps, mom = (ctypes.c_float * n)(*[EPS] * n), (ctypes.c_float * n)(*[MOMENTUM] * n)
    p = L.ptr
    L.check(L.lib.sn_conv_stack_forward_bn(c.B, c.N, n, chans, p(c.x), arr(c.W), arr(c.bias), arr(c.gamma), arr(c.beta), arr(call.rm), arr(call.rv),
                                           arr(call.nbt), eps, mom, arr(call.z), arr(call.coef), p(call.acc), p(pool_val), p(pi.view), p(call.pooled),
                                           p(call.argsel), p(call.zsel), L.stream_of(c.x)), str(call.what))
    return call

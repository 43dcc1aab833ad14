// set_abstraction.hip -- what a PointNet++ set-abstraction level needs around the GEMM walk (gfx950): the grouped points in the ROW
// layout the GEMM entries read, the deterministic gradient of that gather by inverted index, and a max-pool pair sized for tens of
// thousands of tiny groups.  Replaces, on that layout, query_ball_point_gpu + group_point_gpu + group_point_grad_gpu
// (classification/grouping/tf_grouping_g.cu:3-36, 40-57, 61-78) and the centre subtraction between them.  The contracts are written
// out in include/samplenet_hip_internal.h; tests/group_rows_ref.py restates them in numpy.
//
// sn_ball_group_rows_forward   rows (b, m, nsample, Ci), Ci = 3 use_xyz + c, channels contiguous.  The scan is ball_query.hip's
//     (ball_scan.h): a wave owns a query, one query per wave up to 8192 queries.  A grouped row is one contiguous run of Ci floats
//     copied from one contiguous feature row, so the wave walks the group's nsample * Ci output floats FLAT over its lanes: stores
//     are fully coalesced, loads are runs of Ci floats; four rounds (256 floats) are loaded before the first is stored.
// sn_group_rows_backward       grad_features / grad_xyz: a group of LG lanes (the power of two covering the columns, 64 at most)
//     owns a destination row and LG of its columns and takes inverse_walk.h's unweighted sum over the row's list: the terms are
//     grad_rows[e, col], every read of an entry one contiguous segment.  Point 0 collects every empty ball, so its list is the
//     launch's longest.  grad_new_xyz: sn_ball_group_backward's order (lane l adds slots l, l + 64, .. ascending, xor tree 32 .. 1,
//     one negation) on the row layout.
// sn_group_pool_forward        a wave per (group, 64 channels), four of them per workgroup, rows ascending with four loads in
//     flight: the first row wins a tie because a later row replaces the pick only when strictly greater (smaller).
// sn_group_pool_backward       gsel = g * [pooled > 0] and the BatchNorm-backward partial sums as blocks of kGpGroups groups, each
//     summed in one fixed order: the layout sn_bn_backward_coef reduces.
// No LDS but the pool backward's 2 KB, no workspace, no atomics: deterministic, safe under stream capture.
#include "ball_scan.h"
#include "inverse_walk.h"

#pragma clang fp contract(off)  // every sum below is add after add, every product rounded (the pool's one fmaf is written out)

namespace sn {
namespace {

__device__ __forceinline__ float relu_np(float u) { return u < 0.f ? 0.f : u; }  // (mlp_device.h's: a NaN stays a NaN)

// ------------------------------------------------------------------------------------------------ grouping, row layout
constexpr int kRowsFlight = 4;  // rounds of 64 output floats a wave loads before the first store

struct RowsArgs {
    int n, m, nsample, groups, qpw;   // groups: workgroups per cloud; qpw: queries per wave
    float thr;
    const float *xyz;                 // (b,n,3)
    const float *new_xyz;             // (b,m,3)
    const float *features;            // (b,n,c) row-major, NULL with c == 0
    int c, u3;                        // u3 = 3 use_xyz
    int *idx;
    int *pts_cnt;                     // optional
    float *rows;                      // (b, m, nsample, u3 + c)
};

template <int RULE>
__global__ void __launch_bounds__(kBallWaves *kWave) ball_group_rows_kernel(const RowsArgs a)
{
    const int cloud = blockIdx.x / a.groups, group = blockIdx.x - cloud * a.groups;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    const float *P = a.xyz + (size_t)cloud * a.n * 3;
    const float *Q = a.new_xyz + (size_t)cloud * a.m * 3;
    const float *F = a.features + (size_t)cloud * a.n * a.c;
    const int Ci = a.u3 + a.c;
    const long long total = (long long)a.nsample * Ci;      // floats of one group
    const int d64 = kWave / Ci, r64 = kWave - d64 * Ci;     // a step of 64 floats is d64 rows and r64 columns
    const int j0 = (group * kBallWaves + wave) * a.qpw;
    for (int q = 0; q < a.qpw; ++q) {
        const int j = j0 + q;
        if (j >= a.m) return;
        const float qx = Q[(size_t)j * 3], qy = Q[(size_t)j * 3 + 1], qz = Q[(size_t)j * 3 + 2];
        int *row = a.idx + ((size_t)cloud * a.m + j) * a.nsample;
        const int hits = ball_scan_row<RULE>(a.n, a.nsample, a.thr, P, SN_LAYOUT_BNC, qx, qy, qz, lane, row);
        if (a.pts_cnt && lane == 0) a.pts_cnt[(size_t)cloud * a.m + j] = hits;
        // the wave reads back the row its own lanes have just stored: workgroup-scope release / acquire orders the stores of
        // every lane before the loads of every lane (one CU, one L1)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        float *o = a.rows + ((size_t)cloud * a.m + j) * (size_t)total;
        int s = lane / Ci, col = lane - s * Ci;               // (slot, column) of this lane's float in the current round
        for (long long base = 0; base < total; base += kRowsFlight * kWave) {
            float v[kRowsFlight];
#pragma unroll
            for (int i = 0; i < kRowsFlight; ++i) {
                v[i] = 0.f;
                if (base + i * kWave + lane < total) {
                    const int k = row[s];
                    if (col < a.u3)
                        v[i] = P[(size_t)k * 3 + col] - (col == 0 ? qx : (col == 1 ? qy : qz));   // one fp32 subtraction
                    else
                        v[i] = F[(size_t)k * a.c + (col - a.u3)];
                }
                s += d64, col += r64;
                if (col >= Ci) col -= Ci, ++s;
            }
#pragma unroll
            for (int i = 0; i < kRowsFlight; ++i) {
                const long long e = base + i * kWave + lane;
                if (e < total) o[e] = v[i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ its gradient
constexpr int kGrThreads = kLaneThreads;

struct GradRowsArgs {
    int n, ne, Ci, c, u3;
    int col0, ncols;          // the columns of grad_rows this launch sums: [col0, col0 + ncols)
    int lg, chunks;           // lanes per destination row (a power of two <= 64), column chunks of lg per row
    long long items;          // b * n * chunks (row, chunk) pairs
    const int *start;         // (b, n+1)
    const int *order;         // (b, ne)
    const float *grad_rows;   // (b, ne, Ci)
    float *grad_features;     // (b,n,c), optional
    float *grad_xyz;          // (b,n,3), optional
};

__global__ void __launch_bounds__(kGrThreads) group_rows_backward_kernel(const GradRowsArgs a)
{
    const int per = kGrThreads / a.lg;                      // (row, chunk) pairs per workgroup
    const int sub = threadIdx.x / a.lg, l = threadIdx.x - sub * a.lg;
    const long long item = (long long)blockIdx.x * per + sub;
    if (item >= a.items) return;
    const long long rowi = item / a.chunks;                 // cloud * n + r
    const int chunk = (int)(item - rowi * a.chunks);
    const int cloud = (int)(rowi / a.n);
    const int cl = chunk * a.lg + l;
    if (cl >= a.ncols) return;
    const int col = a.col0 + cl;
    const int *start = a.start + rowi + cloud;               // cloud * (n + 1) + r
    const int *order = a.order + (size_t)cloud * a.ne;
    const float *g = a.grad_rows + (size_t)cloud * a.ne * a.Ci + col;
    const float acc = inverse_walk_sum<1, false>(start, order, a.ne, g, a.Ci, nullptr);
    if (col < a.u3)
        a.grad_xyz[rowi * 3 + col] = acc;
    else
        a.grad_features[rowi * a.c + (col - a.u3)] = acc;
}

struct GradCentreArgs {
    int m, nsample, Ci, groups, qpw;
    const float *grad_rows;
    float *grad_new_xyz;
};

// ball_group_backward_kernel's sum of the centre's gradient, reading the three coordinate columns of the row layout
__global__ void __launch_bounds__(kBallWaves *kWave) group_rows_centre_kernel(const GradCentreArgs a)
{
    const int cloud = blockIdx.x / a.groups, group = blockIdx.x - cloud * a.groups;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    const int j0 = (group * kBallWaves + wave) * a.qpw;
    for (int q = 0; q < a.qpw; ++q) {
        const int j = j0 + q;
        if (j >= a.m) return;
        const float *g = a.grad_rows + ((size_t)cloud * a.m + j) * a.nsample * a.Ci;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int s = lane; s < a.nsample; s += kWave) {
            const float *p = g + (size_t)s * a.Ci;
            sx += p[0], sy += p[1], sz += p[2];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o), sy += __shfl_xor(sy, o), sz += __shfl_xor(sz, o);
        if (lane == 0) {
            float *d = a.grad_new_xyz + ((size_t)cloud * a.m + j) * 3;
            d[0] = -sx, d[1] = -sy, d[2] = -sz;
        }
    }
}

// ------------------------------------------------------------------------------------------------ max-pool over small groups
constexpr int kGpWaves = 4;     // (group, 64 channels) pairs per workgroup
constexpr int kGpGroups = 64;   // groups per block of the backward's partial sums

__global__ void __launch_bounds__(kGpWaves *kWave) group_pool_fwd_kernel(long long items, int cblocks, int S, int C, const float *__restrict__ z,
                                                                         const float *__restrict__ coef, float *__restrict__ pooled,
                                                                         int *__restrict__ argsel, float *__restrict__ zsel)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    const long long item = (long long)blockIdx.x * kGpWaves + wave;   // channel block fastest: a workgroup reads whole rows at C <= 256
    if (item >= items) return;
    const long long grp = item / cblocks;
    const int c = (int)(item - grp * cblocks) * kWave + lane;
    if (c >= C) return;
    const float *zb = z + (size_t)grp * S * C + c;
    float vmax = -INFINITY, vmin = INFINITY;
    int imax = 0, imin = 0;
    int r = 0;
    for (; r + 4 <= S; r += 4) {   // four rows' loads in flight; the comparisons keep the rows' order
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = zb[(size_t)(r + i) * C];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (v[i] > vmax) vmax = v[i], imax = r + i;
            if (v[i] < vmin) vmin = v[i], imin = r + i;
        }
    }
    for (; r < S; ++r) {
        const float v = zb[(size_t)r * C];
        if (v > vmax) vmax = v, imax = r;
        if (v < vmin) vmin = v, imin = r;
    }
    const float sc = coef[c], sh = coef[C + c];
    const bool up = sc >= 0.f;
    const float zs = up ? vmax : vmin;
    const size_t o = (size_t)grp * C + c;
    pooled[o] = relu_np(fmaf(zs, sc, sh));   // pool_fwd_kernel's expression
    argsel[o] = up ? imax : imin;
    zsel[o] = zs;
}

// 64 channels x 4 slices per workgroup, one block of kGpGroups groups: slice q adds the block's groups q, q + 4, .. ascending, the
// four slice sums are then added in slice order
__global__ void __launch_bounds__(kGpWaves *kWave) group_pool_bwd_kernel(int G, int C, const float *__restrict__ g, const float *__restrict__ pooled,
                                                                         const float *__restrict__ zsel, float *__restrict__ gsel,
                                                                         float *__restrict__ stats)
{
    __shared__ float red[2][kGpWaves][kWave];
    const int cl = threadIdx.x & (kWave - 1), sl = threadIdx.x >> 6;
    const int c = blockIdx.y * kWave + cl;
    const int g0 = blockIdx.x * kGpGroups, g1 = min(G, g0 + kGpGroups);
    float s = 0.f, sz = 0.f;
    if (c < C) {
        int b = g0 + sl;
        for (; b + 3 * kGpWaves < g1; b += 4 * kGpWaves) {   // four trips' loads in flight; the sums keep their ascending order
            float pv[4], gv[4], zv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t o = (size_t)(b + kGpWaves * i) * C + c;
                pv[i] = pooled[o], gv[i] = g[o], zv[i] = zsel[o];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = pv[i] > 0.f ? gv[i] : 0.f;
                gsel[(size_t)(b + kGpWaves * i) * C + c] = v;
                s += v;
                sz += v * zv[i];
            }
        }
        for (; b < g1; b += kGpWaves) {
            const size_t o = (size_t)b * C + c;
            const float v = pooled[o] > 0.f ? g[o] : 0.f;
            gsel[o] = v;
            s += v;
            sz += v * zsel[o];
        }
    }
    if (!stats) return;   // (uniform)
    red[0][sl][cl] = s, red[1][sl][cl] = sz;
    __syncthreads();
    if (sl == 0 && c < C) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int q = 0; q < kGpWaves; ++q) a0 += red[0][q][cl], a1 += red[1][q][cl];
        float *st = stats + (size_t)blockIdx.x * 2 * C;
        st[c] = a0, st[C + c] = a1;
    }
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_ball_group_rows_forward(int b, int n, int m, int c, float radius, int nsample, int rule, int use_xyz, const float *xyz,
                                          const float *new_xyz, const float *features, int *idx, int *pts_cnt, float *rows,
                                          sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c >= 0, "negative size");
    SN_REQUIRE(nsample >= 1, "nsample must be at least 1");
    SN_REQUIRE(rule == SN_BALL_RULE_SQRT || rule == SN_BALL_RULE_SQUARED, "bad rule");
    SN_REQUIRE(use_xyz == 0 || use_xyz == 1, "use_xyz must be 0 or 1");
    SN_REQUIRE(c > 0 || use_xyz, "no output channel (c == 0 without use_xyz)");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE(n >= 1, "an empty dataset cloud (n == 0) has no index to return");
    SN_REQUIRE(xyz && new_xyz && idx && rows && (c == 0 || features), "null pointer");
    SN_REQUIRE((long long)c + 3 <= INT_MAX, "c + 3 must fit in 31 bits");
    RowsArgs a = {};
    unsigned grid;
    if (int rc = ball_grid(__func__, b, m, &a.qpw, &a.groups, &grid)) return rc;
    a.n = n, a.m = m, a.nsample = nsample, a.thr = ball_threshold(radius, rule);
    a.xyz = xyz, a.new_xyz = new_xyz, a.features = features, a.c = c, a.u3 = 3 * use_xyz;
    a.idx = idx, a.pts_cnt = pts_cnt, a.rows = rows;
    if (rule == SN_BALL_RULE_SQRT)
        hipLaunchKernelGGL(ball_group_rows_kernel<SN_BALL_RULE_SQRT>, dim3(grid), dim3(kBallWaves * kWave), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ball_group_rows_kernel<SN_BALL_RULE_SQUARED>, dim3(grid), dim3(kBallWaves * kWave), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_group_rows_backward(int b, int n, int m, int c, int nsample, int use_xyz, const int *idx, const int *start,
                                      const int *order, const float *grad_rows, float *grad_features, float *grad_xyz,
                                      float *grad_new_xyz, sn_stream_t stream)
{
    (void)idx;  // the lists carry all it says
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c >= 0, "negative size");
    SN_REQUIRE(nsample >= 1, "nsample must be at least 1");
    SN_REQUIRE(use_xyz == 0 || use_xyz == 1, "use_xyz must be 0 or 1");
    SN_REQUIRE(c > 0 || use_xyz, "no output channel (c == 0 without use_xyz)");
    SN_REQUIRE((long long)m * nsample <= INT_MAX && (long long)c + 3 <= INT_MAX, "m * nsample and c + 3 must fit in 31 bits");
    if (b == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const int ne = m * nsample, u3 = 3 * use_xyz, Ci = u3 + c;
    if (c == 0) grad_features = nullptr;
    if (n == 0) grad_features = grad_xyz = nullptr;
    SN_REQUIRE(m == 0 || grad_rows, "null pointer");
    SN_REQUIRE(!(grad_features || (grad_xyz && use_xyz)) || (start && (m == 0 || order)), "null pointer");
    hipError_t e = hipSuccess;
    if (!use_xyz) {  // no coordinate column: both point gradients are zeros
        if (grad_xyz) e = hipMemsetAsync(grad_xyz, 0, (size_t)b * n * 3 * sizeof(float), st);
        if (e == hipSuccess && grad_new_xyz && m > 0) e = hipMemsetAsync(grad_new_xyz, 0, (size_t)b * m * 3 * sizeof(float), st);
        if (e != hipSuccess) return sn_set_error((int)e, "%s: %s", __func__, hipGetErrorString(e));
        grad_xyz = grad_new_xyz = nullptr;
    }
    if (grad_features || grad_xyz) {
        GradRowsArgs a = {};
        a.n = n, a.ne = ne, a.Ci = Ci, a.c = c, a.u3 = u3;
        a.col0 = grad_xyz ? 0 : u3;
        a.ncols = (grad_features ? Ci : u3) - a.col0;
        LaneGrid l;
        if (int rc = lane_grid(__func__, (long long)b * n, a.ncols, true, &l)) return rc;
        a.lg = l.lg, a.chunks = l.chunks, a.items = l.items;
        a.start = start, a.order = order, a.grad_rows = grad_rows, a.grad_features = grad_features, a.grad_xyz = grad_xyz;
        hipLaunchKernelGGL(group_rows_backward_kernel, dim3(l.grid), dim3(kGrThreads), 0, st, a);
    }
    if (grad_new_xyz && m > 0) {
        GradCentreArgs a = {};
        unsigned grid;
        if (int rc = ball_grid(__func__, b, m, &a.qpw, &a.groups, &grid)) return rc;
        a.m = m, a.nsample = nsample, a.Ci = Ci, a.grad_rows = grad_rows, a.grad_new_xyz = grad_new_xyz;
        hipLaunchKernelGGL(group_rows_centre_kernel, dim3(grid), dim3(kBallWaves * kWave), 0, st, a);
    }
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_group_pool_forward(int G, int S, int C, const float *z, const float *coef, float *pooled, int *argsel, float *zsel,
                                     sn_stream_t stream)
{
    SN_REQUIRE(G >= 1 && S >= 1 && C >= 1 && z && coef && pooled && argsel && zsel, "bad argument");
    const int cblocks = (C + kWave - 1) / kWave;
    const long long items = (long long)G * cblocks, grid = (items + kGpWaves - 1) / kGpWaves;
    if (grid > INT_MAX) return sn_too_many_workgroups(__func__);
    hipLaunchKernelGGL(group_pool_fwd_kernel, dim3((unsigned)grid), dim3(kGpWaves * kWave), 0, (hipStream_t)stream, items, cblocks, S, C, z,
                       coef, pooled, argsel, zsel);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_group_pool_stats_blocks(int G) { return G < 1 ? 0 : (G + kGpGroups - 1) / kGpGroups; }

extern "C" int sn_group_pool_backward(int G, int C, const float *g, const float *pooled, const float *zsel, float *gsel, float *stats,
                                      sn_stream_t stream)
{
    SN_REQUIRE(G >= 1 && C >= 1 && g && pooled && zsel && gsel, "bad argument");
    const int cblocks = (C + kWave - 1) / kWave;
    SN_REQUIRE(cblocks <= 65535, "C beyond 65535 * 64 channels");
    hipLaunchKernelGGL(group_pool_bwd_kernel, dim3((unsigned)sn_group_pool_stats_blocks(G), (unsigned)cblocks), dim3(kGpWaves * kWave), 0,
                       (hipStream_t)stream, G, C, g, pooled, zsel, gsel, stats);
    SN_LAUNCH_CHECK();
    return 0;
}

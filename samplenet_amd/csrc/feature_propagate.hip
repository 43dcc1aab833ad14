// feature_propagate.hip -- the three nearest known points of every unknown point, the query of a PointNet++ feature propagation
// (up-sampling) layer (gfx950).  Stands in for Pointnet2_PyTorch's three_nn.  That source is not at hand: the tie order and the
// filling with m < 3 are AS RECALLED, UNPINNED (include/samplenet_hip_internal.h states the contract; tests/interp_ref.py restates
// it in numpy float32).
//
// Regime.  Thousands of unknown points (n) against a small known cloud (m = 16 .. 1024): the opposite of sn_knn, where a wave owns a
// query and its lanes the dataset.  Here A LANE OWNS AN UNKNOWN POINT.  A workgroup is 64 queries (one per lane) times W waves
// (fp_waves: 16, 8 or 4 -- the fewer workgroups a launch has, the more waves each gets).  The known cloud is staged in LDS as
// float4 in chunks of kFpStage points; within a chunk wave w walks its own ascending slice, every lane reading the SAME address
// (one broadcast LDS read of the point's three words, no bank conflict), and keeps a running top-3 in registers across chunks.
// The W partial top-3 lists meet through LDS and are merged by (d2, index) -- the three smallest by that order are unique, so the
// partition cannot show in the result.  No atomics, no workspace: deterministic, safe under stream capture.
#include <climits>
#include <cmath>

#include "sn_common.h"

#pragma clang fp contract(off)  // every product and sum of the contract is rounded on its own (no FMA)

namespace sn {
namespace {

constexpr int kFpQueries = 64;        // queries per workgroup: one per lane
constexpr int kFpStage = 1024;        // known points per LDS stage (16 KB as float4)
constexpr int kFpMaxWaves = 16;       // waves per workgroup at most

// Waves per workgroup.  The scan is split over the waves of a workgroup, so more waves cost nothing but the merge; a launch with
// few workgroups (n = 64 .. 256 at batch 32) needs them to fill the chip at all.
int fp_waves(long long workgroups) { return workgroups >= 1024 ? 4 : (workgroups >= 512 ? 8 : 16); }

struct FpArgs {
    int n, m, groups;
    const float *unknown;        // (b,n,3)
    const float *known;          // (b,m,3)
    int *idx;                    // (b,n,3)
    float *dist2, *dist;         // (b,n,3), optional
};

struct Top3 {
    float d0, d1, d2;
    int i0, i1, i2;
};

// the ascending walk's insertion: strict <, so a tie keeps the lower index in front and a NaN (or +inf) distance never enters
__device__ __forceinline__ void top3_walk(Top3 &t, float d, int k)
{
    if (d < t.d2) {
        if (d < t.d1) {
            t.d2 = t.d1, t.i2 = t.i1;
            if (d < t.d0) {
                t.d1 = t.d0, t.i1 = t.i0;
                t.d0 = d, t.i0 = k;
            } else {
                t.d1 = d, t.i1 = k;
            }
        } else {
            t.d2 = d, t.i2 = k;
        }
    }
}

__device__ __forceinline__ bool fp_before(float d, int k, float e, int j) { return d < e || (d == e && k < j); }

// the merge's insertion: candidates arrive in any index order, so the order is (d2, index) written out.  An unfilled slot holds
// (+inf, 0) and no candidate with d = +inf is ever offered, so every candidate goes in front of an unfilled slot by d < +inf.
__device__ __forceinline__ void top3_merge(Top3 &t, float d, int k)
{
    if (fp_before(d, k, t.d2, t.i2)) {
        if (fp_before(d, k, t.d1, t.i1)) {
            t.d2 = t.d1, t.i2 = t.i1;
            if (fp_before(d, k, t.d0, t.i0)) {
                t.d1 = t.d0, t.i1 = t.i0;
                t.d0 = d, t.i0 = k;
            } else {
                t.d1 = d, t.i1 = k;
            }
        } else {
            t.d2 = d, t.i2 = k;
        }
    }
}

// blockDim.x = 64 * W
__global__ void __launch_bounds__(kFpMaxWaves *kWave) three_nn_kernel(const FpArgs a)
{
    __shared__ float4 stage[kFpStage];
    __shared__ float cand_d[kFpMaxWaves * 3 * kWave];
    __shared__ int cand_i[kFpMaxWaves * 3 * kWave];
    const int cloud = blockIdx.x / a.groups, group = blockIdx.x - cloud * a.groups;
    const int W = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    const long long jl = (long long)group * kFpQueries + lane;
    const bool live = jl < a.n;
    const int j = live ? (int)jl : a.n - 1;  // a lane past the cloud scans a copy of the last query and stores nothing
    const float *U = a.unknown + ((size_t)cloud * a.n + j) * 3;
    const float ux = U[0], uy = U[1], uz = U[2];
    const float *K = a.known + (size_t)cloud * a.m * 3;

    Top3 t = {INFINITY, INFINITY, INFINITY, 0, 0, 0};
    for (int base = 0; base < a.m; base += kFpStage) {
        const int cn = a.m - base < kFpStage ? a.m - base : kFpStage;
        if (base) __syncthreads();  // the previous chunk has been read by every wave
        for (int i = threadIdx.x; i < cn; i += blockDim.x) {
            const float *p = K + (size_t)(base + i) * 3;
            stage[i] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        const int per = (cn + W - 1) / W;
        const int lo = wave * per, hi = lo + per < cn ? lo + per : cn;
        for (int k = lo; k < hi; ++k) {
            const float4 p = stage[k];
            const float dx = ux - p.x, dy = uy - p.y, dz = uz - p.z;
            const float d = ((dx * dx) + (dy * dy)) + (dz * dz);
            top3_walk(t, d, base + k);
        }
    }
    // the W partial lists meet; wave 0 merges them
    cand_d[(wave * 3 + 0) * kWave + lane] = t.d0, cand_i[(wave * 3 + 0) * kWave + lane] = t.i0;
    cand_d[(wave * 3 + 1) * kWave + lane] = t.d1, cand_i[(wave * 3 + 1) * kWave + lane] = t.i1;
    cand_d[(wave * 3 + 2) * kWave + lane] = t.d2, cand_i[(wave * 3 + 2) * kWave + lane] = t.i2;
    __syncthreads();
    if (!live || wave != 0) return;
    t = {INFINITY, INFINITY, INFINITY, 0, 0, 0};
    for (int s = 0; s < W * 3; ++s) {
        const float d = cand_d[s * kWave + lane];
        if (d < INFINITY) top3_merge(t, d, cand_i[s * kWave + lane]);
    }
    const size_t row = ((size_t)cloud * a.n + j) * 3;
    a.idx[row] = t.i0, a.idx[row + 1] = t.i1, a.idx[row + 2] = t.i2;
    if (a.dist2) a.dist2[row] = t.d0, a.dist2[row + 1] = t.d1, a.dist2[row + 2] = t.d2;
    if (a.dist) a.dist[row] = sqrtf(t.d0), a.dist[row + 1] = sqrtf(t.d1), a.dist[row + 2] = sqrtf(t.d2);  // correctly rounded (hipcc's default, kept)
}

int fp_grid(const char *who, int b, int n, int *groups, int *waves, unsigned *grid)
{
    *groups = (int)(((long long)n + kFpQueries - 1) / kFpQueries);
    const long long g = (long long)b * *groups;
    if (g > INT_MAX) return sn_set_error(SN_ERR_UNSUPPORTED, "%s: the launch needs more than 2^31 - 1 workgroups", who);
    *waves = fp_waves(g);
    *grid = (unsigned)g;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The interpolation's gradient towards the features by INVERTED INDEX.  grad_X[b,ch,r] is the sum, in ascending entry order, of
// grad_out[b,ch,e/k] * weights[b,e] over the entries e = j*k + t whose index names row r.  The list of those entries depends on idx
// alone: gather_invert_kernel builds it once per cloud (start: where each row's list begins; order: the entry numbers, row by row,
// each list ascending), gather_bwd_inverted_kernel walks it for every channel and forms the product where it is consumed -- no
// contribution is stored, nothing is added atomically, and the sequence of fp32 operations per element is that of
// weighted_gather_bwd_kernel + index_add_ordered_kernel (soft_projection.hip): bit-identical to sn_weighted_gather_backward_ordered.
constexpr int kInvThreads = 1024;     // one workgroup per cloud
constexpr int kInvWaves = kInvThreads / kWave;
constexpr int kInvTile = 4096;        // destination rows counted in LDS at a time (16 KB); n is not bounded by it
constexpr int kInvPer = kInvTile / kInvThreads;
constexpr int kInvBatch = 4;          // trips of 64 entries whose indices the placement loads at once
// the support bound: ceil(n / 64) * ne, the index loads of index_add_ordered_kernel, held to its kIndexAddOrderedWork
// (soft_projection.hip), so the inverted route exists exactly where the ordered route's sum is ordered (the placement below reads
// fewer: ne per wave up to n = 1024, about n / 1024 * ne beyond)
constexpr long long kInvWork = 1ll << 26;

bool invert_supported(long long n, long long ne) { return n >= 0 && ne >= 0 && n < INT_MAX && ne <= INT_MAX && ((n + 63) / 64) * ne <= kInvWork; }

// grid = b, block = kInvThreads.  Phase A, tile by tile of kInvTile rows: the valid entries of each row counted with integer LDS
// atomics (an integer sum has no order), an exclusive scan over the tile carried on from the tiles before it -> start.  Phase B:
// a wave owns up to 64 rows (a lane one row and its cursor) and walks the cloud's entries in ascending order, 64 per trip, visiting
// only those that name one of its rows -- index_add_ordered_kernel's ballot walk without the channel loop -- so every list ascends.
__global__ void __launch_bounds__(kInvThreads) gather_invert_kernel(int n, int ne, const int *__restrict__ idx, int *start, int *__restrict__ order)
{
    __shared__ int cnt[kInvTile];
    __shared__ int wave_sum[kInvWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    idx += (size_t)blockIdx.x * ne;
    order += (size_t)blockIdx.x * ne;
    start += (size_t)blockIdx.x * ((size_t)n + 1);

    int base = 0;  // valid entries below this tile's first row (the same in every thread)
    for (long long r0 = 0; r0 < n; r0 += kInvTile) {
        const int tn = n - r0 < kInvTile ? (int)(n - r0) : kInvTile;
        for (int i = tid; i < kInvTile; i += kInvThreads) cnt[i] = 0;
        __syncthreads();
        for (int e = tid; e < ne; e += kInvThreads) {
            const long long r = (long long)idx[e] - r0;
            if (r >= 0 && r < tn) atomicAdd(&cnt[(int)r], 1);
        }
        __syncthreads();
        int c[kInvPer], mine = 0;  // thread t owns rows t * kInvPer .. of the tile (counts past tn are zero)
#pragma unroll
        for (int q = 0; q < kInvPer; ++q) c[q] = cnt[tid * kInvPer + q], mine += c[q];
        int incl = mine;  // inclusive scan over the wave's lanes
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int up = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += up;
        }
        if (lane == kWave - 1) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kInvWaves; ++w) {
            const int s = wave_sum[w];
            before += w < wave ? s : 0;
            total += s;
        }
        int at = base + before + incl - mine;
#pragma unroll
        for (int q = 0; q < kInvPer; ++q) {
            if (tid * kInvPer + q < tn) start[r0 + tid * kInvPer + q] = at;
            at += c[q];
        }
        base += total;
        __syncthreads();  // cnt and wave_sum are free again; this tile's start[] is visible to the workgroup
    }
    if (tid == 0) start[n] = base;
    for (int i = base + tid; i < ne; i += kInvThreads) order[i] = -1;  // the slots no valid entry fills

    // rows per wave: the smallest power of two R <= 64 with 16 R >= n, so that a small cloud's walk is shared by all the waves
    int R = 1;
    while (R < kWave && R * kInvWaves < n) R <<= 1;
    const int groups = (int)(((long long)n + R - 1) / R);
    for (int g = wave; g < groups; g += kInvWaves) {
        const long long row0 = (long long)g * R, row = row0 + lane;
        int cur = lane < R && row < n ? start[row] : 0;
        // kInvBatch trips' indices are loaded before any of their stores: the wait for a trip's load also waits for the stores
        // issued before it (one counter), so the loads go first, once per batch
        for (int e0 = 0; e0 < ne; e0 += kInvBatch * kWave) {
            int id[kInvBatch];
#pragma unroll
            for (int u = 0; u < kInvBatch; ++u) id[u] = e0 + u * kWave + lane < ne ? idx[e0 + u * kWave + lane] : -1;
#pragma unroll
            for (int u = 0; u < kInvBatch; ++u) {
                const long long off = (long long)id[u] - row0;
                sn_u64 hits = __ballot(off >= 0 && off < R && id[u] < n);
                while (hits) {
                    const int t = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    if ((long long)__builtin_amdgcn_readlane(id[u], t) == row) order[cur++] = e0 + u * kWave + t;
                }
            }
        }
    }
}

constexpr int kGbThreads = 256;
constexpr int kGbChannels = 8;  // channels a thread accumulates in registers: entry number, query and weight are loaded once for all
constexpr int kGbBatch = 4;     // entries of a list whose operands are in flight together

// A thread owns one destination row and kGbChannels channels of it.  Threads are numbered row-fastest over (channel block, row) of
// a cloud, so a wave's stores run along r (coalesced) and at n < 64 a wave still has 64 busy lanes.  The reads of grad_out are
// scattered over one cloud's channel planes (m floats each): cache hits.
__global__ void __launch_bounds__(kGbThreads) gather_bwd_inverted_kernel(int c, int n, int m, int k, int blocks, const float *__restrict__ w,
                                                                        const float *__restrict__ go, const int *__restrict__ start,
                                                                        const int *__restrict__ order, float *__restrict__ gX)
{
    const int cloud = blockIdx.x / blocks;
    const long long t = (long long)(blockIdx.x - cloud * blocks) * kGbThreads + threadIdx.x;
    const long long cb = t / n;
    const int row = (int)(t - cb * n);
    const long long ch0 = cb * kGbChannels;
    if (ch0 >= c) return;
    const int nch = c - ch0 < kGbChannels ? (int)(c - ch0) : kGbChannels;
    const int ne = m * k;
    w += (size_t)cloud * ne;
    order += (size_t)cloud * ne;
    start += (size_t)cloud * ((size_t)n + 1);
    go += ((size_t)cloud * c + ch0) * m;
    gX += ((size_t)cloud * c + ch0) * n + row;
    float acc[kGbChannels];
#pragma unroll
    for (int q = 0; q < kGbChannels; ++q) acc[q] = 0.f;
    // inverse_walk.h's walk, clamp-and-skip rule included, on the channel-major layout with a run-time k and kGbChannels sums per
    // thread (two memory latencies per batch instead of per entry)
    const int lo = max(start[row], 0), hi = min(start[row + 1], ne);
    for (int i = lo; i < hi; i += kGbBatch) {
        int e[kGbBatch];
        float wt[kGbBatch], gv[kGbBatch][kGbChannels];
#pragma unroll
        for (int u = 0; u < kGbBatch; ++u) e[u] = i + u < hi ? order[i + u] : -1;
#pragma unroll
        for (int u = 0; u < kGbBatch; ++u) {
            const int at = (unsigned)e[u] < (unsigned)ne ? e[u] : 0;  // (an entry that is skipped below reads entry 0's operands)
            wt[u] = w[at];
            const float *g = go + (unsigned)at / (unsigned)k;
#pragma unroll
            for (int q = 0; q < kGbChannels; ++q) gv[u][q] = q < nch ? g[(size_t)q * m] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kGbBatch; ++u) {
            if ((unsigned)e[u] >= (unsigned)ne) continue;
#pragma unroll
            for (int q = 0; q < kGbChannels; ++q)
                if (q < nch) acc[q] += gv[u][q] * wt[u];  // product rounded, then added: weighted_gather_bwd_kernel's g * wt
        }
    }
#pragma unroll
    for (int q = 0; q < kGbChannels; ++q)
        if (q < nch) gX[(size_t)q * n] = acc[q];
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, float *dist, int *idx,
                           sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0, "negative size");
    if (b == 0 || n == 0) return 0;
    SN_REQUIRE(m >= 1, "an empty known cloud (m == 0) has no index to return");
    SN_REQUIRE(unknown && known && idx, "null pointer");
    FpArgs a = {};
    int waves;
    unsigned grid;
    if (int rc = fp_grid(__func__, b, n, &a.groups, &waves, &grid)) return rc;
    a.n = n, a.m = m, a.unknown = unknown, a.known = known, a.idx = idx, a.dist2 = dist2, a.dist = dist;
    hipLaunchKernelGGL(three_nn_kernel, dim3(grid), dim3(waves * kWave), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_gather_invert_supported(int n, int ne) { return invert_supported(n, ne) ? 1 : 0; }

extern "C" int sn_gather_invert(int b, int n, int ne, const int *idx, int *start, int *order, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && ne >= 0, "negative size");
    if (b == 0 || n == 0) return 0;
    SN_REQUIRE(start && (ne == 0 || (idx && order)), "null pointer");
    if (!invert_supported(n, ne))
        return sn_set_error(SN_ERR_UNSUPPORTED, "%s: ceil(n / 64) * ne = %lld exceeds 2^26 (sn_gather_invert_supported)", __func__,
                            ((long long)n + 63) / 64 * ne);
    hipLaunchKernelGGL(gather_invert_kernel, dim3(b), dim3(kInvThreads), 0, (hipStream_t)stream, n, ne, idx, start, order);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_weighted_gather_backward_inverted(int b, int c, int n, int m, int k, const float *weights, const float *grad_out,
                                                    const int *start, const int *order, float *grad_X, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0 && k >= 1, "bad size");
    SN_REQUIRE((long long)m * k <= INT_MAX, "m * k must fit in 31 bits");
    if (b == 0 || c == 0 || n == 0) return 0;
    SN_REQUIRE(start && grad_X && (m == 0 || (weights && grad_out && order)), "null pointer");
    const long long blocks = ((long long)n * (((long long)c + kGbChannels - 1) / kGbChannels) + kGbThreads - 1) / kGbThreads;
    if (blocks * b > INT_MAX) return sn_set_error(SN_ERR_UNSUPPORTED, "%s: the launch needs more than 2^31 - 1 workgroups", __func__);
    hipLaunchKernelGGL(gather_bwd_inverted_kernel, dim3((unsigned)(blocks * b)), dim3(kGbThreads), 0, (hipStream_t)stream, c, n, m, k,
                       (int)blocks, weights, grad_out, start, order, grad_X);
    SN_LAUNCH_CHECK();
    return 0;
}

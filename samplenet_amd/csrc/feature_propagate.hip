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

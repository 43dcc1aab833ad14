// sampling.hip -- farthest-point sampling (gfx950): the pointnet2 / TF op `furthest_point_sample` / `farthest_point_sample`
// (in-tree definition reconstruction/external/sampling/tf_sampling_g.cu:105-170).
//
// Contract (pinned bit for bit by tests/test_gpu_fps.py against a numpy restatement):
//   idx[b][0] = 0; every later pick is the point with the largest running minimum squared distance to the points picked so
//   far, ties to the LOWEST point index (numpy argmax, the rule of sn_nn_matching / sn_knn).  d = (dx*dx + dy*dy) + dz*dz in
//   fp32 with dx = x_k - x_last, one rounding per operation, never contracted; running min = d < cur ? d : cur from +inf.
//   Indices stay in [0, N) whatever the input: a NaN distance never enters the running minimum, so every value the arg-max
//   sees is in [+0, +inf].
//
// An FPS step depends on the previous one: M dependent steps per cloud, latency bound.  The variants differ in how many lanes
// share a cloud (sn_fps_set_variant forces one; all three give identical indices):
//   (a) fps_wave_kernel<PPT>    one wave per cloud, PPT <= 32 points per lane in registers (N <= 2048); the step's arg-max is
//                               DPP + ballot + readlane only, no LDS, no barrier.  kFpsCloudsPerGroup clouds per workgroup.
//   (b) fps_group_kernel<PPT>   one workgroup per cloud, up to 1024 threads x 16 points in registers (N <= 16384); the waves
//                               meet once per step in a double-buffered LDS slot array: one __syncthreads per step.
//   (c) fps_stream_kernel       one workgroup per cloud, any N: coordinates re-read every step (L2 resident), the running
//                               minimum in the caller's temp (B*N floats).
// Per lane the candidate is (distance, index, coordinates) of its first maximum; where lanes own ascending contiguous point
// ranges ((a), (b)) the lowest lane holding the wave's maximum holds the lowest index, otherwise ((c)) a second reduction
// takes the lowest index among the tied lanes.  The winner's coordinates travel with it, so no step re-reads memory.
#include <climits>

#include "fps_select.h"
#include "sn_common.h"

#pragma clang fp contract(off)  // the contract's distance is product-then-sum (no FMA)

namespace sn {
namespace {

constexpr int kFpsCloudsPerGroup = 4;  // (a): waves (= clouds) per workgroup, one per SIMD
constexpr int kFpsWaveMaxPPT = 32;     // (a): N <= 64 * 32
constexpr int kFpsGroupMaxThreads = 1024;
constexpr int kFpsGroupMaxPPT = 16;    // (b): N <= 1024 * 16
constexpr int kFpsMaxWaves = kFpsGroupMaxThreads / kWave;
static_assert(kWave * kFpsWaveMaxPPT == kFpsWaveMaxN && kFpsGroupMaxThreads * kFpsGroupMaxPPT == kFpsGroupMaxN, "fps_select.h");

struct FpsCand {
    float d;  // running minimum distance; -1 for a lane without points (every real value is >= +0)
    int k;
    float x, y, z;
};

// v op= v from the DPP-selected lane; rows outside ROWS keep their value (old operand = v).  Distances are reduced as their
// bit patterns: for -1 (no point) and every value in [+0, +inf] signed-integer order is float order, and an integer max needs
// no NaN canonicalisation, so the compiler can fold the lane move into it.
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_max(int v)
{
    return max(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_min(int v)
{
    return min(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false));
}

// Reduction over the 16 lanes of each row (quad swaps, half-row mirror, row mirror: every lane of the row ends with the
// row's result); WAVE: then across the four rows (row_bcast 15 / 31: lane 63 ends with the wave's result).
template <bool WAVE, bool MAX>
__device__ __forceinline__ int reduce(int v)
{
    v = MAX ? dpp_max<0xb1, 0xf>(v) : dpp_min<0xb1, 0xf>(v);     // quad_perm [1,0,3,2]
    v = MAX ? dpp_max<0x4e, 0xf>(v) : dpp_min<0x4e, 0xf>(v);     // quad_perm [2,3,0,1]
    v = MAX ? dpp_max<0x141, 0xf>(v) : dpp_min<0x141, 0xf>(v);   // row_half_mirror
    v = MAX ? dpp_max<0x140, 0xf>(v) : dpp_min<0x140, 0xf>(v);   // row_mirror
    if (!WAVE) return __builtin_amdgcn_readlane(v, 0);
    v = MAX ? dpp_max<0x142, 0xa>(v) : dpp_min<0x142, 0xa>(v);   // row_bcast:15 into rows 1, 3
    v = MAX ? dpp_max<0x143, 0xc>(v) : dpp_min<0x143, 0xc>(v);   // row_bcast:31 into rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}

// The candidate with the largest distance, ties to the lowest index, over the whole wave (WAVE) or over row 0 (lanes 0..15;
// the other rows must hold d = -1).  ORDERED: lower lanes hold lower indices, so the lowest tied lane is the winner.
// Call with every lane of the wave active.  The result is wave-uniform.
template <bool ORDERED, bool WAVE>
__device__ __forceinline__ FpsCand wave_pick(const FpsCand &c)
{
    const int db = __float_as_int(c.d);
    const int m = reduce<WAVE, true>(db);
    unsigned long long tied = __ballot(db == m);
    if (!ORDERED) {
        const int k = reduce<WAVE, false>(db == m ? c.k : INT_MAX);
        tied = __ballot(db == m && c.k == k);
    }
    const int L = __builtin_ctzll(tied);  // (never empty: m is some lane's value)
    return {__int_as_float(m), __builtin_amdgcn_readlane(c.k, L), readlane_f(c.x, L), readlane_f(c.y, L), readlane_f(c.z, L)};
}

// The register-resident cloud of one lane: points k0 .. k0 + PPT - 1 (slots past N hold cur = -inf and never win).
template <int PPT>
struct LanePoints {
    float x[PPT], y[PPT], z[PPT], cur[PPT];
    int k0;

    __device__ __forceinline__ void load(const float *__restrict__ P, int layout, int N, int first)
    {
        k0 = first;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int k = k0 + i;
            const bool ok = k < N;
            x[i] = ok ? P[pt_off(layout, N, k, 0)] : 0.f;
            y[i] = ok ? P[pt_off(layout, N, k, 1)] : 0.f;
            z[i] = ok ? P[pt_off(layout, N, k, 2)] : 0.f;
            cur[i] = ok ? INFINITY : -INFINITY;
        }
    }
    // fold the last pick into the running minima; return this lane's first maximum
    __device__ __forceinline__ FpsCand step(float lx, float ly, float lz)
    {
        FpsCand c{-1.f, 0, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const float dx = x[i] - lx, dy = y[i] - ly, dz = z[i] - lz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            cur[i] = d < cur[i] ? d : cur[i];
            const bool gt = cur[i] > c.d;  // (selects, not a branch: the chain through c.d is the step's critical path)
            c.d = gt ? cur[i] : c.d;
            c.k = gt ? k0 + i : c.k;
            c.x = gt ? x[i] : c.x;
            c.y = gt ? y[i] : c.y;
            c.z = gt ? z[i] : c.z;
        }
        return c;
    }
};

// (a) one wave per cloud
template <int PPT>
__global__ void __launch_bounds__(kFpsCloudsPerGroup * kWave) fps_wave_kernel(int B, int N, int M, int layout,
                                                                               const float *__restrict__ xyz, int *__restrict__ idx)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * kFpsCloudsPerGroup + (int)(threadIdx.x / kWave);
    if (b >= B) return;  // (wave-uniform)
    const float *P = xyz + (size_t)b * 3 * N;
    int *out = idx + (size_t)b * M;
    LanePoints<PPT> pts;
    pts.load(P, layout, N, lane * PPT);
    float lx = P[pt_off(layout, N, 0, 0)], ly = P[pt_off(layout, N, 0, 1)], lz = P[pt_off(layout, N, 0, 2)];
    if (lane == 0) out[0] = 0;
    for (int j = 1; j < M; ++j) {
        const FpsCand w = wave_pick<true, true>(pts.step(lx, ly, lz));
        if (lane == 0) out[j] = w.k;
        lx = w.x, ly = w.y, lz = w.z;
    }
}

// (b) and (c): the waves' candidates meet in LDS.  Slot array s (= step parity): a wave writes slot s of step j only after
// the barrier of step j - 1, which every wave passes after its reads of step j - 2 -- the last use of the same array.
struct FpsSlots {
    float4 a[2][kFpsMaxWaves];  // (d, k bits, x, y)
    float z[2][kFpsMaxWaves];
};

template <bool ORDERED>
__device__ __forceinline__ FpsCand group_pick(FpsSlots &S, int s, const FpsCand &mine)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    const FpsCand w = wave_pick<ORDERED, true>(mine);
    if (lane == 0) {
        S.a[s][wave] = make_float4(w.d, __int_as_float(w.k), w.x, w.y);
        S.z[s][wave] = w.z;
    }
    __syncthreads();
    FpsCand c{-1.f, 0, 0.f, 0.f, 0.f};
    if (lane < nw) {
        const float4 v = S.a[s][lane];
        c = {v.x, __float_as_int(v.y), v.z, v.w, S.z[s][lane]};
    }
    return wave_pick<ORDERED, false>(c);
}

// (b) one workgroup per cloud, blockDim.x = 64 * ceil(N / (64 PPT)) <= 1024
template <int PPT>
__global__ void __launch_bounds__(kFpsGroupMaxThreads) fps_group_kernel(int N, int M, int layout, const float *__restrict__ xyz,
                                                                        int *__restrict__ idx)
{
    __shared__ FpsSlots S;
    const int b = blockIdx.x;
    const float *P = xyz + (size_t)b * 3 * N;
    int *out = idx + (size_t)b * M;
    LanePoints<PPT> pts;
    pts.load(P, layout, N, threadIdx.x * PPT);
    float lx = P[pt_off(layout, N, 0, 0)], ly = P[pt_off(layout, N, 0, 1)], lz = P[pt_off(layout, N, 0, 2)];
    if (threadIdx.x == 0) out[0] = 0;
    for (int j = 1; j < M; ++j) {
        const FpsCand w = group_pick<true>(S, j & 1, pts.step(lx, ly, lz));
        if (threadIdx.x == 0) out[j] = w.k;
        lx = w.x, ly = w.y, lz = w.z;
    }
}

// (c) one workgroup of 1024 threads per cloud, any N; thread t walks points t, t + 1024, ... (coalesced), so lanes do not
// own ascending ranges and the picks take the lowest index among ties explicitly.  temp: (B, N) running minima, written at
// the first step (no initialisation pass), read and lowered from the second on.
__global__ void __launch_bounds__(kFpsGroupMaxThreads) fps_stream_kernel(int N, int M, int layout, const float *__restrict__ xyz,
                                                                         float *__restrict__ temp, int *__restrict__ idx)
{
    __shared__ FpsSlots S;
    const int b = blockIdx.x, nt = blockDim.x;
    const float *P = xyz + (size_t)b * 3 * N;
    float *T = temp + (size_t)b * N;
    int *out = idx + (size_t)b * M;
    float lx = P[pt_off(layout, N, 0, 0)], ly = P[pt_off(layout, N, 0, 1)], lz = P[pt_off(layout, N, 0, 2)];
    if (threadIdx.x == 0) out[0] = 0;
    for (int j = 1; j < M; ++j) {
        FpsCand c{-1.f, 0, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = threadIdx.x; k < N; k += nt) {
            const float x = P[pt_off(layout, N, k, 0)], y = P[pt_off(layout, N, k, 1)], z = P[pt_off(layout, N, k, 2)];
            const float dx = x - lx, dy = y - ly, dz = z - lz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const float prev = j > 1 ? T[k] : INFINITY;
            const float cur = d < prev ? d : prev;
            if (j == 1 || d < prev) T[k] = cur;
            if (cur > c.d) c = {cur, k, x, y, z};
        }
        const FpsCand w = group_pick<false>(S, j & 1, c);
        if (threadIdx.x == 0) out[j] = w.k;
        lx = w.x, ly = w.y, lz = w.z;
    }
}

// (b): 4 points per lane up to 4096 points (fewer waves meet at the barrier for small clouds), then 8 and 16 per lane
int fps_group_ppt(int N) { return N <= 4096 ? 4 : N <= 8192 ? 8 : 16; }

}  // namespace
}  // namespace sn

using namespace sn;

// xyz (B,N,3) [SN_LAYOUT_BNC] or (B,3,N) [SN_LAYOUT_BCN]; idx (B,M) int32; temp: B*N floats when the streaming path runs
// (sn_workspace_bytes("furthest_point_sample", B, N, M, 0) != 0), else may be NULL.
extern "C" int sn_furthest_point_sample(int B, int N, int M, const float *xyz, int layout, float *temp, int *idx, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && N >= 0 && M >= 0, "negative size");
    SN_REQUIRE(layout == SN_LAYOUT_BNC || layout == SN_LAYOUT_BCN, "bad layout");
    if (B == 0) return 0;
    SN_REQUIRE(N >= 1, "empty clouds (N = 0, B > 0)");
    if (M == 0) return 0;
    SN_REQUIRE(xyz && idx, "null pointer");
    const int v = fps_choose(B, N);
    if (v == 0) return sn_set_error(SN_ERR_UNSUPPORTED, "sn_furthest_point_sample: variant %d does not take N = %d", g_fps_variant, N);
    SN_REQUIRE(v != 3 || temp, "temp is NULL but this shape runs the streaming path (sn_workspace_bytes(\"furthest_point_sample\"))");
    hipStream_t st = (hipStream_t)stream;
    if (v == 1) {
        const dim3 grid((B + kFpsCloudsPerGroup - 1) / kFpsCloudsPerGroup), block(kFpsCloudsPerGroup * kWave);
#define SN_FPS_A(PPT_) hipLaunchKernelGGL(fps_wave_kernel<PPT_>, grid, block, 0, st, B, N, M, layout, xyz, idx)
        if (N <= 64) SN_FPS_A(1);
        else if (N <= 128) SN_FPS_A(2);
        else if (N <= 256) SN_FPS_A(4);
        else if (N <= 512) SN_FPS_A(8);
        else if (N <= 1024) SN_FPS_A(16);
        else SN_FPS_A(32);
#undef SN_FPS_A
    } else if (v == 2) {
        const int ppt = fps_group_ppt(N);
        const int lanes = (N + ppt - 1) / ppt;
        const dim3 block((lanes + kWave - 1) / kWave * kWave);
#define SN_FPS_B(PPT_) hipLaunchKernelGGL(fps_group_kernel<PPT_>, dim3(B), block, 0, st, N, M, layout, xyz, idx)
        if (ppt == 4) SN_FPS_B(4);
        else if (ppt == 8) SN_FPS_B(8);
        else SN_FPS_B(16);
#undef SN_FPS_B
    } else {
        hipLaunchKernelGGL(fps_stream_kernel, dim3(B), dim3(kFpsGroupMaxThreads), 0, st, N, M, layout, xyz, temp, idx);
    }
    SN_LAUNCH_CHECK();
    return 0;
}

// rank_points.hip -- whole clouds ranked on the device (gfx950): the progressive sampler's inference,
// simple_projection_and_continued_fps / fps_from_given_indices of reconstruction/src/samplenet_progressive_pointnet_ae.py:546-600
// (classification/infer_samplenet_progressive.py:207-212 does the same through its own copy).
//
// Contract (pinned bit for bit by tests/test_gpu_rank_points.py against tests/rank_ref.py and against sn_nn_matching_indexed):
//   out_idx[b, :] = the distinct values of idx[b, :] in order of first occurrence, then farthest-point picks up to k: every pick
//   is the point with the largest running minimum squared distance to the points chosen so far, the distance in float64 as
//   ((dx*dx + dy*dy) + dz*dz), one rounding per operation, never contracted; ties to the LOWEST point index (np.argmax).
//   idx values are clamped into [0, N); a NaN distance never enters a running minimum, so every value the arg-max sees lies in
//   [+0, +inf] and every index written lies in [0, N) whatever the input.
//
// A chain of up to 8192 dependent steps per cloud: the design target is the latency of one step.  One workgroup per cloud:
//   * the cloud sits in LDS as fp32 SoA (seed coordinates are broadcast reads, never global loads); a thread owns PPT
//     consecutive points and keeps them and their running minima in registers as doubles;
//   * first occurrences in O(k): an LDS table indexed by point takes the lowest position at which the point occurs (atomic min),
//     position j is a first occurrence iff table[idx[j]] == j; the order-keeping compaction gives every wave one contiguous
//     segment of positions (ballot / popcount prefix inside the wave) and meets the other waves ONCE, for the segment offsets;
//   * the seed pass folds the seeds into the minima without a barrier;
//   * a farthest-point step: per-lane first maximum -> wave arg-max by DPP on the distance's bit pattern (for values in
//     {-1} u [+0, +inf] signed 64-bit integer order is double order) -> the wave's first lane writes (distance, index, x, y, z)
//     into a double-buffered LDS slot -> ONE barrier -> the first 16 lanes of every wave read the slots and reduce them again ->
//     every thread folds the winner's coordinates, which travelled with it: no lookup depends on the winner's index.
//     Threads own ascending point ranges and waves ascending thread ranges, so the lowest tied lane holds the lowest index.
#include <climits>

#include "sn_common.h"

#pragma clang fp contract(off)  // the contract's distance is product-then-sum (no FMA)

namespace sn {
namespace {

constexpr int kRankMaxThreads = 1024;
constexpr int kRankMaxWaves = kRankMaxThreads / kWave;
constexpr int kRankMaxN = 8192, kRankMaxK = 8192;  // (indices fit the 16-bit seed list; the cloud, table and list fit LDS)

int g_rank_ppt = 0;  // sn_rank_points_set_ppt: 0 = by N

struct RankCand {
    double d;  // running minimum distance; -1 for a lane without points (every real value is >= +0)
    int k;
    float x, y, z;
};

// Slot array s (= step parity): a wave writes slot s of step j only after the barrier of step j - 1, which every wave passes
// after its reads of step j - 2 -- the last use of the same array.
struct RankSlots {
    float4 a[2][kRankMaxWaves];  // (distance low word, high word, index, x)
    float2 b[2][kRankMaxWaves];  // (y, z)
    int count[kRankMaxWaves];    // the compaction's first occurrences per wave segment
};

// v = max(v, v of the DPP-selected lane) on 64-bit integers; rows outside ROWS keep their value (old operand = v)
template <int CTRL, int ROWS>
__device__ __forceinline__ long long dpp_max64(long long v)
{
    const int lo = (int)v, hi = (int)(v >> 32);
    const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWS, 0xf, false);
    const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWS, 0xf, false);
    const long long o = (long long)(((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo);
    return o > v ? o : v;
}

// Maximum over the 16 lanes of each row; WAVE: then across the four rows.  The result is that of row 0 / of the wave, uniform.
template <bool WAVE>
__device__ __forceinline__ long long reduce_max64(long long v)
{
    v = dpp_max64<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
    v = dpp_max64<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
    v = dpp_max64<0x141, 0xf>(v);  // row_half_mirror
    v = dpp_max64<0x140, 0xf>(v);  // row_mirror
    int src = 0;
    if (WAVE) {
        v = dpp_max64<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
        v = dpp_max64<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3
        src = 63;
    }
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// The candidate with the largest distance over the whole wave (WAVE) or over row 0 (lanes 0..15; the other rows must hold
// d = -1 and row 0 some d >= 0).  Lower lanes hold lower indices: the lowest tied lane wins.  Every lane active; uniform result.
template <bool WAVE>
__device__ __forceinline__ RankCand wave_pick(const RankCand &c)
{
    const long long db = __double_as_longlong(c.d);
    const long long m = reduce_max64<WAVE>(db);
    const int L = __builtin_ctzll(__ballot(db == m));  // (never empty: m is some lane's value)
    return {__longlong_as_double(m), __builtin_amdgcn_readlane(c.k, L), readlane_f(c.x, L), readlane_f(c.y, L), readlane_f(c.z, L)};
}

__device__ __forceinline__ RankCand group_pick(RankSlots &S, int s, const RankCand &mine)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    const RankCand w = wave_pick<true>(mine);
    if (lane == 0) {
        const long long db = __double_as_longlong(w.d);
        S.a[s][wave] = make_float4(__int_as_float((int)db), __int_as_float((int)(db >> 32)), __int_as_float(w.k), w.x);
        S.b[s][wave] = make_float2(w.y, w.z);
    }
    __syncthreads();
    RankCand c{-1.0, 0, 0.f, 0.f, 0.f};
    if (lane < nw) {
        const float4 a = S.a[s][lane];
        const float2 yz = S.b[s][lane];
        const unsigned long long db = ((unsigned long long)(unsigned)__float_as_int(a.y) << 32) | (unsigned)__float_as_int(a.x);
        c = {__longlong_as_double((long long)db), __float_as_int(a.z), a.w, yz.x, yz.y};
    }
    return wave_pick<false>(c);
}

__device__ __forceinline__ int clamp_index(int v, int N) { return min(max(v, 0), N - 1); }

// blockDim.x = 64 * ceil(ceil(N / PPT) / 64) <= 1024; dynamic LDS: rank_lds_bytes(N, K)
template <int PPT>
__global__ void __launch_bounds__(kRankMaxThreads) rank_points_kernel(int N, int K, int layout, const float *__restrict__ xyz,
                                                                      const int *__restrict__ idx, float *__restrict__ out,
                                                                      int *__restrict__ out_idx, int *__restrict__ n_unique)
{
    extern __shared__ __align__(16) unsigned char s_raw[];
    RankSlots &S = *reinterpret_cast<RankSlots *>(s_raw);
    float *X = reinterpret_cast<float *>(s_raw + sizeof(RankSlots));
    float *Y = X + N, *Z = Y + N;
    int *first = reinterpret_cast<int *>(Z + N);                                // lowest position of every point in idx
    unsigned short *sel = reinterpret_cast<unsigned short *>(first + N);        // the seeds: min(K, N) entries at the most
    const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x, lane = t & (kWave - 1), wave = t / kWave, nw = nt / kWave;
    const float *P = xyz + (size_t)b * 3 * N;
    const int *id = idx + (size_t)b * K;
    float *o = out ? out + (size_t)b * K * 3 : nullptr;
    int *oi = out_idx ? out_idx + (size_t)b * K : nullptr;

    for (int p = t; p < N; p += nt) {
        X[p] = P[pt_off(layout, N, p, 0)];
        Y[p] = P[pt_off(layout, N, p, 1)];
        Z[p] = P[pt_off(layout, N, p, 2)];
        first[p] = INT_MAX;
    }
    __syncthreads();
    for (int j = t; j < K; j += nt) atomicMin(&first[clamp_index(id[j], N)], j);
    __syncthreads();

    // ---- first occurrences, in order: wave w owns positions [w seg, (w + 1) seg), seg a multiple of 64
    const int seg = ((K + nw - 1) / nw + kWave - 1) & ~(kWave - 1);
    const int j0 = wave * seg, j1 = min(K, j0 + seg);
    int count = 0;
    for (int c = j0; c < j1; c += kWave) {
        const int j = c + lane;
        const bool is_first = j < j1 && first[clamp_index(id[j], N)] == j;
        count += __popcll(__ballot(is_first));
    }
    if (lane == 0) S.count[wave] = count;
    __syncthreads();
    int base = 0, nseed = 0;
    for (int w = 0; w < nw; ++w) {
        const int c = S.count[w];
        nseed += c;
        base += w < wave ? c : 0;
    }
    for (int c = j0; c < j1; c += kWave) {
        const int j = c + lane;
        const int v = j < j1 ? clamp_index(id[j], N) : 0;
        const bool is_first = j < j1 && first[v] == j;
        const unsigned long long mask = __ballot(is_first);
        if (is_first) sel[base + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)v;
        base += __popcll(mask);
    }
    if (t == 0 && n_unique) n_unique[b] = nseed;  // distinct values of idx[b, :]
    __syncthreads();
    for (int q = t; q < nseed; q += nt) {
        const int p = sel[q];
        if (oi) oi[q] = p;
        if (o) o[q * 3 + 0] = X[p], o[q * 3 + 1] = Y[p], o[q * 3 + 2] = Z[p];
    }
    if (!o && !oi) return;  // (only the count was wanted: block-uniform)

    // ---- this thread's points and their distance to the seed set
    double px[PPT], py[PPT], pz[PPT], dist[PPT];
    const int k0 = t * PPT;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const bool ok = k0 + i < N;
        const int p = ok ? k0 + i : 0;
        px[i] = ok ? (double)X[p] : 0.0;
        py[i] = ok ? (double)Y[p] : 0.0;
        pz[i] = ok ? (double)Z[p] : 0.0;
        dist[i] = ok ? (double)INFINITY : -1.0;  // (a slot past N keeps -1: no d >= 0 is below it, and it never wins)
    }
    auto fold = [&](double sx, double sy, double sz) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const double dx = sx - px[i], dy = sy - py[i], dz = sz - pz[i];
            const double d = (dx * dx + dy * dy) + dz * dz;
            dist[i] = d < dist[i] ? d : dist[i];
        }
    };
#pragma unroll 4
    for (int q = 0; q < nseed; ++q) {
        const int sp = sel[q];
        fold((double)X[sp], (double)Y[sp], (double)Z[sp]);
    }
    // ---- farthest-point completion
    for (int j = nseed; j < K; ++j) {
        RankCand c{-1.0, 0, 0.f, 0.f, 0.f};
        double cx = 0.0, cy = 0.0, cz = 0.0;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const bool gt = dist[i] > c.d;  // ascending index within the thread: the first maximum (selects, not a branch)
            c.d = gt ? dist[i] : c.d;
            c.k = gt ? k0 + i : c.k;
            cx = gt ? px[i] : cx;
            cy = gt ? py[i] : cy;
            cz = gt ? pz[i] : cz;
        }
        c.x = (float)cx, c.y = (float)cy, c.z = (float)cz;  // (exact: the coordinates are fp32 values)
        const RankCand w = group_pick(S, j & 1, c);
        if (t == 0) {
            if (oi) oi[j] = w.k;
            if (o) o[j * 3 + 0] = w.x, o[j * 3 + 1] = w.y, o[j * 3 + 2] = w.z;
        }
        fold((double)w.x, (double)w.y, (double)w.z);
    }
}

size_t rank_lds_bytes(int N, int K)
{
    const int nsel = ((N < K ? N : K) + 1) & ~1;
    return sizeof(RankSlots) + (size_t)N * 16 + (size_t)nsel * 2;
}

// Measured (profiles/rank/rank_bench.txt, part 2): 512 threads beat 256 and 1024 both at 1024 points (2 per lane) and at 2048
// (4 per lane) -- fewer waves at the barrier cost more serial fp64 work per lane than they save.  8 per lane only where 4 do not fit.
int rank_ppt(int N) { return g_rank_ppt ? g_rank_ppt : N <= 1024 ? 2 : N <= 4096 ? 4 : 8; }

template <int PPT>
int rank_launch(int B, int N, int k, const float *xyz, int layout, const int *idx, float *out, int *out_idx, int *n_unique,
                hipStream_t st)
{
    static SnLdsAttrGrow attr;
    const size_t lds = rank_lds_bytes(N, k);
    if (int rc = sn_lds_attr_grow(attr, (const void *)rank_points_kernel<PPT>, lds, "sn_rank_points")) return rc;
    const int lanes = (N + PPT - 1) / PPT;
    const dim3 block((lanes + kWave - 1) / kWave * kWave);
    hipLaunchKernelGGL(rank_points_kernel<PPT>, dim3(B), block, lds, st, N, k, layout, xyz, idx, out, out_idx, n_unique);
    return 0;
}

}  // namespace
}  // namespace sn

using namespace sn;

// measurement hook (tools/rank_bench.py): points per lane 1, 2, 4 or 8 for every later call, 0 = chosen by N; returns the previous
// value, -1 for a bad one.  All give identical outputs.
extern "C" int sn_rank_points_set_ppt(int ppt)
{
    const int prev = g_rank_ppt;
    if (ppt != 0 && ppt != 1 && ppt != 2 && ppt != 4 && ppt != 8) return -1;
    g_rank_ppt = ppt;
    return prev;
}

// xyz (B,N,3) [SN_LAYOUT_BNC] or (B,3,N) [SN_LAYOUT_BCN]; idx (B,k) int32; out (B,k,3), out_idx (B,k), n_unique (B,) each optional.
// temp is not used (sn_workspace_bytes("rank_points", ...) is 0): everything a cloud needs lives in its workgroup's LDS.
extern "C" int sn_rank_points(int B, int N, int k, const float *xyz, int layout, const int *idx, float *temp, float *out,
                              int *out_idx, int *n_unique, sn_stream_t stream)
{
    (void)temp;
    SN_REQUIRE(B >= 0 && N >= 1 && k >= 1, "bad size");
    if (B == 0) return 0;
    SN_REQUIRE(layout == SN_LAYOUT_BNC || layout == SN_LAYOUT_BCN, "bad layout");
    if (k > kRankMaxK || N > kRankMaxN) return sn_set_error(SN_ERR_UNSUPPORTED, "sn_rank_points: k <= 8192 and N <= 8192");
    if (!(out || out_idx || n_unique)) return 0;
    SN_REQUIRE(xyz && idx, "null pointer");
    const int ppt = rank_ppt(N);
    if (N > kRankMaxThreads * ppt)
        return sn_set_error(SN_ERR_UNSUPPORTED, "sn_rank_points: %d points per lane do not take N = %d", ppt, N);
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    if (ppt == 1) rc = rank_launch<1>(B, N, k, xyz, layout, idx, out, out_idx, n_unique, st);
    else if (ppt == 2) rc = rank_launch<2>(B, N, k, xyz, layout, idx, out, out_idx, n_unique, st);
    else if (ppt == 4) rc = rank_launch<4>(B, N, k, xyz, layout, idx, out, out_idx, n_unique, st);
    else rc = rank_launch<8>(B, N, k, xyz, layout, idx, out, out_idx, n_unique, st);
    if (rc) return rc;
    SN_LAUNCH_CHECK();
    return 0;
}

// retrieval.hip -- all-against-all shape retrieval inside one labelled set, ranked and scored on the device (gfx950).  The reference
// names retrieval as the sampler's fourth application (README.md:13) and its classifier emits the descriptor
// (end_points["retrieval_vectors"], classification/models/pointnet_cls.py:111) but ships no script: the contract below is this
// project's own, restated in numpy by tests/retrieval_ref.py and pinned bit for bit by tests/test_gpu_retrieval.py.
//
// Contract.  desc (S,n,C) fp32: S descriptor sets over the same n shapes; labels (n) int32.  For every set s and query i:
//   d(i,j)   = sum_c (a_ic - a_jc)^2 in fp32 from the differences, products and sums uncontracted, in ONE fixed order: lane l of a
//              wave adds the channels c = l, l + 64, l + 128, .. in ascending order, then the 64 lane sums meet in a balanced tree of
//              adjacent pairs ((l0 + l1) + (l2 + l3)) + ..  Every term is symmetric in (i,j) and the order does not depend on them,
//              so d(i,j) == d(j,i) bit for bit, equal descriptors give exactly +0, and the same inputs give the same bits;
//   ranking  = all j != i ascending by (d(i,j), j): ties to the LOWER index (numpy's stable argsort with the query removed; the rule
//              of sn_knn and sn_furthest_point_sample).  Distances are sums of squares (>= +0 or NaN), whose bit patterns order as
//              unsigned integers, a NaN behind every number;
//   rel(j)   = labels[j] == labels[i];  R = number of relevant others;  H(r) = relevant among the first r ranks;
//   AP       = (sum over the relevant ranks r of H(r) / r) / R, every quotient and the sum in fp64, rounded ONCE to fp32;
//   prec[l]  = H(r*) / r* (one fp64 division, rounded to fp32) at the smallest r* with H(r*) >= t_l, t_l = (l R + L - 1) / L in integers
//              (= ceil(l R / L)), l = 1..L;
//   R == 0 (also n == 1): AP and every prec[l] are NaN, n_relevant 0.
//
// One workgroup per (set, Q consecutive queries), Q = 4 / 2 / 1 so that Q padded rows of 64-bit keys fill 64 KB of LDS whatever n:
//   * distances: a wave takes a gallery row, its lanes the channels (one coalesced 256-byte read per 64 channels, shared by the Q
//     queries), the lane sums meet by DPP -- the set streams from L2 once per Q queries;
//   * sort: keys (distance bits << 32 | index) in LDS, padded to a power of two with an all-ones sentinel that is above every real
//     key (the query's own slot holds the sentinel too: that is how it leaves the ranking), bitonic network, one barrier per stage;
//   * score: a thread owns a run of consecutive ranks, counts its relevant ones, one block scan gives H; the h-th relevant item at
//     rank r is r* of exactly the levels l with ceil(l R / L) == h, i.e. floor((h-1) L / R) < l <= floor(h L / R): every level is
//     written once, by the thread that holds its item, with no search.  The AP terms are added per thread in ascending rank, the
//     thread sums by the xor tree of a wave (offsets 32 .. 1), the wave sums in ascending order: one fixed order, all fp64.
// No workspace, no second launch, nothing shared between workgroups.
#include <cmath>

#include "sn_common.h"

#pragma clang fp contract(off)  // the contract's distance is product-then-sum (no FMA)

namespace sn {
namespace {

constexpr int kRetMaxN = 8192, kRetMaxL = 64, kRetMaxS = 65535;  // (S is the grid's y extent)
constexpr int kRetMaxThreads = 1024;
constexpr int kRetMaxWaves = kRetMaxThreads / kWave;
constexpr int kRetKeys = 8192;  // 64-bit keys per workgroup: Q rows of n2

// v + (v of the DPP-selected lane); rows outside ROWS add +0 (old operand 0)
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, false));
}

// The 64 lane values added as a balanced tree of adjacent pairs: lanes (0,1), quads, halves of 8, rows of 16, row pairs, the wave.
// fp32 addition commutes, so which operand a lane holds first does not matter.  Every lane active; the result is uniform.
__device__ __forceinline__ float wave_tree_sum(float v)
{
    v = dpp_add<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
    v = dpp_add<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);  // row_half_mirror: the other quad of the same 8 (a quad's lanes hold one value by now)
    v = dpp_add<0x140, 0xf>(v);  // row_mirror: the other half of the row
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3
    return readlane_f(v, 63);
}

// blockDim.x: a multiple of 64, <= 1024; grid (ceil(n / Q), S); dynamic LDS: Q * n2 keys; n2: the power of two >= max(n, 2)
template <int Q>
__global__ void __launch_bounds__(kRetMaxThreads) retrieval_kernel(int n, int C, int L, int n2, const float *__restrict__ desc,
                                                                   const int *__restrict__ labels, float *__restrict__ ap,
                                                                   float *__restrict__ prec, int *__restrict__ n_relevant,
                                                                   int *__restrict__ order, float *__restrict__ sorted_dist)
{
    extern __shared__ __align__(16) unsigned char s_raw[];
    sn_u64 *keys = reinterpret_cast<sn_u64 *>(s_raw);  // [Q][n2]
    __shared__ int s_cnt[kRetMaxWaves];
    __shared__ double s_ap[kRetMaxWaves];
    const int t = threadIdx.x, nt = blockDim.x, lane = t & (kWave - 1), wave = t / kWave, nw = nt / kWave;
    const int s = blockIdx.y, q0 = blockIdx.x * Q;
    const float *D = desc + (size_t)s * n * C;
    const float *aq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) aq[q] = D + (size_t)min(q0 + q, n - 1) * C;  // (a query past n repeats the last: computed, never scored)

    // ---- the Q rows of distances
    for (int j = wave; j < n; j += nw) {
        const float *aj = D + (size_t)j * C;
        float d[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) d[q] = 0.f;
        for (int c = lane; c < C; c += kWave) {
            const float x = aj[c];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float u = aq[q][c] - x;
                d[q] = d[q] + u * u;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float tot = wave_tree_sum(d[q]);
            if (lane == 0) keys[q * n2 + j] = j == q0 + q ? kKeyInf : make_key(tot, j);
        }
    }
    for (int j = n + t; j < n2; j += nt) {
#pragma unroll
        for (int q = 0; q < Q; ++q) keys[q * n2 + j] = kKeyInf;
    }
    __syncthreads();

    // ---- ascending bitonic sort of every row (the network of batch_assemble.hip): the n - 1 real keys end up in front
    const int half = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < Q * half; p += nt) {
                const int pp = p & (half - 1);
                sn_u64 *K = keys + (size_t)(p / half) * n2;
                const int i = ((pp & ~(j - 1)) << 1) | (pp & (j - 1)), l = i | j;
                const sn_u64 x = K[i], y = K[l];
                if ((x > y) == ((i & k) == 0)) K[i] = y, K[l] = x;
            }
            __syncthreads();
        }
    }

    // ---- the ranking out, and its score
    const int m = n - 1;  // ranks per query
    const int chunk = (m + nt - 1) / nt, p0 = t * chunk;  // this thread's ranks: p0 + 1 .. p0 + chunk (chunk <= 8: see the launch)
    for (int q = 0; q < Q; ++q) {
        const int i = q0 + q;
        if (i >= n) break;  // (block-uniform)
        const sn_u64 *K = keys + (size_t)q * n2;
        const size_t row = ((size_t)s * n + i) * m;
        if (order)
            for (int p = t; p < m; p += nt) order[row + p] = key_index(K[p]);
        if (sorted_dist)
            for (int p = t; p < m; p += nt) sorted_dist[row + p] = key_dist(K[p]);
        const bool want_count = n_relevant && s == 0;  // (the labels alone decide it: the first set's workgroups write it)
        if (!(ap || prec || want_count)) continue;

        const int li = labels[i];
        unsigned mask = 0;
        int cnt = 0;
        for (int k = 0; k < chunk; ++k) {
            const int p = p0 + k;
            const unsigned rel = p < m && labels[key_index(K[p])] == li ? 1u : 0u;
            mask |= rel << k;
            cnt += (int)rel;
        }
        int inc = cnt;  // inclusive scan over the wave, then the waves before this one
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int v = __shfl_up(inc, off);
            inc += lane >= off ? v : 0;
        }
        if (lane == kWave - 1) s_cnt[wave] = inc;
        __syncthreads();
        int h = inc - cnt, R = 0;
        for (int w = 0; w < nw; ++w) {
            const int c = s_cnt[w];
            R += c;
            h += w < wave ? c : 0;
        }
        float *pr = prec ? prec + ((size_t)s * n + i) * L : nullptr;
        double sum = 0.0;
        for (int k = 0; k < chunk; ++k) {
            if (!((mask >> k) & 1u)) continue;
            ++h;  // this item is the h-th relevant one, at rank p0 + k + 1
            const double v = (double)h / (double)(p0 + k + 1);
            sum += v;
            if (pr) {
                const int lo = ((h - 1) * L) / R + 1, hi = (h * L) / R;  // the levels with ceil(l R / L) == h
                for (int l = lo; l <= hi; ++l) pr[l - 1] = (float)v;
            }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) s_ap[wave] = sum;
        __syncthreads();
        if (t == 0) {
            double tot = 0.0;
            for (int w = 0; w < nw; ++w) tot += s_ap[w];
            if (ap) ap[(size_t)s * n + i] = R > 0 ? (float)(tot / (double)R) : NAN;
            if (want_count) n_relevant[i] = R;
        }
        if (pr && R == 0)
            for (int l = t; l < L; l += nt) pr[l] = NAN;
        __syncthreads();  // (s_cnt and s_ap serve the next query)
    }
}

template <int Q>
int retrieval_launch(int S, int n, int C, int L, int n2, const float *desc, const int *labels, float *ap, float *prec,
                     int *n_relevant, int *order, float *sorted_dist, hipStream_t st)
{
    static SnLdsAttr attr;
    if (int rc = sn_lds_attr(attr, (const void *)retrieval_kernel<Q>, (size_t)kRetKeys * sizeof(sn_u64), "sn_retrieval_metrics"))
        return rc;
    // a thread per pair of keys of one row, 64 at the least: a run of ceil((n - 1) / threads) <= 8 ranks per thread
    const int threads = n2 / 2 < kWave ? kWave : n2 / 2 > kRetMaxThreads ? kRetMaxThreads : n2 / 2;
    hipLaunchKernelGGL(retrieval_kernel<Q>, dim3((n + Q - 1) / Q, S), dim3(threads), (size_t)Q * n2 * sizeof(sn_u64), st, n, C, L, n2,
                       desc, labels, ap, prec, n_relevant, order, sorted_dist);
    return 0;
}

}  // namespace
}  // namespace sn

using namespace sn;

// desc (S,n,C), labels (n); ap (S,n), prec (S,n,L), n_relevant (n), order (S,n,n-1), sorted_dist (S,n,n-1), each optional.
// workspace is not used (sn_workspace_bytes("retrieval_metrics", ...) is 0): a query's keys live in its workgroup's LDS.
extern "C" int sn_retrieval_metrics(int S, int n, int C, const float *desc, const int *labels, int L, float *ap, float *prec,
                                    int *n_relevant, int *order, float *sorted_dist, void *workspace, sn_stream_t stream)
{
    (void)workspace;
    SN_REQUIRE(S >= 0 && n >= 0 && C >= 1 && L >= 1, "bad size");
    if (n > kRetMaxN || L > kRetMaxL || S > kRetMaxS)
        return sn_set_error(SN_ERR_UNSUPPORTED, "sn_retrieval_metrics: n <= %d, L <= %d and S <= %d (got n = %d, L = %d, S = %d)",
                            kRetMaxN, kRetMaxL, kRetMaxS, n, L, S);
    if (S == 0 || n == 0) return 0;
    if (!(ap || prec || n_relevant || order || sorted_dist)) return 0;
    SN_REQUIRE(desc, "null pointer");
    SN_REQUIRE(labels || !(ap || prec || n_relevant), "the scores need the labels");
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    if (n2 * 4 <= kRetKeys) rc = retrieval_launch<4>(S, n, C, L, n2, desc, labels, ap, prec, n_relevant, order, sorted_dist, st);
    else if (n2 * 2 <= kRetKeys) rc = retrieval_launch<2>(S, n, C, L, n2, desc, labels, ap, prec, n_relevant, order, sorted_dist, st);
    else rc = retrieval_launch<1>(S, n, C, L, n2, desc, labels, ap, prec, n_relevant, order, sorted_dist, st);
    if (rc) return rc;
    SN_LAUNCH_CHECK();
    return 0;
}

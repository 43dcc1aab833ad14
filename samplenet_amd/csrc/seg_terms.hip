// seg_terms.hip -- the per-point (segmentation) loss and prediction terms: softmax cross-entropy with ignored labels and class
// weights (torch's F.cross_entropy(weight=, ignore_index=), reduction 'none' and 'mean'), numpy's argmax, and the per-cloud,
// per-class counts every IoU / accuracy figure is formed from.  R = B * N rows of C logits; cls_terms.hip serves tens of rows with a
// wave per row, this unit serves 10^5 rows of 13 .. 50 classes.
//
// MAPPING.  A LANE GROUP of G lanes owns a row, G = the power of two covering C, at most 64 (C = 13: 16 lanes, C = 50: 64); lane l
// of the group takes the classes l, l + G, ... ascending (more than one only when C > 64).  A workgroup is 256 threads = 256 / G
// groups and takes kSegPasses = 4 passes: workgroup g owns the rows [g * RB, (g + 1) * RB), RB = 4 * 256 / G, and in pass p the group
// q takes row g * RB + p * (256 / G) + q -- a wave's groups take consecutive rows, its loads are one contiguous run.  Which rows a
// workgroup owns depends on R and C alone, never on the device.  The row is read once (C <= 64: it lives in one register per lane).
// Counts: integers.  A workgroup whose rows lie in at most two clouds (rows_per_cloud >= RB) and C <= 128 counts in LDS (integer
// atomics, exact in any order) and adds its non-zero slots to cloud_counts with global integer atomics; otherwise a group's first
// lane adds straight to cloud_counts.  The entry clears cloud_counts on the stream first.  No float atomics anywhere.
// Batch sums: per-workgroup partials in `workspace` (num[g], den[g], valid[g], correct[g]) and a CLOSING LAUNCH of one workgroup on
// the same stream -- no arrival counter, no ticket, no cross-workgroup barrier.
//
// ORDER OF THE FP32 OPERATIONS (compiled with -ffp-contract=off; tests/seg_terms_ref.py counts its bounds from this text):
//   m   = max_c x_c: per lane in ascending class order with a strict >, then the xor butterfly over the group's lanes (offsets
//         G / 2, .., 1), ties to the lower class: the FIRST maximum, numpy's argmax.  A NaN logit never enters the maximum; the
//         smallest class index holding a NaN is carried beside it (integer min) and, when there is one, IS the prediction.
//   s   = sum_c expf(x_c - m): one subtraction and one expf per class; a lane adds its terms in ascending class order starting
//         from 0.0f, the lanes combine by the xor butterfly (offsets G / 2, .., 1; every lane ends with the same bits).
//   ce  = (logf(s) + m) - x_label on a valid row (0 <= label < C), NaN if the row holds a NaN logit; exactly 0.0f on an ignored row.
//   t   = w_label * ce (ce itself without weights) and w_label (1 without weights) of a valid row; an ignored row adds nothing.
//   partial num[g] (and den[g] with weights): a group adds its passes' t (w_label) ascending from 0.0f (4 additions); the wave adds
//         its groups' sums by the 64-lane xor butterfly (offsets 32, .., 1; lanes that are not a group's first hold 0.0f); thread 0
//         adds the 4 wave sums ascending from 0.0f.  valid[g], correct[g]: integers.
//   closing launch: thread t of 256 adds the partials t, t + 256, ... ascending from 0.0f; the wave's 64 sums combine by the xor
//         butterfly (offsets 32, .., 1); thread 0 adds the 4 wave sums ascending from 0.0f -> num, den.  Without weights
//         den = (float)valid (one conversion).  means[0] = num / den; means[1] = (float)correct / (float)valid, 0 when valid = 0;
//         means[2] = den.
//   backward: k_r = (g_means[0] * w_label) / means[2] + g_ce[r] (w_label = 1: g_means[0] / means[2]; a NULL part is left out, not
//         added as zero);  p_c = expf(x_c - m) / s (m, s as above);  g_logits[r][c] = k_r * (p_c - (c == label ? 1.0f : 0.0f));
//         an ignored row is written as 0.0f without arithmetic.
#pragma clang fp contract(off)
#include "sn_common.h"

namespace {

constexpr int kSegThreads = 256;
constexpr int kSegPasses = 4;
constexpr int kSegLdsClasses = 128;  // the LDS counting route: C <= this and a workgroup's rows in at most two clouds
constexpr int kNone = 0x7fffffff;

inline int seg_group_lanes(int C)
{
    int g = 1;
    while (g < C && g < 64) g <<= 1;
    return g;
}
inline long long seg_rows_per_block(int C) { return (long long)kSegPasses * (kSegThreads / seg_group_lanes(C)); }
inline long long seg_blocks(long long R, int C)
{
    const long long rb = seg_rows_per_block(C);
    return (R + rb - 1) / rb;
}

// m, the first-maximum index, the first NaN index (kNone: none) and s of one row; every lane of the group returns the same values.
// l: the lane's index in its group; v0: the lane's first class x[l] (0 when l >= C or the row is past R); x is only read for the
// classes l + G, l + 2 G, .. (C > 64).  Groups whose row is past R pass C = 0 classes' worth of data through the same shuffles.
template <int G>
__device__ __forceinline__ void seg_row_stats(const float *__restrict__ x, const int C, const int l, const float v0, float &m,
                                              int &am, int &nan_at, float &s)
{
    float best = -INFINITY;
    int arg = l < C ? l : kNone, nanc = kNone;
    if (l < C) {
        if (v0 > best) best = v0;                 // (arg is the lane's first class already)
        if (v0 != v0) nanc = l;
    }
    if (G == 64)
        for (int c = l + 64; c < C; c += 64) {
            const float v = x[c];
            if (v > best) best = v, arg = c;      // strict: the first maximum of the lane's ascending classes
            if (v != v) nanc = min(nanc, c);
        }
#pragma unroll
    for (int ofs = G / 2; ofs > 0; ofs >>= 1) {
        const float ob = __shfl_xor(best, ofs);
        const int oa = __shfl_xor(arg, ofs);
        const int on = __shfl_xor(nanc, ofs);
        if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
        nanc = min(nanc, on);
    }
    float acc = 0.0f;
    if (l < C) acc = acc + expf(v0 - best);
    if (G == 64)
        for (int c = l + 64; c < C; c += 64) acc = acc + expf(x[c] - best);
#pragma unroll
    for (int ofs = G / 2; ofs > 0; ofs >>= 1) acc = acc + __shfl_xor(acc, ofs);
    m = best, am = arg, nan_at = nanc, s = acc;
}

// the 64-lane sum of the xor butterfly, offsets 32 .. 1
__device__ __forceinline__ float seg_wave_sum(float v)
{
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v = v + __shfl_xor(v, ofs);
    return v;
}
__device__ __forceinline__ int seg_wave_sum(int v)
{
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v += __shfl_xor(v, ofs);
    return v;
}

template <int G>
__global__ void __launch_bounds__(kSegThreads) seg_terms_fwd_kernel(long long R, int rows_per_cloud, int C,
                                                                    const float *__restrict__ logits, const int *__restrict__ labels,
                                                                    const float *__restrict__ class_weights, float *__restrict__ ce,
                                                                    int *__restrict__ pred, int *__restrict__ cloud_counts,
                                                                    float *__restrict__ part_num, float *__restrict__ part_den,
                                                                    int *__restrict__ part_valid, int *__restrict__ part_correct,
                                                                    int lds_counts)
{
    constexpr int kGroups = kSegThreads / G;
    __shared__ int s_cnt[2 * kSegLdsClasses * 3];
    __shared__ float s_num[4], s_den[4];
    __shared__ int s_val[4], s_cor[4];
    const int l = threadIdx.x & (G - 1), q = threadIdx.x / G, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * (kSegPasses * kGroups);
    const long long cloud0 = row0 / rows_per_cloud;
    const long long clouds = R / rows_per_cloud;
    if (cloud_counts && lds_counts) {
        for (int i = threadIdx.x; i < 2 * C * 3; i += kSegThreads) s_cnt[i] = 0;
        __syncthreads();
    }
    float gnum = 0.0f, gden = 0.0f;
    int gval = 0, gcor = 0;
#pragma unroll
    for (int p = 0; p < kSegPasses; ++p) {
        const long long r = row0 + p * kGroups + q;
        const bool live = r < R;
        const float *x = logits + (live ? r : 0) * C;
        const float v0 = live && l < C ? x[l] : 0.0f;
        const int label = live ? labels[r] : -1;
        const bool valid = label >= 0 && label < C;  // every other label is ignored and never indexes the row or the weights
        const float xl = valid ? x[label] : 0.0f;
        const float w = valid && class_weights ? class_weights[label] : 1.0f;
        float m, s;
        int am, nan_at;
        seg_row_stats<G>(x, live ? C : 0, l, v0, m, am, nan_at, s);
        const int pr = nan_at != kNone ? nan_at : am;
        float v = 0.0f;
        if (valid) v = nan_at == kNone ? (logf(s) + m) - xl : NAN;
        const int ok = valid && pr == label ? 1 : 0;
        if (l == 0 && live) {
            if (ce) ce[r] = v;
            if (pred) pred[r] = pr;
            if (valid) {
                gnum = gnum + (class_weights ? w * v : v);
                gden = gden + w;
                gval += 1, gcor += ok;
                if (cloud_counts) {
                    const long long cloud = r / rows_per_cloud;
                    if (lds_counts) {
                        int *c3 = s_cnt + (int)(cloud - cloud0) * C * 3;
                        atomicAdd(c3 + label * 3 + 0, 1);
                        atomicAdd(c3 + pr * 3 + 1, 1);
                        if (ok) atomicAdd(c3 + label * 3 + 2, 1);
                    } else {
                        int *c3 = cloud_counts + cloud * C * 3;
                        atomicAdd(c3 + label * 3 + 0, 1);
                        atomicAdd(c3 + pr * 3 + 1, 1);
                        if (ok) atomicAdd(c3 + label * 3 + 2, 1);
                    }
                }
            }
        }
    }
    if (cloud_counts && lds_counts) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * C * 3; i += kSegThreads) {
            const int n = s_cnt[i];
            const long long cloud = cloud0 + i / (C * 3);
            if (n != 0 && cloud < clouds) atomicAdd(cloud_counts + cloud0 * C * 3 + i, n);
        }
    }
    if (!part_num) return;
    // (lanes that are not a group's first hold zeros: their additions are exact)
    const float wnum = seg_wave_sum(gnum), wden = seg_wave_sum(gden);
    const int wval = seg_wave_sum(gval), wcor = seg_wave_sum(gcor);
    if ((threadIdx.x & 63) == 0) s_num[wave] = wnum, s_den[wave] = wden, s_val[wave] = wval, s_cor[wave] = wcor;
    __syncthreads();
    if (threadIdx.x == 0) {
        float num = 0.0f, den = 0.0f;
        int val = 0, cor = 0;
        for (int w = 0; w < 4; ++w) num = num + s_num[w], den = den + s_den[w], val += s_val[w], cor += s_cor[w];
        part_num[blockIdx.x] = num, part_den[blockIdx.x] = den, part_valid[blockIdx.x] = val, part_correct[blockIdx.x] = cor;
    }
}

__global__ void __launch_bounds__(kSegThreads) seg_terms_close_kernel(int nblk, const float *__restrict__ part_num,
                                                                      const float *__restrict__ part_den,
                                                                      const int *__restrict__ part_valid,
                                                                      const int *__restrict__ part_correct, int weighted,
                                                                      float *__restrict__ means)
{
    __shared__ float s_num[4], s_den[4];
    __shared__ long long s_val[4], s_cor[4];
    float num = 0.0f, den = 0.0f;
    long long val = 0, cor = 0;
    for (int i = threadIdx.x; i < nblk; i += kSegThreads)
        num = num + part_num[i], den = den + part_den[i], val += part_valid[i], cor += part_correct[i];
    num = seg_wave_sum(num), den = seg_wave_sum(den);
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) val += __shfl_xor(val, ofs), cor += __shfl_xor(cor, ofs);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_num[wave] = num, s_den[wave] = den, s_val[wave] = val, s_cor[wave] = cor;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tn = 0.0f, td = 0.0f;
        long long tv = 0, tc = 0;
        for (int w = 0; w < 4; ++w) tn = tn + s_num[w], td = td + s_den[w], tv += s_val[w], tc += s_cor[w];
        if (!weighted) td = (float)tv;
        means[0] = tn / td;
        means[1] = tv > 0 ? (float)tc / (float)tv : 0.0f;
        means[2] = td;
    }
}

template <int G>
__global__ void __launch_bounds__(kSegThreads) seg_terms_bwd_kernel(long long R, int C, const float *__restrict__ logits,
                                                                    const int *__restrict__ labels,
                                                                    const float *__restrict__ class_weights,
                                                                    const float *__restrict__ means, const float *__restrict__ g_means,
                                                                    const float *__restrict__ g_ce, float *__restrict__ g_logits)
{
    constexpr int kGroups = kSegThreads / G;
    const int l = threadIdx.x & (G - 1), q = threadIdx.x / G;
    const long long row0 = (long long)blockIdx.x * (kSegPasses * kGroups);
    const float gm = g_means ? g_means[0] : 0.0f, den = g_means ? means[2] : 1.0f;
#pragma unroll
    for (int p = 0; p < kSegPasses; ++p) {
        const long long r = row0 + p * kGroups + q;
        const bool live = r < R;
        const float *x = logits + (live ? r : 0) * C;
        const float v0 = live && l < C ? x[l] : 0.0f;
        const int label = live ? labels[r] : -1;
        const bool valid = label >= 0 && label < C;
        float k = 0.0f;
        if (valid) {
            if (g_means) k = class_weights ? (gm * class_weights[label]) / den : gm / den;
            if (g_ce) k = g_means ? k + g_ce[r] : g_ce[r];
        }
        float m, s;
        int am, nan_at;
        seg_row_stats<G>(x, live ? C : 0, l, v0, m, am, nan_at, s);
        if (!live) continue;
        float *g = g_logits + r * C;
        for (int c = l; c < C; c += G) {
            const float pc = expf((c == l ? v0 : x[c]) - m) / s;
            g[c] = valid ? k * (pc - (c == label ? 1.0f : 0.0f)) : 0.0f;
        }
    }
}

template <int G>
void seg_launch_fwd(int nblk, hipStream_t st, long long R, int rpc, int C, const float *logits, const int *labels, const float *cw,
                    float *ce, int *pred, int *counts, float *pn, float *pd, int *pv, int *pc, int lds)
{
    hipLaunchKernelGGL(seg_terms_fwd_kernel<G>, dim3(nblk), dim3(kSegThreads), 0, st, R, rpc, C, logits, labels, cw, ce, pred, counts, pn,
                       pd, pv, pc, lds);
}
template <int G>
void seg_launch_bwd(int nblk, hipStream_t st, long long R, int C, const float *logits, const int *labels, const float *cw,
                    const float *means, const float *g_means, const float *g_ce, float *g_logits)
{
    hipLaunchKernelGGL(seg_terms_bwd_kernel<G>, dim3(nblk), dim3(kSegThreads), 0, st, R, C, logits, labels, cw, means, g_means, g_ce,
                       g_logits);
}

#define SEG_DISPATCH(G, CALL)      \
    switch (G) {                   \
    case 1: CALL(1); break;        \
    case 2: CALL(2); break;        \
    case 4: CALL(4); break;        \
    case 8: CALL(8); break;        \
    case 16: CALL(16); break;      \
    case 32: CALL(32); break;      \
    default: CALL(64); break;      \
    }

}  // namespace

extern "C" long long sn_segmentation_terms_workspace_bytes(long long R, int C)
{
    if (R < 0 || C < 1 || R * (long long)C >= (1ll << 31)) return -1;
    return seg_blocks(R, C) * 16;
}

extern "C" int sn_segmentation_terms_forward(long long R, int rows_per_cloud, int C, const float *logits, const int *labels,
                                             const float *class_weights, float *ce, int *pred, int *cloud_counts, float *means,
                                             void *workspace, sn_stream_t stream)
{
    SN_REQUIRE(R >= 0 && C >= 1 && rows_per_cloud >= 1, "bad size");
    SN_REQUIRE(R % rows_per_cloud == 0, "rows_per_cloud does not divide R");
    SN_REQUIRE(R * (long long)C < (1ll << 31), "R * C must stay below 2^31");
    if (R == 0 || !(ce || pred || cloud_counts || means)) return 0;
    SN_REQUIRE(logits && labels, "null pointer");
    SN_REQUIRE(!means || workspace, "means needs the workspace of sn_segmentation_terms_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)seg_blocks(R, C), G = seg_group_lanes(C);
    if (cloud_counts) {
        const hipError_t e = hipMemsetAsync(cloud_counts, 0, (size_t)(R / rows_per_cloud) * C * 3 * sizeof(int), st);
        if (e != hipSuccess) return sn_set_error((int)e, "%s: %s", __func__, hipGetErrorString(e));
    }
    float *pn = means ? (float *)workspace : nullptr, *pd = pn ? pn + nblk : nullptr;
    int *pv = pn ? (int *)(pd + nblk) : nullptr, *pc = pn ? pv + nblk : nullptr;
    const int lds = C <= kSegLdsClasses && rows_per_cloud >= seg_rows_per_block(C) ? 1 : 0;
#define SEG_FWD(GG) seg_launch_fwd<GG>(nblk, st, R, rows_per_cloud, C, logits, labels, class_weights, ce, pred, cloud_counts, pn, pd, pv, pc, lds)
    SEG_DISPATCH(G, SEG_FWD)
#undef SEG_FWD
    SN_LAUNCH_CHECK();
    if (means) {
        hipLaunchKernelGGL(seg_terms_close_kernel, dim3(1), dim3(kSegThreads), 0, st, nblk, pn, pd, pv, pc, class_weights ? 1 : 0, means);
        SN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int sn_segmentation_terms_backward(long long R, int C, const float *logits, const int *labels, const float *class_weights,
                                              const float *means, const float *g_means, const float *g_ce, float *g_logits,
                                              sn_stream_t stream)
{
    SN_REQUIRE(R >= 0 && C >= 1, "bad size");
    SN_REQUIRE(R * (long long)C < (1ll << 31), "R * C must stay below 2^31");
    if (R == 0) return 0;
    SN_REQUIRE(logits && labels && g_logits, "null pointer");
    SN_REQUIRE(!g_means || means, "g_means needs the forward's means");
    const int nblk = (int)seg_blocks(R, C), G = seg_group_lanes(C);
#define SEG_BWD(GG) seg_launch_bwd<GG>(nblk, (hipStream_t)stream, R, C, logits, labels, class_weights, means, g_means, g_ce, g_logits)
    SEG_DISPATCH(G, SEG_BWD)
#undef SEG_BWD
    SN_LAUNCH_CHECK();
    return 0;
}

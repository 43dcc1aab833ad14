// cls_terms.hip -- the classification task's loss and prediction terms in one launch per direction:
// tf.nn.sparse_softmax_cross_entropy_with_logits + its batch mean (classification/models/pointnet_cls.py:117-122) and the
// prediction / accuracy of the evaluation (classification/evaluate_samplenet.py:237-262: np.argmax, correct, the per-item loss).
//
// MAPPING.  One wave per row, the 64 lanes striding the classes (lane l takes classes l, l + 64, ... in ascending order); a
// workgroup is 16 waves (1024 threads), wave w of workgroup g takes rows (g * 16 + w), + 16 * gridDim.x, ...  The forward with
// `means` runs as ONE workgroup (its waves walk the batch: classification batches are tens of rows) so that the batch sums have
// one fixed order without a second launch, persistent counters or atomics; without `means`, and in the backward, rows are
// independent and the grid covers the batch.
//
// ORDER OF THE FP32 OPERATIONS (compiled with -ffp-contract=off; tests/cls_terms_ref.py counts its bounds from this text):
//   m   = max_c x_c: per lane in ascending class order with a strict >, then the xor butterfly over the lanes (offsets 32, 16, ..
//         1), ties to the lower class: the FIRST maximum, numpy's argmax.  A NaN logit never enters the maximum; the smallest
//         class index holding a NaN is carried beside it (integer min) and, when there is one, IS the prediction (numpy's argmax
//         returns the first NaN) and ce = NaN.
//   s   = sum_c expf(x_c - m): one subtraction and one expf per class; a lane adds its terms in ascending class order starting
//         from 0.0f, the lanes combine by the xor butterfly (offsets 32, 16, .. 1; every lane ends with the same bits).
//   ce  = (logf(s) + m) - x_label.
//   means[0] = (sum_b ce[b]) / (float)B: wave w adds its rows' ce in ascending row order from 0.0f, thread 0 adds the 16 wave
//         sums in ascending wave order from 0.0f, one division.  means[1] = (float)(number of correct rows) / (float)B: the count is
//         an integer (exact), one conversion and one division.
//   backward: w_b = g_means[0] / (float)B + g_ce[b] (a NULL part is left out, not added as zero);
//         p_c = expf(x_c - m) / s (m, s as above);  g_logits[b][c] = w_b * (p_c - (c == label ? 1.0f : 0.0f)).
#pragma clang fp contract(off)
#include "sn_common.h"

namespace {

constexpr int kClsWaves = 16;
constexpr int kClsThreads = kClsWaves * 64;

// m, the first-maximum index, the first NaN index (INT_MAX: none) and s of one row; every lane returns the same values.  v0 is the
// lane's first class x[lane] (0 when lane >= C), loaded once by the caller and used by both passes: the row is read once when
// C <= 64 and the caller's other loads (label, x[label], upstream) are in flight beside it instead of behind the reductions.
__device__ __forceinline__ void cls_row_stats(const float *__restrict__ x, const int C, const int lane, const float v0, float &m,
                                              int &am, int &nan_at, float &s)
{
    float best = -INFINITY;
    int arg = lane < C ? lane : 0x7fffffff, nanc = 0x7fffffff;
    if (lane < C) {
        if (v0 > best) best = v0;                 // (arg is the lane's first class already)
        if (v0 != v0) nanc = lane;
    }
    for (int c = lane + 64; c < C; c += 64) {
        const float v = x[c];
        if (v > best) best = v, arg = c;          // strict: the first maximum of the lane's ascending classes
        if (v != v) nanc = min(nanc, c);
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        const float ob = __shfl_xor(best, ofs);
        const int oa = __shfl_xor(arg, ofs);
        const int on = __shfl_xor(nanc, ofs);
        if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
        nanc = min(nanc, on);
    }
    float acc = 0.0f;
    if (lane < C) acc = acc + expf(v0 - best);
    for (int c = lane + 64; c < C; c += 64) acc = acc + expf(x[c] - best);
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) acc = acc + __shfl_xor(acc, ofs);
    m = best, am = arg, nan_at = nanc, s = acc;
}

__global__ void __launch_bounds__(kClsThreads) cls_terms_fwd_kernel(int B, int C, const float *__restrict__ logits,
                                                                    const int *__restrict__ labels, float *__restrict__ ce,
                                                                    int *__restrict__ pred, int *__restrict__ correct,
                                                                    float *__restrict__ means)
{
    __shared__ float s_sum[kClsWaves];
    __shared__ int s_cnt[kClsWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wsum = 0.0f;
    int wcnt = 0;
    for (int b = blockIdx.x * kClsWaves + wave; b < B; b += gridDim.x * kClsWaves) {
        const float *x = logits + (size_t)b * C;
        const float v0 = lane < C ? x[lane] : 0.0f;
        const int label = labels[b];
        const bool inside = label >= 0 && label < C;  // a label outside [0, C) never indexes the row
        const float xl = inside ? x[label] : 0.0f;
        float m, s;
        int am, nan_at;
        cls_row_stats(x, C, lane, v0, m, am, nan_at, s);
        const int p = nan_at != 0x7fffffff ? nan_at : am;
        float v = NAN;
        if (inside && nan_at == 0x7fffffff) v = (logf(s) + m) - xl;
        const int ok = inside && p == label ? 1 : 0;
        if (lane == 0) {
            if (ce) ce[b] = v;
            if (pred) pred[b] = p;
            if (correct) correct[b] = ok;
        }
        wsum = wsum + v, wcnt += ok;
    }
    if (!means) return;  // (the host launches ONE workgroup when the means are wanted)
    if (lane == 0) s_sum[wave] = wsum, s_cnt[wave] = wcnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        int cnt = 0;
        for (int w = 0; w < kClsWaves; ++w) tot = tot + s_sum[w], cnt += s_cnt[w];
        means[0] = tot / (float)B;
        means[1] = (float)cnt / (float)B;
    }
}

__global__ void __launch_bounds__(kClsThreads) cls_terms_bwd_kernel(int B, int C, const float *__restrict__ logits,
                                                                    const int *__restrict__ labels, const float *__restrict__ g_means,
                                                                    const float *__restrict__ g_ce, float *__restrict__ g_logits)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x * kClsWaves + wave; b < B; b += gridDim.x * kClsWaves) {
        const float *x = logits + (size_t)b * C;
        float *g = g_logits + (size_t)b * C;
        const float v0 = lane < C ? x[lane] : 0.0f;
        const int label = labels[b];
        float w = 0.0f;
        if (g_means && g_ce) w = g_means[0] / (float)B + g_ce[b];
        else if (g_means) w = g_means[0] / (float)B;
        else if (g_ce) w = g_ce[b];
        if (label < 0 || label >= C) w = NAN;  // a bad label: the whole row NaN
        float m, s;
        int am, nan_at;
        cls_row_stats(x, C, lane, v0, m, am, nan_at, s);
        for (int c = lane; c < C; c += 64) {
            const float p = expf((c == lane ? v0 : x[c]) - m) / s;
            g[c] = w * (p - (c == label ? 1.0f : 0.0f));
        }
    }
}

}  // namespace

extern "C" int sn_classification_terms_forward(int B, int C, const float *logits, const int *labels, float *ce, int *pred,
                                               int *correct, float *means, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && C >= 1, "bad size");
    if (B == 0 || !(ce || pred || correct || means)) return 0;
    SN_REQUIRE(logits && labels, "null pointer");
    const int groups = means ? 1 : min((B + kClsWaves - 1) / kClsWaves, 1024);
    hipLaunchKernelGGL(cls_terms_fwd_kernel, dim3(groups), dim3(kClsThreads), 0, (hipStream_t)stream, B, C, logits, labels, ce, pred,
                       correct, means);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_classification_terms_backward(int B, int C, const float *logits, const int *labels, const float *g_means,
                                                const float *g_ce, float *g_logits, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && C >= 1, "bad size");
    if (B == 0) return 0;
    SN_REQUIRE(logits && labels && g_logits, "null pointer");
    const int groups = min((B + kClsWaves - 1) / kClsWaves, 1024);
    hipLaunchKernelGGL(cls_terms_bwd_kernel, dim3(groups), dim3(kClsThreads), 0, (hipStream_t)stream, B, C, logits, labels, g_means,
                       g_ce, g_logits);
    SN_LAUNCH_CHECK();
    return 0;
}

// soft_projection.hip -- SoftProjection's backward and the small gather / scatter ops of the hot path (gfx950).
//
//   soft_project_backward fused backward of SoftProjection.project (soft_projection.py:138-152)
//   soft_weights_*, weighted_gather_*   the same math split at the weights, for the
//                         propagate / project_and_propagate actions (soft_projection.py:101-136)
//   group_point*, grouping_operation*   tf_grouping_g.cu:40-78 and the pointnet2 layout twin
#pragma clang fp contract(off)  // reference arithmetic is product-then-sum (no FMA)

#include <algorithm>

#include "chamfer_owner.h"
#include "soft_query.h"

namespace sn {

template <bool FUSED>
__global__ void __launch_bounds__(256) soft_bwd_kernel(SoftBwdArgs a)
{
    __shared__ float s_part[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x;
    const int n = a.n, m = a.m;
    const float *__restrict__ Pb = a.P + (size_t)b * 3 * n;
    const float *__restrict__ Qb = a.Q + (size_t)b * 3 * m;
    const float T = *a.temperature;
    const float sigma = sn_sigma(T, a.min_sigma);
    float gsig = 0.f;  // this wave's share of d loss / d sigma

    for (int j = blockIdx.y * nwaves + wave; j < m; j += gridDim.y * nwaves) {
        float aqx, aqy, aqz, asg;
        soft_bwd_query<FUSED>(a, b, j, lane, sigma, Pb, Qb, aqx, aqy, aqz, asg);
        gsig += asg;
        if (a.grad_Q && lane < 3) {
            const float o = lane == 0 ? aqx : (lane == 1 ? aqy : aqz);
            float *dst = a.grad_Q + (size_t)b * 3 * m + pt_off(a.gq_layout, m, j, lane);
            *dst = a.accumulate_q ? *dst + o : o;
        }
    }
    // fixed-order block reduction of the sigma gradient: wave 0..3 in order
    if (lane == 0) s_part[wave] = gsig;
    __syncthreads();
    if (threadIdx.x == 0 && a.grad_sigma_partial) {
        float tot = 0.f;
        for (int w2 = 0; w2 < nwaves; ++w2) tot += s_part[w2];
        a.grad_sigma_partial[(size_t)b * gridDim.y + blockIdx.y] = tot;
    }
}

void launch_soft_bwd_fused(int b, int splits, const SoftBwdArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(soft_bwd_kernel<true>, dim3(b, splits), dim3(256), 0, st, a);
}

// softmax weights alone (split path)
__global__ void __launch_bounds__(256) soft_weights_fwd_kernel(int n, int m, int K, const float *__restrict__ P,
                                                               const float *__restrict__ Q,
                                                               const int *__restrict__ idx,
                                                               const float *__restrict__ temperature,
                                                               float min_sigma, float *__restrict__ weights)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x;
    const float *Pb = P + (size_t)b * 3 * n, *Qb = Q + (size_t)b * 3 * m;
    const float T = *temperature;
    const float sigma = sn_sigma(T, min_sigma);
    for (int j = blockIdx.y * nwaves + wave; j < m; j += gridDim.y * nwaves) {
        const bool act = lane < K;
        const int id = act ? idx[((size_t)b * m + j) * K + lane] : 0;
        const float dx = (act ? Pb[id] : 0.f) - Qb[j];
        const float dy = (act ? Pb[n + id] : 0.f) - Qb[m + j];
        const float dz = (act ? Pb[2 * n + id] : 0.f) - Qb[2 * m + j];
        const float d = (dx * dx + dy * dy) + dz * dz;
        const float s = act ? -(d / sigma) : -INFINITY;
        float mx = s;
#pragma unroll
        for (int t = 1; t < 64; t <<= 1) mx = fmaxf(mx, __shfl_xor(mx, t));
        const float e = act ? expf(s - mx) : 0.f;
        float den = 0.f;
        for (int t = 0; t < K; ++t) den += readlane_f(e, t);
        if (act) weights[((size_t)b * m + j) * K + lane] = e / den;
    }
}

// out[b,c,j] = sum_t w[b,j,t] * X[b,c,idx[b,j,t]]   (ascending t, product then sum)
__global__ void __launch_bounds__(256) weighted_gather_fwd_kernel(int c, int n, int m, int K,
                                                                  const float *__restrict__ X,
                                                                  const int *__restrict__ idx,
                                                                  const float *__restrict__ w,
                                                                  float *__restrict__ out)
{
    const int b = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over c*m
    if (e >= (size_t)c * m) return;
    const int ch = (int)(e / m), j = (int)(e % m);
    const float *Xc = X + ((size_t)b * c + ch) * n;
    const int *id = idx + ((size_t)b * m + j) * K;
    const float *wj = w + ((size_t)b * m + j) * K;
    float acc = 0.f;
    for (int t = 0; t < K; ++t) acc += Xc[id[t]] * wj[t];
    out[((size_t)b * c + ch) * m + j] = acc;
}

// grad_w[b,j,t] = sum_c go[b,c,j] X[b,c,idx];  grad_X[b,c,idx] += go[b,c,j] w[b,j,t]  (atomics)
__global__ void __launch_bounds__(256) weighted_gather_bwd_kernel(int c, int n, int m, int K,
                                                                  const float *__restrict__ X,
                                                                  const int *__restrict__ idx,
                                                                  const float *__restrict__ w,
                                                                  const float *__restrict__ go,
                                                                  float *__restrict__ gw, float *__restrict__ gX,
                                                                  float *__restrict__ contrib = nullptr)
{
    const int b = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over m*K
    if (e >= (size_t)m * K) return;
    const int j = (int)(e / K);
    const int id = idx[(size_t)b * m * K + e];
    const float wt = w[(size_t)b * m * K + e];
    float acc = 0.f;
    for (int ch = 0; ch < c; ++ch) {
        const float g = go[((size_t)b * c + ch) * m + j];
        acc += g * X[((size_t)b * c + ch) * n + id];
        if (contrib) contrib[((size_t)b * c + ch) * m * K + e] = g * wt;  // (b, c, m k): summed in entry order afterwards
        else if (gX) atomicAdd(&gX[((size_t)b * c + ch) * n + id], g * wt);
    }
    if (gw) gw[(size_t)b * m * K + e] = acc;
}

// ------------------------------------------------------------------------------------------------
// group_point (TF layout) and grouping_operation (channel-major layout)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) group_point_kernel(int n, int c, int m, int ns, const float *__restrict__ points,
                                                          const int *__restrict__ idx, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const size_t tot = (size_t)m * ns * c;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(e % c);
        const size_t jk = e / c;
        const int ii = idx[(size_t)b * m * ns + jk];
        out[(size_t)b * tot + e] = points[((size_t)b * n + ii) * c + l];
    }
}

// Gradient of the two gathers: dst row r = sum of the src entries e whose index names r, added in ASCENDING entry order -- the
// order of the reference's CPU loops (tf_grouping.cpp's group_point_grad_cpu; its GPU kernels, tf_grouping_g.cu:60-78, use
// unordered float atomics), hence deterministic and bit-identical to the oracle.  A thread owns one destination row and walks
// the cloud's ne = m * nsample indices adding the rare hits; no atomics, no memset (every row is written).  Indices outside
// [0, n) name no row and are ignored.
//   CHANNEL_MAJOR = false: src (ne, c) / dst (n, c)  [group_point];  true: src (c, ne) / dst (c, n)  [grouping_operation]
template <bool CHANNEL_MAJOR>
__global__ void __launch_bounds__(256) index_add_ordered_kernel(int n, int c, int ne, const int *__restrict__ idx,
                                                                const float *__restrict__ src, float *__restrict__ dst)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row0 = blockIdx.x * 256 + (threadIdx.x & ~63);  // this wave's 64 rows
    const int row = row0 + lane;
    const bool live = row < n;
    idx += (size_t)b * ne;
    src += (size_t)b * ne * c;
    dst += (size_t)b * n * c;
    auto d = [&](int l) -> float & { return dst[CHANNEL_MAJOR ? (size_t)l * n + row : (size_t)row * c + l]; };
    if (live)
        for (int l = 0; l < c; ++l) d(l) = 0.f;
    // 64 indices per trip (one coalesced load); the wave then visits, in ascending order, only the entries that name one of
    // ITS rows (on average one in n / 64), each handled by the lane that owns the row
    for (int e0 = 0; e0 < ne; e0 += 64) {
        const int mine = e0 + lane < ne ? idx[e0 + lane] : -1;
        sn_u64 hits = __ballot((unsigned)(mine - row0) < 64u);
        while (hits) {
            const int t = __builtin_ctzll(hits);
            hits &= hits - 1;
            const int id = __builtin_amdgcn_readlane(mine, t), e = e0 + t;
            if (live && id == row)
                for (int l = 0; l < c; ++l) d(l) += src[CHANNEL_MAJOR ? (size_t)l * ne + e : (size_t)e * c + l];
        }
    }
}

// Large gathers (PointNet++-sized grouping: n and m * nsample both in the tens of thousands): the ordered scan above costs
// (n / 64) * ne index loads per cloud, so beyond kIndexAddOrderedWork the gradient is scattered with float atomics into a
// zeroed destination -- what the reference's own GPU kernels do (tf_grouping_g.cu:60-78): same sums, unordered additions.
constexpr long long kIndexAddOrderedWork = 1ll << 26;
template <bool CHANNEL_MAJOR>
__global__ void __launch_bounds__(256) index_add_atomic_kernel(int n, int c, long long ne, const int *__restrict__ idx,
                                                               const float *__restrict__ src, float *__restrict__ dst)
{
    const int b = blockIdx.y;
    idx += (size_t)b * ne;
    src += (size_t)b * ne * c;
    dst += (size_t)b * n * c;
    const size_t tot = (size_t)ne * c;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += (size_t)gridDim.x * blockDim.x) {
        const size_t e = CHANNEL_MAJOR ? t % (size_t)ne : t / c;
        const int l = (int)(CHANNEL_MAJOR ? t / (size_t)ne : t % c);
        const int row = idx[e];
        if ((unsigned)row < (unsigned)n) atomicAdd(&dst[CHANNEL_MAJOR ? (size_t)l * n + row : (size_t)row * c + l], src[t]);
    }
}

__global__ void __launch_bounds__(256) grouping_operation_kernel(int c, int n, int m, int ns,
                                                                 const float *__restrict__ feat,
                                                                 const int *__restrict__ idx, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const size_t mk = (size_t)m * ns, tot = (size_t)c * mk;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        const int ch = (int)(e / mk);
        const size_t jk = e % mk;
        const int ii = idx[(size_t)b * mk + jk];
        out[(size_t)b * tot + e] = feat[((size_t)b * c + ch) * n + ii];
    }
}

static inline unsigned grid_for(size_t tot, int block = 256, unsigned cap = 4096)
{
    size_t g = (tot + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace sn

using namespace sn;

// workgroups per cloud of the soft-projection backward kernels; grad_sigma_partial holds b * this many floats
extern "C" int sn_soft_bwd_splits(int b, int m)
{
    // query slices per cloud of the soft-projection / fused loss backward: ~1024 workgroups in all (swept 512 / 1024 / 2048 / 4096
    // at 64 .. 2048 clouds: 1024 is fastest everywhere -- chamfer_soft_bwd_kernel 57.5 -> 43.8 us at 512 clouds against 512; a wave
    // walks its queries one after the other, each behind two dependent memory round trips)
    return std::max(1, std::min((m + 3) / 4, (kChamferBwdGroups + b - 1) / std::max(b, 1)));
}

// dst (b, n, c) [or (b, c, n)] = index-add of src over idx (b, ne): ordered and deterministic up to kIndexAddOrderedWork
// index loads per cloud, float atomics into a zeroed destination beyond
template <bool CHANNEL_MAJOR>
static int launch_index_add(const char *who, int b, int n, int c, long long ne, const int *idx, const float *src, float *dst,
                            hipStream_t st)
{
    SN_REQUIRE_AS(who, ne <= 0x7fffffffll, "m * nsample must fit in 31 bits");
    if ((long long)((n + 63) / 64) * ne <= kIndexAddOrderedWork) {
        hipLaunchKernelGGL(index_add_ordered_kernel<CHANNEL_MAJOR>, dim3((n + 255) / 256, b), dim3(256), 0, st, n, c, (int)ne, idx,
                           src, dst);
    } else {
        const hipError_t e = hipMemsetAsync(dst, 0, (size_t)b * n * c * sizeof(float), st);
        if (e != hipSuccess) return sn_set_error((int)e, "%s: %s", who, hipGetErrorString(e));
        hipLaunchKernelGGL(index_add_atomic_kernel<CHANNEL_MAJOR>, dim3(grid_for((size_t)ne * c), b), dim3(256), 0, st, n, c, ne,
                           idx, src, dst);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sn_set_error((int)e, "%s: %s", who, hipGetErrorString(e));
    return 0;
}

// The three backward entries below come in pairs: NAME sums the gradient towards the point cloud / the features by unordered
// float atomics (scratch == NULL here), NAME_ordered (ordered) needs grad_P / grad_X and scratch.
static int soft_project_backward_impl(const char *who, int b, int n, int m, int k, const float *P, int p_layout, const float *Q,
                                      int q_layout, const int *idx, const float *temperature, float min_sigma,
                                      const float *grad_proj, int gproj_layout, float *grad_Q, int gq_layout, float *grad_P,
                                      float *grad_sigma_partial, float *scratch, bool ordered, sn_stream_t stream)
{
    SN_REQUIRE_AS(who, b >= 0 && n >= 1 && m >= 0 && k >= 1 && k <= 64, "bad size");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE_AS(who, (p_layout == SN_LAYOUT_BNC || p_layout == SN_LAYOUT_BCN) && (q_layout == SN_LAYOUT_BNC || q_layout == SN_LAYOUT_BCN),
                  "bad p_layout / q_layout");
    SN_REQUIRE_AS(who, (gproj_layout == SN_LAYOUT_BNC || gproj_layout == SN_LAYOUT_BCN) && (gq_layout == SN_LAYOUT_BNC || gq_layout == SN_LAYOUT_BCN),
                  "bad gproj_layout / gq_layout");
    SN_REQUIRE_AS(who, P && Q && idx && temperature && grad_proj && (!ordered || (grad_P && scratch)),
                  ordered ? "null pointer" : "null input");
    SoftBwdArgs a{};
    a.P = P, a.Q = Q, a.idx = idx, a.temperature = temperature, a.min_sigma = min_sigma;
    a.p_layout = p_layout, a.q_layout = q_layout, a.n = n, a.m = m, a.k = k;
    a.grad_proj = grad_proj, a.gproj_layout = gproj_layout;
    a.grad_Q = grad_Q, a.gq_layout = gq_layout, a.grad_P = grad_P, a.gp_contrib = scratch, a.grad_sigma_partial = grad_sigma_partial;
    launch_soft_bwd_fused(b, sn_soft_bwd_splits(b, m), a, (hipStream_t)stream);
    if (ordered)
        return p_layout == SN_LAYOUT_BNC ? launch_index_add<false>(who, b, n, 3, (long long)m * k, idx, scratch, grad_P, (hipStream_t)stream)
                                         : launch_index_add<true>(who, b, n, 3, (long long)m * k, idx, scratch, grad_P, (hipStream_t)stream);
    SN_LAUNCH_CHECK_AS(who);
    return 0;
}

extern "C" int sn_soft_project_backward(int b, int n, int m, int k, const float *P, int p_layout, const float *Q,
                                        int q_layout, const int *idx, const float *temperature, float min_sigma,
                                        const float *grad_proj, int gproj_layout, float *grad_Q, int gq_layout,
                                        float *grad_P, float *grad_sigma_partial, sn_stream_t stream)
{
    return soft_project_backward_impl(__func__, b, n, m, k, P, p_layout, Q, q_layout, idx, temperature, min_sigma, grad_proj,
                                      gproj_layout, grad_Q, gq_layout, grad_P, grad_sigma_partial, nullptr, false, stream);
}

extern "C" int sn_soft_weights_forward(int b, int n, int m, int k, const float *P, const float *Q, const int *idx,
                                       const float *temperature, float min_sigma, float *weights,
                                       sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 1 && m >= 0 && k >= 1 && k <= 64, "bad size");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE(P && Q && idx && temperature && weights, "null pointer");
    const int y = std::max(1, std::min((m + 3) / 4, (1024 + b - 1) / b));
    hipLaunchKernelGGL(soft_weights_fwd_kernel, dim3(b, y), dim3(256), 0, (hipStream_t)stream, n, m, k, P, Q, idx,
                       temperature, min_sigma, weights);
    SN_LAUNCH_CHECK();
    return 0;
}

static int soft_weights_backward_impl(const char *who, int b, int n, int m, int k, const float *P, const float *Q, const int *idx,
                                      const float *temperature, float min_sigma, const float *weights, const float *grad_weights,
                                      float *grad_Q, float *grad_P, float *grad_sigma_partial, float *scratch, bool ordered,
                                      sn_stream_t stream)
{
    SN_REQUIRE_AS(who, b >= 0 && n >= 1 && m >= 0 && k >= 1 && k <= 64, "bad size");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE_AS(who, P && Q && idx && temperature && grad_weights && (!ordered || (grad_P && scratch)),
                  ordered ? "null pointer" : "null input");
    SoftBwdArgs a{};
    a.P = P, a.Q = Q, a.idx = idx, a.temperature = temperature, a.min_sigma = min_sigma;
    a.p_layout = SN_LAYOUT_BCN, a.q_layout = SN_LAYOUT_BCN, a.n = n, a.m = m, a.k = k;
    a.weights_in = weights, a.grad_weights = grad_weights;
    a.grad_Q = grad_Q, a.gq_layout = SN_LAYOUT_BCN, a.grad_P = grad_P, a.gp_contrib = scratch, a.grad_sigma_partial = grad_sigma_partial;
    hipLaunchKernelGGL(soft_bwd_kernel<false>, dim3(b, sn_soft_bwd_splits(b, m)), dim3(256), 0, (hipStream_t)stream, a);
    if (ordered) return launch_index_add<true>(who, b, n, 3, (long long)m * k, idx, scratch, grad_P, (hipStream_t)stream);
    SN_LAUNCH_CHECK_AS(who);
    return 0;
}

extern "C" int sn_soft_weights_backward(int b, int n, int m, int k, const float *P, const float *Q, const int *idx,
                                        const float *temperature, float min_sigma, const float *weights,
                                        const float *grad_weights, float *grad_Q, float *grad_P,
                                        float *grad_sigma_partial, sn_stream_t stream)
{
    return soft_weights_backward_impl(__func__, b, n, m, k, P, Q, idx, temperature, min_sigma, weights, grad_weights, grad_Q, grad_P,
                                      grad_sigma_partial, nullptr, false, stream);
}

extern "C" int sn_weighted_gather_forward(int b, int c, int n, int m, int k, const float *X, const int *idx,
                                          const float *weights, float *out, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && c >= 0 && n >= 1 && m >= 0 && k >= 1, "bad size");
    if (b == 0 || m == 0 || c == 0) return 0;
    SN_REQUIRE(X && idx && weights && out, "null pointer");
    hipLaunchKernelGGL(weighted_gather_fwd_kernel, dim3(((size_t)c * m + 255) / 256, b), dim3(256), 0,
                       (hipStream_t)stream, c, n, m, k, X, idx, weights, out);
    SN_LAUNCH_CHECK();
    return 0;
}

static int weighted_gather_backward_impl(const char *who, int b, int c, int n, int m, int k, const float *X, const int *idx,
                                         const float *weights, const float *grad_out, float *grad_weights, float *grad_X,
                                         float *scratch, bool ordered, sn_stream_t stream)
{
    SN_REQUIRE_AS(who, b >= 0 && c >= 0 && n >= 1 && m >= 0 && k >= 1, "bad size");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE_AS(who, X && idx && weights && grad_out && (!ordered || (grad_X && scratch)), "null pointer");
    hipLaunchKernelGGL(weighted_gather_bwd_kernel, dim3(((size_t)m * k + 255) / 256, b), dim3(256), 0, (hipStream_t)stream, c, n, m,
                       k, X, idx, weights, grad_out, grad_weights, grad_X, scratch);
    if (ordered) return c == 0 ? 0 : launch_index_add<true>(who, b, n, c, (long long)m * k, idx, scratch, grad_X, (hipStream_t)stream);
    SN_LAUNCH_CHECK_AS(who);
    return 0;
}

extern "C" int sn_weighted_gather_backward(int b, int c, int n, int m, int k, const float *X, const int *idx,
                                           const float *weights, const float *grad_out, float *grad_weights,
                                           float *grad_X, sn_stream_t stream)
{
    return weighted_gather_backward_impl(__func__, b, c, n, m, k, X, idx, weights, grad_out, grad_weights, grad_X, nullptr, false,
                                         stream);
}

// The three backward entries above with the gradient towards the point cloud / the features summed in the ORDER of the
// reference's CPU loops (query ascending, neighbour ascending) instead of by unordered float atomics: the kernels store the
// per-(query, neighbour) contributions in `scratch` (b * m * k * 3 floats; b * c * m * k for the gather) and
// index_add_ordered_kernel adds, per destination row, the entries that name it in ascending entry order.  grad_P / grad_X are
// OVERWRITTEN (every row is written), bit-identical to oracle/samplenet_oracle.c: orc_softproj_backward, run to run.
extern "C" int sn_soft_project_backward_ordered(int b, int n, int m, int k, const float *P, int p_layout, const float *Q,
                                                int q_layout, const int *idx, const float *temperature, float min_sigma,
                                                const float *grad_proj, int gproj_layout, float *grad_Q, int gq_layout,
                                                float *grad_P, float *grad_sigma_partial, float *scratch, sn_stream_t stream)
{
    return soft_project_backward_impl(__func__, b, n, m, k, P, p_layout, Q, q_layout, idx, temperature, min_sigma, grad_proj,
                                      gproj_layout, grad_Q, gq_layout, grad_P, grad_sigma_partial, scratch, true, stream);
}

extern "C" int sn_soft_weights_backward_ordered(int b, int n, int m, int k, const float *P, const float *Q, const int *idx,
                                                const float *temperature, float min_sigma, const float *weights,
                                                const float *grad_weights, float *grad_Q, float *grad_P,
                                                float *grad_sigma_partial, float *scratch, sn_stream_t stream)
{
    return soft_weights_backward_impl(__func__, b, n, m, k, P, Q, idx, temperature, min_sigma, weights, grad_weights, grad_Q, grad_P,
                                      grad_sigma_partial, scratch, true, stream);
}

extern "C" int sn_weighted_gather_backward_ordered(int b, int c, int n, int m, int k, const float *X, const int *idx,
                                                   const float *weights, const float *grad_out, float *grad_weights,
                                                   float *grad_X, float *scratch, sn_stream_t stream)
{
    return weighted_gather_backward_impl(__func__, b, c, n, m, k, X, idx, weights, grad_out, grad_weights, grad_X, scratch, true,
                                         stream);
}

extern "C" int sn_group_point(int b, int n, int c, int m, int nsample, const float *points, const int *idx,
                              float *out, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && c >= 0 && m >= 0 && nsample >= 0, "negative size");
    const size_t tot = (size_t)m * nsample * c;
    if (b == 0 || tot == 0) return 0;
    SN_REQUIRE(points && idx && out, "null pointer");
    hipLaunchKernelGGL(group_point_kernel, dim3(grid_for(tot), b), dim3(256), 0, (hipStream_t)stream, n, c, m,
                       nsample, points, idx, out);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_group_point_grad(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                                   float *grad_points, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && c >= 0 && m >= 0 && nsample >= 0, "negative size");
    if (b == 0 || (size_t)n * c == 0) return 0;
    SN_REQUIRE(grad_points, "null pointer");
    SN_REQUIRE((size_t)m * nsample == 0 || (grad_out && idx), "null pointer");
    return launch_index_add<false>(__func__, b, n, c, (long long)m * nsample, idx, grad_out, grad_points, (hipStream_t)stream);
}

extern "C" int sn_grouping_operation(int b, int c, int n, int m, int nsample, const float *features,
                                     const int *idx, float *out, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && c >= 0 && m >= 0 && nsample >= 0, "negative size");
    const size_t tot = (size_t)m * nsample * c;
    if (b == 0 || tot == 0) return 0;
    SN_REQUIRE(features && idx && out, "null pointer");
    hipLaunchKernelGGL(grouping_operation_kernel, dim3(grid_for(tot), b), dim3(256), 0, (hipStream_t)stream, c, n, m,
                       nsample, features, idx, out);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_grouping_operation_grad(int b, int c, int n, int m, int nsample, const float *grad_out,
                                          const int *idx, float *grad_features, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && c >= 0 && m >= 0 && nsample >= 0, "negative size");
    if (b == 0 || (size_t)n * c == 0) return 0;
    SN_REQUIRE(grad_features, "null pointer");
    SN_REQUIRE((size_t)m * nsample == 0 || (grad_out && idx), "null pointer");
    return launch_index_add<true>(__func__, b, n, c, (long long)m * nsample, idx, grad_out, grad_features, (hipStream_t)stream);
}

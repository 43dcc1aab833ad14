// soft_query.h -- one query of the SoftProjection backward as three __forceinline__ steps, shared by the kernels that run it:
// soft_bwd_kernel (soft_projection.hip) and chamfer_soft_bwd_kernel (sampler_step_loss.hip).
#pragma once
#include "sn_common.h"

namespace sn {

// ------------------------------------------------------------------------------------------------
// SoftProjection backward (fused 'project').  One wave per query, lane t < K = neighbour t.
// ------------------------------------------------------------------------------------------------
struct SoftBwdArgs {
    const float *P;
    const float *Q;
    const int *idx;
    const float *temperature;
    float min_sigma;
    int p_layout, q_layout;
    int n, m, k;
    const float *grad_proj;  // fused mode
    int gproj_layout;
    const float *weights_in;    // split mode: saved weights (unused, recomputed) -- kept for ABI symmetry
    const float *grad_weights;  // split mode
    float *grad_Q;
    int gq_layout;
    float *grad_P;  // (b,3,n) channel-major in split mode, p_layout in fused mode; atomics
    // ordered route (sn_*_backward_ordered): the per-(query, neighbour) contributions to grad_P are STORED here instead of added
    // with atomics -- entry e = j * k + t; (b, m k, 3) for a point-major grad_P, (b, 3, m k) for a channel-major one -- and summed
    // by index_add_ordered_kernel in ascending entry order: the reference's CPU loop, deterministic
    float *gp_contrib;
    float *grad_sigma_partial;
    // fused mode, grad_proj == NULL: the upstream gradient is the same for every element, *gconst / gconst_div
    // (the sampler step's mean(proj) term); accumulate_q: add to grad_Q instead of overwriting it
    const float *gconst;
    float gconst_div;
    int accumulate_q;
};

// One query of the soft-projection backward, executed by a whole wave: returns the gradient to the query (aq*,
// wave-uniform) and its share of d loss / d sigma; accumulates grad_P if requested.  Three steps, so that a caller can
// request the query's memory operands ahead of other work: the neighbour indices, the neighbours' coordinates, the math.
//   K <= 16: every row of 16 lanes holds the K neighbours (lane t of a row = neighbour t) and the ascending-k sums run
//            as sequential DPP scans inside the rows (lane t adds its term to lane t-1's running sum -- the order of the
//            loops below), the four closing sums (gradient x, y, z and the sigma term) one per row;
//   else   : lane t < K = neighbour t, sums by v_readlane loops.
struct SoftQuery {
    float qx, qy, qz;  // the query
    int id;            // this lane's neighbour
    float gx, gy, gz;  // its coordinates
    float go0, go1, go2;  // fused mode with an explicit upstream gradient: d loss / d proj of this query
};

__device__ __forceinline__ float dpp_row_shr1(float x)  // lane below within the row of 16; 0 into the row's lane 0
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_row_shr1_self(float x)  // ... the row's lane 0 reads itself
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x111, 0xf, 0xf, false));
}

__device__ __forceinline__ void soft_bwd_load_index(const SoftBwdArgs &a, int b, int j, int lane, const float *__restrict__ Qb,
                                                    SoftQuery &q)
{
    const int m = a.m, K = a.k;
    q.qx = Qb[pt_off(a.q_layout, m, j, 0)];
    q.qy = Qb[pt_off(a.q_layout, m, j, 1)];
    q.qz = Qb[pt_off(a.q_layout, m, j, 2)];
    const int sub = K <= 16 ? (lane & 15) : lane;
    q.id = sub < K ? a.idx[((size_t)b * m + j) * K + sub] : 0;
    q.go0 = q.go1 = q.go2 = 0.f;
    if (a.grad_proj) {  // (requested here, with the query's other first-round loads, not in front of its use)
        const float *gp = a.grad_proj + (size_t)b * 3 * m;
        q.go0 = gp[pt_off(a.gproj_layout, m, j, 0)];
        q.go1 = gp[pt_off(a.gproj_layout, m, j, 1)];
        q.go2 = gp[pt_off(a.gproj_layout, m, j, 2)];
    }
}

__device__ __forceinline__ void soft_bwd_load_points(const SoftBwdArgs &a, int lane, const float *__restrict__ Pb, SoftQuery &q)
{
    const int n = a.n, K = a.k;
    const int sub = K <= 16 ? (lane & 15) : lane;
    q.gx = q.gy = q.gz = 0.f;
    if (sub < K) {
        q.gx = Pb[pt_off(a.p_layout, n, q.id, 0)];
        q.gy = Pb[pt_off(a.p_layout, n, q.id, 1)];
        q.gz = Pb[pt_off(a.p_layout, n, q.id, 2)];
    }
}

template <bool FUSED>
__device__ __forceinline__ void soft_bwd_math(const SoftBwdArgs &a, int b, int j, int lane, float sigma, const SoftQuery &q,
                                              float &aqx_o, float &aqy_o, float &aqz_o, float &asg_o)
{
    const int n = a.n, m = a.m, K = a.k;
    const bool rows = K <= 16;
    const int sub = rows ? (lane & 15) : lane;
    const bool act = sub < K;
    const int id = q.id;
    const float gx = q.gx, gy = q.gy, gz = q.gz;
    const float dx = gx - q.qx, dy = gy - q.qy, dz = gz - q.qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    const float s = act ? -(d / sigma) : -INFINITY;
    float mx, den;
    if (rows) {
        mx = s;
        for (int t = 1; t < K; ++t) mx = fmaxf(s, dpp_row_shr1_self(mx));
        mx = readlane_f(mx, K - 1);
    } else {
        mx = readlane_f(s, 0);  // neighbours are stored ascending in distance; the scan below only matters
        for (int t = 1; t < K; ++t) mx = fmaxf(mx, readlane_f(s, t));  // if a caller passes unsorted indices
    }
    const float e = act ? expf(s - mx) : 0.f;
    if (rows) {
        den = e;
        for (int t = 1; t < K; ++t) den = e + dpp_row_shr1(den);
        den = readlane_f(den, K - 1);
    } else {
        den = 0.f;
        for (int t = 0; t < K; ++t) den += readlane_f(e, t);
    }
    const float w = e / den;

    float gw;  // d loss / d w_t
    float go0 = 0.f, go1 = 0.f, go2 = 0.f;
    if (FUSED) {
        if (a.grad_proj) {
            go0 = q.go0, go1 = q.go1, go2 = q.go2;
        } else {
            go0 = go1 = go2 = *a.gconst / a.gconst_div;
        }
        gw = (go0 * gx + go1 * gy) + go2 * gz;
    } else {
        gw = act ? a.grad_weights[((size_t)b * m + j) * K + sub] : 0.f;
    }
    float dot;
    if (rows) {
        const float wg = w * gw;
        dot = wg;
        for (int t = 1; t < K; ++t) dot = wg + dpp_row_shr1(dot);
        dot = readlane_f(dot, K - 1);
    } else {
        dot = 0.f;
        for (int t = 0; t < K; ++t) dot += readlane_f(w, t) * readlane_f(gw, t);
    }
    const float gs = act ? w * (gw - dot) : 0.f;  // softmax backward
    const float gd = -gs / sigma;                 // s = -d / sigma
    const float cx = 2.0f * gd * dx, cy = 2.0f * gd * dy, cz = 2.0f * gd * dz;
    const float sg = act ? gs * d / (sigma * sigma) : 0.f;
    float aqx = 0.f, aqy = 0.f, aqz = 0.f, asg = 0.f;
    if (rows) {
        // row 0: 0 - cx_0 - cx_1 ..., row 1: cy, row 2: cz, row 3: 0 + sg_0 + sg_1 ...
        const int row = lane >> 4;
        const float v = row == 0 ? -cx : (row == 1 ? -cy : (row == 2 ? -cz : sg));
        float acc = v;
        for (int t = 1; t < K; ++t) acc = v + dpp_row_shr1(acc);
        aqx = readlane_f(acc, K - 1), aqy = readlane_f(acc, 16 + K - 1), aqz = readlane_f(acc, 32 + K - 1);
        asg = readlane_f(acc, 48 + K - 1);
    } else {
        for (int t = 0; t < K; ++t) {
            aqx -= readlane_f(cx, t);
            aqy -= readlane_f(cy, t);
            aqz -= readlane_f(cz, t);
            asg += readlane_f(sg, t);
        }
    }
    if (a.gp_contrib && lane < K) {
        const int lay = FUSED ? a.p_layout : SN_LAYOUT_BCN;
        const float ex = FUSED ? go0 * w : 0.f, ey = FUSED ? go1 * w : 0.f, ez = FUSED ? go2 * w : 0.f;
        const size_t ne = (size_t)m * K, e = (size_t)j * K + lane;
        float *cb = a.gp_contrib + (size_t)b * ne * 3;
        if (lay == SN_LAYOUT_BNC) cb[e * 3] = ex + cx, cb[e * 3 + 1] = ey + cy, cb[e * 3 + 2] = ez + cz;
        else cb[e] = ex + cx, cb[ne + e] = ey + cy, cb[2 * ne + e] = ez + cz;
    } else if (a.grad_P && lane < K) {
        float *gpb = a.grad_P + (size_t)b * 3 * n;
        const int lay = FUSED ? a.p_layout : SN_LAYOUT_BCN;
        const float ex = FUSED ? go0 * w : 0.f, ey = FUSED ? go1 * w : 0.f, ez = FUSED ? go2 * w : 0.f;
        atomicAdd(&gpb[pt_off(lay, n, id, 0)], ex + cx);
        atomicAdd(&gpb[pt_off(lay, n, id, 1)], ey + cy);
        atomicAdd(&gpb[pt_off(lay, n, id, 2)], ez + cz);
    }
    aqx_o = aqx, aqy_o = aqy, aqz_o = aqz, asg_o = asg;
}

template <bool FUSED>
__device__ __forceinline__ void soft_bwd_query(const SoftBwdArgs &a, int b, int j, int lane, float sigma,
                                               const float *__restrict__ Pb, const float *__restrict__ Qb, float &aqx_o,
                                               float &aqy_o, float &aqz_o, float &asg_o)
{
    SoftQuery q;
    soft_bwd_load_index(a, b, j, lane, Qb, q);
    soft_bwd_load_points(a, lane, Pb, q);
    soft_bwd_math<FUSED>(a, b, j, lane, sigma, q, aqx_o, aqy_o, aqz_o, asg_o);
}

// soft_bwd_kernel<true> as a launch of its own, grid (b, splits) (soft_projection.hip); the sampler step's loss backward takes it for
// clouds its one-launch kernel does not hold
void launch_soft_bwd_fused(int b, int splits, const SoftBwdArgs &a, hipStream_t st);

}  // namespace sn

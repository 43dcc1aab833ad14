// chamfer_backward.hip -- the Chamfer distance's backward and the loss reductions built on it (gfx950).
//
//   chamfer_backward      deterministic, sequential-order accumulation (bit-exact with the CPU
//                         reference loops chamfer_distance.cpp:114-177; the reference GPU path uses
//                         unordered float atomics, chamfer_distance.cu:158-187)
//   simplification_loss_*, chamfer_mean_loss_* (+ _grouped)   the losses' fixed-order reductions forward, the same backward
//                         kernels with implicit upstream gradients (chamfer_owner.h)
#pragma clang fp contract(off)  // reference arithmetic is product-then-sum (no FMA)

#include <algorithm>

#include "chamfer_owner.h"

namespace sn {

// ------------------------------------------------------------------------------------------------
// Chamfer backward.  For the target set T (nt points) against the source set S (ns points):
//   grad_T[j] = 2 gT[j] (t_j - s_{idxT[j]})  -  sum_{l : idxS[l] == j} 2 gS[l] (s_l - t_j)
// own_first selects where the 1:1 term enters the sequential sum, to mirror the reference order:
//   xyz1 side: own term first, then scatter terms in ascending l   (chamfer_distance.cpp:140-155 then :169-171)
//   xyz2 side: scatter terms in ascending j first, then own term    (:152-154 then :166-168)
// A wave owns one target; its lanes scan 64 sources per step, a ballot yields the matching
// sources and they are accumulated in ascending order (wave-uniform arithmetic).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) chamfer_bwd_kernel(int nt, int ns, const float *__restrict__ T,
                                                          const float *__restrict__ S,
                                                          const float *__restrict__ gT,
                                                          const int *__restrict__ idxT,
                                                          const float *__restrict__ gS,
                                                          const int *__restrict__ idxS, float *__restrict__ gradT,
                                                          int own_first, ImplicitGrad ig, int t_layout)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x;
    T += (size_t)b * nt * 3, S += (size_t)b * ns * 3;
    idxT += (size_t)b * nt, idxS += (size_t)b * ns;
    const bool implicit = ig.gL != nullptr;
    float gLv = 0.f;
    int amt = -1, ams = -1;
    if (implicit) {
        gLv = *ig.gL * ig.gscale;
        if (ig.argmax_t) amt = ig.argmax_t[b];
        if (ig.argmax_s) ams = ig.argmax_s[b];
    } else {
        gT += (size_t)b * nt, gS += (size_t)b * ns;
    }
    gradT += (size_t)b * nt * 3;
    for (int j = blockIdx.y * nwaves + wave; j < nt; j += gridDim.y * nwaves) {
        // target coordinates / gradient: point-major (nt,3) or channel-major (3,nt) -- the sampler's FC head emits (3,M)
        const int o0 = t_layout ? j : j * 3, os = t_layout ? nt : 1;
        const float tx = T[o0], ty = T[o0 + os], tz = T[o0 + 2 * os];
        const int j2 = idxT[j];
        const float g = (implicit ? gLv * (ig.ct + (j == amt ? ig.cmax_t : 0.f)) : gT[j]) * 2;
        const float ox = g * (tx - S[j2 * 3 + 0]);
        const float oy = g * (ty - S[j2 * 3 + 1]);
        const float oz = g * (tz - S[j2 * 3 + 2]);
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (own_first) ax += ox, ay += oy, az += oz;
        for (int l0 = 0; l0 < ns; l0 += 64 * 8) {
            int is[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {  // 8 independent index loads in flight
                const int l = l0 + q * 64 + lane;
                is[q] = idxS[l < ns ? l : 0];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int l = l0 + q * 64 + lane;
                sn_u64 mask = __ballot(l < ns && is[q] == j);
                while (mask) {  // matching sources in ascending index order
                    const int ll = l0 + q * 64 + __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const float gg = (implicit ? gLv * (ig.cs + (ll == ams ? ig.cmax_s : 0.f)) : gS[ll]) * 2;
                    ax -= gg * (S[ll * 3 + 0] - tx);
                    ay -= gg * (S[ll * 3 + 1] - ty);
                    az -= gg * (S[ll * 3 + 2] - tz);
                }
            }
        }
        if (!own_first) ax += ox, ay += oy, az += oz;
        if (lane < 3) gradT[o0 + lane * os] = lane == 0 ? ax : (lane == 1 ? ay : az);
    }
}

// Register-resident variant for ns <= 64*PPL (the sampler's 1024-point clouds): every lane loads its PPL sources
// (coordinates, nearest-target index, upstream gradient) ONCE, all loads in flight together; per target the matching
// lanes form their contribution in parallel and only the ordered accumulation (ascending source index, as the
// reference CPU loop) is sequential -- owner_sum (chamfer_owner.h), no memory latency inside it.
template <int PPL>
__global__ void __launch_bounds__(256) chamfer_bwd_reg_kernel(int nt, int ns, const float *__restrict__ T,
                                                              const float *__restrict__ S,
                                                              const float *__restrict__ gT,
                                                              const int *__restrict__ idxT,
                                                              const float *__restrict__ gS,
                                                              const int *__restrict__ idxS, float *__restrict__ gradT,
                                                              int own_first, ImplicitGrad ig, int t_layout)
{
    __shared__ OwnerList s_own[4];  // one per wave (256 threads)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x;
    T += (size_t)b * nt * 3, S += (size_t)b * ns * 3;
    idxT += (size_t)b * nt, idxS += (size_t)b * ns;
    const bool implicit = ig.gL != nullptr;
    float gLv = 0.f;
    int amt = -1, ams = -1;
    if (implicit) {
        gLv = *ig.gL * ig.gscale;
        if (ig.argmax_t) amt = ig.argmax_t[b];
        if (ig.argmax_s) ams = ig.argmax_s[b];
    } else {
        gT += (size_t)b * nt, gS += (size_t)b * ns;
    }
    gradT += (size_t)b * nt * 3;

    float sx[PPL], sy[PPL], sz[PPL], gg[PPL];
    int is[PPL];
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
        const int l = i * 64 + lane;
        const int lc = l < ns ? l : 0;
        const sn_xyz3 sv = *reinterpret_cast<const sn_xyz3 *>(S + (size_t)lc * 3);  // one 12-byte load per source point
        sx[i] = sv.x, sy[i] = sv.y, sz[i] = sv.z;
        is[i] = l < ns ? idxS[lc] : -1;
        gg[i] = (implicit ? gLv * (ig.cs + (l == ams ? ig.cmax_s : 0.f)) : gS[lc]) * 2;
    }
    for (int j = blockIdx.y * nwaves + wave; j < nt; j += gridDim.y * nwaves) {
        // target coordinates / gradient: point-major (nt,3) or channel-major (3,nt) -- the sampler's FC head emits (3,M)
        const int o0 = t_layout ? j : j * 3, os = t_layout ? nt : 1;
        const float tx = T[o0], ty = T[o0 + os], tz = T[o0 + 2 * os];
        const int j2 = idxT[j];
        const float g = (implicit ? gLv * (ig.ct + (j == amt ? ig.cmax_t : 0.f)) : gT[j]) * 2;
        const float ox = g * (tx - S[j2 * 3 + 0]);
        const float oy = g * (ty - S[j2 * 3 + 1]);
        const float oz = g * (tz - S[j2 * 3 + 2]);
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (own_first) ax += ox, ay += oy, az += oz;
        owner_sum<PPL>(s_own[wave], lane, j, is, gg, sx, sy, sz, tx, ty, tz, ax, ay, az);
        if (!own_first) ax += ox, ay += oy, az += oz;
        if (lane < 3) gradT[o0 + lane * os] = lane == 0 ? ax : (lane == 1 ? ay : az);
    }
}

void launch_chamfer_bwd(int b, int ysplit, int nt, int ns, const float *T, const float *S, const float *gT,
                        const int *idxT, const float *gS, const int *idxS, float *gradT, int own_first,
                        const ImplicitGrad &ig, hipStream_t st, int t_layout)
{
    const dim3 grid(b, ysplit), block(256);
#define SN_CB(PPL_) \
    hipLaunchKernelGGL(chamfer_bwd_reg_kernel<PPL_>, grid, block, 0, st, nt, ns, T, S, gT, idxT, gS, idxS, gradT, own_first, ig, t_layout)
    if (ns <= 64) SN_CB(1);
    else if (ns <= 256) SN_CB(4);
    else if (ns <= 1024) SN_CB(16);
    else if (ns <= 2048) SN_CB(32);
    else
        hipLaunchKernelGGL(chamfer_bwd_kernel, grid, block, 0, st, nt, ns, T, S, gT, idxT, gS, idxS, gradT, own_first, ig, t_layout);
#undef SN_CB
}

}  // namespace sn

using namespace sn;

extern "C" int sn_chamfer_backward(int b, int n, const float *xyz1, int m, const float *xyz2,
                                   const float *grad_dist1, const int *idx1, const float *grad_dist2,
                                   const int *idx2, float *grad_xyz1, float *grad_xyz2, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0, "negative size");
    if (b == 0 || n == 0 || m == 0) return 0;
    SN_REQUIRE(xyz1 && xyz2 && grad_dist1 && grad_dist2 && idx1 && idx2, "null input");
    hipStream_t st = (hipStream_t)stream;
    auto ysplit = [&](int nt) { return sn_soft_bwd_splits(b, nt); };
    const ImplicitGrad none{};
    if (grad_xyz1) launch_chamfer_bwd(b, ysplit(n), n, m, xyz1, xyz2, grad_dist1, idx1, grad_dist2, idx2, grad_xyz1, 1, none, st);
    if (grad_xyz2) launch_chamfer_bwd(b, ysplit(m), m, n, xyz2, xyz1, grad_dist2, idx2, grad_dist1, idx1, grad_xyz2, 0, none, st);
    SN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Fused simplification loss (samplenet.py:171-181):
//   loss = mean(dist1) + mean_b(max_m dist1) + w * mean(dist2),   w = gamma + delta * pc_size
// forward: one workgroup per cloud reduces its (sum dist1, max dist1 + first argmax, sum dist2) in a fixed order,
// a single-workgroup kernel combines the clouds; backward: sn_chamfer_backward with implicit upstream gradients.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) simp_loss_partial_kernel(int n1, int n2, const float *__restrict__ d1,
                                                                const float *__restrict__ d2, float *__restrict__ part,
                                                                int *__restrict__ argmax1)
{
    __shared__ float r0[256], r1[256], r2[256];
    __shared__ int ri[256];
    const int b = blockIdx.x, t = threadIdx.x;
    float s1 = 0.f, mx = -INFINITY, s2 = 0.f;
    int am = 0;
    for (int j = t; j < n1; j += 256) {
        const float v = d1[(size_t)b * n1 + j];
        s1 += v;
        if (v > mx) mx = v, am = j;
    }
    for (int j = t; j < n2; j += 256) s2 += d2[(size_t)b * n2 + j];
    r0[t] = s1, r1[t] = mx, r2[t] = s2, ri[t] = am;
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            r0[t] += r0[t + s];
            r2[t] += r2[t + s];
            if (r1[t + s] > r1[t] || (r1[t + s] == r1[t] && ri[t + s] < ri[t])) r1[t] = r1[t + s], ri[t] = ri[t + s];
        }
    }
    if (t == 0) {
        part[b * 3 + 0] = r0[0], part[b * 3 + 1] = r1[0], part[b * 3 + 2] = r2[0];
        argmax1[b] = ri[0];
    }
}

template <bool WITH_MAX>
__global__ void __launch_bounds__(64) simp_loss_final_kernel(int B, int n1, int n2, float w, const float *__restrict__ part,
                                                             float *__restrict__ loss)
{
    if (threadIdx.x != 0) return;
    float s1 = 0.f, mx = 0.f, s2 = 0.f;
    for (int b = 0; b < B; ++b) s1 += part[b * 3], mx += part[b * 3 + 1], s2 += part[b * 3 + 2];
    const float c12 = s1 / ((float)B * (float)n1), cmax = mx / (float)B, c21 = s2 / ((float)B * (float)n2);
    loss[0] = WITH_MAX ? c12 + cmax + w * c21 : c12 + w * c21;
}

extern "C" int sn_simplification_loss_forward(int B, int n1, int n2, const float *dist1, const float *dist2, float weight,
                                              float *partial, int *argmax1, float *loss, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && n1 >= 1 && n2 >= 1, "bad size");
    SN_REQUIRE(dist1 && dist2 && partial && argmax1 && loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(simp_loss_partial_kernel, dim3(B), dim3(256), 0, st, n1, n2, dist1, dist2, partial, argmax1);
    hipLaunchKernelGGL(simp_loss_final_kernel<true>, dim3(1), dim3(64), 0, st, B, n1, n2, weight, partial, loss);
    SN_LAUNCH_CHECK();
    return 0;
}

// grad_xyz1 (B,n1,3) / grad_xyz2 (B,n2,3) of the fused loss; grad_loss: device scalar.  Either output may be NULL.
extern "C" int sn_simplification_loss_backward(int B, int n1, const float *xyz1, int n2, const float *xyz2, const int *idx1,
                                               const int *idx2, const int *argmax1, float weight, const float *grad_loss,
                                               float *grad_xyz1, float *grad_xyz2, int layout1, sn_stream_t stream)
{
    SN_REQUIRE(layout1 == 0 || layout1 == 1, "layout1 must be 0 (B,n1,3) or 1 (B,3,n1)");
    SN_REQUIRE(layout1 == 0 || !grad_xyz2, "grad_xyz2 needs xyz1 in (B,n1,3) layout");
    SN_REQUIRE(B >= 1 && n1 >= 1 && n2 >= 1, "bad size");
    SN_REQUIRE(xyz1 && xyz2 && idx1 && idx2 && argmax1 && grad_loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    auto ysplit = [&](int nt) { return sn_soft_bwd_splits(B, nt); };
    const float c1 = 1.0f / ((float)B * (float)n1), cm = 1.0f / (float)B, c2 = weight / ((float)B * (float)n2);
    if (grad_xyz1) {
        ImplicitGrad ig{grad_loss, argmax1, nullptr, c1, cm, c2, 0.f};
        launch_chamfer_bwd(B, ysplit(n1), n1, n2, xyz1, xyz2, nullptr, idx1, nullptr, idx2, grad_xyz1, 1, ig, st, layout1);
    }
    if (grad_xyz2) {
        ImplicitGrad ig{grad_loss, nullptr, argmax1, c2, 0.f, c1, cm};
        launch_chamfer_bwd(B, ysplit(n2), n2, n1, xyz2, xyz1, nullptr, idx2, nullptr, idx1, grad_xyz2, 0, ig, st);
    }
    SN_LAUNCH_CHECK();
    return 0;
}

// The Chamfer loss of the registration task (registration/main.py:573-577): mean(dist1) + mean(dist2) -- the simplification loss
// without its maximum term; same kernels (partial: 3 B floats, argmax1: B ints of scratch), same implicit-gradient backward.
extern "C" int sn_chamfer_mean_loss_forward(int B, int n1, int n2, const float *dist1, const float *dist2, float *partial,
                                            int *argmax1, float *loss, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && n1 >= 1 && n2 >= 1, "bad size");
    SN_REQUIRE(dist1 && dist2 && partial && argmax1 && loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(simp_loss_partial_kernel, dim3(B), dim3(256), 0, st, n1, n2, dist1, dist2, partial, argmax1);
    hipLaunchKernelGGL(simp_loss_final_kernel<false>, dim3(1), dim3(64), 0, st, B, n1, n2, 1.0f, partial, loss);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_chamfer_mean_loss_backward(int B, int n1, const float *xyz1, int n2, const float *xyz2, const int *idx1,
                                             const int *idx2, const float *grad_loss, float *grad_xyz1, float *grad_xyz2,
                                             sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && n1 >= 1 && n2 >= 1, "bad size");
    SN_REQUIRE(xyz1 && xyz2 && idx1 && idx2 && grad_loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    auto ysplit = [&](int nt) { return sn_soft_bwd_splits(B, nt); };
    const float c1 = 1.0f / ((float)B * (float)n1), c2 = 1.0f / ((float)B * (float)n2);
    if (grad_xyz1) {
        ImplicitGrad ig{grad_loss, nullptr, nullptr, c1, 0.f, c2, 0.f};
        launch_chamfer_bwd(B, ysplit(n1), n1, n2, xyz1, xyz2, nullptr, idx1, nullptr, idx2, grad_xyz1, 1, ig, st);
    }
    if (grad_xyz2) {
        ImplicitGrad ig{grad_loss, nullptr, nullptr, c2, 0.f, c1, 0.f};
        launch_chamfer_bwd(B, ysplit(n2), n2, n1, xyz2, xyz1, nullptr, idx2, nullptr, idx1, grad_xyz2, 0, ig, st);
    }
    SN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The Chamfer term of the registration task loss for SEVERAL evaluations in one batch (the progressive sampler's prefixes against one
// template: clouds [e group, (e + 1) group) are evaluation e): xyz1 (R, n1, 3) holds clouds of nv[e] <= n1 valid points each -- the rest
// are cyclic copies (sn_cyclic_pad_cat), which the scan may see (a copy never wins a minimum: the lowest index does) but the loss must
// not count --, xyz2 (R, n2, 3).  loss[e] = mean over the evaluation's clouds and VALID points of dist1 + mean of dist2, reduced in
// sn_chamfer_mean_loss_forward's order; the backward is chamfer_bwd_reg_kernel's with the evaluation's own upstream gradient and
// 1 / (group nv[e]), copies as targets get zero and as sources are skipped: every number equals the evaluation's own
// sn_chamfer_mean_loss_forward / _backward on the unpadded cloud, bit for bit -- 2 + 2 launches where E evaluations take 2 E + 2 E.
// ------------------------------------------------------------------------------------------------
struct GroupSizes {
    int n;
    int nv[kMaxPrefixes];
};
__global__ void __launch_bounds__(256) chamfer_mean_grouped_partial_kernel(int n1, int n2, int group, GroupSizes gs,
                                                                           const float *__restrict__ d1, const float *__restrict__ d2,
                                                                           float *__restrict__ part)
{
    __shared__ float r0[256], r2[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nv = gs.nv[b / group];
    float s1 = 0.f, s2 = 0.f;
    for (int j = t; j < nv; j += 256) s1 += d1[(size_t)b * n1 + j];
    for (int j = t; j < n2; j += 256) s2 += d2[(size_t)b * n2 + j];
    r0[t] = s1, r2[t] = s2;
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) r0[t] += r0[t + s], r2[t] += r2[t + s];
    }
    if (t == 0) part[b * 2] = r0[0], part[b * 2 + 1] = r2[0];
}
__global__ void __launch_bounds__(64) chamfer_mean_grouped_final_kernel(int n2, int group, GroupSizes gs, const float *__restrict__ part,
                                                                        float *__restrict__ loss)
{
    const int e = threadIdx.x;
    if (e >= gs.n) return;
    float s1 = 0.f, s2 = 0.f;
    for (int b = e * group; b < (e + 1) * group; ++b) s1 += part[b * 2], s2 += part[b * 2 + 1];
    const float c12 = s1 / ((float)group * (float)gs.nv[e]), c21 = s2 / ((float)group * (float)n2);
    loss[e] = c12 + 1.0f * c21;
}

// (`who` names the entry in the error text)
static int group_sizes(const char *who, int R, int n1, int group, int nev, const int *nvalid, GroupSizes &gs)
{
    SN_REQUIRE_AS(who, group >= 1 && nev >= 1 && nev <= kMaxPrefixes && R == nev * group && nvalid, "R = nev * group, at most 16 evaluations");
    gs.n = nev;
    for (int e = 0; e < nev; ++e) {
        SN_REQUIRE_AS(who, nvalid[e] >= 1 && nvalid[e] <= n1, "valid points outside [1, n1]");
        gs.nv[e] = nvalid[e];
    }
    return 0;
}

// dist1 (R, n1), dist2 (R, n2): sn_chamfer_forward's products of the padded batch; partial: 2 R floats; loss: nev floats
extern "C" int sn_chamfer_mean_loss_forward_grouped(int R, int n1, int n2, int group, int nev, const int *nvalid, const float *dist1,
                                                    const float *dist2, float *partial, float *loss, sn_stream_t stream)
{
    SN_REQUIRE(R >= 1 && n1 >= 1 && n2 >= 1 && dist1 && dist2 && partial && loss, "bad argument");
    GroupSizes gs{};
    if (int rc = group_sizes(__func__, R, n1, group, nev, nvalid, gs)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chamfer_mean_grouped_partial_kernel, dim3(R), dim3(256), 0, st, n1, n2, group, gs, dist1, dist2, partial);
    hipLaunchKernelGGL(chamfer_mean_grouped_final_kernel, dim3(1), dim3(64), 0, st, n2, group, gs, partial, loss);
    SN_LAUNCH_CHECK();
    return 0;
}

// chamfer_bwd_reg_kernel for grouped evaluations: gL one upstream gradient per evaluation; ntv / nsv = the evaluation's valid targets /
// sources (the other side: all of them); ct / cs as sn_chamfer_mean_loss_backward forms them, per evaluation
struct GroupedGrad {
    const float *gL;
    int group;
    int t_valid;  // 1: the TARGET side is the padded one (nv[] bounds the targets), 0: the source side
    GroupSizes gs;
    float c_pad[kMaxPrefixes];  // 1 / (group nv[e]): the coefficient of the padded side
    float c_full;               // 1 / (group n_other)
};
template <int PPL>
__global__ void __launch_bounds__(256) chamfer_bwd_grouped_kernel(int nt, int ns, const float *__restrict__ T, const float *__restrict__ S,
                                                                  const int *__restrict__ idxT, const int *__restrict__ idxS,
                                                                  float *__restrict__ gradT, int own_first, GroupedGrad gg)
{
    __shared__ OwnerList s_own[4];  // one per wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x, e = b / gg.group;
    T += (size_t)b * nt * 3, S += (size_t)b * ns * 3;
    idxT += (size_t)b * nt, idxS += (size_t)b * ns;
    gradT += (size_t)b * nt * 3;
    const float gLv = gg.gL[e] * 1.f;
    const float ct = gg.t_valid ? gg.c_pad[e] : gg.c_full, cs = gg.t_valid ? gg.c_full : gg.c_pad[e];
    const int ntv = gg.t_valid ? gg.gs.nv[e] : nt, nsv = gg.t_valid ? ns : gg.gs.nv[e];
    float sx[PPL], sy[PPL], sz[PPL], gs2[PPL];
    int is[PPL];
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
        const int l = i * 64 + lane;
        const int lc = l < ns ? l : 0;
        const sn_xyz3 sv = *reinterpret_cast<const sn_xyz3 *>(S + (size_t)lc * 3);
        sx[i] = sv.x, sy[i] = sv.y, sz[i] = sv.z;
        is[i] = l < nsv ? idxS[lc] : -1;  // (copies among the sources are not counted)
        gs2[i] = (gLv * (cs + 0.f)) * 2;
    }
    for (int j = blockIdx.y * nwaves + wave; j < nt; j += gridDim.y * nwaves) {
        if (j >= ntv) {  // a copy among the targets: no gradient
            if (lane < 3) gradT[j * 3 + lane] = 0.f;
            continue;
        }
        const float tx = T[j * 3], ty = T[j * 3 + 1], tz = T[j * 3 + 2];
        const int j2 = idxT[j];
        const float g = (gLv * (ct + 0.f)) * 2;
        const float ox = g * (tx - S[j2 * 3 + 0]);
        const float oy = g * (ty - S[j2 * 3 + 1]);
        const float oz = g * (tz - S[j2 * 3 + 2]);
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (own_first) ax += ox, ay += oy, az += oz;
        owner_sum<PPL>(s_own[wave], lane, j, is, gs2, sx, sy, sz, tx, ty, tz, ax, ay, az);
        if (!own_first) ax += ox, ay += oy, az += oz;
        if (lane < 3) gradT[j * 3 + lane] = lane == 0 ? ax : (lane == 1 ? ay : az);
    }
}

// grad_xyz1 (R, n1, 3) [zero at the copies] and / or grad_xyz2 (R, n2, 3); grad_loss: nev floats on the device; n1, n2 <= 2048
extern "C" int sn_chamfer_mean_loss_backward_grouped(int R, int n1, const float *xyz1, int n2, const float *xyz2, int group, int nev,
                                                     const int *nvalid, const int *idx1, const int *idx2, const float *grad_loss,
                                                     float *grad_xyz1, float *grad_xyz2, sn_stream_t stream)
{
    SN_REQUIRE(R >= 1 && n1 >= 1 && n2 >= 1 && n1 <= 2048 && n2 <= 2048, "bad size (at most 2048 points a side)");
    SN_REQUIRE(xyz1 && xyz2 && idx1 && idx2 && grad_loss, "null pointer");
    GroupedGrad gg{};
    if (int rc = group_sizes(__func__, R, n1, group, nev, nvalid, gg.gs)) return rc;
    gg.gL = grad_loss, gg.group = group;
    for (int e = 0; e < nev; ++e) gg.c_pad[e] = 1.0f / ((float)group * (float)nvalid[e]);
    gg.c_full = 1.0f / ((float)group * (float)n2);
    hipStream_t st = (hipStream_t)stream;
    auto ysplit = [&](int nt) { return sn_soft_bwd_splits(R, nt); };
#define SN_CBG(PPL_, NT, NS, TT, SS, IT, IS, GT, OF)                                                                              \
    hipLaunchKernelGGL(chamfer_bwd_grouped_kernel<PPL_>, dim3(R, ysplit(NT)), dim3(256), 0, st, NT, NS, TT, SS, IT, IS, GT, OF, gg)
#define SN_CBG_ANY(NT, NS, TT, SS, IT, IS, GT, OF)           \
    do {                                                     \
        if (NS <= 64) SN_CBG(1, NT, NS, TT, SS, IT, IS, GT, OF);        \
        else if (NS <= 256) SN_CBG(4, NT, NS, TT, SS, IT, IS, GT, OF);  \
        else if (NS <= 1024) SN_CBG(16, NT, NS, TT, SS, IT, IS, GT, OF); \
        else SN_CBG(32, NT, NS, TT, SS, IT, IS, GT, OF);                \
    } while (0)
    if (grad_xyz1) {
        gg.t_valid = 1;
        SN_CBG_ANY(n1, n2, xyz1, xyz2, idx1, idx2, grad_xyz1, 1);
    }
    if (grad_xyz2) {
        gg.t_valid = 0;
        SN_CBG_ANY(n2, n1, xyz2, xyz1, idx2, idx1, grad_xyz2, 0);
    }
#undef SN_CBG_ANY
#undef SN_CBG
    SN_LAUNCH_CHECK();
    return 0;
}

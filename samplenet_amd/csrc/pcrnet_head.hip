// pcrnet_head.hip -- PCRNet's output head and the rotation of a cloud by one quaternion per cloud, apart and as one launch (gfx950).
//
// ------------------------------------------------------------------------------------------------
// PCRNet's output head (registration/models/pcrnet.py:78-82 + the QuaterNet regulariser of registration/main.py:565):
//   twist (B,7) = [ y[:, 0:4] / max(||y[:, 0:4]||, 1e-12) | y[:, 4:7] ],   qnorm = mean_b (||y[:, 0:4]||^2 - 1)^2
// one single-workgroup launch forward, one backward (torch: slice, norm, clamp, expand, div, cat + pow, sum, sub, pow, mean and
// their ~15 backward launches).  Sums over the batch run in a fixed order.
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)  // reference arithmetic is product-then-sum (no FMA)

#include <algorithm>

#include "chamfer_owner.h"  // sn_xyz3

using namespace sn;

__global__ void __launch_bounds__(256) pcrnet_head_fwd_kernel(int B, const float *__restrict__ y, float *__restrict__ twist,
                                                              float *__restrict__ quat, float *__restrict__ qnorm)
{
    __shared__ float red[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float *r = y + (size_t)b * 7;
        const float n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
        const float inv = 1.0f / fmaxf(sqrtf(n2), 1e-12f);
        const float q0 = r[0] * inv, q1 = r[1] * inv, q2 = r[2] * inv, q3 = r[3] * inv;
        float *o = twist + (size_t)b * 7;
        o[0] = q0, o[1] = q1, o[2] = q2, o[3] = q3, o[4] = r[4], o[5] = r[5], o[6] = r[6];
        if (quat) quat[b * 4 + 0] = q0, quat[b * 4 + 1] = q1, quat[b * 4 + 2] = q2, quat[b * 4 + 3] = q3;
        acc += (n2 - 1.0f) * (n2 - 1.0f);
    }
    if (!qnorm) return;
    red[threadIdx.x] = acc;
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    }
    if (threadIdx.x == 0) qnorm[0] = red[0] / (float)B;
}

__global__ void __launch_bounds__(256) pcrnet_head_bwd_kernel(int B, const float *__restrict__ y, const float *__restrict__ g_twist,
                                                              const float *__restrict__ g_quat, const float *__restrict__ g_qnorm,
                                                              float *__restrict__ g_y)
{
    const float gq = g_qnorm ? g_qnorm[0] : 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float *r = y + (size_t)b * 7;
        const float n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
        const float nrm = sqrtf(n2);
        float *o = g_y + (size_t)b * 7;
        // upstream gradient of the normalised quaternion: through twist[:, 0:4] and / or through the separate copy
        float gt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) gt[i] = (g_twist ? g_twist[(size_t)b * 7 + i] : 0.f) + (g_quat ? g_quat[b * 4 + i] : 0.f);
        float gp[4];
        if (nrm > 1e-12f) {  // d(p / ||p||) = (g - q (q . g)) / ||p||
            const float inv = 1.0f / nrm;
            const float q[4] = {r[0] * inv, r[1] * inv, r[2] * inv, r[3] * inv};
            const float dot = q[0] * gt[0] + q[1] * gt[1] + q[2] * gt[2] + q[3] * gt[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) gp[i] = (gt[i] - q[i] * dot) * inv;
        } else {  // clamped denominator: p / 1e-12
#pragma unroll
            for (int i = 0; i < 4; ++i) gp[i] = gt[i] * 1e12f;
        }
#pragma unroll
        for (int i = 4; i < 7; ++i) o[i] = g_twist ? g_twist[(size_t)b * 7 + i] : 0.f;
        const float cq = gq * 4.0f * (n2 - 1.0f) / (float)B;  // d/dp mean (||p||^2 - 1)^2 = 4 (||p||^2 - 1) p / B
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = gp[i] + cq * r[i];
    }
}

extern "C" int sn_pcrnet_head_forward(int B, const float *y, float *twist, float *quat, float *qnorm, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && y && twist, "bad argument");
    hipLaunchKernelGGL(pcrnet_head_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, y, twist, quat, qnorm);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_pcrnet_head_backward(int B, const float *y, const float *g_twist, const float *g_quat, const float *g_qnorm, float *g_y,
                                       sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && y && g_y, "bad argument");
    hipLaunchKernelGGL(pcrnet_head_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, y, g_twist, g_quat, g_qnorm, g_y);
    SN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Rotation of a cloud by one quaternion per cloud (the registration task loss rotates the template by the
// estimated pose -- registration/main.py:569-571 est_transform.rotate(p0) = src/quaternion.py:35-53 qrot with the quaternion
// expanded over the points).  The reference composes it from two cross products, a scale and two adds per point on
// materialised (B,N,4) / (B,N,3) tensors: ~8 launches forward, ~16 backward.  Here: one launch each way.
//   out = v + 2 (w (u x v) + u x (u x v)),   q = (w, u)
//   backward:  dv = g - 2 w (u x g) + 2 u x (u x g)                                   (rotation by the conjugate)
//              dw = sum_n 2 (u x v_n) . g_n
//              du = sum_n 2 w (v_n x g_n) + 2 (u . g_n) v_n + 2 (u . v_n) g_n - 4 (v_n . g_n) u
// one workgroup per cloud; the per-cloud sums in a fixed order (strided per-thread partials, xor tree, waves in order).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ sn_xyz3 cross3(sn_xyz3 a, sn_xyz3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot3(sn_xyz3 a, sn_xyz3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__global__ void __launch_bounds__(256) qrot_fwd_kernel(int N, const float *__restrict__ q, const float *__restrict__ v,
                                                       float *__restrict__ out)
{
    const int b = blockIdx.y;
    const float w = q[b * 4];
    const sn_xyz3 u{q[b * 4 + 1], q[b * 4 + 2], q[b * 4 + 3]};
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const sn_xyz3 p = *reinterpret_cast<const sn_xyz3 *>(v + ((size_t)b * N + n) * 3);
        const sn_xyz3 x{p.x, p.y, p.z};
        const sn_xyz3 uv = cross3(u, x), uuv = cross3(u, uv);
        sn_xyz3 o;
        o.x = x.x + 2.0f * (w * uv.x + uuv.x), o.y = x.y + 2.0f * (w * uv.y + uuv.y), o.z = x.z + 2.0f * (w * uv.z + uuv.z);
        *reinterpret_cast<sn_xyz3 *>(out + ((size_t)b * N + n) * 3) = o;
    }
}

__global__ void __launch_bounds__(256) qrot_bwd_kernel(int N, const float *__restrict__ q, const float *__restrict__ v,
                                                       const float *__restrict__ g, float *__restrict__ gq,
                                                       float *__restrict__ gv)
{
    __shared__ float red[4][4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float w = q[b * 4];
    const sn_xyz3 u{q[b * 4 + 1], q[b * 4 + 2], q[b * 4 + 3]};
    float aw = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        const sn_xyz3 gp = *reinterpret_cast<const sn_xyz3 *>(g + ((size_t)b * N + n) * 3);
        const sn_xyz3 gg{gp.x, gp.y, gp.z};
        if (gv) {
            const sn_xyz3 ug = cross3(u, gg), uug = cross3(u, ug);
            sn_xyz3 o;
            o.x = gg.x + 2.0f * (uug.x - w * ug.x), o.y = gg.y + 2.0f * (uug.y - w * ug.y), o.z = gg.z + 2.0f * (uug.z - w * ug.z);
            *reinterpret_cast<sn_xyz3 *>(gv + ((size_t)b * N + n) * 3) = o;
        }
        if (gq) {
            const sn_xyz3 p = *reinterpret_cast<const sn_xyz3 *>(v + ((size_t)b * N + n) * 3);
            const sn_xyz3 x{p.x, p.y, p.z};
            const sn_xyz3 uv = cross3(u, x), vg = cross3(x, gg);
            const float ug = dot3(u, gg), ux = dot3(u, x), xg = dot3(x, gg);
            aw += 2.0f * dot3(uv, gg);
            ax += 2.0f * (w * vg.x + ug * x.x + ux * gg.x) - 4.0f * xg * u.x;
            ay += 2.0f * (w * vg.y + ug * x.y + ux * gg.y) - 4.0f * xg * u.y;
            az += 2.0f * (w * vg.z + ug * x.z + ux * gg.z) - 4.0f * xg * u.z;
        }
    }
    if (!gq) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        aw += __shfl_xor(aw, o), ax += __shfl_xor(ax, o), ay += __shfl_xor(ay, o), az += __shfl_xor(az, o);
    }
    if (lane == 0) red[wave][0] = aw, red[wave][1] = ax, red[wave][2] = ay, red[wave][3] = az;
    __syncthreads();
    if (threadIdx.x < 4) gq[b * 4 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// PCRNet's output head AND the rotation of the template by the estimated quaternion as ONE launch each way (the registration
// task term, registration/main.py:557-577: twist = model(p0, p1); p1_est = rotate(p0, twist[:, 0:4])): the arithmetic of
// pcrnet_head_fwd_kernel + qrot_fwd_kernel / qrot_bwd_kernel + pcrnet_head_bwd_kernel, expression for expression (results are
// bit-identical to the two launches), one dependent launch less in either direction of a latency-bound step.
//   forward : grid (x, B); every workgroup normalises its cloud's quaternion from y[b] itself and rotates its share of the points;
//             workgroup (0, b) stores twist[b] / quat[b]; workgroup (0, 0) also the regulariser (fixed-order sum over the batch).
//   backward: one workgroup per cloud: gv (optional), the quaternion's gradient by the fixed-order reduction of qrot_bwd_kernel,
//             then the head's backward of row b with that gradient in the place of g_quat.
// group > 0 (several evaluations against ONE template, the progressive sampler's prefixes): rows [e group, (e + 1) group) are evaluation e,
// v holds `group` clouds (row b rotates v[b % group]) and qnorm / g_qnorm hold one value per evaluation; 0: one evaluation of B rows.
__global__ void __launch_bounds__(256) pcrnet_head_rot_fwd_kernel(int B, int N, const float *__restrict__ y, const float *__restrict__ v,
                                                                  float *__restrict__ twist, float *__restrict__ quat,
                                                                  float *__restrict__ qnorm, float *__restrict__ out, int group)
{
    __shared__ float red[256];
    const int b = blockIdx.y;
    const int vb = group ? b % group : b;
    const float *r = y + (size_t)b * 7;
    const float n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
    const float inv = 1.0f / fmaxf(sqrtf(n2), 1e-12f);
    const float q0 = r[0] * inv, q1 = r[1] * inv, q2 = r[2] * inv, q3 = r[3] * inv;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float *o = twist + (size_t)b * 7;
        o[0] = q0, o[1] = q1, o[2] = q2, o[3] = q3, o[4] = r[4], o[5] = r[5], o[6] = r[6];
        quat[b * 4 + 0] = q0, quat[b * 4 + 1] = q1, quat[b * 4 + 2] = q2, quat[b * 4 + 3] = q3;
    }
    const float w = q0;
    const sn_xyz3 u{q1, q2, q3};
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const sn_xyz3 p = *reinterpret_cast<const sn_xyz3 *>(v + ((size_t)vb * N + n) * 3);
        const sn_xyz3 x{p.x, p.y, p.z};
        const sn_xyz3 uv = cross3(u, x), uuv = cross3(u, uv);
        sn_xyz3 o;
        o.x = x.x + 2.0f * (w * uv.x + uuv.x), o.y = x.y + 2.0f * (w * uv.y + uuv.y), o.z = x.z + 2.0f * (w * uv.z + uuv.z);
        *reinterpret_cast<sn_xyz3 *>(out + ((size_t)b * N + n) * 3) = o;
    }
    if (blockIdx.x != 0 || vb != 0 || !qnorm) return;  // (the first row of an evaluation: its regulariser)
    const int base = b;
    if (group) B = group, qnorm += b / group;
    float acc = 0.f;  // (pcrnet_head_fwd_kernel's sum: strided per-thread partials, halving tree)
    for (int bb = threadIdx.x; bb < B; bb += 256) {
        const float *rr = y + (size_t)(base + bb) * 7;
        const float m2 = rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3];
        acc += (m2 - 1.0f) * (m2 - 1.0f);
    }
    red[threadIdx.x] = acc;
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    }
    if (threadIdx.x == 0) qnorm[0] = red[0] / (float)B;
}

__global__ void __launch_bounds__(256) pcrnet_head_rot_bwd_kernel(int B, int N, const float *__restrict__ y, const float *__restrict__ q,
                                                                  const float *__restrict__ v, const float *__restrict__ g,
                                                                  const float *__restrict__ g_twist, const float *__restrict__ g_quat,
                                                                  const float *__restrict__ g_qnorm, float *__restrict__ gv,
                                                                  float *__restrict__ g_y, int group)
{
    __shared__ float red[4][4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v += (long long)((group ? b % group : b) - b) * N * 3;  // (v[b] below = the template of row b)
    if (group) B = group;
    if (group && g_qnorm) g_qnorm += b / group;
    const float w = q[b * 4];
    const sn_xyz3 u{q[b * 4 + 1], q[b * 4 + 2], q[b * 4 + 3]};
    float aw = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    if (g)
        for (int n = threadIdx.x; n < N; n += 256) {
            const sn_xyz3 gp = *reinterpret_cast<const sn_xyz3 *>(g + ((size_t)b * N + n) * 3);
            const sn_xyz3 gg{gp.x, gp.y, gp.z};
            if (gv) {
                const sn_xyz3 ug = cross3(u, gg), uug = cross3(u, ug);
                sn_xyz3 o;
                o.x = gg.x + 2.0f * (uug.x - w * ug.x), o.y = gg.y + 2.0f * (uug.y - w * ug.y), o.z = gg.z + 2.0f * (uug.z - w * ug.z);
                *reinterpret_cast<sn_xyz3 *>(gv + ((size_t)b * N + n) * 3) = o;
            }
            const sn_xyz3 p = *reinterpret_cast<const sn_xyz3 *>(v + ((size_t)b * N + n) * 3);
            const sn_xyz3 x{p.x, p.y, p.z};
            const sn_xyz3 uv = cross3(u, x), vg = cross3(x, gg);
            const float ug = dot3(u, gg), ux = dot3(u, x), xg = dot3(x, gg);
            aw += 2.0f * dot3(uv, gg);
            ax += 2.0f * (w * vg.x + ug * x.x + ux * gg.x) - 4.0f * xg * u.x;
            ay += 2.0f * (w * vg.y + ug * x.y + ux * gg.y) - 4.0f * xg * u.y;
            az += 2.0f * (w * vg.z + ug * x.z + ux * gg.z) - 4.0f * xg * u.z;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        aw += __shfl_xor(aw, o), ax += __shfl_xor(ax, o), ay += __shfl_xor(ay, o), az += __shfl_xor(az, o);
    }
    if (lane == 0) red[wave][0] = aw, red[wave][1] = ax, red[wave][2] = ay, red[wave][3] = az;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float gq4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gq4[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    // ---- the head's backward of row b (pcrnet_head_bwd_kernel) with gq4 (+ an explicit g_quat) as the normalised quaternion's gradient
    const float gqn = g_qnorm ? g_qnorm[0] : 0.f;
    const float *r = y + (size_t)b * 7;
    const float n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
    const float nrm = sqrtf(n2);
    float *o = g_y + (size_t)b * 7;
    float gt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gt[i] = (g_twist ? g_twist[(size_t)b * 7 + i] : 0.f) + ((g ? gq4[i] : 0.f) + (g_quat ? g_quat[b * 4 + i] : 0.f));
    float gp[4];
    if (nrm > 1e-12f) {
        const float inv = 1.0f / nrm;
        const float qq[4] = {r[0] * inv, r[1] * inv, r[2] * inv, r[3] * inv};
        const float dot = qq[0] * gt[0] + qq[1] * gt[1] + qq[2] * gt[2] + qq[3] * gt[3];
#pragma unroll
        for (int i = 0; i < 4; ++i) gp[i] = (gt[i] - qq[i] * dot) * inv;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) gp[i] = gt[i] * 1e12f;
    }
#pragma unroll
    for (int i = 4; i < 7; ++i) o[i] = g_twist ? g_twist[(size_t)b * 7 + i] : 0.f;
    const float cq = gqn * 4.0f * (n2 - 1.0f) / (float)B;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = gp[i] + cq * r[i];
}

// y (B,7), v (B,N,3) -> twist (B,7), quat (B,4), qnorm (scalar, may be NULL), out (B,N,3) = v rotated by quat.
extern "C" int sn_pcrnet_head_rot_forward(int B, int N, const float *y, const float *v, float *twist, float *quat, float *qnorm,
                                          float *out, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && N >= 1 && y && v && twist && quat && out, "bad argument");
    hipLaunchKernelGGL(pcrnet_head_rot_fwd_kernel, dim3(std::min((N + 255) / 256, 64), B), dim3(256), 0, (hipStream_t)stream, B, N, y, v,
                       twist, quat, qnorm, out, 0);
    SN_LAUNCH_CHECK();
    return 0;
}
// R = E * group rows: E evaluations against the SAME `group` template clouds v (group, N, 3); qnorm: E values (may be NULL)
extern "C" int sn_pcrnet_head_rot_forward_grouped(int R, int N, int group, const float *y, const float *v, float *twist, float *quat,
                                                  float *qnorm, float *out, sn_stream_t stream)
{
    SN_REQUIRE(R >= 1 && N >= 1 && group >= 1 && R % group == 0 && y && v && twist && quat && out, "bad argument");
    hipLaunchKernelGGL(pcrnet_head_rot_fwd_kernel, dim3(std::min((N + 255) / 256, 64), R), dim3(256), 0, (hipStream_t)stream, R, N, y, v,
                       twist, quat, qnorm, out, group);
    SN_LAUNCH_CHECK();
    return 0;
}

// Backward of sn_pcrnet_head_rot_forward: grad_out (B,N,3) (NULL: no gradient came through the rotated cloud), grad_twist (B,7),
// grad_quat (B,4), grad_qnorm (scalar) -- each may be NULL -- -> grad_y (B,7) and, when grad_v != NULL, grad_v (B,N,3) (needs grad_out).
extern "C" int sn_pcrnet_head_rot_backward(int B, int N, const float *y, const float *quat, const float *v, const float *grad_out,
                                           const float *grad_twist, const float *grad_quat, const float *grad_qnorm, float *grad_v,
                                           float *grad_y, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && N >= 1 && y && quat && v && grad_y, "bad argument");
    SN_REQUIRE(!grad_v || grad_out, "grad_v needs grad_out");
    hipLaunchKernelGGL(pcrnet_head_rot_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, B, N, y, quat, v, grad_out, grad_twist,
                       grad_quat, grad_qnorm, grad_v, grad_y, 0);
    SN_LAUNCH_CHECK();
    return 0;
}
// backward of the grouped form: grad_qnorm E values (may be NULL); no gradient to the shared template clouds
extern "C" int sn_pcrnet_head_rot_backward_grouped(int R, int N, int group, const float *y, const float *quat, const float *v,
                                                   const float *grad_out, const float *grad_twist, const float *grad_quat,
                                                   const float *grad_qnorm, float *grad_y, sn_stream_t stream)
{
    SN_REQUIRE(R >= 1 && N >= 1 && group >= 1 && R % group == 0 && y && quat && v && grad_y, "bad argument");
    hipLaunchKernelGGL(pcrnet_head_rot_bwd_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, R, N, y, quat, v, grad_out, grad_twist,
                       grad_quat, grad_qnorm, (float *)nullptr, grad_y, group);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_qrot_forward(int B, int N, const float *quat, const float *v, float *out, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && N >= 0, "negative size");
    if (B == 0 || N == 0) return 0;
    SN_REQUIRE(quat && v && out, "null pointer");
    hipLaunchKernelGGL(qrot_fwd_kernel, dim3(std::min((N + 255) / 256, 64), B), dim3(256), 0, (hipStream_t)stream, N, quat, v, out);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_qrot_backward(int B, int N, const float *quat, const float *v, const float *grad_out, float *grad_quat,
                                float *grad_v, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && N >= 0, "negative size");
    if (B == 0) return 0;
    SN_REQUIRE(quat && v && grad_out && (grad_quat || grad_v), "null pointer");
    hipLaunchKernelGGL(qrot_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, N, quat, v, grad_out, grad_quat, grad_v);
    SN_LAUNCH_CHECK();
    return 0;
}

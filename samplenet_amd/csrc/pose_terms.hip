// pose_terms.hip -- the pose-error terms of the registration task loss and of its evaluation
// (registration/src/qdataset.py:62-95 QuaternionTransform.compute_errors, registration/main.py:579-585 `--loss-type 0`) and the
// per-cloud Chamfer mean the batched evaluation needs (main.py:540-555, 573-577 one cloud at a time).
//
// Every expression below is written out operation by operation and the file is compiled with -ffp-contract=off: the order of the
// fp32 operations is the contract tests/pose_ref.py counts its bounds from.  Where a comment says "left to right" the sum
// a + b + c + d is ((a + b) + c) + d.
#pragma clang fp contract(off)
#include "sn_common.h"

namespace {

constexpr int kPoseThreads = 256;

// rotation matrix (row-major, 9 entries) of a UNIT quaternion (w, x, y, z); 1 - 2 (a + b) and 2 (a +- b), products first
__device__ __forceinline__ void quat_to_matrix(const float w, const float x, const float y, const float z, float R[9])
{
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, xz = x * z, yz = y * z;
    const float wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0f - 2.0f * (yy + zz), R[1] = 2.0f * (xy - wz), R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz), R[4] = 1.0f - 2.0f * (xx + zz), R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy), R[7] = 2.0f * (yz + wx), R[8] = 1.0f - 2.0f * (xx + yy);
}

// q / max(||q||, 1e-12): squares summed left to right, one square root, four divisions; -> the denominator
__device__ __forceinline__ float quat_normalize(const float *__restrict__ q, float n[4])
{
    const float s = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const float den = fmaxf(sqrtf(s), 1e-12f);
    n[0] = q[0] / den, n[1] = q[1] / den, n[2] = q[2] / den, n[3] = q[3] / den;
    return den;
}

// D = R1 R2^T - I (row-major): every product entry a three-term sum left to right, then the diagonal's - 1
__device__ __forceinline__ void matrix_deviation(const float R1[9], const float R2[9], float D[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float m = R1[i * 3 + 0] * R2[j * 3 + 0] + R1[i * 3 + 1] * R2[j * 3 + 1] + R1[i * 3 + 2] * R2[j * 3 + 2];
            D[i * 3 + j] = i == j ? m - 1.0f : m;
        }
}

// One workgroup: thread t takes the clouds t, t + 256, ... (any B); the batch means are each thread's partial sum in that
// order, then a halving tree over the 256 partials (pcrnet_head_fwd_kernel's order), then one division by B.
__global__ void __launch_bounds__(kPoseThreads) pose_error_fwd_kernel(int B, const float *__restrict__ est, const float *__restrict__ gt,
                                                                       float *__restrict__ rot_err, float *__restrict__ norm_err,
                                                                       float *__restrict__ trans_err, float *__restrict__ means)
{
    __shared__ float red[3][kPoseThreads];
    const int t = threadIdx.x;
    float ar = 0.f, an = 0.f, at = 0.f;
    for (int b = t; b < B; b += kPoseThreads) {
        const float *e = est + (size_t)b * 7, *g = gt + (size_t)b * 7;
        // rot_err: the quaternions AS GIVEN (qdataset.py:85); the clamp is the deviation from the reference (NaN where rounding
        // lifts 2 d^2 - 1 above 1); a NaN argument stays NaN (fminf / fmaxf would drop it)
        const float d = e[0] * g[0] + e[1] * g[1] + e[2] * g[2] + e[3] * g[3];
        const float x = 2.0f * (d * d) - 1.0f;
        const float xc = x != x ? x : fminf(fmaxf(x, -1.0f), 1.0f);
        const float r = 2.0f * acosf(xc);
        // norm_err: || R(q1) R(q2)^T - I ||_F^2 on the NORMALISED quaternions, nine squares summed in row-major order
        float n1[4], n2[4], R1[9], R2[9], D[9];
        quat_normalize(e, n1);
        quat_normalize(g, n2);
        quat_to_matrix(n1[0], n1[1], n1[2], n1[3], R1);
        quat_to_matrix(n2[0], n2[1], n2[2], n2[3], R2);
        matrix_deviation(R1, R2, D);
        float nerr = D[0] * D[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) nerr = nerr + D[k] * D[k];
        // trans_err: mean |dt| over the three components (qdataset.py:93 takes sqrt(dt^2))
        const float terr = (fabsf(e[4] - g[4]) + fabsf(e[5] - g[5]) + fabsf(e[6] - g[6])) / 3.0f;
        if (rot_err) rot_err[b] = r;
        if (norm_err) norm_err[b] = nerr;
        if (trans_err) trans_err[b] = terr;
        ar += r, an += nerr, at += terr;
    }
    if (!means) return;
    red[0][t] = ar, red[1][t] = an, red[2][t] = at;
    for (int s = kPoseThreads / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) red[0][t] += red[0][t + s], red[1][t] += red[1][t + s], red[2][t] += red[2][t + s];
    }
    if (t == 0) {  // (thread 0 wrote all three sums in the last step of the tree: it reads only its own writes)
        const float fb = (float)B;
        means[0] = red[0][0] / fb, means[1] = red[1][0] / fb, means[2] = red[2][0] / fb;
    }
}

// g_est (B,7) of  sum_b [ (g_means[1] / B + g_norm_err[b]) norm_err[b] + (g_means[2] / B + g_trans_err[b]) trans_err[b] ];
// rot_err carries no gradient (g_means[0] is not read).
__global__ void __launch_bounds__(kPoseThreads) pose_error_bwd_kernel(int B, const float *__restrict__ est, const float *__restrict__ gt,
                                                                       const float *__restrict__ g_means,
                                                                       const float *__restrict__ g_norm_err,
                                                                       const float *__restrict__ g_trans_err, float *__restrict__ g_est)
{
    const float gmn = g_means ? g_means[1] / (float)B : 0.f, gmt = g_means ? g_means[2] / (float)B : 0.f;
    for (int b = threadIdx.x; b < B; b += kPoseThreads) {
        const float *e = est + (size_t)b * 7, *g = gt + (size_t)b * 7;
        float *o = g_est + (size_t)b * 7;
        const float wn = gmn + (g_norm_err ? g_norm_err[b] : 0.f);
        const float wt = gmt + (g_trans_err ? g_trans_err[b] : 0.f);
        float n1[4], n2[4], R1[9], R2[9], D[9], G[9];
        const float den = quat_normalize(e, n1);
        quat_normalize(g, n2);
        quat_to_matrix(n1[0], n1[1], n1[2], n1[3], R1);
        quat_to_matrix(n2[0], n2[1], n2[2], n2[3], R2);
        matrix_deviation(R1, R2, D);
        // d norm_err / d R1 = 2 D R2  (norm_err = sum D^2, D = R1 R2^T - I), times the cloud's upstream weight
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                G[i * 3 + k] = wn * (2.0f * (D[i * 3 + 0] * R2[0 * 3 + k] + D[i * 3 + 1] * R2[1 * 3 + k] + D[i * 3 + 2] * R2[2 * 3 + k]));
        // through quat_to_matrix to the normalised quaternion n = (w, x, y, z)
        const float w = n1[0], x = n1[1], y = n1[2], z = n1[3];
        float gn[4];
        gn[0] = 2.0f * (z * (G[3] - G[1]) + y * (G[2] - G[6]) + x * (G[7] - G[5]));
        gn[1] = 2.0f * (y * (G[1] + G[3]) + z * (G[2] + G[6]) + w * (G[7] - G[5]) - 2.0f * x * (G[4] + G[8]));
        gn[2] = 2.0f * (x * (G[1] + G[3]) + z * (G[5] + G[7]) + w * (G[2] - G[6]) - 2.0f * y * (G[0] + G[8]));
        gn[3] = 2.0f * (x * (G[2] + G[6]) + y * (G[5] + G[7]) + w * (G[3] - G[1]) - 2.0f * z * (G[0] + G[4]));
        // through the normalisation: (g_n - n (n . g_n)) / max(||q||, 1e-12)
        const float dot = n1[0] * gn[0] + n1[1] * gn[1] + n1[2] * gn[2] + n1[3] * gn[3];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (gn[i] - n1[i] * dot) / den;
        // d |dt| / d est = sign(dt) with sign(0) = 0 (the reference's sqrt(dt^2) has no derivative there: NaN); a NaN stays
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float dt = e[4 + c] - g[4 + c];
            const float sg = dt != dt ? dt : (dt > 0.f ? 1.0f : (dt < 0.f ? -1.0f : 0.f));
            o[4 + c] = wt * (sg / 3.0f);
        }
    }
}

// out[b] = mean(dist1[b, :]) + mean(dist2[b, :]): one workgroup per cloud, strided per-thread partials and a halving tree
// (simp_loss_partial_kernel's order), one division per side.
__global__ void __launch_bounds__(256) chamfer_mean_per_cloud_kernel(int n1, int n2, const float *__restrict__ d1,
                                                                     const float *__restrict__ d2, float *__restrict__ out)
{
    __shared__ float r1[256], r2[256];
    const int b = blockIdx.x, t = threadIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int j = t; j < n1; j += 256) s1 += d1[(size_t)b * n1 + j];
    for (int j = t; j < n2; j += 256) s2 += d2[(size_t)b * n2 + j];
    r1[t] = s1, r2[t] = s2;
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) r1[t] += r1[t + s], r2[t] += r2[t + s];
    }
    if (t == 0) out[b] = r1[0] / (float)n1 + r2[0] / (float)n2;
}

}  // namespace

extern "C" int sn_pose_error_forward(int B, const float *est, const float *gt, float *rot_err, float *norm_err, float *trans_err,
                                     float *means, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0, "negative batch");
    if (B == 0 || !(rot_err || norm_err || trans_err || means)) return 0;
    SN_REQUIRE(est && gt, "null pointer");
    hipLaunchKernelGGL(pose_error_fwd_kernel, dim3(1), dim3(kPoseThreads), 0, (hipStream_t)stream, B, est, gt, rot_err, norm_err,
                       trans_err, means);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_pose_error_backward(int B, const float *est, const float *gt, const float *g_means, const float *g_norm_err,
                                      const float *g_trans_err, float *g_est, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0, "negative batch");
    if (B == 0) return 0;
    SN_REQUIRE(est && gt && g_est, "null pointer");
    hipLaunchKernelGGL(pose_error_bwd_kernel, dim3(1), dim3(kPoseThreads), 0, (hipStream_t)stream, B, est, gt, g_means, g_norm_err,
                       g_trans_err, g_est);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_chamfer_mean_per_cloud(int B, int n1, int n2, const float *dist1, const float *dist2, float *out, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && n1 >= 1 && n2 >= 1, "bad size");
    if (B == 0) return 0;
    SN_REQUIRE(dist1 && dist2 && out, "null pointer");
    hipLaunchKernelGGL(chamfer_mean_per_cloud_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, n1, n2, dist1, dist2, out);
    SN_LAUNCH_CHECK();
    return 0;
}

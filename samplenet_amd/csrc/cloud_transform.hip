// cloud_transform.hip -- the per-cloud transforms of PointNet's classifier (classification/models/pointnet_cls.py:27-29, 55-59:
// every cloud's points times that cloud's own 3 x 3 matrix, its 64-channel features times its own 64 x 64 matrix), their gradients
// to both operands, and the orthogonality regulariser of the feature transform (pointnet_cls.py:124-130).
//
//   Y[b] = X[b] . T[b]        X (B, N, K) row-major, T (B, K, K), K in {3, 64}
//   dX[b] = dY[b] . T[b]^T    dT[b] = X[b]^T . dY[b]
//
// K = 64 runs on v_mfma_f32_32x32x2_f32 (true fp32: every product rounded once into an fp32 accumulator, so integer data whose sums
// stay below 2^24 come out exact); K = 3 on the VALU.  Every sum has one fixed order: nothing is accumulated with atomics.
// The file also holds the element-wise BatchNorm + ReLU of a conv stack's OUTPUT (the GEMM entries apply a layer's activation when
// the NEXT layer loads its operand; the feature transform is no GEMM entry and needs the activated features materialised).
#include "sn_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLd = 65;  // row pitch of a 64 x 64 matrix in LDS: column walks and row walks both hit 32 distinct banks

__device__ __forceinline__ int frag_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// T (64 x 64, global) -> S[r * kLd + c] = T[r][c], or its transpose when TRANS; 256 threads
template <bool TRANS>
__device__ __forceinline__ void stage_t64(const float *__restrict__ T, float *S, int tid)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = (q * 256 + tid) * 4, r = e >> 6, c = e & 63;
        const float4 v = *reinterpret_cast<const float4 *>(T + e);
        if (TRANS) {
            S[(c + 0) * kLd + r] = v.x, S[(c + 1) * kLd + r] = v.y, S[(c + 2) * kLd + r] = v.z, S[(c + 3) * kLd + r] = v.w;
        } else {
            S[r * kLd + c + 0] = v.x, S[r * kLd + c + 1] = v.y, S[r * kLd + c + 2] = v.z, S[r * kLd + c + 3] = v.w;
        }
    }
}

// out[b] (N, 64) = in[b] (N, 64) . M, M = T[b] or T[b]^T.  Workgroup = 128 rows of one cloud, a wave = 32 rows x 64 columns: lane
// (l31, h) holds k = 32 h .. 32 h + 31 of row l31 (eight 16-byte loads, the wave covers its 32 rows completely) and reads M's
// rows k from LDS.  k ascends inside each half, the two halves are added by the matrix core.
template <bool TRANS>
__global__ __launch_bounds__(256) void transform64_kernel(int N, const float *__restrict__ in, const float *__restrict__ T, float *__restrict__ out)
{
    __shared__ float S[64 * kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    stage_t64<TRANS>(T + (size_t)b * 4096, S, tid);
    const int row0 = blockIdx.x * 128 + wave * 32;
    const float *xp = in + ((size_t)b * N + min(row0 + l31, N - 1)) * 64 + h * 32;
    float4 a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = *reinterpret_cast<const float4 *>(xp + 4 * q);
    __syncthreads();
    if (row0 >= N) return;
    f32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc0[e] = 0.f, acc1[e] = 0.f;
    const float *sp = S + (h * 32) * kLd + l31;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * q + j;
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], sp[k * kLd], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], sp[k * kLd + 32], acc1, 0, 0, 0);
        }
    }
    float *op = out + ((size_t)b * N + row0) * 64 + l31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = frag_row(e, lane);
        if (row0 + r < N) {
            op[(size_t)r * 64] = acc0[e];
            op[(size_t)r * 64 + 32] = acc1[e];
        }
    }
}

// dT[b] (64, 64) = X[b]^T . dY[b].  Workgroup (qb, b) owns the 32 x 32 block (qb >> 1, qb & 1) of cloud b; its four waves take the
// four quarters of the rows in ascending order (a quarter = a whole number of 32-row chunks), each stages its chunk's 32 columns of
// X and dY in LDS with 16-byte loads and feeds two rows per MFMA; the quarters are added wave 0 + 1 + 2 + 3: ascending rows.
constexpr int kLc = 36;  // pitch of a staged 32 x 32 chunk: 16-byte aligned rows
__global__ __launch_bounds__(256) void transform64_dt_kernel(int N, const float *__restrict__ X, const float *__restrict__ dY, float *__restrict__ dT)
{
    __shared__ float Xs[4][32 * kLc];
    __shared__ float Ys[4][32 * kLc];
    __shared__ float red[3][32 * 33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, ib = (blockIdx.x >> 1) * 32, jb = (blockIdx.x & 1) * 32;
    const int chunks = ((N + 3) / 4 + 31) / 32;  // per wave
    const float *xb = X + (size_t)b * N * 64 + ib, *yb = dY + (size_t)b * N * 64 + jb;
    float *xs = Xs[wave], *ys = Ys[wave];
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    // staging: lane -> (row = lane / 8 + 8 p, 4 columns at (lane % 8) * 4)
    const int sr = lane >> 3, sc = (lane & 7) * 4;
    for (int c = 0; c < chunks; ++c) {
        const int n0 = (wave * chunks + c) * 32;
        float4 xv[4], yv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int n = n0 + sr + 8 * p;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            xv[p] = n < N ? *reinterpret_cast<const float4 *>(xb + (size_t)n * 64 + sc) : z;
            yv[p] = n < N ? *reinterpret_cast<const float4 *>(yb + (size_t)n * 64 + sc) : z;
        }
        __syncthreads();  // (every wave runs the same number of chunks) the previous chunk's reads are done
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<float4 *>(xs + (sr + 8 * p) * kLc + sc) = xv[p];
            *reinterpret_cast<float4 *>(ys + (sr + 8 * p) * kLc + sc) = yv[p];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 16; ++t)  // rows 2 t + h of the chunk
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(2 * t + h) * kLc + l31], ys[(2 * t + h) * kLc + l31], acc, 0, 0, 0);
    }
    // waves 1..3 leave their block in LDS, wave 0 adds them in order
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) red[wave - 1][frag_row(e, lane) * 33 + l31] = acc[e];
    }
    __syncthreads();
    if (wave > 0) return;
    float *op = dT + (size_t)b * 4096 + (size_t)ib * 64 + jb + l31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = frag_row(e, lane);
        float v = acc[e];
        v += red[0][r * 33 + l31];
        v += red[1][r * 33 + l31];
        v += red[2][r * 33 + l31];
        op[(size_t)r * 64] = v;
    }
}

// K = 3: a thread per point, k ascending.  TRANS: the product with T^T (the data gradient).
template <bool TRANS>
__global__ __launch_bounds__(256) void transform3_kernel(int N, const float *__restrict__ in, const float *__restrict__ T, float *__restrict__ out)
{
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    float t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = T[b * 9 + i];
    if (n >= N) return;
    const float *x = in + ((size_t)b * N + n) * 3;
    float *y = out + ((size_t)b * N + n) * 3;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float m0 = TRANS ? t[j * 3 + 0] : t[0 + j], m1 = TRANS ? t[j * 3 + 1] : t[3 + j], m2 = TRANS ? t[j * 3 + 2] : t[6 + j];
        y[j] = fmaf(x2, m2, fmaf(x1, m1, x0 * m0));
    }
}

// dT[b] (3, 3) = X[b]^T . dY[b]: one workgroup per cloud; thread t adds rows t, t + 256, ... in ascending order, the 256 partials
// are added by a fixed binary tree.
__global__ __launch_bounds__(256) void transform3_dt_kernel(int N, const float *__restrict__ X, const float *__restrict__ dY, float *__restrict__ dT)
{
    __shared__ float red[9][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0.f;
    for (int n = tid; n < N; n += 256) {
        const float *x = X + ((size_t)b * N + n) * 3, *g = dY + ((size_t)b * N + n) * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2], g0 = g[0], g1 = g[1], g2 = g[2];
        s[0] = fmaf(x0, g0, s[0]), s[1] = fmaf(x0, g1, s[1]), s[2] = fmaf(x0, g2, s[2]);
        s[3] = fmaf(x1, g0, s[3]), s[4] = fmaf(x1, g1, s[4]), s[5] = fmaf(x1, g2, s[5]);
        s[6] = fmaf(x2, g0, s[6]), s[7] = fmaf(x2, g1, s[7]), s[8] = fmaf(x2, g2, s[8]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) red[i][tid] = s[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int i = 0; i < 9; ++i) red[i][tid] += red[i][tid + w];
        }
        __syncthreads();
    }
    if (tid < 9) dT[b * 9 + tid] = red[tid][0];
}

// ---- orthogonality regulariser: one workgroup per cloud, T and M = T T^T - I in LDS (K <= 64) ----------------------------------
__device__ __forceinline__ void ortho_stage(int K, const float *__restrict__ T, float *Ts, float *Ms, int tid)
{
    for (int e = tid; e < K * K; e += 256) Ts[(e / K) * kLd + e % K] = T[e];
    __syncthreads();
    for (int e = tid; e < K * K; e += 256) {
        const int i = e / K, j = e % K;
        float s = 0.f;
        for (int k = 0; k < K; ++k) s = fmaf(Ts[i * kLd + k], Ts[j * kLd + k], s);
        Ms[i * kLd + j] = s - (i == j ? 1.f : 0.f);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void ortho_forward_kernel(int K, const float *__restrict__ T, float *__restrict__ partial)
{
    __shared__ float Ts[64 * kLd];
    __shared__ float Ms[64 * kLd];
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    ortho_stage(K, T + (size_t)b * K * K, Ts, Ms, tid);
    float s = 0.f;
    for (int e = tid; e < K * K; e += 256) {
        const float m = Ms[(e / K) * kLd + e % K];
        s = fmaf(m, m, s);
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial[b] = 0.5f * red[0];
}

__global__ void ortho_sum_kernel(int B, const float *__restrict__ partial, float *__restrict__ loss)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += partial[b];  // ascending cloud order
    loss[0] = s;
}

// dT[b] = g * 2 (T T^T - I) T
__global__ __launch_bounds__(256) void ortho_backward_kernel(int K, const float *__restrict__ T, const float *__restrict__ grad_loss, float *__restrict__ dT)
{
    __shared__ float Ts[64 * kLd];
    __shared__ float Ms[64 * kLd];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float g2 = 2.f * grad_loss[0];
    ortho_stage(K, T + (size_t)b * K * K, Ts, Ms, tid);
    for (int e = tid; e < K * K; e += 256) {
        const int i = e / K, c = e % K;
        float s = 0.f;
        for (int j = 0; j < K; ++j) s = fmaf(Ms[i * kLd + j], Ts[j * kLd + c], s);
        dT[(size_t)b * K * K + e] = g2 * s;
    }
}

// ---- y = relu(scale z + shift) per channel, and dy = g [y > 0] -------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_relu_kernel(long long n4, int C, const float *__restrict__ z, const float *__restrict__ coef,
                                                     const float *__restrict__ g, int with_scale, float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    const float4 v = reinterpret_cast<const float4 *>(z)[i];
    const float4 sc = *reinterpret_cast<const float4 *>(coef + c), sh = *reinterpret_cast<const float4 *>(coef + C + c);
    float4 y = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
    if (g) {
        const float4 gv = reinterpret_cast<const float4 *>(g)[i];
        y = make_float4(y.x > 0.f ? gv.x : 0.f, y.y > 0.f ? gv.y : 0.f, y.z > 0.f ? gv.z : 0.f, y.w > 0.f ? gv.w : 0.f);
        if (with_scale) y = make_float4(y.x * sc.x, y.y * sc.y, y.z * sc.z, y.w * sc.w);
    } else {
        y = make_float4(fmaxf(y.x, 0.f), fmaxf(y.y, 0.f), fmaxf(y.z, 0.f), fmaxf(y.w, 0.f));
    }
    reinterpret_cast<float4 *>(out)[i] = y;
}

}  // namespace

extern "C" int sn_cloud_transform_forward(int B, int N, int K, const float *X, const float *T, float *Y, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && N >= 0, "negative size");
    SN_REQUIRE(K == 3 || K == 64, "K must be 3 or 64");
    SN_REQUIRE(B <= 65535, "B > 65535");
    if (B == 0 || N == 0) return 0;
    SN_REQUIRE(X && T && Y, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (K == 64)
        transform64_kernel<false><<<dim3((N + 127) / 128, B), 256, 0, st>>>(N, X, T, Y);
    else
        transform3_kernel<false><<<dim3((N + 255) / 256, B), 256, 0, st>>>(N, X, T, Y);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_cloud_transform_backward(int B, int N, int K, const float *X, const float *T, const float *dY, float *dX, float *dT,
                                           sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && N >= 0, "negative size");
    SN_REQUIRE(K == 3 || K == 64, "K must be 3 or 64");
    SN_REQUIRE(B <= 65535, "B > 65535");
    if (B == 0) return 0;
    SN_REQUIRE(dY && (!dX || T) && (!dT || X), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dX && N > 0) {
        if (K == 64)
            transform64_kernel<true><<<dim3((N + 127) / 128, B), 256, 0, st>>>(N, dY, T, dX);
        else
            transform3_kernel<true><<<dim3((N + 255) / 256, B), 256, 0, st>>>(N, dY, T, dX);
        SN_LAUNCH_CHECK();
    }
    if (dT) {  // (N == 0: the empty sum, zeros)
        if (K == 64)
            transform64_dt_kernel<<<dim3(4, B), 256, 0, st>>>(N, X, dY, dT);
        else
            transform3_dt_kernel<<<B, 256, 0, st>>>(N, X, dY, dT);
        SN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int sn_orthogonality_loss_forward(int B, int K, const float *T, float *partial, float *loss, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0, "negative size");
    SN_REQUIRE(K == 3 || K == 64, "K must be 3 or 64");
    if (B == 0) return 0;
    SN_REQUIRE(T && partial && loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    ortho_forward_kernel<<<B, 256, 0, st>>>(K, T, partial);
    SN_LAUNCH_CHECK();
    ortho_sum_kernel<<<1, 64, 0, st>>>(B, partial, loss);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_orthogonality_loss_backward(int B, int K, const float *T, const float *grad_loss, float *dT, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0, "negative size");
    SN_REQUIRE(K == 3 || K == 64, "K must be 3 or 64");
    if (B == 0) return 0;
    SN_REQUIRE(T && grad_loss && dT, "null pointer");
    ortho_backward_kernel<<<B, 256, 0, (hipStream_t)stream>>>(K, T, grad_loss, dT);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_bn_relu_forward(long long R, int C, const float *z, const float *coef, float *y, sn_stream_t stream)
{
    SN_REQUIRE(R >= 0 && C >= 0, "negative size");
    SN_REQUIRE(C % 4 == 0, "C must be a multiple of 4");
    const long long n4 = R * C / 4;
    SN_REQUIRE(n4 <= 0x7fffffffLL * 256, "too many elements");
    if (n4 == 0) return 0;
    SN_REQUIRE(z && coef && y, "null pointer");
    bn_relu_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(n4, C, z, coef, nullptr, 0, y);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_bn_relu_backward(long long R, int C, const float *z, const float *coef, const float *g, int with_scale, float *dy,
                                   sn_stream_t stream)
{
    SN_REQUIRE(R >= 0 && C >= 0, "negative size");
    SN_REQUIRE(C % 4 == 0, "C must be a multiple of 4");
    const long long n4 = R * C / 4;
    SN_REQUIRE(n4 <= 0x7fffffffLL * 256, "too many elements");
    if (n4 == 0) return 0;
    SN_REQUIRE(z && coef && g && dy, "null pointer");
    bn_relu_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(n4, C, z, coef, g, with_scale, dy);
    SN_LAUNCH_CHECK();
    return 0;
}

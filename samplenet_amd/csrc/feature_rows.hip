// feature_rows.hip -- what a PointNet++ feature-propagation (up-sampling) level needs around the GEMM walk (gfx950): the level's
// input assembled in the ROW layout the GEMM entries read (the three-neighbour interpolation of the known features beside the skip
// features, channels contiguous), the deterministic gradient of that interpolation by inverted index on the same layout, and the
// backward of the walk's top activation with the top BatchNorm's partial sums in the same launch.  The query stays sn_three_nn
// (feature_propagate.hip).  The contracts are written out in include/samplenet_hip_internal.h; tests/fp_rows_ref.py restates them.
//
// sn_interp_rows_forward      a group of LG lanes (the power of two covering the c2 + c1 columns, 64 at most) owns an output row and
//     walks its columns LG at a time: stores are fully coalesced, every neighbour read is one contiguous run of c2 floats, the skip
//     row one contiguous run of c1.  The row's three indices, distances and weights are formed once, in front of the column walk,
//     from loads every lane of the group makes at the same address (one transaction); the group's first lane stores the weights.
// sn_interp_rows_backward     a group of LG lanes (the power of two covering c2, 64 at most) owns a destination row of the known cloud
//     and LG of its columns and takes inverse_walk.h's weighted sum over the row's list, three entries to a source row: the terms are
//     fl(grad_rows[e / 3, col] * weights[e]), every read of an entry one contiguous segment.
// sn_bn_relu_backward_stats   dy = g . [relu(scale z + shift) > 0] as sn_bn_relu_backward writes it, and (sum dy, sum fl(dy * z))
//     over blocks of kBsRows rows, each in one fixed order: the layout sn_bn_backward_coef reduces.
// No workspace, no atomics: deterministic, safe under stream capture.
#include <cmath>

#include "inverse_walk.h"

#pragma clang fp contract(off)  // every product and sum of the contracts is rounded on its own (the activation's one fmaf is written out)

namespace sn {
namespace {

constexpr int kFrThreads = kLaneThreads;

// ------------------------------------------------------------------------------------------------ the assembly
struct InterpArgs {
    int m, c2, c1, rule, lg;
    long long rows;               // b * n
    int n;
    const float *known_rows;      // (b,m,c2)
    const float *skip_rows;       // (b,n,c1), NULL with c1 == 0
    const int *idx;               // (b,n,3)
    const float *dist2;           // (b,n,3)
    float *weights;               // (b,n,3)
    float *out;                   // (b,n,c2+c1)
};

__device__ __forceinline__ float recip_weight(float d2, int rule)
{
    return rule == 0 ? 1.f / (sqrtf(d2) + 1e-8f) : 1.f / fmaxf(d2, 1e-10f);   // sqrtf, / : correctly rounded (hipcc's default, kept)
}

__global__ void __launch_bounds__(kFrThreads) interp_rows_kernel(const InterpArgs a)
{
    const int per = kFrThreads / a.lg;
    const int sub = threadIdx.x / a.lg, l = threadIdx.x - sub * a.lg;
    const long long row = (long long)blockIdx.x * per + sub;   // cloud * n + j
    if (row >= a.rows) return;
    const long long cloud = row / a.n;
    const int *id = a.idx + row * 3;
    const float *d = a.dist2 + row * 3;
    // an index outside [0, m) is CLAMPED into the cloud
    const int i0 = min(max(id[0], 0), a.m - 1), i1 = min(max(id[1], 0), a.m - 1), i2 = min(max(id[2], 0), a.m - 1);
    const float r0 = recip_weight(d[0], a.rule), r1 = recip_weight(d[1], a.rule), r2 = recip_weight(d[2], a.rule);
    const float norm = (r0 + r1) + r2;
    const float w0 = r0 / norm, w1 = r1 / norm, w2 = r2 / norm;
    if (l == 0) {
        float *w = a.weights + row * 3;
        w[0] = w0, w[1] = w1, w[2] = w2;
    }
    const float *K = a.known_rows + (size_t)cloud * a.m * a.c2;
    const float *f0 = K + (size_t)i0 * a.c2, *f1 = K + (size_t)i1 * a.c2, *f2 = K + (size_t)i2 * a.c2;
    const float *s = a.skip_rows + (size_t)row * a.c1 - a.c2;   // (read at col >= c2 only)
    const int width = a.c2 + a.c1;
    float *o = a.out + (size_t)row * width;
    for (int col = l; col < width; col += a.lg) {
        float v;
        if (col < a.c2)
            v = ((w0 * f0[col]) + (w1 * f1[col])) + (w2 * f2[col]);
        else
            v = s[col];
        o[col] = v;
    }
}

// ------------------------------------------------------------------------------------------------ its gradient
struct InterpGradArgs {
    int m, ne, c2, Ci, lg, chunks;
    long long items;              // b * m * chunks (row, chunk) pairs
    const float *weights;         // (b,ne)
    const float *grad_rows;       // (b,n,Ci)
    const int *start;             // (b,m+1)
    const int *order;             // (b,ne)
    float *grad_known;            // (b,m,c2)
};

__global__ void __launch_bounds__(kFrThreads) interp_rows_backward_kernel(const InterpGradArgs a)
{
    const int per = kFrThreads / a.lg;
    const int sub = threadIdx.x / a.lg, l = threadIdx.x - sub * a.lg;
    const long long item = (long long)blockIdx.x * per + sub;
    if (item >= a.items) return;
    const long long rowi = item / a.chunks;                 // cloud * m + r
    const int chunk = (int)(item - rowi * a.chunks);
    const long long cloud = rowi / a.m;
    const int col = chunk * a.lg + l;
    if (col >= a.c2) return;
    const int *start = a.start + rowi + cloud;              // cloud * (m + 1) + r
    const int *order = a.order + (size_t)cloud * a.ne;
    const float *w = a.weights + (size_t)cloud * a.ne;
    const float *g = a.grad_rows + (size_t)cloud * (a.ne / 3) * a.Ci + col;
    a.grad_known[rowi * a.c2 + col] = inverse_walk_sum<3, true>(start, order, a.ne, g, a.Ci, w);
}

// ------------------------------------------------------------------------------------------------ top activation backward + sums
constexpr int kBsRows = 256;   // rows per block of partial sums

// A workgroup owns one block of kBsRows rows and LR float4 columns of it (LR: the power of two covering C / 4, 64 at most);
// S = 256 / LR slices.  Slice q adds the block's rows q, q + S, .. ascending; the S slice sums are then added in slice order.
__global__ void __launch_bounds__(kFrThreads) bn_relu_bwd_stats_kernel(long long R, int C, int lr, const float *__restrict__ z,
                                                                      const float *__restrict__ coef, const float *__restrict__ g,
                                                                      float *__restrict__ dy, float *__restrict__ stats)
{
    __shared__ float4 red[2][kFrThreads];
    const int S = kFrThreads / lr;
    const int sl = threadIdx.x / lr, cl = threadIdx.x - sl * lr;
    const int c = (blockIdx.y * lr + cl) * 4;
    const long long r0 = (long long)blockIdx.x * kBsRows;
    const int rows = R - r0 < kBsRows ? (int)(R - r0) : kBsRows;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), sz = s;
    if (c < C) {
        const float4 sc = *reinterpret_cast<const float4 *>(coef + c), sh = *reinterpret_cast<const float4 *>(coef + C + c);
        const size_t base = (size_t)r0 * C + c;
        int r = sl;
        for (; r + 3 * S < rows; r += 4 * S) {   // four trips' loads in flight; the sums keep their ascending order
            float4 zv[4], gv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t o = base + (size_t)(r + i * S) * C;
                zv[i] = *reinterpret_cast<const float4 *>(z + o), gv[i] = *reinterpret_cast<const float4 *>(g + o);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4 d;
                d.x = fmaf(zv[i].x, sc.x, sh.x) > 0.f ? gv[i].x : 0.f;   // bn_relu_kernel's expression
                d.y = fmaf(zv[i].y, sc.y, sh.y) > 0.f ? gv[i].y : 0.f;
                d.z = fmaf(zv[i].z, sc.z, sh.z) > 0.f ? gv[i].z : 0.f;
                d.w = fmaf(zv[i].w, sc.w, sh.w) > 0.f ? gv[i].w : 0.f;
                *reinterpret_cast<float4 *>(dy + base + (size_t)(r + i * S) * C) = d;
                s.x += d.x, s.y += d.y, s.z += d.z, s.w += d.w;
                sz.x += d.x * zv[i].x, sz.y += d.y * zv[i].y, sz.z += d.z * zv[i].z, sz.w += d.w * zv[i].w;
            }
        }
        for (; r < rows; r += S) {
            const size_t o = base + (size_t)r * C;
            const float4 zv = *reinterpret_cast<const float4 *>(z + o), gv = *reinterpret_cast<const float4 *>(g + o);
            float4 d;
            d.x = fmaf(zv.x, sc.x, sh.x) > 0.f ? gv.x : 0.f;
            d.y = fmaf(zv.y, sc.y, sh.y) > 0.f ? gv.y : 0.f;
            d.z = fmaf(zv.z, sc.z, sh.z) > 0.f ? gv.z : 0.f;
            d.w = fmaf(zv.w, sc.w, sh.w) > 0.f ? gv.w : 0.f;
            *reinterpret_cast<float4 *>(dy + o) = d;
            s.x += d.x, s.y += d.y, s.z += d.z, s.w += d.w;
            sz.x += d.x * zv.x, sz.y += d.y * zv.y, sz.z += d.z * zv.z, sz.w += d.w * zv.w;
        }
    }
    red[0][threadIdx.x] = s, red[1][threadIdx.x] = sz;
    __syncthreads();
    if (sl == 0 && c < C) {
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
        for (int q = 0; q < S; ++q) {
            const float4 u = red[0][q * lr + cl], v = red[1][q * lr + cl];
            a0.x += u.x, a0.y += u.y, a0.z += u.z, a0.w += u.w;
            a1.x += v.x, a1.y += v.y, a1.z += v.z, a1.w += v.w;
        }
        float *st = stats + (size_t)blockIdx.x * 2 * C;
        *reinterpret_cast<float4 *>(st + c) = a0;
        *reinterpret_cast<float4 *>(st + C + c) = a1;
    }
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_interp_rows_forward(int b, int n, int m, int c2, int c1, int rule, const float *known_rows, const float *skip_rows,
                                      const int *idx, const float *dist2, float *weights, float *rows, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c2 >= 0 && c1 >= 0, "negative size");
    SN_REQUIRE(rule == 0 || rule == 1, "bad rule");
    SN_REQUIRE((long long)c2 + c1 >= 1, "no output column (c2 + c1 == 0)");
    SN_REQUIRE((long long)c2 + c1 <= INT_MAX, "c2 + c1 must fit in 31 bits");
    if (b == 0 || n == 0) return 0;
    SN_REQUIRE(m >= 1, "an empty known cloud (m == 0) has no row to read");
    SN_REQUIRE(idx && dist2 && weights && rows && (c2 == 0 || known_rows) && (c1 == 0 || skip_rows), "null pointer");
    LaneGrid l;
    if (int rc = lane_grid(__func__, (long long)b * n, c2 + c1, false, &l)) return rc;
    InterpArgs a = {};
    a.m = m, a.c2 = c2, a.c1 = c1, a.rule = rule, a.lg = l.lg;
    a.rows = l.items, a.n = n;
    a.known_rows = known_rows, a.skip_rows = skip_rows, a.idx = idx, a.dist2 = dist2, a.weights = weights, a.out = rows;
    hipLaunchKernelGGL(interp_rows_kernel, dim3(l.grid), dim3(kFrThreads), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_interp_rows_backward(int b, int n, int m, int c2, int c1, const float *weights, const float *grad_rows, const int *start,
                                       const int *order, float *grad_known, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c2 >= 0 && c1 >= 0, "negative size");
    SN_REQUIRE(3ll * n <= INT_MAX && (long long)c2 + c1 <= INT_MAX, "3 n and c2 + c1 must fit in 31 bits");
    if (b == 0 || m == 0 || c2 == 0) return 0;
    SN_REQUIRE(start && grad_known && (n == 0 || (weights && grad_rows && order)), "null pointer");
    LaneGrid l;
    if (int rc = lane_grid(__func__, (long long)b * m, c2, true, &l)) return rc;
    InterpGradArgs a = {};
    a.m = m, a.ne = 3 * n, a.c2 = c2, a.Ci = c2 + c1, a.lg = l.lg, a.chunks = l.chunks, a.items = l.items;
    a.weights = weights, a.grad_rows = grad_rows, a.start = start, a.order = order, a.grad_known = grad_known;
    hipLaunchKernelGGL(interp_rows_backward_kernel, dim3(l.grid), dim3(kFrThreads), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_bn_relu_stats_blocks(long long R) { return R < 1 || (R + kBsRows - 1) / kBsRows > INT_MAX ? 0 : (int)((R + kBsRows - 1) / kBsRows); }

extern "C" int sn_bn_relu_backward_stats(long long R, int C, const float *z, const float *coef, const float *g, float *dy, float *stats,
                                         sn_stream_t stream)
{
    SN_REQUIRE(R >= 0 && C >= 0, "negative size");
    SN_REQUIRE(C % 4 == 0, "C must be a multiple of 4");
    if (R == 0 || C == 0) return 0;
    SN_REQUIRE(z && coef && g && dy && stats, "null pointer");
    const int lr = lane_group(C / 4);
    const int nblk = sn_bn_relu_stats_blocks(R), cblocks = (C / 4 + lr - 1) / lr;
    if (nblk == 0) return sn_too_many_workgroups(__func__);
    SN_REQUIRE(cblocks <= 65535, "C beyond 65535 * 256 channels");
    hipLaunchKernelGGL(bn_relu_bwd_stats_kernel, dim3((unsigned)nblk, (unsigned)cblocks), dim3(kFrThreads), 0, (hipStream_t)stream, R, C, lr, z,
                       coef, g, dy, stats);
    SN_LAUNCH_CHECK();
    return 0;
}

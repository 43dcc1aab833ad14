// ball_query.hip -- radius neighbourhoods (ball query) and the fused query-and-group of a PointNet++ set abstraction (gfx950).
// Replaces query_ball_point_gpu (classification/grouping/tf_grouping_g.cu:3-36; launcher :125-128, op shell tf_grouping.cpp:66-100,
// Python tf_grouping.py:13-28) and, fused with the gather behind it, Pointnet2_PyTorch's QueryAndGroup (ball_query + grouping_operation
// + the centre subtraction).  CPU twin of the scan: query_ball_point_cpu, classification/grouping/test/query_ball_point.cpp:19-47;
// tests/ball_ref.py restates the contract below in numpy float32 and tests/test_ball_host.py holds that restatement to the twin.
//
// Contract.  Dataset xyz1 (b,n,3) or (b,3,n), queries xyz2 (b,m,3) or (b,3,m).  For query j and dataset point k, all in fp32, every
// operation rounded once, nothing contracted:
//     dx = x2 - x1 (query - dataset), dy, dz likewise;   d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
//     SN_BALL_RULE_SQRT    : s = sqrtf(d2) correctly rounded;  pass = (s < 1e-20f ? 1e-20f : s) < radius     (the reference's rule)
//     SN_BALL_RULE_SQUARED : pass = d2 < fl(radius * radius), and nothing passes unless radius > 0
// A NaN distance passes under neither rule (the twin's std::max keeps the NaN; the comparison is then false).
// Row j of idx holds the FIRST nsample passing indices in ascending order; with 0 < cnt < nsample hits the slots cnt .. nsample-1
// repeat the first hit; pts_cnt[j] = min(hits, nsample).  A row with no hit is written as zeros with pts_cnt 0 (the reference leaves
// such a row unwritten -- whatever the caller's buffer held).
//
// Scan.  A wave owns a query, its lanes own 64 consecutive dataset points per round: one __ballot of the predicate, a lane's slot is
// the running count plus the number of passing lanes below it, only slots < nsample store -- straight to memory, so nothing bounds
// nsample --, and the wave leaves the loop (wave-uniformly: the count lives in scalar registers) as soon as the count reaches
// nsample.  The padding pass is strided over the remaining slots.  A workgroup is four waves; every wave takes 1 to 4 queries in
// sequence -- one while the launch has no more queries than the chip has wave slots, more beyond (ball_queries_per_wave).  The
// dataset is read through the caches: a cloud of a set-abstraction level is 6-24 KB, every wave of a
// workgroup sweeps the same lines at about the same time, and the early exit means most queries never reach the end of the cloud.
// No LDS, no barrier, no workspace, no atomics in the forward kernels: deterministic, safe under stream capture.
#include "ball_scan.h"  // the scan of one query by one wave, the launch rule (shared with set_abstraction.hip)

#pragma clang fp contract(off)  // the contract's distance is product-then-sum (no FMA)

namespace sn {
namespace {

struct BallArgs {
    int n, m, nsample, groups, qpw;   // groups: workgroups per cloud; qpw: queries per wave
    float thr;
    const float *xyz1;
    const float *xyz2;
    int layout1, layout2;
    int *idx;
    int *pts_cnt;                // optional
    // the fused form only (both clouds point-major)
    int c, use_xyz;
    const float *features;       // (b,c,n), NULL with c == 0
    float *out;                  // (b, 3 use_xyz + c, m, nsample)
};

template <int RULE, bool GROUP>
__global__ void __launch_bounds__(kBallWaves *kWave) ball_query_kernel(const BallArgs a)
{
    const int cloud = blockIdx.x / a.groups, group = blockIdx.x - cloud * a.groups;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    const float *P = a.xyz1 + (size_t)cloud * a.n * 3;
    const float *Q = a.xyz2 + (size_t)cloud * a.m * 3;
    const int j0 = (group * kBallWaves + wave) * a.qpw;
    for (int q = 0; q < a.qpw; ++q) {
        const int j = j0 + q;
        if (j >= a.m) return;
        const float qx = Q[pt_off(a.layout2, a.m, j, 0)], qy = Q[pt_off(a.layout2, a.m, j, 1)], qz = Q[pt_off(a.layout2, a.m, j, 2)];
        int *row = a.idx + ((size_t)cloud * a.m + j) * a.nsample;
        const int hits = ball_scan_row<RULE>(a.n, a.nsample, a.thr, P, a.layout1, qx, qy, qz, lane, row);
        if (a.pts_cnt && lane == 0) a.pts_cnt[(size_t)cloud * a.m + j] = hits;
        if (GROUP) {
            // the wave reads back the row its own lanes have just stored: workgroup-scope release / acquire orders the stores of
            // every lane before the loads of every lane (one CU, one L1)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const size_t plane = (size_t)a.m * a.nsample;   // one channel of one cloud
            const int ch = 3 * a.use_xyz + a.c;
            float *o = a.out + (size_t)cloud * ch * plane + (size_t)j * a.nsample;
            const float *F = a.features + (size_t)cloud * a.c * a.n;
            for (int s = lane; s < a.nsample; s += kWave) {
                const int k = row[s];
                if (a.use_xyz) {
                    const float *p = P + (size_t)k * 3;
                    o[s] = p[0] - qx;
                    o[plane + s] = p[1] - qy;
                    o[2 * plane + s] = p[2] - qz;
                }
                float *of = o + (size_t)(3 * a.use_xyz) * plane + s;
                const float *f = F + k;
                int c = 0;
                for (; c + 8 <= a.c; c += 8) {  // eight gathers in flight before the first store
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = f[(size_t)(c + i) * a.n];
#pragma unroll
                    for (int i = 0; i < 8; ++i) of[(size_t)(c + i) * plane] = v[i];
                }
                for (; c < a.c; ++c) of[(size_t)c * plane] = f[(size_t)c * a.n];
            }
        }
    }
}

struct BallGradArgs {
    int n, m, nsample, groups, qpw, c, use_xyz;
    const int *idx;
    const float *grad_out;       // (b, 3 use_xyz + c, m, nsample), read where it lies
    float *grad_features;        // (b,c,n), zeroed by the entry; optional
    float *grad_xyz;             // (b,n,3), zeroed by the entry; optional
    float *grad_new_xyz;         // (b,m,3); optional
};

// A wave owns a query, lane l its slots l, l + 64, ..: the centre's gradient is summed per channel in ONE order -- a lane adds its
// slots ascending, the 64 lane sums meet by the xor tree (offsets 32, 16, .. 1) -- and negated once.  The scatter towards features /
// xyz runs here only for clouds beyond the LDS route (ball_scatter_lds_kernel below): one global float atomic per (slot, channel)
// into a destination the entry has zeroed.
__global__ void __launch_bounds__(kBallWaves *kWave) ball_group_backward_kernel(const BallGradArgs a)
{
    const int cloud = blockIdx.x / a.groups, group = blockIdx.x - cloud * a.groups;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    const size_t plane = (size_t)a.m * a.nsample;
    const int ch = 3 * a.use_xyz + a.c;
    const int j0 = (group * kBallWaves + wave) * a.qpw;
    for (int q = 0; q < a.qpw; ++q) {
        const int j = j0 + q;
        if (j >= a.m) return;
        const int *row = a.idx + ((size_t)cloud * a.m + j) * a.nsample;
        const float *g = a.grad_out + (size_t)cloud * ch * plane + (size_t)j * a.nsample;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int s = lane; s < a.nsample; s += kWave) {
            const int k = row[s];
            const bool ok = k >= 0 && k < a.n;   // an index outside the cloud contributes to no point
            if (a.use_xyz) {
                const float gx = g[s], gy = g[plane + s], gz = g[2 * plane + s];
                sx += gx, sy += gy, sz += gz;
                if (a.grad_xyz && ok) {
                    float *d = a.grad_xyz + ((size_t)cloud * a.n + k) * 3;
                    atomicAdd(d, gx), atomicAdd(d + 1, gy), atomicAdd(d + 2, gz);
                }
            }
            if (a.grad_features && ok) {
                const float *gf = g + (size_t)(3 * a.use_xyz) * plane + s;
                float *d = a.grad_features + (size_t)cloud * a.c * a.n + k;
                int c = 0;
                for (; c + 8 <= a.c; c += 8) {  // eight loads in flight before the first atomic
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = gf[(size_t)(c + i) * plane];
#pragma unroll
                    for (int i = 0; i < 8; ++i) atomicAdd(d + (size_t)(c + i) * a.n, v[i]);
                }
                for (; c < a.c; ++c) atomicAdd(d + (size_t)c * a.n, gf[(size_t)c * plane]);
            }
        }
        if (a.grad_new_xyz) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o), sy += __shfl_xor(sy, o), sz += __shfl_xor(sz, o);
            if (lane == 0) {
                float *d = a.grad_new_xyz + ((size_t)cloud * a.m + j) * 3;
                d[0] = a.use_xyz ? -sx : 0.f, d[1] = a.use_xyz ? -sy : 0.f, d[2] = a.use_xyz ? -sz : 0.f;
            }
        }
    }
}

// The scatter of the backward without a global atomic: a workgroup owns `nc` consecutive gradient channels of one cloud as dense
// rows of n floats in LDS, sweeps ALL m * nsample index entries of the cloud (coalesced reads of idx and of grad_out where it lies),
// adds with LDS float atomics and writes every row out with plain stores -- the destination is overwritten, no zero-fill.  Global
// float atomics of this pattern are 64 scattered dwords per wave-instruction and ran at an eighth of the chip's atomic rate.
constexpr int kBallScatterFloats = 16384;   // LDS accumulator floats per workgroup (64 KB): n <= this takes the LDS route
constexpr int kBallScatterChannels = 16;    // channels per workgroup at most

struct BallScatterArgs {
    int n, nchan, per, slices;     // nchan channels in all, `per` per workgroup, slices = ceil(nchan / per)
    long long entries;             // m * nsample
    int chtot, ch0;                // channels of grad_out, first channel of this scatter
    const int *idx;
    const float *grad_out;
    float *dst;                    // element (cloud, c, k) at dst[cloud * nchan * n + c * c_stride + k * k_stride]
    int c_stride, k_stride;
};

__global__ void __launch_bounds__(256) ball_scatter_lds_kernel(const BallScatterArgs a)
{
    extern __shared__ float acc[];  // per * n
    const int cloud = blockIdx.x / a.slices, slice = blockIdx.x - cloud * a.slices;
    const int c0 = slice * a.per, nc = a.nchan - c0 < a.per ? a.nchan - c0 : a.per;
    const int tot = nc * a.n;
    for (int i = threadIdx.x; i < tot; i += 256) acc[i] = 0.f;
    __syncthreads();
    const int *idx = a.idx + (size_t)cloud * a.entries;
    const float *g = a.grad_out + ((size_t)cloud * a.chtot + a.ch0 + c0) * a.entries;
    for (long long e = threadIdx.x; e < a.entries; e += 256) {
        const int k = idx[e];
        if (k < 0 || k >= a.n) continue;   // an index outside the cloud contributes to no point
        for (int c = 0; c < nc; ++c) atomicAdd(&acc[c * a.n + k], g[(size_t)c * a.entries + e]);
    }
    __syncthreads();
    float *d = a.dst + (size_t)cloud * a.nchan * a.n;
    for (int i = threadIdx.x; i < tot; i += 256) {
        const int c = i / a.n, k = i - c * a.n;
        d[(size_t)(c0 + c) * a.c_stride + (size_t)k * a.k_stride] = acc[i];
    }
}

int ball_scatter_lds(const char *who, int b, int n, long long entries, int chtot, int ch0, int nchan, const int *idx, const float *grad_out,
                     float *dst, int c_stride, int k_stride, hipStream_t st)
{
    BallScatterArgs a = {};
    const int fit = kBallScatterFloats / n;
    a.per = fit < kBallScatterChannels ? fit : kBallScatterChannels;
    if (a.per > nchan) a.per = nchan;
    a.slices = (nchan + a.per - 1) / a.per;
    if ((long long)b * a.slices > INT_MAX) return sn_set_error(SN_ERR_UNSUPPORTED, "%s: the launch needs more than 2^31 - 1 workgroups", who);
    a.n = n, a.nchan = nchan, a.entries = entries, a.chtot = chtot, a.ch0 = ch0, a.idx = idx, a.grad_out = grad_out, a.dst = dst;
    a.c_stride = c_stride, a.k_stride = k_stride;
    hipLaunchKernelGGL(ball_scatter_lds_kernel, dim3((unsigned)(b * a.slices)), dim3(256), (size_t)a.per * n * sizeof(float), st, a);
    return 0;
}

template <bool GROUP>
int ball_launch(int rule, unsigned grid, const BallArgs &a, hipStream_t st)
{
    if (rule == SN_BALL_RULE_SQRT)
        hipLaunchKernelGGL((ball_query_kernel<SN_BALL_RULE_SQRT, GROUP>), dim3(grid), dim3(kBallWaves * kWave), 0, st, a);
    else
        hipLaunchKernelGGL((ball_query_kernel<SN_BALL_RULE_SQUARED, GROUP>), dim3(grid), dim3(kBallWaves * kWave), 0, st, a);
    return 0;
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_ball_query(int b, int n, int m, float radius, int nsample, int rule, const float *xyz1, int layout1, const float *xyz2,
                             int layout2, int *idx, int *pts_cnt, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0, "negative size");
    SN_REQUIRE(nsample >= 1, "nsample must be at least 1");
    SN_REQUIRE(rule == SN_BALL_RULE_SQRT || rule == SN_BALL_RULE_SQUARED, "bad rule");
    SN_REQUIRE((layout1 == SN_LAYOUT_BNC || layout1 == SN_LAYOUT_BCN) && (layout2 == SN_LAYOUT_BNC || layout2 == SN_LAYOUT_BCN), "bad layout");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE(n >= 1, "an empty dataset cloud (n == 0) has no index to return");
    SN_REQUIRE(xyz1 && xyz2 && idx, "null pointer");
    BallArgs a = {};
    unsigned grid;
    if (int rc = ball_grid(__func__, b, m, &a.qpw, &a.groups, &grid)) return rc;
    a.n = n, a.m = m, a.nsample = nsample, a.thr = ball_threshold(radius, rule);
    a.xyz1 = xyz1, a.xyz2 = xyz2, a.layout1 = layout1, a.layout2 = layout2, a.idx = idx, a.pts_cnt = pts_cnt;
    ball_launch<false>(rule, grid, a, (hipStream_t)stream);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_ball_group_forward(int b, int n, int m, int c, float radius, int nsample, int rule, int use_xyz, const float *xyz,
                                     const float *new_xyz, const float *features, int *idx, int *pts_cnt, float *out, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c >= 0, "negative size");
    SN_REQUIRE(nsample >= 1, "nsample must be at least 1");
    SN_REQUIRE(rule == SN_BALL_RULE_SQRT || rule == SN_BALL_RULE_SQUARED, "bad rule");
    SN_REQUIRE(use_xyz == 0 || use_xyz == 1, "use_xyz must be 0 or 1");
    SN_REQUIRE(c > 0 || use_xyz, "no output channel (c == 0 without use_xyz)");
    if (b == 0 || m == 0) return 0;
    SN_REQUIRE(n >= 1, "an empty dataset cloud (n == 0) has no index to return");
    SN_REQUIRE(xyz && new_xyz && idx && out && (c == 0 || features), "null pointer");
    BallArgs a = {};
    unsigned grid;
    if (int rc = ball_grid(__func__, b, m, &a.qpw, &a.groups, &grid)) return rc;
    a.n = n, a.m = m, a.nsample = nsample, a.thr = ball_threshold(radius, rule);
    a.xyz1 = xyz, a.xyz2 = new_xyz, a.layout1 = SN_LAYOUT_BNC, a.layout2 = SN_LAYOUT_BNC, a.idx = idx, a.pts_cnt = pts_cnt;
    a.c = c, a.use_xyz = use_xyz, a.features = features, a.out = out;
    ball_launch<true>(rule, grid, a, (hipStream_t)stream);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_ball_group_backward(int b, int n, int m, int c, int nsample, int use_xyz, const int *idx, const float *grad_out,
                                      float *grad_features, float *grad_xyz, float *grad_new_xyz, sn_stream_t stream)
{
    SN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && c >= 0, "negative size");
    SN_REQUIRE(nsample >= 1, "nsample must be at least 1");
    SN_REQUIRE(use_xyz == 0 || use_xyz == 1, "use_xyz must be 0 or 1");
    SN_REQUIRE(c > 0 || use_xyz, "no output channel (c == 0 without use_xyz)");
    if (b == 0) return 0;
    SN_REQUIRE(m == 0 || (idx && grad_out), "null pointer");
    const hipStream_t st = (hipStream_t)stream;
    if (c == 0) grad_features = nullptr;
    if (n == 0) grad_features = grad_xyz = nullptr;   // (then m == 0 too, or the indices name nothing)
    const long long entries = (long long)m * nsample;
    if (n >= 1 && n <= kBallScatterFloats && m > 0) {
        // the scatter through LDS: every element of the two outputs is written, nothing to zero first
        if (grad_features)
            if (int rc = ball_scatter_lds(__func__, b, n, entries, 3 * use_xyz + c, 3 * use_xyz, c, idx, grad_out, grad_features, n, 1, st)) return rc;
        if (grad_xyz && use_xyz) {
            if (int rc = ball_scatter_lds(__func__, b, n, entries, 3 + c, 0, 3, idx, grad_out, grad_xyz, 1, 3, st)) return rc;
            grad_xyz = nullptr;
        }
        grad_features = nullptr;
    }
    hipError_t e = hipSuccess;
    if (grad_features) e = hipMemsetAsync(grad_features, 0, (size_t)b * c * n * sizeof(float), st);
    if (e == hipSuccess && grad_xyz) e = hipMemsetAsync(grad_xyz, 0, (size_t)b * n * 3 * sizeof(float), st);
    if (e != hipSuccess) return sn_set_error((int)e, "%s: %s", __func__, hipGetErrorString(e));
    if (m == 0) return 0;
    if (!(grad_features || grad_xyz || grad_new_xyz)) {
        SN_LAUNCH_CHECK();   // (of the scatter launches, if any)
        return 0;
    }
    BallGradArgs a = {};
    unsigned grid;
    if (int rc = ball_grid(__func__, b, m, &a.qpw, &a.groups, &grid)) return rc;
    a.n = n, a.m = m, a.nsample = nsample, a.c = c, a.use_xyz = use_xyz, a.idx = idx, a.grad_out = grad_out;
    a.grad_features = c > 0 ? grad_features : nullptr, a.grad_xyz = grad_xyz, a.grad_new_xyz = grad_new_xyz;
    hipLaunchKernelGGL(ball_group_backward_kernel, dim3(grid), dim3(kBallWaves * kWave), 0, st, a);
    SN_LAUNCH_CHECK();
    return 0;
}

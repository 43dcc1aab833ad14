// batch_assemble.hip -- a training batch assembled on the device from an HBM-resident dataset in ONE launch
// (samplenet_amd/device_data.py; the reference does this per item on the host: registration/data/modelnet_loader_torch.py:114-125,
// src/pctransforms.py, src/qdataset.py:133-179).  The contract -- item order, Philox draw layout, the nine stages and their fp32
// operation order, the state block -- is written out in include/samplenet_hip_internal.h above sn_batch_assemble; this file follows
// that text line by line and tests/batch_ref.py restates it in numpy.
//
// One workgroup of 256 threads per output cloud.  LDS: 16 KB of 64-bit sort composites (the point order of the cloud), 48 bytes of
// reduction partials, 8 bytes of (item, epoch).  The cloud itself is NOT staged: a cloud's first N points (24 KB at N = 2048) are read
// where they lie, once per reduction pass of unit_cube and once by the output pass -- the second and third reads are cache hits, and
// the kernel then takes any N <= P without the shuffle.  No scratch memory: nothing is indexed per thread.
//
// State block: as sn_adam_update's -- lane 0 of every workgroup reads the position, then counts itself as arrived (acq_rel, agent
// scope); the last arrival is the only writer.  Nothing waits.
#include "sn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSort = 2048;
constexpr float kTwoPi = 6.28318530717958647692f;

enum : unsigned { kStreamSort = 0, kStreamJitter = 1, kStreamDropout = 2, kStreamPairNoise = 3, kStreamCloud = 4, kStreamAngles = 5,
                  kStreamOrder = 6 };

struct SnBatchState {  // 64 bytes; samplenet_amd/device_data.py addresses word 0 as an int64
    long long position;
    unsigned arrive;  // zero between launches
    unsigned pad[13];
};
static_assert(sizeof(SnBatchState) == 64, "state block layout");

struct BatchArgs {
    const float *points;
    const long long *labels;
    const float *pair_quat;
    float *p0, *p1;
    long long *out_labels;
    float *igt;
    int *items;
    SnBatchState *state;
    long long position;  // < 0: the state block's
    unsigned k0, k1;     // Philox key = seed
    unsigned Lset;
    int L, N, P, B, rank, world, layout, half;  // half = Feistel half width in bits
    float ax, ay, az;                           // unit rotation axis
    sn_batch_recipe r;
};

struct U4 {
    unsigned x, y, z, w;
};

__device__ __forceinline__ U4 philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

__device__ __forceinline__ float uniform24(unsigned x) { return (float)(x >> 8) * 0x1p-24f; }

__device__ __forceinline__ void gauss2(unsigned xa, unsigned xb, float &g0, float &g1)
{
    const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f, u2 = (float)(xb >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(kTwoPi * u2, &s, &c);
    g0 = rad * c, g1 = rad * s;
}

__device__ __forceinline__ void gauss3(const U4 &x, float &g0, float &g1, float &g2)
{
    float g3;
    gauss2(x.x, x.y, g0, g1);
    gauss2(x.z, x.w, g2, g3);
}

__device__ __forceinline__ float clipf(float v, float c) { return fminf(fmaxf(v, -c), c); }

__device__ __forceinline__ unsigned feistel_f(unsigned v)
{
    v ^= v >> 16, v *= 0x7FEB352Du, v ^= v >> 15, v *= 0x846CA68Bu, v ^= v >> 16;
    return v;
}

__device__ __forceinline__ unsigned feistel(unsigned x, int half, const U4 &rk)
{
    const unsigned mask = (1u << half) - 1u;
    unsigned l = x >> half, r = x & mask, t;
    t = l ^ (feistel_f(r + rk.x) & mask), l = r, r = t;
    t = l ^ (feistel_f(r + rk.y) & mask), l = r, r = t;
    t = l ^ (feistel_f(r + rk.z) & mask), l = r, r = t;
    t = l ^ (feistel_f(r + rk.w) & mask), l = r, r = t;
    return (l << half) | r;
}

template <int OP>  // 0 sum, 1 min, 2 max
__device__ __forceinline__ float combine(float a, float b)
{
    return OP == 0 ? a + b : OP == 1 ? fminf(a, b) : fmaxf(a, b);
}

// three per-thread values -> the workgroup's, in every thread; one fixed order (xor tree over the wave, waves ascending)
template <int OP>
__device__ __forceinline__ void block_reduce3(float (&v)[3], float (*s_red)[3])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[c] = combine<OP>(v[c], __shfl_xor(v[c], off, 64));
    }
    __syncthreads();  // (the previous use of s_red has been read)
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s_red[wave][c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = combine<OP>(combine<OP>(combine<OP>(s_red[0][c], s_red[1][c]), s_red[2][c]), s_red[3][c]);
}

__global__ __launch_bounds__(kThreads) void batch_assemble_kernel(BatchArgs a)
{
    __shared__ sn_u64 s_keys[kMaxSort];
    __shared__ float s_red[4][3];
    __shared__ unsigned s_item, s_epoch;
    const int tid = threadIdx.x, b = blockIdx.x, N = a.N;
    const sn_batch_recipe &rc = a.r;

    // ---- which item this slot holds (lane 0; one 64-bit division per workgroup) ----
    if (tid == 0) {
        const bool own = a.position < 0;
        const long long pos = own ? __hip_atomic_load(&a.state->position, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.position;
        const sn_u64 g = (sn_u64)pos + (sn_u64)a.rank * (sn_u64)a.B + (sn_u64)b;
        const sn_u64 ep = g / a.Lset;
        unsigned item = (unsigned)(g - ep * a.Lset);
        if (rc.order == SN_BATCH_ORDER_SHUFFLED) {
            const U4 rk = philox(0u, kStreamOrder, 0u, (unsigned)ep, a.k0, a.k1);
            do item = feistel(item, a.half, rk);
            while (item >= a.Lset);  // at most 2^k - Lset + 1 applications
        }
        s_item = item, s_epoch = (unsigned)ep;
        if (own) {
            // (acq_rel: this workgroup's read of the position is done before it counts as arrived; the last arrival sees them all)
            const unsigned n = __hip_atomic_fetch_add(&a.state->arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (n == (unsigned)(a.B - 1)) {
                __hip_atomic_store(&a.state->position, pos + (long long)a.B * a.world, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&a.state->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // armed for the next launch
            }
        }
    }
    __syncthreads();
    const unsigned item = s_item, epoch = s_epoch;
    const int cloud = (int)(item % (unsigned)a.L);
    if (tid == 0) {
        if (a.out_labels) a.out_labels[b] = a.labels[cloud];
        if (a.items) a.items[b] = (int)item;
    }
    if (a.igt && tid < 7) a.igt[(size_t)b * 7 + tid] = tid < 4 ? a.pair_quat[(size_t)item * 4 + tid] : 0.f;

    // ---- stage 1: the point order ----
    const bool shuffle = rc.shuffle_points != 0;
    if (shuffle) {
        int n2 = 2;
        while (n2 < N) n2 <<= 1;  // N <= kMaxSort (host check)
        for (int i = tid; i < n2; i += kThreads)
            s_keys[i] = i < N ? ((sn_u64)philox((unsigned)i, kStreamSort, item, epoch, a.k0, a.k1).x << 32) | (unsigned)i : sn::kKeyInf;
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int p = tid; p < (n2 >> 1); p += kThreads) {
                    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                    const sn_u64 x = s_keys[i], y = s_keys[l];
                    if ((x > y) == ((i & k) == 0)) s_keys[i] = y, s_keys[l] = x;
                }
                __syncthreads();
            }
        }
    }
    const float *src = a.points + (size_t)cloud * a.P * 3;
    auto source = [&](int j) { return shuffle ? (int)(unsigned)s_keys[j] : j; };  // (positions j < N hold real composites)

    // ---- per-cloud constants (every thread forms its own copy: two draws, four sincosf) ----
    const U4 cs = philox(0u, kStreamCloud, item, epoch, a.k0, a.k1);
    float ext = 0.f, mean[3] = {0.f, 0.f, 0.f};  // ext: the largest per-axis extent s
    if (rc.unit_cube) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int j = tid; j < N; j += kThreads) {
            const float *p = src + (size_t)source(j) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) lo[c] = fminf(lo[c], p[c]), hi[c] = fmaxf(hi[c], p[c]);
        }
        block_reduce3<1>(lo, s_red);
        block_reduce3<2>(hi, s_red);
        ext = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
        float sum[3] = {0.f, 0.f, 0.f};
        for (int j = tid; j < N; j += kThreads) {
            const float *p = src + (size_t)source(j) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += p[c] / ext;
        }
        block_reduce3<0>(sum, s_red);
#pragma unroll
        for (int c = 0; c < 3; ++c) mean[c] = sum[c] / (float)N;
    }
    const float scale = rc.scale ? rc.scale_lo + uniform24(cs.x) * (rc.scale_hi - rc.scale_lo) : 1.f;
    float R[3][3] = {};
    if (rc.rotate) {
        float s, c;
        sincosf(uniform24(cs.y) * kTwoPi, &s, &c);
        const float t = 1.f - c, ax[3] = {a.ax, a.ay, a.az};
        const float K[3][3] = {{0.f, -a.az, a.ay}, {a.az, 0.f, -a.ax}, {-a.ay, a.ax, 0.f}};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = (c * (i == j ? 1.f : 0.f) + s * K[i][j]) + (t * ax[i]) * ax[j];
    }
    float ps[3] = {}, pc[3] = {};
    if (rc.perturb) {
        float g[3];
        gauss3(philox(0u, kStreamAngles, item, epoch, a.k0, a.k1), g[0], g[1], g[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) sincosf(clipf(rc.perturb_sigma * g[k], rc.perturb_clip), &ps[k], &pc[k]);
    }
    const float shift = rc.translate ? uniform24(cs.z) * (rc.translate_range + rc.translate_range) - rc.translate_range : 0.f;
    const float ratio = uniform24(cs.w) * rc.dropout_max;

    // stages 2..7 of output point j
    auto transform = [&](int j, float (&v)[3]) {
        const float *p = src + (size_t)source(j) * 3;
        v[0] = p[0], v[1] = p[1], v[2] = p[2];
        if (rc.unit_cube) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] / ext - mean[c];
        }
        if (rc.scale) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] * scale;
        }
        if (rc.rotate) {
            const float x = v[0], y = v[1], z = v[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) v[i] = (R[i][0] * x + R[i][1] * y) + R[i][2] * z;
        }
        if (rc.perturb) {
            float x = v[0], y = v[1], z = v[2], t;
            t = pc[0] * y - ps[0] * z, z = ps[0] * y + pc[0] * z, y = t;  // about x
            t = pc[1] * x + ps[1] * z, z = pc[1] * z - ps[1] * x, x = t;  // about y
            t = pc[2] * x - ps[2] * y, y = ps[2] * x + pc[2] * y, x = t;  // about z
            v[0] = x, v[1] = y, v[2] = z;
        }
        if (rc.translate) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] + shift;
        }
        if (rc.jitter) {
            float g[3];
            gauss3(philox((unsigned)j, kStreamJitter, item, epoch, a.k0, a.k1), g[0], g[1], g[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] + clipf(rc.jitter_std * g[c], rc.jitter_clip);
        }
    };

    float first[3] = {0.f, 0.f, 0.f};
    if (rc.dropout && N > 0) transform(0, first);
    float qw = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
    if (a.p1) {
        const float *q = a.pair_quat + (size_t)item * 4;
        qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    }
    const size_t base = (size_t)b * N * 3;
    for (int j = tid; j < N; j += kThreads) {
        float v[3];
        transform(j, v);
        if (rc.dropout && uniform24(philox((unsigned)j, kStreamDropout, item, epoch, a.k0, a.k1).x) <= ratio)
            v[0] = first[0], v[1] = first[1], v[2] = first[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.p0[base + sn::pt_off(a.layout, N, j, c)] = v[c];
        if (a.p1) {
            // sn_qrot_forward's expression (pcrnet_head.hip: qrot_fwd_kernel)
            const float uvx = qy * v[2] - qz * v[1], uvy = qz * v[0] - qx * v[2], uvz = qx * v[1] - qy * v[0];
            const float wx = qy * uvz - qz * uvy, wy = qz * uvx - qx * uvz, wz = qx * uvy - qy * uvx;
            float o[3] = {v[0] + 2.0f * (qw * uvx + wx), v[1] + 2.0f * (qw * uvy + wy), v[2] + 2.0f * (qw * uvz + wz)};
            if (rc.pair_noise) {
                float g[3];
                gauss3(philox((unsigned)j, kStreamPairNoise, item, epoch, a.k0, a.k1), g[0], g[1], g[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = o[c] + rc.pair_noise_std * g[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) a.p1[base + sn::pt_off(a.layout, N, j, c)] = o[c];
        }
    }
}

}  // namespace

extern "C" long long sn_batch_state_bytes(void) { return (long long)sizeof(SnBatchState); }

extern "C" int sn_batch_assemble(int B, int N, int P, int L, int repeat, const float *points, const long long *labels,
                                 const sn_batch_recipe *recipe, unsigned long long seed, int rank, int world, long long position,
                                 void *state, const float *pair_quat, int layout, float *p0, float *p1, long long *out_labels,
                                 float *igt, int *items, sn_stream_t stream)
{
    SN_REQUIRE(B >= 0 && N >= 0 && P >= 0 && L >= 0, "negative size");
    SN_REQUIRE(repeat >= 1, "repeat must be at least 1");
    SN_REQUIRE(N <= P, "N > P: more points asked for than a cloud holds");
    SN_REQUIRE(world >= 1 && rank >= 0 && rank < world, "rank must lie in [0, world)");
    SN_REQUIRE(layout == SN_LAYOUT_BNC || layout == SN_LAYOUT_BCN, "layout selector");
    SN_REQUIRE(recipe != nullptr, "null recipe");
    const sn_batch_recipe r = *recipe;
    SN_REQUIRE(r.order == SN_BATCH_ORDER_SHUFFLED || r.order == SN_BATCH_ORDER_SEQUENTIAL, "order selector");
    SN_REQUIRE(!r.scale || r.scale_lo <= r.scale_hi, "scale_lo > scale_hi");  // (a NaN fails too)
    SN_REQUIRE(!r.perturb || (r.perturb_sigma >= 0.f && r.perturb_clip >= 0.f), "negative perturbation sigma or clip");
    SN_REQUIRE(!r.translate || r.translate_range >= 0.f, "negative translation range");
    SN_REQUIRE(!r.jitter || (r.jitter_std >= 0.f && r.jitter_clip >= 0.f), "negative jitter std or clip");
    SN_REQUIRE(!r.dropout || (r.dropout_max >= 0.f && r.dropout_max < 1.f), "dropout_max must lie in [0, 1)");
    SN_REQUIRE(!r.pair_noise || r.pair_noise_std >= 0.f, "negative pair noise std");
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (r.rotate) {
        const double n2 = (double)r.axis[0] * r.axis[0] + (double)r.axis[1] * r.axis[1] + (double)r.axis[2] * r.axis[2];
        SN_REQUIRE(n2 > 0.0 && n2 < INFINITY, "rotation axis must be a finite non-zero vector");
        const double n = sqrt(n2);
        ax = r.axis[0] / n, ay = r.axis[1] / n, az = r.axis[2] / n;
    }
    if (B == 0) return 0;
    SN_REQUIRE(L >= 1 && (long long)L * repeat < (1ll << 31), "the set must hold 1 .. 2^31 - 1 items");
    SN_REQUIRE(position >= 0 || state != nullptr, "null state block without an explicit position");
    SN_REQUIRE(position >= 0 || ((size_t)state & 7) == 0, "misaligned state block");
    SN_REQUIRE(points != nullptr && p0 != nullptr, "null pointer");
    SN_REQUIRE(out_labels == nullptr || labels != nullptr, "labels wanted from a set without labels");
    SN_REQUIRE((p1 == nullptr && igt == nullptr) || pair_quat != nullptr, "p1 / igt wanted without a quaternion table");
    SN_REQUIRE(((size_t)out_labels & 7) == 0 && ((size_t)labels & 7) == 0, "misaligned labels");
    if (r.shuffle_points && N > kMaxSort)
        return sn_set_error(SN_ERR_UNSUPPORTED, "%s: shuffle_points sorts at most %d points per cloud (N = %d)", __func__, kMaxSort, N);
    BatchArgs a;
    a.points = points, a.labels = labels, a.pair_quat = pair_quat, a.p0 = p0, a.p1 = p1, a.out_labels = out_labels, a.igt = igt;
    a.items = items, a.state = (SnBatchState *)state, a.position = position;
    a.k0 = (unsigned)(seed & 0xFFFFFFFFull), a.k1 = (unsigned)(seed >> 32);
    a.Lset = (unsigned)((long long)L * repeat);
    a.L = L, a.N = N, a.P = P, a.B = B, a.rank = rank, a.world = world, a.layout = layout;
    int k = 2;
    while ((1ull << k) < (unsigned long long)a.Lset) k += 2;
    a.half = k / 2;
    a.ax = (float)ax, a.ay = (float)ay, a.az = (float)az;
    a.r = r;
    batch_assemble_kernel<<<B, kThreads, 0, (hipStream_t)stream>>>(a);
    SN_LAUNCH_CHECK();
    return 0;
}

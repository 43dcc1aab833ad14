// optimizer.hip -- the Adam update of every parameter of an optimizer group as ONE launch (samplenet_amd/optim.py; the reference
// trains everything with Adam: registration/main.py:167 torch.optim.Adam, classification/train_samplenet.py:194 and
// reconstruction/src/samplenet_pointnet_ae.py:206 tf.train.AdamOptimizer).
//
// A device-side chunk table (built once on the host, multi-tensor-apply style) maps workgroup c to
//     { parameter pointer, gradient pointer, element offset into the two flat moment buffers, element count <= kChunk };
// a chunk never straddles two tensors.  Parameters and gradients are addressed where they lie (captured graphs and forward plans hold
// raw pointers into the parameters; the gradient bucket of parallel.FlatGradAllReducer is not padded, so after its one-element
// temperature every gradient offset is odd); the moments live in two flat fp32 buffers whose per-tensor segments start on 16-byte
// boundaries.  A chunk with a NULL gradient is skipped: parameter and moments stay as they are (torch: p.grad is None).
//
// What changes during training lives in a 64-byte device block (SnAdamState below): the launch reads t, uses t + 1 for the bias
// corrections, and the LAST workgroup to arrive advances the block (t, the running fp64 powers beta^t) and clears the arrival
// counter -- a captured graph replays the update unchanged, and nothing here synchronises with the host.
//
// Per element, fp32, IEEE division and square root, no contraction beyond the fmaf's written out (the unit is built with
// -ffp-contract=off).  THE OPERATION ORDER IS PINNED (tests/test_gpu_adam.py derives its rounding bound from it):
//     g1 = fl((double)g * grad_scale + wd * (double)p)      formed in fp64 and rounded ONCE: its error is relative to g1 itself even
//                                                           where g and wd p cancel (exact for grad_scale = 1, wd = 0)
//     m' = fmaf(b1, m, omb1 * g1)                           b1 = fl(beta1), omb1 = fl(1 - beta1)   (rounded once from fp64)
//     v' = fmaf(b2, v, (omb2 * g1) * g1)                    b2 = fl(beta2), omb2 = fl(1 - beta2)
//   torch form:       den = sqrtf(v') / rbc2 + eps          rbc2 = fl(sqrt(bc2)),  step = fl(lr / bc1)
//   TensorFlow form:  den = sqrtf(v') + eps                 step = fl(lr sqrt(bc2) / bc1)
//     p' = fmaf(-step, m' / den, p)
// with bc1 = 1 - beta1^(t+1), bc2 = 1 - beta2^(t+1) formed in fp64 once per workgroup from the block's running powers.
#include "sn_common.h"

namespace {

constexpr int kChunk = 1024;    // elements per chunk = 256 threads x 4
constexpr int kThreads = 256;

struct SnAdamChunk {            // 32 bytes; samplenet_amd/optim.py packs the same layout ("<QQqii")
    float *p;
    const float *g;
    long long moff;             // element offset into exp_avg / exp_avg_sq, a multiple of 4
    int count;                  // 1 .. kChunk
    int pad;
};
static_assert(sizeof(SnAdamChunk) == 32, "chunk table entry layout");

struct SnAdamState {            // 64 bytes; samplenet_amd/optim.py addresses it as 8 fp64 / int64 words
    double lr;                  // word 0
    double b1pow;               // word 1: beta1^t
    double b2pow;               // word 2: beta2^t
    long long t;                // word 3: updates applied so far
    unsigned arrive;            // word 4 (low half): arrival counter, zero between launches
    unsigned pad[7];
};
static_assert(sizeof(SnAdamState) == 64, "state block layout");

struct AdamCoef {
    float b1, omb1, b2, omb2, eps;
    double beta1, beta2, wd, gscale;
    int tf_epsilon;
};

__device__ __forceinline__ bool aligned16(const void *q) { return (reinterpret_cast<size_t>(q) & 15) == 0; }

// four consecutive elements from q[0..3]: one 16-byte access when `vec` (q 16-byte aligned, all four in range), else scalar ones
__device__ __forceinline__ void load4(const float *q, bool vec, int n, float (&x)[4])
{
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(q);
        x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = j < n ? q[j] : 0.f;
    }
}
__device__ __forceinline__ void store4(float *q, bool vec, int n, const float (&x)[4])
{
    if (vec) {
        *reinterpret_cast<float4 *>(q) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) q[j] = x[j];
    }
}

__global__ __launch_bounds__(kThreads) void adam_update_kernel(int nchunks, const SnAdamChunk *__restrict__ table, float *__restrict__ exp_avg,
                                                               float *__restrict__ exp_avg_sq, SnAdamState *__restrict__ state, AdamCoef c)
{
    __shared__ float s_step, s_rbc2;
    const int tid = threadIdx.x;
    const SnAdamChunk ch = table[blockIdx.x];
    // the block's words are read by ONE lane before this workgroup arrives; the last arrival is the only writer
    double b1n = 0.0, b2n = 0.0;
    long long t = 0;
    if (tid == 0) {
        const double lr = state->lr;
        t = state->t;
        b1n = state->b1pow * c.beta1;  // beta^(t+1)
        b2n = state->b2pow * c.beta2;
        const double bc1 = 1.0 - b1n, rbc2 = sqrt(1.0 - b2n);
        s_step = (float)(c.tf_epsilon ? lr * rbc2 / bc1 : lr / bc1);
        s_rbc2 = (float)rbc2;
    }
    __syncthreads();
    if (ch.g != nullptr) {
        const float step = s_step, rbc2 = s_rbc2;
        const int i0 = tid * 4, n = ch.count - i0;  // this thread's elements i0 .. i0 + min(n, 4) - 1
        if (n > 0) {
            const bool full = n >= 4;
            float *pp = ch.p + i0;
            const float *gp = ch.g + i0;
            float *mp = exp_avg + ch.moff + i0, *vp = exp_avg_sq + ch.moff + i0;
            // (chunk offsets are multiples of 4 elements: an array's phase is that of its chunk pointer)
            const bool pvec = full && aligned16(pp), gvec = full && aligned16(gp), mvec = full && aligned16(mp), vvec = full && aligned16(vp);
            float p[4], g[4], m[4], v[4];
            load4(pp, pvec, n, p);
            load4(gp, gvec, n, g);
            load4(mp, mvec, n, m);
            load4(vp, vvec, n, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g1 = (float)((double)g[j] * c.gscale + c.wd * (double)p[j]);
                m[j] = fmaf(c.b1, m[j], c.omb1 * g1);
                v[j] = fmaf(c.b2, v[j], (c.omb2 * g1) * g1);
                const float den = c.tf_epsilon ? sqrtf(v[j]) + c.eps : sqrtf(v[j]) / rbc2 + c.eps;
                p[j] = fmaf(-step, m[j] / den, p[j]);
            }
            store4(pp, pvec, n, p);
            store4(mp, mvec, n, m);
            store4(vp, vvec, n, v);
        }
    }
    if (tid == 0) {
        // (acq_rel: this workgroup's reads of the block are done before it counts as arrived, and the last arrival sees them all)
        const unsigned a = __hip_atomic_fetch_add(&state->arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (a == (unsigned)(nchunks - 1)) {
            state->b1pow = b1n;
            state->b2pow = b2n;
            state->t = t + 1;
            __hip_atomic_store(&state->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // armed for the next launch
        }
    }
}

}  // namespace

extern "C" int sn_adam_chunk_elems(void) { return kChunk; }

extern "C" long long sn_adam_state_bytes(void) { return (long long)sizeof(SnAdamState); }

extern "C" int sn_adam_update(int nchunks, const void *chunks, float *exp_avg, float *exp_avg_sq, void *state, double beta1, double beta2,
                              double eps, double weight_decay, double grad_scale, int tf_epsilon, sn_stream_t stream)
{
    SN_REQUIRE(nchunks >= 0, "negative chunk count");
    SN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas must lie in [0, 1)");
    SN_REQUIRE(eps >= 0.0 && weight_decay >= 0.0, "negative eps or weight_decay");
    if (nchunks == 0) return 0;  // (no parameters: the step count does not advance either)
    SN_REQUIRE(chunks != nullptr, "null chunk table with chunks > 0");
    SN_REQUIRE(exp_avg && exp_avg_sq && state, "null pointer");
    SN_REQUIRE(exp_avg != exp_avg_sq, "the two moment buffers must be distinct");
    SN_REQUIRE(((size_t)chunks & 7) == 0 && ((size_t)state & 7) == 0 && ((size_t)exp_avg & 15) == 0 && ((size_t)exp_avg_sq & 15) == 0,
               "misaligned table, state block or moment buffer");
    AdamCoef c;
    c.b1 = (float)beta1, c.omb1 = (float)(1.0 - beta1), c.b2 = (float)beta2, c.omb2 = (float)(1.0 - beta2);
    c.eps = (float)eps, c.wd = weight_decay, c.gscale = grad_scale, c.beta1 = beta1, c.beta2 = beta2, c.tf_epsilon = tf_epsilon != 0;
    adam_update_kernel<<<nchunks, kThreads, 0, (hipStream_t)stream>>>(nchunks, (const SnAdamChunk *)chunks, exp_avg, exp_avg_sq,
                                                                      (SnAdamState *)state, c);
    SN_LAUNCH_CHECK();
    return 0;
}

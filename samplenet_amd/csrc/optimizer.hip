// optimizer.hip -- the update of every parameter of an optimizer group as ONE launch (samplenet_amd/optim.py): Adam (the reference
// trains everything with Adam: registration/main.py:167 torch.optim.Adam, classification/train_samplenet.py:194 and
// reconstruction/src/samplenet_pointnet_ae.py:206 tf.train.AdamOptimizer), and the two other choices of registration/main.py:166-171,
// SGD with momentum (also classification/train_classifier.py:133 tf.train.MomentumOptimizer) and RMSprop.
//
// A device-side chunk table (built once on the host, multi-tensor-apply style) maps workgroup c to
//     { parameter pointer, gradient pointer, element offset into the flat state buffers, element count <= kChunk };
// a chunk never straddles two tensors.  Parameters and gradients are addressed where they lie (captured graphs and forward plans hold
// raw pointers into the parameters; the gradient bucket of parallel.FlatGradAllReducer is not padded, so after its one-element
// temperature every gradient offset is odd); the per-element state (Adam's two moments, SGD's momentum buffer, RMSprop's square average
// and momentum buffer) lives in flat fp32 buffers whose per-tensor segments start on 16-byte boundaries.  A chunk with a NULL gradient
// is skipped: parameter and state stay as they are (torch: p.grad is None).
//
// What changes during training lives in a 64-byte device block (SnAdamState below): the launch reads t (Adam uses t + 1 for the bias
// corrections, SGD takes t == 0 for "no momentum buffer yet"), and the LAST workgroup to arrive advances the block (t; for Adam the
// running fp64 powers beta^t, which the other two kernels leave as found) and clears the arrival counter -- a captured graph replays
// the update unchanged, and nothing here synchronises with the host.
//
// Per element, fp32, IEEE division and square root, no contraction beyond the fmaf's written out (the unit is built with
// -ffp-contract=off).  THE OPERATION ORDER IS PINNED (tests/adam_ref.py and tests/optim_ref.py derive their rounding bounds from it):
//   all three:
//     g1 = fl((double)g * grad_scale + wd * (double)p)      formed in fp64 and rounded ONCE: its error is relative to g1 itself even
//                                                           where g and wd p cancel (exact for grad_scale = 1, wd = 0)
//   Adam:
//     m' = fmaf(b1, m, omb1 * g1)                           b1 = fl(beta1), omb1 = fl(1 - beta1)   (rounded once from fp64)
//     v' = fmaf(b2, v, (omb2 * g1) * g1)                    b2 = fl(beta2), omb2 = fl(1 - beta2)
//   torch form:       den = sqrtf(v') / rbc2 + eps          rbc2 = fl(sqrt(bc2)),  step = fl(lr / bc1)
//   TensorFlow form:  den = sqrtf(v') + eps                 step = fl(lr sqrt(bc2) / bc1)
//     p' = fmaf(-step, m' / den, p)
//   with bc1 = 1 - beta1^(t+1), bc2 = 1 - beta2^(t+1) formed in fp64 once per workgroup from the block's running powers.
//   SGD (lrf = fl(lr) from the block; mu = fl(momentum), omd = fl(1 - dampening), each rounded once from fp64 on the host):
//     momentum != 0:  b' = (t == 0) ? g1 : fmaf(mu, b, omd * g1)       t == 0: torch's "momentum_buffer is None" (the first step
//                     d  = nesterov ? fmaf(mu, b', g1) : b'            clones the gradient, dampening applies from the second)
//     momentum == 0:  d  = g1                                           (no buffer is read or written)
//     p' = fmaf(-lrf, d, p)
//   RMSprop (al = fl(alpha), oma = fl(1 - alpha), mu = fl(momentum)):
//     s'  = fmaf(al, s, (oma * g1) * g1)
//     den = sqrtf(s') + fl(eps)
//     q   = g1 / den
//     momentum == 0:  p' = fmaf(-lrf, q, p)
//     momentum != 0:  b' = fmaf(mu, b, q),  p' = fmaf(-lrf, b', p)
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

struct SgdCoef {
    float mu, omd;
    double wd, gscale;
    int nesterov;
};

struct RmspropCoef {
    float al, oma, eps, mu;
    double wd, gscale;
};

// SGD and RMSprop: the block's words (lr, t) were read by the calling lane before this; the last workgroup to arrive is the only
// writer: it advances t, leaves words 1 and 2 as found and re-arms the counter
// (acq_rel: this workgroup's reads of the block are done before it counts as arrived, and the last arrival sees them all)
__device__ __forceinline__ void arrive_and_advance(SnAdamState *state, int nchunks, long long t)
{
    const unsigned a = __hip_atomic_fetch_add(&state->arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (a == (unsigned)(nchunks - 1)) {
        state->t = t + 1;
        __hip_atomic_store(&state->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // armed for the next launch
    }
}

// momentum_buf == nullptr: momentum 0
__global__ __launch_bounds__(kThreads) void sgd_update_kernel(int nchunks, const SnAdamChunk *__restrict__ table, float *__restrict__ momentum_buf,
                                                              SnAdamState *__restrict__ state, SgdCoef c)
{
    __shared__ float s_lr;
    __shared__ int s_first;
    const int tid = threadIdx.x;
    const SnAdamChunk ch = table[blockIdx.x];
    long long t = 0;
    if (tid == 0) {
        s_lr = (float)state->lr;
        t = state->t;
        s_first = t == 0;
    }
    __syncthreads();
    if (ch.g != nullptr) {
        const float lrf = s_lr;
        const bool first = s_first != 0;
        const int i0 = tid * 4, n = ch.count - i0;
        if (n > 0) {
            const bool full = n >= 4;
            float *pp = ch.p + i0;
            const float *gp = ch.g + i0;
            float *bp = momentum_buf ? momentum_buf + ch.moff + i0 : nullptr;
            const bool pvec = full && aligned16(pp), gvec = full && aligned16(gp), bvec = full && aligned16(bp);
            float p[4], g[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            load4(pp, pvec, n, p);
            load4(gp, gvec, n, g);
            if (bp && !first) load4(bp, bvec, n, b);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g1 = (float)((double)g[j] * c.gscale + c.wd * (double)p[j]);
                float d = g1;
                if (bp) {
                    b[j] = first ? g1 : fmaf(c.mu, b[j], c.omd * g1);
                    d = c.nesterov ? fmaf(c.mu, b[j], g1) : b[j];
                }
                p[j] = fmaf(-lrf, d, p[j]);
            }
            store4(pp, pvec, n, p);
            if (bp) store4(bp, bvec, n, b);
        }
    }
    if (tid == 0) arrive_and_advance(state, nchunks, t);
}

// momentum_buf == nullptr: momentum 0
__global__ __launch_bounds__(kThreads) void rmsprop_update_kernel(int nchunks, const SnAdamChunk *__restrict__ table, float *__restrict__ square_avg,
                                                                  float *__restrict__ momentum_buf, SnAdamState *__restrict__ state, RmspropCoef c)
{
    __shared__ float s_lr;
    const int tid = threadIdx.x;
    const SnAdamChunk ch = table[blockIdx.x];
    long long t = 0;
    if (tid == 0) {
        s_lr = (float)state->lr;
        t = state->t;
    }
    __syncthreads();
    if (ch.g != nullptr) {
        const float lrf = s_lr;
        const int i0 = tid * 4, n = ch.count - i0;
        if (n > 0) {
            const bool full = n >= 4;
            float *pp = ch.p + i0;
            const float *gp = ch.g + i0;
            float *sp = square_avg + ch.moff + i0;
            float *bp = momentum_buf ? momentum_buf + ch.moff + i0 : nullptr;
            const bool pvec = full && aligned16(pp), gvec = full && aligned16(gp), svec = full && aligned16(sp), bvec = full && aligned16(bp);
            float p[4], g[4], s[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            load4(pp, pvec, n, p);
            load4(gp, gvec, n, g);
            load4(sp, svec, n, s);
            if (bp) load4(bp, bvec, n, b);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g1 = (float)((double)g[j] * c.gscale + c.wd * (double)p[j]);
                s[j] = fmaf(c.al, s[j], (c.oma * g1) * g1);
                const float den = sqrtf(s[j]) + c.eps;
                float q = g1 / den;
                if (bp) q = b[j] = fmaf(c.mu, b[j], q);
                p[j] = fmaf(-lrf, q, p[j]);
            }
            store4(pp, pvec, n, p);
            store4(sp, svec, n, s);
            if (bp) store4(bp, bvec, n, b);
        }
    }
    if (tid == 0) arrive_and_advance(state, nchunks, t);
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

extern "C" int sn_sgd_update(int nchunks, const void *chunks, float *momentum_buf, void *state, double momentum, double dampening,
                             double weight_decay, double grad_scale, int nesterov, sn_stream_t stream)
{
    SN_REQUIRE(nchunks >= 0, "negative chunk count");
    SN_REQUIRE(momentum >= 0.0 && dampening >= 0.0 && weight_decay >= 0.0, "negative momentum, dampening or weight_decay");
    SN_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "nesterov requires a momentum and zero dampening");
    if (nchunks == 0) return 0;  // (no parameters: the step count does not advance either)
    SN_REQUIRE(chunks != nullptr, "null chunk table with chunks > 0");
    SN_REQUIRE(state != nullptr, "null pointer");
    SN_REQUIRE((momentum_buf == nullptr) == (momentum == 0.0), "momentum_buf must be null exactly when momentum == 0");
    SN_REQUIRE(((size_t)chunks & 7) == 0 && ((size_t)state & 7) == 0 && ((size_t)momentum_buf & 15) == 0,
               "misaligned table, state block or momentum buffer");
    SgdCoef c;
    c.mu = (float)momentum, c.omd = (float)(1.0 - dampening), c.wd = weight_decay, c.gscale = grad_scale, c.nesterov = nesterov != 0;
    sgd_update_kernel<<<nchunks, kThreads, 0, (hipStream_t)stream>>>(nchunks, (const SnAdamChunk *)chunks, momentum_buf, (SnAdamState *)state, c);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_rmsprop_update(int nchunks, const void *chunks, float *square_avg, float *momentum_buf, void *state, double alpha,
                                 double eps, double weight_decay, double momentum, double grad_scale, sn_stream_t stream)
{
    SN_REQUIRE(nchunks >= 0, "negative chunk count");
    SN_REQUIRE(alpha >= 0.0 && alpha < 1.0, "alpha must lie in [0, 1)");
    SN_REQUIRE(eps >= 0.0 && weight_decay >= 0.0 && momentum >= 0.0, "negative eps, weight_decay or momentum");
    if (nchunks == 0) return 0;  // (no parameters: the step count does not advance either)
    SN_REQUIRE(chunks != nullptr, "null chunk table with chunks > 0");
    SN_REQUIRE(square_avg && state, "null pointer");
    SN_REQUIRE((momentum_buf == nullptr) == (momentum == 0.0), "momentum_buf must be null exactly when momentum == 0");
    SN_REQUIRE(square_avg != momentum_buf, "the two state buffers must be distinct");
    SN_REQUIRE(((size_t)chunks & 7) == 0 && ((size_t)state & 7) == 0 && ((size_t)square_avg & 15) == 0 && ((size_t)momentum_buf & 15) == 0,
               "misaligned table, state block or state buffer");
    RmspropCoef c;
    c.al = (float)alpha, c.oma = (float)(1.0 - alpha), c.eps = (float)eps, c.mu = (float)momentum, c.wd = weight_decay, c.gscale = grad_scale;
    rmsprop_update_kernel<<<nchunks, kThreads, 0, (hipStream_t)stream>>>(nchunks, (const SnAdamChunk *)chunks, square_avg, momentum_buf,
                                                                         (SnAdamState *)state, c);
    SN_LAUNCH_CHECK();
    return 0;
}

// sampler_step_loss.hip -- the sampler step's fused loss, its one-launch backward and the captured-surface values (gfx950).
//
// ------------------------------------------------------------------------------------------------
// The sampler's training-step loss in as few launches as the data dependencies allow (engine fast path; the op-by-op
// route through sn_simplification_loss_* / sn_sampler_loss_* / sn_soft_project_backward computes the same numbers):
//   L = alpha * (mean dq + mean_b max_m dq + weight * mean dp) + lmbda * max(T^2, min_sigma) + mean(proj)
// forward : [per cloud: finish the per-point minima from the pair scan's G partial key sets -> dp / ip, and reduce
//            sum dq, max dq (+ first argmax), sum dp, sum proj]  ->  [combine the clouds in order -> L]
// backward: [Chamfer backward with implicit upstream gradients (scaled by alpha) -> grad_Q]
//           [soft-projection backward with the constant upstream gradient g / nproj, ADDED to grad_Q; sigma partials]
//           [sigma partials + the direct lmbda term -> grad_T]
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)  // reference arithmetic is product-then-sum (no FMA)

#include <cstring>

#include "chamfer_owner.h"
#include "soft_query.h"
#include "step_tail.h"

using namespace sn;

// scalar of the sampler step's loss from the per-cloud partials (see sn_sampler_step_loss_forward)
struct StepLossFinal {
    int B, M, N, nproj;
    float w, alpha, lmbda, min_sigma;
    const float *part;
    const float *temperature;
    float *loss;  // NULL: nothing to do
};

// one wave: lane b carries clouds b, b + 64, ...; the lanes are then combined by a fixed xor tree (all loads in flight at
// once; a single thread walking the B partials pays one memory round trip per cloud)
__device__ __forceinline__ void step_loss_final(const StepLossFinal &f, int t)
{
    float s1 = 0.f, mx = 0.f, s2 = 0.f, sp = 0.f;
    for (int b = t; b < f.B; b += 64) s1 += f.part[b * 4], mx += f.part[b * 4 + 1], s2 += f.part[b * 4 + 2], sp += f.part[b * 4 + 3];
    const float T = *f.temperature;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        mx += __shfl_xor(mx, o);
        s2 += __shfl_xor(s2, o);
        sp += __shfl_xor(sp, o);
    }
    if (t != 0) return;
    const float c12 = s1 / ((float)f.B * (float)f.M), cmax = mx / (float)f.B, c21 = s2 / ((float)f.B * (float)f.N);
    const float lsimp = c12 + cmax + f.w * c21;
    f.loss[0] = f.alpha * lsimp + f.lmbda * sn_sigma(T, f.min_sigma) + sp / ((float)f.B * (float)f.nproj);
    f.loss[1] = lsimp;
}

// Chamfer backward (implicit upstream gradients, targets = the simplified cloud) + soft-projection backward of the same
// query in ONE launch: a wave finishes the Chamfer gradient of target j exactly as chamfer_bwd_reg_kernel does, then runs
// the soft-projection backward of query j (same point: the simplified cloud is both) and stores the sum -- the same
// numbers as the two launches with accumulate_q (chamfer term first, soft term added), one kernel boundary less.
// Optional (engine path: no launch between the pair scan and the backward), keys mode = sn_pairscan_forward_keys +
// sn_sampler_step_loss_keys: the per-point minima are already complete, as INVERTED (distance, query) keys [B][ns]; the argmax
// of dist_q comes from the scan's per-workgroup maxima qmax [B][G]; the y == 0 workgroup leaves sum dist_p of its cloud in
// dpsum [B].  keys == NULL: idxS / argmax come from memory.
struct StepLossFold {
    int G;
    const sn_u64 *keys;
    const sn_u64 *qmax;
    float *dpsum;
};


// Debug build only (-DSN_CS_TIMELINE=1|2, tools/pairscan_timeline.py): thread 0 of every workgroup of chamfer_soft_bwd_kernel
// stamps the 100 MHz wall clock at the phase boundaries of its first query (2: every stamp first drains the memory counters).
#ifdef SN_CS_TIMELINE
__device__ unsigned long long g_cs_tl[8192 * 16];
#define CS_TL(slot)                                                                                              \
    do {                                                                                                         \
        if (threadIdx.x == 0) g_cs_tl[((blockIdx.y * gridDim.x + blockIdx.x) & 8191) * 16 + (slot)] = wall_clock64(); \
    } while (0)
#if SN_CS_TIMELINE >= 2
#define CS_TL_DRAIN() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#else
#define CS_TL_DRAIN()
#endif
// ... and lane 0 of EVERY wave records the longest ordered owner sum among its queries (ticks; the operands have landed before
// the first stamp and the sum is complete before the second, at either level)
__device__ unsigned g_cs_walk[8192 * 4];
#define CS_WALK_BEGIN()                                              \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    const unsigned long long walk_t0 = wall_clock64()
#define CS_WALK_END(x, y, z)                                                                          \
    do {                                                                                              \
        asm volatile("; owner sum done" ::"v"(x), "v"(y), "v"(z) : "memory");                         \
        const unsigned walk_dt = (unsigned)(wall_clock64() - walk_t0);                                \
        walk_max = walk_dt > walk_max ? walk_dt : walk_max;                                           \
    } while (0)
#define CS_WALK_STORE()                                                                                                   \
    do {                                                                                                                  \
        if (lane == 0) g_cs_walk[((blockIdx.y * gridDim.x + blockIdx.x) & 8191) * 4 + wave] = walk_max + 1u; /* 0 = no query */ \
    } while (0)
#else
#define CS_TL(slot)
#define CS_TL_DRAIN()
#define CS_WALK_BEGIN()
#define CS_WALK_END(x, y, z)
#define CS_WALK_STORE()
#endif

template <int PPL>
__global__ void __launch_bounds__(256) chamfer_soft_bwd_kernel(int nt, int ns, const float *__restrict__ T,
                                                               const float *__restrict__ S, const int *__restrict__ idxT,
                                                               const int *__restrict__ idxS, float *__restrict__ gradT,
                                                               ImplicitGrad ig, SoftBwdArgs sa, StepLossFinal fin,
                                                               StepLossFold fold)
{
    __shared__ float s_part[4];
    __shared__ int s_ip[PPL * 64];
    __shared__ float s_red[3][4];
    __shared__ int s_am;
    __shared__ OwnerList s_own[4];  // one per wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int b = blockIdx.x;
    CS_TL(0);
    kernarg_warm_for<24, int, int, const float *, const float *, const int *, const int *, float *, ImplicitGrad, SoftBwdArgs,
                     StepLossFinal, StepLossFold>();  // (-0.3 us: see sn_common.h)
    const int nsplit = fin.loss ? (int)gridDim.y - 1 : (int)gridDim.y;  // the last y-slice only combines the loss value
    if ((int)blockIdx.y == nsplit) {
        if (b == 0 && wave == 0) step_loss_final(fin, lane);
        return;
    }
    // ---- everything that does not wait for the keys is requested first (one memory round trip instead of a chain of them:
    // cloud, scalars, the first query's coordinates / nearest point / neighbour indices), the loads that depend on those
    // (the nearest point's and the neighbours' coordinates) while the keys are on their way
    T += (size_t)b * nt * 3, S += (size_t)b * ns * 3;
    idxT += (size_t)b * nt;
    if (idxS) idxS += (size_t)b * ns;
    gradT += (size_t)b * nt * 3;
    float sx[PPL], sy[PPL], sz[PPL], gg[PPL];
    int is[PPL];
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
        const int l = i * 64 + lane;
        const int lc = l < ns ? l : 0;
        const sn_xyz3 sv = *reinterpret_cast<const sn_xyz3 *>(S + (size_t)lc * 3);
        sx[i] = sv.x, sy[i] = sv.y, sz[i] = sv.z;
    }
    const float gLv = *ig.gL * ig.gscale;
    const float Tm = *sa.temperature;
    const float sigma = sn_sigma(Tm, sa.min_sigma);
    const int jfirst = blockIdx.y * nwaves + wave, jstep = nsplit * nwaves;
    // the first query of this wave (the simplified cloud is target and query at once: T = sa.Q of this cloud)
    float tx = 0.f, ty = 0.f, tz = 0.f, ox = 0.f, oy = 0.f, oz = 0.f;
    int j2 = 0;
    SoftQuery sq{};
    auto load_query = [&](int j) {
        tx = T[j], ty = T[j + nt], tz = T[j + 2 * nt];  // targets channel-major (3, nt)
        j2 = idxT[j];
        soft_bwd_load_index(sa, b, j, lane, T, sq);
    };
    auto load_dependent = [&]() {
        ox = S[j2 * 3 + 0], oy = S[j2 * 3 + 1], oz = S[j2 * 3 + 2];
        soft_bwd_load_points(sa, lane, S, sq);
    };
    if (jfirst < nt) load_query(jfirst);
    CS_TL_DRAIN();
    CS_TL(8);

    if (fold.keys) {
        // nearest query of every point of the cloud, fetched ONCE per workgroup (the four waves all need all of them; keys that
        // were updated by device-scope atomics are slow to read: 4 x 8 KB per workgroup cost +4 us) and handed over in LDS
        sn_u64 kv[PPL * 64 / 256 > 0 ? PPL * 64 / 256 : 1];
#pragma unroll
        for (int r = 0; r < (PPL * 64 + 255) / 256; ++r) {
            const int n = threadIdx.x + r * 256;
            // (unconditional: the loads leave as ONE batch -- behind a select each waited for the one before it, 1.16 us
            //  until the keys had landed against 0.36 us now)
            kv[r] = fold.keys[(size_t)b * ns + (n < ns ? n : ns - 1)];
        }
        sn_u64 mk = 0;
        if (wave == 0) {  // argmax of dist_q: maximum of the (dist_q, ~query) keys of the cloud's scan workgroups
            for (int g = lane; g < fold.G; g += 64) {
                const sn_u64 v = fold.qmax[(size_t)b * fold.G + g];
                mk = v > mk ? v : mk;
            }
        }
#if defined(SN_CS_TIMELINE) && SN_CS_TIMELINE >= 2  // (the keys alone)
        CS_TL_DRAIN();
        CS_TL(11);
#endif
        if (jfirst < nt) load_dependent();
        CS_TL_DRAIN();
        CS_TL(9);
        float sdp = 0.f;
#pragma unroll
        for (int r = 0; r < (PPL * 64 + 255) / 256; ++r) {  // (ascending n per thread, as a strided loop would visit them)
            const int n = threadIdx.x + r * 256;
            if (n < ns) {
                const sn_u64 k = ~kv[r];
                s_ip[n] = key_index(k);
                sdp += key_dist(k);
            }
        }
        if (blockIdx.y == 0) {  // sum dist_p of the cloud (for the loss value), fixed order
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sdp += __shfl_xor(sdp, o);
            if (lane == 0) s_red[2][wave] = sdp;
        }
        if (wave == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned hi = __shfl_xor((unsigned)(mk >> 32), o), lo = __shfl_xor((unsigned)mk, o);
                const sn_u64 v = ((sn_u64)hi << 32) | lo;
                mk = v > mk ? v : mk;
            }
            if (lane == 0) s_am = (int)(0xFFFFFFFFu - (unsigned)mk);
        }
        CS_TL(10);
        __syncthreads();
        if (blockIdx.y == 0 && threadIdx.x == 0) fold.dpsum[b] = (s_red[2][0] + s_red[2][1]) + (s_red[2][2] + s_red[2][3]);
    } else if (jfirst < nt) {
        load_dependent();
    }
    CS_TL(1);
    const int amt = fold.keys ? s_am : (ig.argmax_t ? ig.argmax_t[b] : -1), ams = ig.argmax_s ? ig.argmax_s[b] : -1;
    float gsig = 0.f;
#ifdef SN_CS_TIMELINE
    unsigned walk_max = 0;
#endif
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
        const int l = i * 64 + lane;
        const int lc = l < ns ? l : 0;
        is[i] = l < ns ? (fold.keys ? s_ip[lc] : idxS[lc]) : -1;
        gg[i] = gLv * (ig.cs + (l == ams ? ig.cmax_s : 0.f)) * 2;
    }
    CS_TL_DRAIN();
    CS_TL(2);

    for (int j = jfirst; j < nt; j += jstep) {
        if (j != jfirst) {
            load_query(j);
            load_dependent();
        }
        const float g = gLv * (ig.ct + (j == amt ? ig.cmax_t : 0.f)) * 2;
        float ax = g * (tx - ox), ay = g * (ty - oy), az = g * (tz - oz);  // own term first
        if (j == (int)blockIdx.y * nwaves) { CS_TL_DRAIN(); CS_TL(3); }
        CS_WALK_BEGIN();
        owner_sum<PPL>(s_own[wave], lane, j, is, gg, sx, sy, sz, tx, ty, tz, ax, ay, az);
        CS_WALK_END(ax, ay, az);
        if (j == (int)blockIdx.y * nwaves) CS_TL(4);
        float qx, qy, qz, asg;
        soft_bwd_math<true>(sa, b, j, lane, sigma, sq, qx, qy, qz, asg);
        if (j == (int)blockIdx.y * nwaves) CS_TL(5);
        gsig += asg;
        if (lane < 3) gradT[j + lane * nt] = lane == 0 ? ax + qx : (lane == 1 ? ay + qy : az + qz);
    }
    if (lane == 0) s_part[wave] = gsig;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.f;
        for (int w2 = 0; w2 < nwaves; ++w2) tot += s_part[w2];
        sa.grad_sigma_partial[(size_t)b * nsplit + blockIdx.y] = tot;
    }
    if (jfirst < nt) CS_WALK_STORE();
    CS_TL_DRAIN();
    CS_TL(6);
}

// ------------------------------------------------------------------------------------------------
// The sampler's total loss as registration/main.py:507-531 composes it, with the benchmark's stand-in task term
// (SURVEY.md 8d):   L = alpha * L_simp + lmbda * max(T^2, min_sigma) + mean(proj)
// One single-workgroup kernel forward, one backward (replaces ~20 elementwise / reduction launches of the op-by-op
// composition).  Reductions run in a fixed order.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) sampler_loss_fwd_kernel(int nproj, const float *__restrict__ proj,
                                                                const float *__restrict__ lsimp,
                                                                const float *__restrict__ temperature, float alpha,
                                                                float lmbda, float min_sigma, float *__restrict__ loss)
{
    __shared__ float red[1024];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nproj; i += 1024) acc += proj[i];
    red[threadIdx.x] = acc;
    for (int s = 512; s > 0; s >>= 1) {
        __syncthreads();
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    }
    if (threadIdx.x == 0) {
        const float T = *temperature;
        loss[0] = alpha * lsimp[0] + lmbda * sn_sigma(T, min_sigma) + red[0] / (float)nproj;
    }
}

__global__ void __launch_bounds__(256) sampler_loss_bwd_kernel(int nproj, const float *__restrict__ grad_loss,
                                                               const float *__restrict__ temperature, float alpha,
                                                               float lmbda, float min_sigma, float *__restrict__ grad_proj,
                                                               float *__restrict__ grad_lsimp, float *__restrict__ grad_T)
{
    const float g = grad_loss[0];
    const float gp = g / (float)nproj;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nproj; i += gridDim.x * blockDim.x) grad_proj[i] = gp;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        grad_lsimp[0] = alpha * g;
        const float T = *temperature, t2 = T * T;
        const float w = t2 > min_sigma ? 1.f : (t2 == min_sigma ? 0.5f : 0.f);
        grad_T[0] = lmbda * g * w * 2.0f * T;
    }
}

extern "C" int sn_sampler_loss_forward(int nproj, const float *proj, const float *lsimp, const float *temperature,
                                       float alpha, float lmbda, float min_sigma, float *loss, sn_stream_t stream)
{
    SN_REQUIRE(nproj >= 1 && proj && lsimp && temperature && loss, "bad argument");
    hipLaunchKernelGGL(sampler_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, nproj, proj, lsimp, temperature,
                       alpha, lmbda, min_sigma, loss);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_sampler_loss_backward(int nproj, const float *grad_loss, const float *temperature, float alpha,
                                        float lmbda, float min_sigma, float *grad_proj, float *grad_lsimp, float *grad_T,
                                        sn_stream_t stream)
{
    SN_REQUIRE(nproj >= 1 && grad_loss && temperature && grad_proj && grad_lsimp && grad_T, "bad argument");
    hipLaunchKernelGGL(sampler_loss_bwd_kernel, dim3((nproj + 255) / 256), dim3(256), 0, (hipStream_t)stream, nproj, grad_loss,
                       temperature, alpha, lmbda, min_sigma, grad_proj, grad_lsimp, grad_T);
    SN_LAUNCH_CHECK();
    return 0;
}

// d loss / dT from the per-workgroup partials of d loss / d sigma:  sigma = max(T^2, min_sigma)
//   dT = (sum partial) * 2T * [T^2 > min_sigma]   (torch.max splits the gradient evenly on an exact tie)
__global__ void __launch_bounds__(256) sigma_grad_kernel(int nparts, const float *__restrict__ partial,
                                                         const float *__restrict__ temperature, float min_sigma,
                                                         float *__restrict__ grad_T, const float *__restrict__ gsigma_direct,
                                                         float direct_scale, StepLossFinal fin = StepLossFinal{},
                                                         sn::StepLossKeysFinal kf = sn::StepLossKeysFinal{})
{
    if (fin.loss && blockIdx.x == 1) {  // second workgroup (fold mode): the step's loss value from the per-cloud partials
        if (threadIdx.x < 64) step_loss_final(fin, threadIdx.x);
        return;
    }
    if (kf.loss && blockIdx.x >= 1) {  // keys mode: workgroup 1 combines the loss value, the others re-zero the key table
        if (blockIdx.x == 1) {
            if (threadIdx.x < 64) sn::step_loss_keys_final(kf, threadIdx.x);
        } else {
            const long long nb = gridDim.x - 2, per = (kf.nkeys + nb - 1) / nb;
            const long long i0 = (long long)(blockIdx.x - 2) * per, i1 = i0 + per < kf.nkeys ? i0 + per : kf.nkeys;
            for (long long i = i0 + threadIdx.x; i < i1; i += 256) kf.keys[i] = 0;
        }
        return;
    }
    __shared__ float red[4];
    sn::sigma_grad_block(nparts, partial, temperature, min_sigma, grad_T, gsigma_direct, direct_scale, red);
}

// sigma = max(T^2, min_sigma) (soft_projection.py:97-99) as a device scalar: the projection loss of a script, one launch
// (torch: pow + maximum forward, seven launches backward; sn_sigma_grad with the upstream gradient as its one partial is the backward)
__global__ void sigma_forward_kernel(const float *__restrict__ temperature, float min_sigma, float *__restrict__ sigma)
{
    if (threadIdx.x == 0) sigma[0] = sn_sigma(temperature[0], min_sigma);
}
extern "C" int sn_sigma_forward(const float *temperature, float min_sigma, float *sigma, sn_stream_t stream)
{
    SN_REQUIRE(temperature && sigma, "null pointer");
    hipLaunchKernelGGL(sigma_forward_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, temperature, min_sigma, sigma);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_sigma_grad(int nparts, const float *partial, const float *temperature, float min_sigma, float *grad_T,
                             sn_stream_t stream)
{
    SN_REQUIRE(nparts >= 1 && partial && temperature && grad_T, "bad argument");
    hipLaunchKernelGGL(sigma_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nparts, partial, temperature,
                       min_sigma, grad_T, (const float *)nullptr, 0.f);
    SN_LAUNCH_CHECK();
    return 0;
}

__global__ void __launch_bounds__(1024) step_loss_partial_kernel(int M, int N, int G, int nproj, const float *__restrict__ dq,
                                                                 const sn_u64 *__restrict__ ws, const float *__restrict__ proj,
                                                                 float *__restrict__ dp, int *__restrict__ ip,
                                                                 float *__restrict__ part, int *__restrict__ argmax1)
{
    // one workgroup of 1024 threads per cloud: at N = 1024 every thread finishes one point (its G keys in flight together)
    constexpr int NT = 1024;
    __shared__ float r0[NT], r1[NT], r2[NT], r3[NT];
    __shared__ int ri[NT];
    const int b = blockIdx.x, t = threadIdx.x;
    float s1 = 0.f, mx = -INFINITY, s2 = 0.f, sp = 0.f;
    int am = 0;
    for (int j = t; j < M; j += NT) {
        const float v = dq[(size_t)b * M + j];
        s1 += v;
        if (v > mx) mx = v, am = j;
    }
    for (int n = t; n < N; n += NT) {
        sn_u64 k = kKeyInf;
        for (int g = 0; g < G; ++g) {  // minimum of (distance, query) keys = lowest query on ties
            const sn_u64 v = ws[((size_t)b * G + g) * N + n];
            k = v < k ? v : k;
        }
        const float d = key_dist(k);
        dp[(size_t)b * N + n] = d;
        ip[(size_t)b * N + n] = key_index(k);
        s2 += d;
    }
    for (int i = t; i < nproj; i += NT) sp += proj[(size_t)b * nproj + i];
    r0[t] = s1, r1[t] = mx, r2[t] = s2, r3[t] = sp, ri[t] = am;
    for (int s = NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            r0[t] += r0[t + s];
            r2[t] += r2[t + s];
            r3[t] += r3[t + s];
            if (r1[t + s] > r1[t] || (r1[t + s] == r1[t] && ri[t + s] < ri[t])) r1[t] = r1[t + s], ri[t] = ri[t + s];
        }
    }
    if (t == 0) {
        part[b * 4 + 0] = r0[0], part[b * 4 + 1] = r1[0], part[b * 4 + 2] = r2[0], part[b * 4 + 3] = r3[0];
        argmax1[b] = ri[0];
    }
}

__global__ void __launch_bounds__(64) step_loss_final_kernel(StepLossFinal f) { step_loss_final(f, threadIdx.x); }

// the tail of both forward entries: the clouds' partials, in order, -> loss.  defer_value: the scalar is combined by an extra
// wave of sn_sampler_step_loss_backward's first launch instead (the gradients do not need it; a launch of its own costs
// ~4.7 us inside the step's graph) -- only for callers that always run backward
static void launch_step_loss_final(int B, int M, int N, float weight, float alpha, float lmbda, float min_sigma,
                                   const float *partial, const float *temperature, float *loss, int defer_value, hipStream_t st)
{
    if (defer_value) return;
    const StepLossFinal f{B, M, N, 3 * M, weight, alpha, lmbda, min_sigma, partial, temperature, loss};
    hipLaunchKernelGGL(step_loss_final_kernel, dim3(1), dim3(64), 0, st, f);
}

extern "C" int sn_sampler_step_loss_forward(int B, int M, int N, int G, const float *dist_q, const void *colmin_ws,
                                            const float *proj, const float *temperature, float alpha, float lmbda,
                                            float weight, float min_sigma, float *dist_p, int *idx_p, int *argmax1,
                                            float *partial, float *loss, int defer_value, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && M >= 1 && N >= 1 && G >= 1, "bad size");
    SN_REQUIRE(dist_q && colmin_ws && proj && temperature && dist_p && idx_p && argmax1 && partial && loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(step_loss_partial_kernel, dim3(B), dim3(1024), 0, st, M, N, G, 3 * M, dist_q, (const sn_u64 *)colmin_ws,
                       proj, dist_p, idx_p, partial, argmax1);
    launch_step_loss_final(B, M, N, weight, alpha, lmbda, min_sigma, partial, temperature, loss, defer_value, st);
    SN_LAUNCH_CHECK();
    return 0;
}

// sn_sampler_step_loss_forward behind a scan that ran ONE workgroup per cloud (batches that fill the chip on their own:
// sn_pairscan_colmin_splits(B, N, M) <= 1 -- dist_p / idx_p are complete, there are no partial key sets): per-cloud sums over
// dist_q / dist_p / proj and the arg-max of dist_q, then the clouds in order.  Same partial layout, same final kernel.
__global__ void __launch_bounds__(256) step_loss_partial_direct_kernel(int M, int N, int nproj, const float *__restrict__ dq,
                                                                       const float *__restrict__ dp, const float *__restrict__ proj,
                                                                       float *__restrict__ part, int *__restrict__ argmax1)
{
    constexpr int NT = 256;
    __shared__ float r0[NT], r1[NT], r2[NT], r3[NT];
    __shared__ int ri[NT];
    const int b = blockIdx.x, t = threadIdx.x;
    float s1 = 0.f, mx = -INFINITY, s2 = 0.f, sp = 0.f;
    int am = 0;
    for (int j = t; j < M; j += NT) {
        const float v = dq[(size_t)b * M + j];
        s1 += v;
        if (v > mx) mx = v, am = j;
    }
    for (int n = t; n < N; n += NT) s2 += dp[(size_t)b * N + n];
    for (int i = t; i < nproj; i += NT) sp += proj[(size_t)b * nproj + i];
    r0[t] = s1, r1[t] = mx, r2[t] = s2, r3[t] = sp, ri[t] = am;
    for (int s = NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            r0[t] += r0[t + s];
            r2[t] += r2[t + s];
            r3[t] += r3[t + s];
            if (r1[t + s] > r1[t] || (r1[t + s] == r1[t] && ri[t + s] < ri[t])) r1[t] = r1[t + s], ri[t] = ri[t + s];
        }
    }
    if (t == 0) {
        part[b * 4 + 0] = r0[0], part[b * 4 + 1] = r1[0], part[b * 4 + 2] = r2[0], part[b * 4 + 3] = r3[0];
        argmax1[b] = ri[0];
    }
}

extern "C" int sn_sampler_step_loss_forward_direct(int B, int M, int N, const float *dist_q, const float *dist_p, const float *proj,
                                                   const float *temperature, float alpha, float lmbda, float weight,
                                                   float min_sigma, int *argmax1, float *partial, float *loss, int defer_value,
                                                   sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && M >= 1 && N >= 1, "bad size");
    SN_REQUIRE(dist_q && dist_p && proj && temperature && argmax1 && partial && loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(step_loss_partial_direct_kernel, dim3(B), dim3(256), 0, st, M, N, 3 * M, dist_q, dist_p, proj, partial, argmax1);
    launch_step_loss_final(B, M, N, weight, alpha, lmbda, min_sigma, partial, temperature, loss, defer_value, st);
    SN_LAUNCH_CHECK();
    return 0;
}

// What both backward entries of the step hand to their kernels.  Implicit upstream gradients of the simplification loss -- same
// roundings as the op-by-op route: (alpha * g) first, then the per-term coefficients.  argmax1: NULL in keys mode (the kernel
// takes the farthest query from StepLossFold::qmax).
static ImplicitGrad step_implicit_grad(int B, int N, int M, float weight, float alpha, const float *grad_loss, const int *argmax1)
{
    const float c1 = 1.0f / ((float)B * (float)M), cm = 1.0f / (float)B, c2 = weight / ((float)B * (float)N);
    return ImplicitGrad{grad_loss, argmax1, nullptr, c1, cm, c2, 0.f, alpha};
}

// Soft-projection backward ADDED to grad_Q (B,3,M), sigma partials into gsig_scratch.  grad_proj (B,M,3), optional: the task
// loss's gradient w.r.t. the projected points (main.py:507-531: the task network sits on proj); NULL = the benchmark's
// stand-in term mean(proj) inside this loss, upstream gradient grad_loss / (3BM)
static SoftBwdArgs step_soft_bwd_args(int B, int N, int M, int K, const float *P, const float *Q, const int *knn_idx,
                                      const float *temperature, float min_sigma, const float *grad_loss, const float *grad_proj,
                                      float *grad_Q, float *gsig_scratch)
{
    SoftBwdArgs a{};
    a.P = P, a.Q = Q, a.idx = knn_idx, a.temperature = temperature, a.min_sigma = min_sigma;
    a.p_layout = SN_LAYOUT_BNC, a.q_layout = SN_LAYOUT_BCN, a.n = N, a.m = M, a.k = K;
    a.grad_proj = grad_proj, a.gproj_layout = SN_LAYOUT_BNC, a.gconst = grad_loss, a.gconst_div = (float)(B * 3 * M);
    a.grad_Q = grad_Q, a.gq_layout = SN_LAYOUT_BCN, a.accumulate_q = 1;
    a.grad_P = nullptr, a.grad_sigma_partial = gsig_scratch;
    return a;
}

// alpha * d L_simp / d Q  +  d mean(proj) / d Q  (and the sigma partials) in one launch, N <= 2048.  fin: the deferred loss
// value (an extra row of workgroups in the caller's grid); fold: the keys-mode operands; either may be empty.
static void launch_chamfer_soft_bwd(dim3 grid, int M, int N, const float *Q, const float *P, const int *idx_q, const int *idx_p,
                                    float *grad_Q, const ImplicitGrad &ig, const SoftBwdArgs &a, const StepLossFinal &fin,
                                    const StepLossFold &fold, hipStream_t st)
{
    const dim3 block(256);
    if (N <= 64)
        hipLaunchKernelGGL(chamfer_soft_bwd_kernel<1>, grid, block, 0, st, M, N, Q, P, idx_q, idx_p, grad_Q, ig, a, fin, fold);
    else if (N <= 256)
        hipLaunchKernelGGL(chamfer_soft_bwd_kernel<4>, grid, block, 0, st, M, N, Q, P, idx_q, idx_p, grad_Q, ig, a, fin, fold);
    else if (N <= 1024)
        hipLaunchKernelGGL(chamfer_soft_bwd_kernel<16>, grid, block, 0, st, M, N, Q, P, idx_q, idx_p, grad_Q, ig, a, fin, fold);
    else
        hipLaunchKernelGGL(chamfer_soft_bwd_kernel<32>, grid, block, 0, st, M, N, Q, P, idx_q, idx_p, grad_Q, ig, a, fin, fold);
}

// grad_Q (B,3,M) channel-major (the FC head's layout), grad_T (1).  P: (B,N,3) only -- any p_layout but SN_LAYOUT_BNC is refused
// (the fused kernel loads a point as one 12-byte word); Q: (B,3,M).
// gsig_scratch: B * sn_soft_bwd_splits(B, M) floats.
extern "C" int sn_sampler_step_loss_backward(int B, int N, int M, int K, const float *P, int p_layout, const float *Q,
                                             const int *knn_idx, const int *idx_q, const int *idx_p, const int *argmax1,
                                             const float *temperature, float min_sigma, float alpha, float lmbda,
                                             float weight, const float *grad_loss, float *grad_Q, float *gsig_scratch,
                                             float *grad_T, const float *deferred_partial, float *deferred_loss,
                                             sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && N >= 1 && M >= 1 && K >= 1 && K <= 64, "bad size");
    SN_REQUIRE(!deferred_loss || deferred_partial, "deferred loss value needs the forward's partials");
    SN_REQUIRE(p_layout == SN_LAYOUT_BNC, "the reference cloud must be (B,N,3) here");
    SN_REQUIRE(P && Q && knn_idx && idx_q && idx_p && argmax1 && temperature && grad_loss && grad_Q && gsig_scratch && grad_T,
               "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const ImplicitGrad ig = step_implicit_grad(B, N, M, weight, alpha, grad_loss, argmax1);
    const SoftBwdArgs a = step_soft_bwd_args(B, N, M, K, P, Q, knn_idx, temperature, min_sigma, grad_loss, nullptr, grad_Q, gsig_scratch);
    const int splits = sn_soft_bwd_splits(B, M);  // gsig_scratch is sized by the caller for that many
    const StepLossFinal fin{B, M, N, 3 * M, weight, alpha, lmbda, min_sigma, deferred_partial, temperature, deferred_loss};
    if (N <= 2048) {
        // 1+2. in one launch; the deferred loss value in an extra row of workgroups
        launch_chamfer_soft_bwd(dim3(B, splits + (deferred_loss ? 1 : 0)), M, N, Q, P, idx_q, idx_p, grad_Q, ig, a, fin, StepLossFold{}, st);
    } else {
        // 1. alpha * d L_simp / d Q   (targets = Q, channel-major; sources = P)
        launch_chamfer_bwd(B, splits, M, N, Q, P, nullptr, idx_q, nullptr, idx_p, grad_Q, 1, ig, st, 1);
        // 2. + d mean(proj) / d Q, and the sigma partials
        launch_soft_bwd_fused(B, splits, a, st);
        if (deferred_loss) hipLaunchKernelGGL(step_loss_final_kernel, dim3(1), dim3(64), 0, st, fin);
    }
    // 3. grad_T from the sigma partials and the direct lmbda * sigma term
    hipLaunchKernelGGL(sigma_grad_kernel, dim3(1), dim3(256), 0, st, B * splits, gsig_scratch, temperature, min_sigma, grad_T,
                       grad_loss, lmbda);
    SN_LAUNCH_CHECK();
    return 0;
}

// Loss side of the sampler step behind sn_pairscan_forward_keys (engine): backward + loss value in 2 launches, nothing
// between the scan and the backward.  colmin_keys / qpart / qmax as the scan left them; colmin_keys is zero again afterwards.
// dpsum: B floats of scratch; loss[0] = L, loss[1] = L_simp.  N <= 2048.
extern "C" int sn_sampler_step_loss_keys(int B, int N, int M, int K, const float *P, int p_layout, const float *Q,
                                         const int *knn_idx, const int *idx_q, void *colmin_keys, const float *qpart,
                                         const void *qmax, int G, const float *temperature, float min_sigma, float alpha,
                                         float lmbda, float weight, const float *grad_loss, float *grad_Q,
                                         float *gsig_scratch, float *grad_T, float *dpsum, float *loss, sn_stream_t stream,
                                         void *deferred_tail, const float *grad_proj, const float *grad_sigma)
{
    SN_REQUIRE(B >= 1 && N >= 1 && M >= 1 && K >= 1 && K <= 64 && G >= 1, "bad size");
    SN_REQUIRE(p_layout == SN_LAYOUT_BNC, "the reference cloud must be (B,N,3) here");
    SN_REQUIRE(P && Q && knn_idx && idx_q && colmin_keys && qpart && qmax && temperature && grad_loss && grad_Q && gsig_scratch &&
                   grad_T && dpsum && loss,
               "null pointer");
    if (N > 2048) return sn_set_error(SN_ERR_UNSUPPORTED, "sn_sampler_step_loss_keys: N <= 2048");
    hipStream_t st = (hipStream_t)stream;
    const ImplicitGrad ig = step_implicit_grad(B, N, M, weight, alpha, grad_loss, nullptr);
    const SoftBwdArgs a = step_soft_bwd_args(B, N, M, K, P, Q, knn_idx, temperature, min_sigma, grad_loss, grad_proj, grad_Q, gsig_scratch);
    const int splits = sn_soft_bwd_splits(B, M);  // gsig_scratch is sized by the caller for that many
    StepLossFold fold{};
    fold.G = G, fold.keys = (const sn_u64 *)colmin_keys, fold.qmax = (const sn_u64 *)qmax, fold.dpsum = dpsum;
    launch_chamfer_soft_bwd(dim3(B, splits), M, N, Q, P, idx_q, nullptr, grad_Q, ig, a, StepLossFinal{}, fold, st);
    const StepLossKeysFinal kf{B, G, M, N, 3 * M, weight, alpha, lmbda, min_sigma, qpart, (const sn_u64 *)qmax, dpsum, temperature,
                               loss, (sn_u64 *)colmin_keys, (long long)B * N, grad_proj ? 0 : 1, {nullptr, nullptr}};
    if (deferred_tail) {
        // the caller hands this blob to a later launch of the same step (sn_conv_stack_backward runs it in two extra
        // workgroups of its closing kernel): no launch of its own for the sigma gradient / loss value / key reset
        StepTail t{};
        t.nparts = B * splits, t.gsig = gsig_scratch, t.temperature = temperature, t.min_sigma = min_sigma, t.grad_T = grad_T;
        // (grad_sigma: sigma is an output of the caller's node with an upstream gradient of its own -- the drop-in surface,
        //  where the script forms lmbda * get_projection_loss() itself; else the direct term is lmbda * grad_loss)
        t.grad_loss = grad_sigma ? grad_sigma : grad_loss, t.lmbda = grad_sigma ? 1.f : lmbda, t.kf = kf;
        memcpy(deferred_tail, &t, sizeof(t));
        SN_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(sigma_grad_kernel, dim3(2 + 64), dim3(256), 0, st, B * splits, gsig_scratch, temperature, min_sigma, grad_T,
                       grad_sigma ? grad_sigma : grad_loss, grad_sigma ? 1.f : lmbda, StepLossFinal{}, kf);
    SN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The drop-in module surface on captured work (samplenet_amd/surface.py): registration/main.py:507-531 calls net(x), then
// get_simplification_loss() / get_projection_loss(), weights them itself and calls backward().  The forward graph therefore
// needs the VALUES of L_simp and sigma right behind the keys-mode scan (the engine's fused step gets them from the backward's
// tail), and the backward graph takes three upstream gradients (d / d L_simp, d / d sigma, d / d proj) from device memory.
//   sn_surface_values_keys:  [per cloud: sum of the per-point minima out of the key table (same order as the loss backward's
//                            own sum: strided per-thread sums, xor tree, waves in order); simplified cloud (B,3,M) -> (B,M,3)]
//                            -> [one wave: the clouds in the order of step_loss_keys_final]   values[0] = L_simp,
//                            values[1] = sigma, values[2..4] = mean dist_q, mean_b max dist_q, mean dist_p
//   sn_surface_gather_upstream: the three upstream gradients into the static operands of the captured backward (an absent one
//                            becomes zero) -- one launch instead of three copies
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) surface_cloud_values_kernel(int N, int M, const sn_u64 *__restrict__ keys,
                                                                   const float *__restrict__ y_bcn, float *__restrict__ simp_bnc,
                                                                   float *__restrict__ dpsum)
{
    __shared__ float red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    float sdp = 0.f;
    for (int n = t; n < N; n += 256) sdp += key_dist(~keys[(size_t)b * N + n]);
    if (simp_bnc)
        for (int i = t; i < 3 * M; i += 256) simp_bnc[(size_t)b * 3 * M + i] = y_bcn[(size_t)b * 3 * M + (i % 3) * M + i / 3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sdp += __shfl_xor(sdp, o);
    if ((t & 63) == 0) red[t >> 6] = sdp;
    __syncthreads();
    if (t == 0) dpsum[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(64) surface_values_final_kernel(int B, int G, int M, int N, float w, float min_sigma,
                                                                  const float *__restrict__ qpart, const sn_u64 *__restrict__ qmax,
                                                                  const float *__restrict__ dpsum,
                                                                  const float *__restrict__ temperature, float *__restrict__ values)
{
    const int t = threadIdx.x;
    float s1 = 0.f, mx = 0.f, s2 = 0.f;
    for (int b = t; b < B; b += 64) {
        float a1 = 0.f;
        sn_u64 mk = 0;
        for (int g = 0; g < G; ++g) {
            const size_t o = (size_t)b * G + g;
            a1 += qpart[o * 2];
            mk = qmax[o] > mk ? qmax[o] : mk;
        }
        s1 += a1, mx += key_dist(mk), s2 += dpsum[b];
    }
    const float T = *temperature;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        mx += __shfl_xor(mx, o);
        s2 += __shfl_xor(s2, o);
    }
    if (t != 0) return;
    const float c12 = s1 / ((float)B * (float)M), cmax = mx / (float)B, c21 = s2 / ((float)B * (float)N);
    values[0] = c12 + cmax + w * c21;
    values[1] = sn_sigma(T, min_sigma);
    values[2] = c12, values[3] = cmax, values[4] = c21;
}

extern "C" int sn_surface_values_keys(int B, int N, int M, int G, const void *colmin_keys, const float *qpart, const void *qmax,
                                      const float *temperature, float min_sigma, float weight, const float *y_bcn,
                                      float *simp_bnc, float *dpsum, float *values, sn_stream_t stream)
{
    SN_REQUIRE(B >= 1 && N >= 1 && M >= 1 && G >= 1, "bad size");
    SN_REQUIRE(colmin_keys && qpart && qmax && temperature && dpsum && values && (y_bcn || !simp_bnc), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(surface_cloud_values_kernel, dim3(B), dim3(256), 0, st, N, M, (const sn_u64 *)colmin_keys, y_bcn, simp_bnc,
                       dpsum);
    hipLaunchKernelGGL(surface_values_final_kernel, dim3(1), dim3(64), 0, st, B, G, M, N, weight, min_sigma, qpart,
                       (const sn_u64 *)qmax, dpsum, temperature, values);
    SN_LAUNCH_CHECK();
    return 0;
}

__global__ void __launch_bounds__(256) surface_gather_upstream_kernel(int nproj, const float *__restrict__ g_lsimp,
                                                                      const float *__restrict__ g_sigma,
                                                                      const float *__restrict__ g_proj, float *__restrict__ scalars,
                                                                      float *__restrict__ proj_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nproj) proj_out[i] = g_proj ? g_proj[i] : 0.f;
    if (i == 0) scalars[0] = g_lsimp ? *g_lsimp : 0.f, scalars[1] = g_sigma ? *g_sigma : 0.f;
}

extern "C" int sn_surface_gather_upstream(int nproj, const float *g_lsimp, const float *g_sigma, const float *g_proj,
                                          float *scalars, float *proj_out, sn_stream_t stream)
{
    SN_REQUIRE(nproj >= 1 && scalars && proj_out, "bad argument");
    hipLaunchKernelGGL(surface_gather_upstream_kernel, dim3((nproj + 255) / 256), dim3(256), 0, (hipStream_t)stream, nproj,
                       g_lsimp, g_sigma, g_proj, scalars, proj_out);
    SN_LAUNCH_CHECK();
    return 0;
}

extern "C" int sn_step_tail_bytes(void) { return (int)sizeof(sn::StepTail); }

// Names the error words of the step's FC chain launches (sn_fc_chain_forward* / sn_fc_chain_backward: word 15 of their sync
// buffers; either may be NULL) in a tail blob: the deferred loss value becomes NaN when one of them is set.
extern "C" int sn_step_tail_set_error_words(void *tail_blob, const void *fwd_sync, const void *bwd_sync)
{
    SN_REQUIRE(tail_blob, "null blob");
    StepTail t;
    memcpy(&t, tail_blob, sizeof(t));
    t.kf.chain_err[0] = fwd_sync ? (const unsigned *)fwd_sync + 15 * kFcSyncStride : nullptr;
    t.kf.chain_err[1] = bwd_sync ? (const unsigned *)bwd_sync + 15 * kFcSyncStride : nullptr;
    memcpy(tail_blob, &t, sizeof(t));
    return 0;
}

#ifdef SN_CS_TIMELINE
// copies the first nblocks x 16 stamps of the last chamfer_soft_bwd_kernel launch to the host and clears them
extern "C" int sn_debug_chamfer_soft_bwd_timeline(void *host, int nblocks)
{
    if (nblocks < 0 || nblocks > 8192) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_cs_tl), (size_t)nblocks * 16 * 8) != hipSuccess) return -3;
    static unsigned long long zeros[8192 * 16];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_cs_tl), zeros, sizeof(zeros)) == hipSuccess ? 0 : -4;
}
// ... the per-wave owner-sum durations of the first nblocks workgroups (nblocks x 4 words: ticks + 1, 0 = the wave had no query)
extern "C" int sn_debug_chamfer_soft_bwd_walk(void *host, int nblocks)
{
    if (nblocks < 0 || nblocks > 8192) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_cs_walk), (size_t)nblocks * 4 * 4) != hipSuccess) return -3;
    static unsigned zeros[8192 * 4];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_cs_walk), zeros, sizeof(zeros)) == hipSuccess ? 0 : -4;
}
#endif

/*
 * samplenet_hip_internal.h -- entry points of libsamplenet_hip.so BEHIND the drop-in boundary: the fused
 * multi-layer / single-node forms of the public operations (include/samplenet_hip.h) that the package's own host
 * side drives (samplenet_amd/pointnet.py, fused_step.py, engine.py).  Same calling conventions as the public
 * header (caller-owned device buffers, stream-ordered, 0 / error code).  None of these replaces a reference
 * interface one to one -- each names the public entries / reference lines whose composition it computes -- and
 * they may change with the kernels (no ABI promise: sn_abi_version() covers samplenet_hip.h only).
 */
#ifndef SAMPLENET_HIP_INTERNAL_H
#define SAMPLENET_HIP_INTERNAL_H

#include "samplenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The sampler's total loss with the benchmark's stand-in task term (registration/main.py:507-531):
 *     L = alpha * L_simp + lmbda * max(T^2, min_sigma) + mean(proj)        (all operands device scalars / tensors)
 * forward: loss (1 float).  backward: grad_proj (nproj floats, = grad_loss / nproj), grad_lsimp (1), grad_T (1). */
int sn_sampler_loss_forward(int nproj, const float *proj, const float *lsimp, const float *temperature,
                            float alpha, float lmbda, float min_sigma, float *loss, sn_stream_t stream);
int sn_sampler_loss_backward(int nproj, const float *grad_loss, const float *temperature, float alpha, float lmbda,
                             float min_sigma, float *grad_proj, float *grad_lsimp, float *grad_T, sn_stream_t stream);

/* The sampler's training-step loss with the benchmark's stand-in task term, in the fewest launches the dependencies allow
 * (the op-by-op route above computes the same numbers):
 *   sn_pairscan_forward_partial   pair scan that leaves the per-point minima as G = sn_pairscan_colmin_splits(B,N,M) partial
 *                                 key sets (workspace [B][G][N] u64); SN_ERR_UNSUPPORTED when G <= 1
 *   sn_sampler_step_loss_forward  finishes dist_p / idx_p from those partials while reducing the loss; loss[0] = L,
 *                                 loss[1] = L_simp; partial: B*4 floats; argmax1: B ints
 *   sn_sampler_step_loss_backward grad_Q (B,3,M) = d L / d simplified cloud, grad_T; gsig_scratch: B*sn_soft_bwd_splits(B,M) */
int sn_pairscan_colmin_splits(int B, int N, int M);
int sn_pairscan_forward_partial(int B, int N, int M, int K, const float *P, int p_layout, const float *Q, int q_layout,
                                int *knn_idx, float *dist_q, int *idx_q, float *proj, int proj_layout,
                                const float *temperature, float min_sigma, void *workspace, long long workspace_bytes,
                                sn_stream_t stream);
/* sn_pairscan_forward_partial with the queries PRODUCED inside the scan by the head's last fully connected layer
 * (samplenet.py:103-104): q[b][c][j] = fc_bias[c*M+j] + sum_k relu(fc_z[b][k]*fc_scale[k] + fc_shift[k]) * fc_w[c*M+j][k];
 * q_out (B,3,M) receives the simplified cloud.  Kfc % 4 == 0.  One launch less than FC layer + scan. */
int sn_pairscan_forward_partial_fc(int B, int N, int M, int K, const float *P, int p_layout, const float *fc_z,
                                   const float *fc_scale, const float *fc_shift, const float *fc_w, const float *fc_bias,
                                   int Kfc, float *q_out, int *knn_idx, float *dist_q, int *idx_q, float *proj,
                                   int proj_layout, const float *temperature, float min_sigma, void *workspace,
                                   long long workspace_bytes, sn_stream_t stream);
int sn_sampler_step_loss_forward(int B, int M, int N, int G, const float *dist_q, const void *colmin_ws, const float *proj,
                                 const float *temperature, float alpha, float lmbda, float weight, float min_sigma,
                                 float *dist_p, int *idx_p, int *argmax1, float *partial, float *loss, int defer_value,
                                 sn_stream_t stream);
/* sn_sampler_step_loss_forward behind a scan that ran one workgroup per cloud (sn_pairscan_colmin_splits <= 1: batches that
 * fill the chip on their own; dist_p / idx_p complete, e.g. from sn_pairscan_forward_ws): same partial / loss outputs. */
int sn_sampler_step_loss_forward_direct(int B, int M, int N, const float *dist_q, const float *dist_p, const float *proj,
                                        const float *temperature, float alpha, float lmbda, float weight, float min_sigma,
                                        int *argmax1, float *partial, float *loss, int defer_value, sn_stream_t stream);
int sn_sampler_step_loss_backward(int B, int N, int M, int K, const float *P, int p_layout, const float *Q,
                                  const int *knn_idx, const int *idx_q, const int *idx_p, const int *argmax1,
                                  const float *temperature, float min_sigma, float alpha, float lmbda, float weight,
                                  const float *grad_loss, float *grad_Q, float *gsig_scratch, float *grad_T,
                                  const float *deferred_partial, float *deferred_loss, sn_stream_t stream);
/* The same step with NO launch between the scan and the backward (engine default): sn_pairscan_forward_keys combines the
 * per-point minima across a cloud's workgroups by 64-bit atomicMax on inverted (distance, query) keys (max / min are
 * order-independent: deterministic) in colmin_keys [B][N] -- u64, zero on entry, zero again after
 * sn_sampler_step_loss_keys -- and leaves the query-side loss partials qpart [B][G][2] floats / qmax [B][G] u64,
 * G = sn_pairscan_colmin_splits(B,N,M) > 1.  Q (B,3,M) is read, or written when fc_w != NULL (queries produced by the
 * head's last layer as in sn_pairscan_forward_partial_fc).  dpsum: B floats of scratch; loss: 2 floats.  N <= 2048.
 * deferred_tail (optional, host buffer of sn_step_tail_bytes() bytes): the launch that produces grad_T / loss and resets
 * colmin_keys is not issued at all; its description is written there and handed to sn_conv_stack_backward(step_tail) of the same step, whose closing kernel runs it. */
int sn_pairscan_forward_keys(int B, int N, int M, int K, const float *P, int p_layout, float *Q, const float *fc_z,
                             const float *fc_scale, const float *fc_shift, const float *fc_w, const float *fc_bias, int Kfc,
                             int *knn_idx, float *dist_q, int *idx_q, float *proj, int proj_layout, const float *temperature,
                             float min_sigma, void *colmin_keys, float *qpart, void *qmax, sn_stream_t stream);
int sn_sampler_step_loss_keys(int B, int N, int M, int K, const float *P, int p_layout, const float *Q, const int *knn_idx,
                              const int *idx_q, void *colmin_keys, const float *qpart, const void *qmax, int G,
                              const float *temperature, float min_sigma, float alpha, float lmbda, float weight,
                              const float *grad_loss, float *grad_Q, float *gsig_scratch, float *grad_T, float *dpsum,
                              float *loss, sn_stream_t stream, void *deferred_tail, const float *grad_proj,
                              const float *grad_sigma);
/* grad_proj (B,M,3), optional: gradient of a task loss that lives OUTSIDE this node w.r.t. the projected points (the task
 * network of registration/main.py:507-531 sits on proj); the loss value then carries no mean(proj) term.  NULL: the
 * benchmark's stand-in term mean(proj) is part of the loss and its gradient grad_loss / (3 B M) is implicit. */
/* grad_sigma (1 float, optional): upstream gradient of sigma = max(T^2, min_sigma) as an OUTPUT of the caller's node (the
 * drop-in surface: the script forms lmbda * get_projection_loss() itself); grad_T's direct term is then grad_sigma * d sigma / dT
 * instead of lmbda * grad_loss * d sigma / dT. */
/* The drop-in module surface on captured work (samplenet_amd/surface.py; registration/main.py:507-531 calls net(x), the two
 * loss getters and backward() itself): values of L_simp and sigma right behind sn_pairscan_forward_keys -- values[0] = L_simp
 * (samplenet.py:171-181 with `weight` = gamma + delta * pc_size), [1] = sigma, [2..4] = mean dist_q, mean_b max_m dist_q,
 * mean dist_p; simp_bnc (optional): y_bcn (B,3,M) transposed to (B,M,3); dpsum: B floats of scratch; the key table is read,
 * not reset.  sn_surface_gather_upstream: the node's three upstream gradients (each optional: NULL = zero) into the static
 * operands of the captured backward: scalars[0] = d / d L_simp, scalars[1] = d / d sigma, proj_out (nproj floats). */
int sn_surface_values_keys(int B, int N, int M, int G, const void *colmin_keys, const float *qpart, const void *qmax,
                           const float *temperature, float min_sigma, float weight, const float *y_bcn, float *simp_bnc,
                           float *dpsum, float *values, sn_stream_t stream);
int sn_surface_gather_upstream(int nproj, const float *g_lsimp, const float *g_sigma, const float *g_proj, float *scalars,
                               float *proj_out, sn_stream_t stream);
/* From how many 64-row tiles per workgroup sn_conv_stack_forward_bn runs its GEMM layers as persistent weight-stationary
 * kernels (large batches; default 4, 0: never).  Returns the previous value.  A test / A-B hook: results are bit-identical. */
int sn_conv_stack_set_persist_min_tiles(int tiles);
/* Test / A-B hook of sn_furthest_point_sample: 0 = auto (default), 1 / 2 / 3 = force (a) one wave per cloud (N <= 2048),
 * (b) one workgroup per cloud (N <= 16384), (c) streaming (any N).  A forced variant that cannot take the shape makes the call
 * return SN_ERR_UNSUPPORTED.  Returns the previous value (-1 and no change for v outside 0..3).  Indices are bit-identical
 * across the variants. */
int sn_fps_set_variant(int v);
int sn_step_tail_bytes(void);
/* Names the error words of the step's FC chain launches (the `sync` buffers of sn_fc_chain_forward[_pool] /
 * sn_fc_chain_backward, either may be NULL) in a deferred-tail blob: the loss value the tail writes is NaN when a hand-off
 * of one of those launches timed out (sync[15] != 0). */
int sn_step_tail_set_error_words(void *tail_blob, const void *fwd_sync, const void *bwd_sync);
/* defer_value != 0: the forward leaves loss[] unwritten; pass its `partial` and `loss` to the backward call as
 * deferred_partial / deferred_loss and the scalar is combined by an extra wave of the backward's first launch (the
 * gradients do not depend on it) -- for callers that always run the backward (samplenet_amd.engine).  Else pass NULLs. */


/* layer-level entry points (what samplenet_amd/pointnet.py calls): a layer's forward INCLUDING its BatchNorm
 * finalisation, and a layer's backward (dW, optional db, dYprev) INCLUDING the BatchNorm backward coefficients of the
 * layer below; they pick the fused single-/dual-launch kernels by shape and fall back to the pieces above otherwise. */
int sn_layer_forward_bn(int R, int Ci, int Co, const float *ain, const float *coef_prev, const float *W,
                        const float *bias, float *z, float *stats, const float *gamma, const float *beta,
                        float eps, float momentum, float *running_mean, float *running_var,
                        long long *num_batches_tracked, float *coef, sn_stream_t stream);
/* sn_layer_forward_bn of the last conv layer with the max-pool over the npts points of every cloud folded in (the forward
 * epilogue leaves per-block maxima / minima, the BatchNorm finalisation picks): pooled / argsel / zsel as sn_pool_forward;
 * pool_val / pool_idx: scratch of sn_linear_stats_blocks(R) * 2 * Co elements each.  SN_ERR_UNSUPPORTED unless R, npts, Ci,
 * Co are multiples of 64. */
int sn_conv_forward_bn_pool(int R, int Ci, int Co, int npts, const float *ain, const float *coef_prev, const float *W,
                            const float *bias, float *z, float *stats, const float *gamma, const float *beta, float eps,
                            float momentum, float *running_mean, float *running_var, long long *num_batches_tracked,
                            float *coef, float *pool_val, int *pool_idx, float *pooled, int *argsel, float *zsel,
                            sn_stream_t stream);
/* The training-mode conv stack (conv/bn/relu x nlayers on the xyz cloud + max over the points, samplenet.py:90-95) in one
 * call and nlayers + 1 launches.  Batch statistics travel as 64-bit fixed-point sums accumulated with integer atomics
 * (order-independent, hence deterministic); each layer finalises the BatchNorm of its input itself, so no reduction launch
 * sits between layers.  channels [nlayers+1] = 3, C1..Cn (64 or 128 each; inner layers up to 256 --
 * reconstruction/src/samplers.py:23-38 -- when pooled != NULL and B * N / 64 row blocks can carry the weight split); N % 64 == 0
 * (query _supported first).
 * Arrays of nlayers device pointers: W (C_{l+1},C_l), bias, gamma, beta, running_mean, running_var, num_batches_tracked,
 * z (B*N,C_{l+1}) pre-BN outputs, coef (4,C_{l+1}); eps / momentum: host arrays.  acc: sn_conv_stack_acc_elems(nlayers) long long of persistent
 * device scratch, zero before the first call (every call leaves it zero).  pool_val / pool_idx: (B*N/64)*2*Cn scratch.
 * pooled = argsel = zsel = NULL: stop after the last GEMM; sn_fc_chain_forward_pool must follow (it finishes the pool).  The last
 * layer then leaves, instead of block partials, (B, 2, Cn) 64-bit keys in pool_val -- per cloud and channel (max Z, first row)
 * and (min Z, first row), combined by atomicMax -- which sn_fc_chain_forward_pool decodes; pool_val must then hold at least
 * 4 * B * Cn floats (16 bytes per cloud and channel: more than the block partials only when N < 128). */
int sn_conv_stack_forward_supported(int B, int N, int nlayers, const int *channels);
long long sn_conv_stack_acc_elems(int nlayers);
/* 1: z[0] may be NULL in sn_conv_stack_forward_bn / sn_conv_stack_backward for this shape -- the xyz layer then runs as a
 * statistics-only pass and its activation (B*N, C1) is never written: conv2's forward and backward rebuild it from the cloud
 * with the xyz layer's own expression (bit-identical results, 8 MB less written and 16 MB less read per step at B = 32). */
int sn_conv_stack_z1_free_supported(int B, int N, int nlayers, const int *channels);
/* the leading part of acc that holds the statistics accumulators (zero between calls): one block of sums per layer, two when a
 * layer of the stack is wider than 128 channels (channels: the nlayers + 1 widths as passed to sn_conv_stack_forward_bn, or NULL for
 * the narrow layout); behind it: scratch of the forward (the layers' weights split into bf16 planes by the first kernel of the
 * call), which is not zero between calls */
long long sn_conv_stack_acc_sum_elems(int nlayers, const int *channels);
int sn_conv_stack_forward_bn(int B, int N, int nlayers, const int *channels, const float *x, const float *const *W,
                             const float *const *bias, const float *const *gamma, const float *const *beta,
                             float *const *running_mean, float *const *running_var, long long *const *num_batches_tracked,
                             const float *eps, const float *momentum, float *const *z, float *const *coef, long long *acc,
                             float *pool_val, int *pool_idx, float *pooled, int *argsel, float *zsel, sn_stream_t stream);
/* Backward of the conv stack, the mirror of sn_conv_stack_forward_bn, in nlayers launches: one fused dgrad + wgrad kernel
 * per GEMM layer (top first) and one closing kernel that reduces every layer's weight-gradient partials and finishes the
 * xyz layer (BatchNorm backward, closed-form weight gradient).  The BatchNorm-backward sums travel between the kernels as
 * fixed-point atomics; each kernel derives its own layer's dZ coefficients in its prologue.
 * gsel / argsel (B,Cn), kcoef_top (3,Cn): pooled gradient at the selected points and the top BatchNorm's dZ coefficients
 * (sn_layer_backward with prev_bn_rows, or sn_pool_backward_bn).  dW: nlayers outputs; dgamma / dbeta / dbias: outputs for
 * layers 0 .. nlayers-2.  acc: sn_conv_stack_acc_elems(nlayers) long long of persistent zeroed scratch (its own buffer, not
 * the forward's); scratch: sn_conv_stack_backward_scratch_floats(...) floats (0 = shape not supported). */
long long sn_conv_stack_backward_scratch_floats(int B, int N, int nlayers, const int *channels);
int sn_conv_stack_backward(int B, int N, int nlayers, const int *channels, const float *x, const float *const *W,
                           const float *bias0, const float *const *z, const float *const *coef, const float *gsel,
                           const int *argsel, const float *kcoef_top, long long *acc, float *scratch, float *const *dW,
                           float *const *dgamma, float *const *dbeta, float *const *dbias, const void *step_tail,
                           sn_stream_t stream);
int sn_layer_backward(int R, int Ci, int Co, int dz_mode, const float *dy, const float *z, const float *kcoef,
                      const float *gsel, const int *argsel, int npts, const float *W, const float *zprev,
                      const float *coef_prev, float *dyprev, float *stats, float *part, float *dW, float *db,
                      float *prev_dgamma, float *prev_dbeta, float *prev_dbias, float *prev_kcoef, long long prev_bn_rows,
                      sn_stream_t stream);
/* sn_layer_backward (dz_mode = SN_DZ_BN) for the layer that sits on the xyz input layer (3 -> Ci, x_in (R,3), W_in (Ci,3),
 * b_in (Ci) or NULL): also returns dW_in (Ci,3), the input layer's weight gradient, in closed form from three extra
 * per-channel sums and the second moments of x_in accumulated by the same kernel -- no separate pass over dYprev, which
 * is not written at all (the input layer has no gradient to pass further down).
 * stats: sn_layer_backward_in3_stats_floats(R, Ci, Co) floats; that function returns 0 when the shape is not supported. */
long long sn_layer_backward_in3_stats_floats(int R, int Ci, int Co);
int sn_layer_backward_in3(int R, int Ci, int Co, const float *dy, const float *z, const float *kcoef, const float *W,
                          const float *zprev, const float *coef_prev, float *stats, float *part, float *dW,
                          float *prev_dgamma, float *prev_dbeta, float *prev_dbias, float *prev_kcoef, const float *x_in,
                          const float *W_in, const float *b_in, float *dW_in, sn_stream_t stream);
/* prev_bn_rows (> 0: R <= 32 only; 0 = R): rows seen by the BatchNorm of the layer below when they differ from R -- the FC head's
 * first layer on top of the max-pool: zprev = pooled pre-BN values (B rows), BatchNorm over B*N rows; replaces sn_pool_backward.
 * prev_bn_rows < 0 (any R): that BatchNorm normalised with FIXED statistics (eval mode: coef_prev from sn_bn_eval_coef), so its
 * backward is dZ = scale * dY (k2 = k3 = 0); dgamma / dbeta as usual.  Likewise R < 0 in sn_pool_backward_bn. */

/* The FC head's BatchNorm + ReLU layers (R <= 32 rows; a0 (R, C0) -> H -> ... -> H, nl layers) as ONE launch: the H / 32
 * workgroups of a layer stay resident and exchange each layer's activations through xbuf with write-through stores and an
 * arrival counter instead of ending the kernel per layer.  Per layer l: W[l] (H, K), bias, BatchNorm parameters / running
 * statistics (training-mode update as sn_layer_forward_bn; running_mean[l] set needs running_var[l] set), outputs z[l] (R, H)
 * pre-BN and coef[l] (4, H).  Against nl calls of sn_layer_forward_bn fed with the same inputs (tests/test_gpu_fc_chain.py; observed
 * values in profiles/fc_chain/errors.txt): every z[l] and the mean row of coef[l] are bit-identical; scale, invstd within 4 ulps;
 * shift within 4 ulps of |beta| + |mean scale|; running_mean within 2 and running_var within 8 ulps of the sum of their two terms'
 * magnitudes (this kernel: fp32 reciprocal square root refined in double, reciprocals from the host, a differently contracted
 * epilogue).  A row count outside 1..32 is SN_ERR_BAD_ARGUMENT, a width / depth not served SN_ERR_UNSUPPORTED (nl = 4 never fits the
 * LDS).  xbuf: 2 * 32 * H floats of scratch; sync: 16 WORDS of state spaced 128 bytes apart (16 x 32 unsigned = 2 KB; "sync[i]"
 * below is the 32-bit word at byte offset 128 i: every counter on its own cache line), PERSISTENT and zero-initialised
 * once by the caller (epoch + monotonic arrival counters).  The workgroups of a launch must be RESIDENT TOGETHER (8 x ~137 KB
 * of LDS on otherwise free CUs).  A hand-off poll that gives up -- after sync[13] polls when that word is non-zero, else 2^22 --
 * sets sync[15] and the workgroup writes NaN instead of its outputs; afterwards the counters are out of step: the caller zeroes
 * `sync` before the next launch (samplenet_amd.pointnet.check_chain_errors).  ONE sync block per depth: a launch advances the
 * counters of the seams IT has (forward: sync[1 .. nl - 1]; backward: sync[1 .. ns - 1] and sync[14]) to 8 (16) times the epoch, so a
 * block shared between launches of different nl / ns leaves the other depth's counters out of step with sync[0].  The counters wrap
 * modulo 2^32 by design (the polls compare the signed difference). */
int sn_fc_chain_forward_supported(int R, int C0, int H, int nl);
int sn_fc_chain_forward(int R, int C0, int H, int nl, const float *a0, const float *const *W, const float *const *bias,
                        const float *const *gamma, const float *const *beta, float *const *running_mean,
                        float *const *running_var, long long *const *num_batches_tracked, const float *eps,
                        const float *momentum, float *const *z, float *const *coef, float *xbuf, unsigned *sync,
                        sn_stream_t stream);
/* sn_fc_chain_forward with the tail of the conv stack in front (samplenet.py:90-101: bn5 / relu / max over the points /
 * fc1..fc3): call sn_conv_stack_forward_bn with pooled = argsel = zsel = NULL -- it then stops after its last GEMM, leaving
 * the last layer's fixed-point sums in acc and the block maxima / minima in pool_val / pool_idx -- and this entry right after:
 * its first stage finalises that BatchNorm (gamma5 .. coef5, clearing acc) and decodes the max-pool from the keys (pooled /
 * argsel / zsel as sn_pool_forward) in EVERY workgroup -- no exchange in front of fc1.  B <= 32 clouds, N % 64 == 0, conv stack
 * of nconv layers ending in C0 = 128 channels, H = 256, nl = 3 (query _supported).  Same results as the two separate calls.
 * pool_val: the keys; pool_idx: unused. */
int sn_fc_chain_forward_pool_supported(int B, int N, int C0, int H, int nl);
int sn_fc_chain_forward_pool(int B, int N, int nconv, long long *acc, const float *pool_val, const int *pool_idx,
                             const float *gamma5, const float *beta5, float *running_mean5, float *running_var5,
                             long long *num_batches_tracked5, float eps5, float momentum5, float *coef5, float *pooled,
                             int *argsel, float *zsel, int H, int nl, const float *const *W, const float *const *bias,
                             const float *const *gamma, const float *const *beta, float *const *running_mean,
                             float *const *running_var, long long *const *num_batches_tracked, const float *eps,
                             const float *momentum, float *const *z, float *const *coef, float *xbuf, unsigned *sync,
                             sn_stream_t stream);
/* sn_fc_chain_forward_pool with the head's OUTPUT layer behind the hidden layers as the chain's last stage: Linear (Co x H) +
 * BatchNorm WITHOUT activation -- the classification task's sampler (classification/models/samplenet_model.py:100-108).  Wo (Co, H),
 * bo (Co), gamma_o / beta_o (Co), running statistics of that BatchNorm (may be NULL), eps_o / momentum_o -> zo (B, Co) pre-BatchNorm
 * output, coef_o (4, Co), y (B, Co) = zo scale + shift.  Co: a multiple of 32, at most H.  One launch instead of this one +
 * sn_layer_forward_bn_out. */
int sn_fc_chain_forward_pool_out_supported(int B, int N, int C0, int H, int nl, int Co);
int sn_fc_chain_forward_pool_out(int B, int N, int nconv, long long *acc, const float *pool_val, const int *pool_idx,
                                 const float *gamma5, const float *beta5, float *running_mean5, float *running_var5,
                                 long long *num_batches_tracked5, float eps5, float momentum5, float *coef5, float *pooled,
                                 int *argsel, float *zsel, int H, int nl, const float *const *W, const float *const *bias,
                                 const float *const *gamma, const float *const *beta, float *const *running_mean,
                                 float *const *running_var, long long *const *num_batches_tracked, const float *eps,
                                 const float *momentum, float *const *z, float *const *coef, float *xbuf, unsigned *sync, int Co,
                                 const float *Wo, const float *bo, const float *gamma_o, const float *beta_o, float *running_mean_o,
                                 float *running_var_o, long long *num_batches_tracked_o, float eps_o, float momentum_o, float *zo,
                                 float *coef_o, float *y, sn_stream_t stream);
/* The FC head's backward (R <= 32 rows) as ONE launch, the mirror of sn_fc_chain_forward.  Stage s = GEMM layer, TOP first:
 * W[s] (Co[s], Ci[s]); below it: zprev[s] (R, Ci[s]) pre-BN output seen through coefprev[s] (4, Ci[s]) (the pooled-feature
 * stage: zsel with the last conv layer's coefficients and bn_rows[s] = B * N; bn_rows < 0: fixed statistics); outputs per
 * stage: dW[s], the layer below's dgamma / dbeta / dbias; db_top: bias gradient of the top layer; aprev[s] / araw[s]: the
 * weight-gradient operand (zprev with ReLU(BN) applied, or a raw input such as the pooled features).  Last stage also
 * returns gout (R, Ci) = the masked gradient and kout (3, Ci) = the dZ coefficients of the BatchNorm below (what
 * sn_conv_stack_backward takes as gsel / kcoef_top).  gy: (R, Co[0]).  db_top, any dbias[s], gout and kout may be NULL (the other
 * outputs do not change by a bit).  Same arithmetic as the sn_layer_backward chain up to the contraction of the epilogues (the module
 * tests hold the two to 2e-5 / 6e-5); against fp64 every output stays under the first-order bounds counted in tests/fc_chain_ref.py,
 * and integer data comes out bit-exact.  One sync block per depth ns (see sn_fc_chain_forward).
 * xbuf: ns * 32 * 256 floats of scratch; sync: 16 x 32 unsigned (same layout) of its OWN persistent zero-initialised state (launch epoch, one
 * monotonic arrival counter per stage, epoch-reader count; sync[13] / sync[15] and the NaN poisoning as sn_fc_chain_forward;
 * 16 workgroups must be resident together). */
int sn_fc_chain_backward_supported(int R, int ns, const int *Co, const int *Ci);
int sn_fc_chain_backward(int R, int ns, const int *Co, const int *Ci, const float *gy, const float *const *W,
                         const float *const *zprev, const float *const *coefprev, const long long *bn_rows,
                         float *const *dgamma, float *const *dbeta, float *const *dbias, float *const *dW, float *db_top,
                         const float *const *aprev, const int *araw, float *gout, float *kout, float *xbuf,
                         unsigned *sync, sn_stream_t stream);
/* sn_fc_chain_backward for a head whose output went through a BatchNorm WITHOUT activation (the classification sampler's output
 * layer: sn_layer_forward_bn_out / sn_fc_chain_forward_pool_out): gy is the gradient behind that BatchNorm, zo (R, Co[0]) its
 * input, coef_o (4, Co[0]) the forward's coefficients; the launch opens with that BatchNorm's backward (the arithmetic of
 * sn_bn_output_backward, rows summed in order) and leaves dgamma_o / dbeta_o (Co[0]).  fixed != 0: running statistics.
 * Bit-identical, every output, to sn_bn_output_backward followed by sn_fc_chain_backward on its dz. */
int sn_fc_chain_backward_obn(int R, int ns, const int *Co, const int *Ci, const float *gy, const float *zo, const float *coef_o, int fixed,
                             float *dgamma_o, float *dbeta_o, const float *const *W, const float *const *zprev,
                             const float *const *coefprev, const long long *bn_rows, float *const *dgamma, float *const *dbeta,
                             float *const *dbias, float *const *dW, float *db_top, const float *const *aprev, const int *araw, float *gout,
                             float *kout, float *xbuf, unsigned *sync, sn_stream_t stream);
/* sn_bn_finalize for a SHORT matrix z (R, C) (the FC head at batches above 32): statistics in two passes over z itself (mean,
 * then squares around it) instead of from sum / sum-of-squares partials -- behind the max-pool |mean| / std reaches 10..100. */
int sn_bn_batch_stats_twopass(int R, int C, const float *z, const float *gamma, const float *beta, float eps, float momentum,
                              float *running_mean, float *running_var, long long *num_batches_tracked, float *coef,
                              sn_stream_t stream);

/* The BatchNorm WITHOUT activation on the head's output -- the classification task's sampler (classification/models/
 * samplenet_model.py:100-108: fc14b with bn=True, activation_fn=None; the registration sampler has no such layer, registration/
 * src/samplenet.py:59,104).
 *   sn_layer_forward_bn_out   R <= 32 rows, Ci a power of two in 64 .. 512: ONE launch -- z (R, Co) = act(ain) W^T + bias (act =
 *                             relu(scale x + shift) with coef_prev, identity when NULL), training-mode batch statistics over the R
 *                             rows -> coef (4, Co) = scale, shift, mean, invstd + running statistics as torch.nn.BatchNorm1d, and
 *                             y (R, Co) = z scale + shift.  Other shapes: SN_ERR_UNSUPPORTED (sn_linear_forward_rows + the next one).
 *   sn_bn_output_forward      any R, any C: training != 0: two-pass batch statistics of z (as sn_bn_batch_stats_twopass), else
 *                             coefficients from the running statistics; then y = z scale + shift.
 *   sn_bn_output_backward     gy (R, C) -> dz (R, C), dgamma (C), dbeta (C); fixed != 0: the forward ran on running statistics
 *                             (dz = scale gy).  Sums in double, fixed order (deterministic). */
int sn_layer_forward_bn_out(int R, int Ci, int Co, const float *ain, const float *coef_prev, const float *W, const float *bias,
                            float *z, const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                            float *running_var, long long *num_batches_tracked, float *coef, float *y, sn_stream_t stream);
int sn_bn_output_forward(int R, int C, int training, const float *z, const float *gamma, const float *beta, float eps,
                         float momentum, float *running_mean, float *running_var, long long *num_batches_tracked, float *coef,
                         float *y, sn_stream_t stream);
int sn_bn_output_backward(int R, int C, int fixed, const float *gy, const float *z, const float *coef, float *dz, float *dgamma,
                          float *dbeta, sn_stream_t stream);

/* sn_pool_backward + sn_bn_backward_coef of the last conv layer (R = B * N rows seen by its BatchNorm) in one launch */
int sn_pool_backward_bn(int B, int C, long long R, const float *g, const float *pooled, const float *zsel, float *gsel,
                        const float *coef, float *dgamma, float *dbeta, float *dbias, float *kcoef, sn_stream_t stream);

/* dgrad + wgrad of one layer in ONE launch (both kinds of workgroups resident together); same arguments, no bias column */
int sn_linear_backward(int R, int Ci, int Co, int dz_mode, const float *dy, const float *z, const float *kcoef,
                       const float *gsel, const int *argsel, int npts, const float *W, const float *zprev,
                       const float *coef_prev, float *dyprev, float *stats, float *part, float *dW, sn_stream_t stream);

/* the fused data+weight gradient kernel of a 64/128-channel 1x1 convolution on its own: dYprev, stats partials [G][2][Ci],
 * dW partials [G][Co][Ci], G = sn_linear_wgrad_splits(R,Ci,Co,0); SN_ERR_UNSUPPORTED for other shapes */
int sn_conv_backward_partials(int R, int Ci, int Co, int dz_mode, const float *dy, const float *z, const float *kcoef,
                              const float *gsel, const int *argsel, int npts, const float *W, const float *zprev,
                              const float *coef_prev, float *dyprev, float *stats, float *part, sn_stream_t stream);

/* Task network (registration/models/pcrnet.py:23-41 PointNetFeatures: 1x1 convolutions + ReLU without BatchNorm, max over the
 * points) -- fused form of sn_linear_forward + sn_pool_forward:
 *   sn_linear_forward_maxpool   last layer + max over the npts points of every cloud in one GEMM launch (+ a 2 KB-per-cloud key
 *                               clear and a decode launch): pooled (B,Co) = relu(max_n Z), argsel / zsel (optional) as
 *                               sn_pool_forward; z (R,Co) optional -- NULL: the activations are never written (a branch
 *                               that needs no gradient).  coef_prev: the previous layer's (scale, shift) = (1, 0) table.
 *                               keys: B * 2 * Co 64-bit words of scratch, cleared here unless keys_cleared != 0 (an earlier launch
 *                               on the stream did: sn_pointnet_narrow_forward's zero_keys).  Query _supported (64-aligned shapes). */
int sn_linear_forward_maxpool_supported(int R, int Ci, int Co, int npts);
int sn_linear_forward_maxpool(int R, int Ci, int Co, int npts, const float *ain, const float *coef_prev, const float *W,
                              const float *bias, float *z, unsigned long long *keys, float *pooled, int *argsel, float *zsel,
                              int keys_cleared, sn_stream_t stream);

/*   sn_linear_forward_maxpool_wide   the same for a WIDE last layer (PCRNet: 128 -> 1024): a workgroup keeps the split A fragments
 *                               of its 128 rows in registers for all of its columns, the weights are split once per call into
 *                               wplanes (3 * Co * Ci bf16; planes_ready != 0: already holds the split of this W); the maxima
 *                               leave as one key per column and min(128, npts) rows (scratch: _scratch_bytes) -- no atomics, no
 *                               clear; results bit-identical to sn_linear_forward_maxpool.  coef_prev == NULL (which the tile
 *                               entry refuses): the operand is used as is, no ReLU.  Query _supported. */
int sn_linear_forward_maxpool_wide_supported(int R, int Ci, int Co, int npts);
long long sn_linear_forward_maxpool_wide_scratch_bytes(int R, int Ci, int Co, int npts);
int sn_linear_forward_maxpool_wide(int R, int Ci, int Co, int npts, const float *ain, const float *coef_prev, const float *W,
                                   const float *bias, float *z, void *scratch, float *pooled, int *argsel, float *zsel,
                                   void *wplanes, int planes_ready, sn_stream_t stream);
/*   sn_pool_dgrad_sparse        data gradient of that last layer for a BatchNorm-free stack (dZ has ONE non-zero per cloud and
 *                               channel): dyprev (B*npts, Ci) = relu'_prev . sum_c [argsel[b][c] == n] (pooled > 0 ? g : 0)[b][c]
 *                               W[c][:] -- sn_pool_backward + sn_linear_dgrad(DZ_POOL) without the dense (R, Co) operand.
 *                               zprev / coef_prev (scale | shift): the previous layer's pre-activations and operand
 *                               coefficients for its ReLU mask (NULL: no mask).  Deterministic.  Query _supported (npts <= 256). */
int sn_pool_dgrad_sparse_supported(int B, int npts, int Ci, int Co);
int sn_pool_dgrad_sparse(int B, int npts, int Ci, int Co, const float *g, const float *pooled, const int *argsel, const float *W,
                         const float *zprev, const float *coef_prev, float *dyprev, sn_stream_t stream);

/*   sn_pointnet_narrow_forward  the extractor's narrow front 3 -> 64 -> 64 -> 64 -> 128 (ReLU between, no BatchNorm: conv1..conv4 of
 *                               registration/models/pcrnet.py:23-38) in one launch: a wave takes 32 rows through all four layers;
 *                               every layer's pre-activations bit-identical to the layer-by-layer launches.  z1..z3 (R,64): all
 *                               three (a backward will read them) or none; z4 (R,128).  wplanes: 3 * 16384 bf16 for the split
 *                               weights (planes_ready != 0: already holds the split of these weights).  zero_keys / zero_n: optional
 *                               rider -- that many 64-bit words are cleared (the key scratch of the sn_linear_forward_maxpool
 *                               that follows).  The entry runs any R >= 1 (rows at and beyond R are not written); _supported
 *                               demands R % 64 == 0 only because the layer-by-layer route is bit-identical there alone. */
int sn_pointnet_narrow_forward_supported(int R, int c1, int c2, int c3, int c4);
int sn_pointnet_narrow_forward(int R, const float *x, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                               const float *b3, const float *W4, const float *b4, void *wplanes, int planes_ready, float *z1, float *z2,
                               float *z3, float *z4, unsigned long long *zero_keys, int zero_n, sn_stream_t stream);

/*   sn_pointnet_narrow_backward the data gradient back through that front in one launch (frozen weights): dx (R,3) from dz4 (R,128) =
 *                               dL/d(conv4's pre-activations) and the saved z1..z3; wplanes_t: 3 * 16384 bf16 for the transposed split
 *                               weights (planes_ready != 0: already there). */
int sn_pointnet_narrow_backward_supported(int R, int c1, int c2, int c3, int c4);
int sn_pointnet_narrow_backward(int R, const float *dz4, const float *z1, const float *z2, const float *z3, const float *W1, const float *W2,
                                const float *W3, const float *W4, void *wplanes_t, int planes_ready, float *dx, sn_stream_t stream);

/* The per-cloud transforms of PointNet's classifier (classification/models/pointnet_cls.py:27-29, 55-59) and their gradients:
 *   sn_cloud_transform_forward   Y[b] (N, K) = X[b] (N, K) . T[b] (K, K), K = 3 (VALU) or 64 (fp32 MFMA); any N >= 0.
 *   sn_cloud_transform_backward  dX[b] = dY[b] . T[b]^T and dT[b] = X[b]^T . dY[b]; dX or dT may be NULL (not wanted; T / X may then
 *                                be NULL too).  dT is OVERWRITTEN; every sum has one fixed order (rows ascending within a quarter of the
 *                                cloud, the quarters added in ascending order; no atomics): two calls give the same bits.
 * True fp32 arithmetic: integer-valued operands whose sums stay below 2^24 give exact results.
 *   sn_orthogonality_loss_forward   loss[0] = sum over b of 1/2 |T[b] T[b]^T - I|^2 (pointnet_cls.py:124-130, tf.nn.l2_loss);
 *                                partial: B floats of scratch (the per-cloud terms, added in ascending b).
 *   sn_orthogonality_loss_backward  dT[b] = grad_loss[0] * 2 (T[b] T[b]^T - I) T[b]; grad_loss: device scalar.
 *   sn_bn_relu_forward / _backward  y (R, C) = relu(scale z + shift) with coef = {scale[C], shift[C], ...} -- the activation the GEMM
 *                                entries apply when the next layer loads its operand, materialised for a consumer that is no GEMM
 *                                entry (the feature transform) -- and dy = g . [y > 0] for the layer's backward (with_scale != 0: times scale,
 *                                the whole backward of a BatchNorm on FIXED statistics).  C % 4 == 0.
 * An empty batch (B == 0; no rows) is a no-op that succeeds whatever the pointers; sn_cloud_transform_backward with dX == NULL and
 * dT == NULL checks its arguments and launches nothing. */
int sn_cloud_transform_forward(int B, int N, int K, const float *X, const float *T, float *Y, sn_stream_t stream);
int sn_cloud_transform_backward(int B, int N, int K, const float *X, const float *T, const float *dY, float *dX, float *dT,
                                sn_stream_t stream);
int sn_orthogonality_loss_forward(int B, int K, const float *T, float *partial, float *loss, sn_stream_t stream);
int sn_orthogonality_loss_backward(int B, int K, const float *T, const float *grad_loss, float *dT, sn_stream_t stream);
int sn_bn_relu_forward(long long R, int C, const float *z, const float *coef, float *y, sn_stream_t stream);
int sn_bn_relu_backward(long long R, int C, const float *z, const float *coef, const float *g, int with_scale, float *dy,
                        sn_stream_t stream);

/* Linear layers on at most 32 rows (PCRNet's trunk, registration/models/pcrnet.py:56-77): out (R, N) = act((x . [gate > 0]) (R, K) .
 * W^T + bias), the weight stream cut into (32-column tile) x (K slice) workgroups, slices summed in order by the last workgroup to
 * arrive (deterministic); fp32 products as split-bf16 MFMAs.
 *   transposed == 0: W (N, K) -- forward;  != 0: W (K, N) -- data gradient dX = (dY . [y > 0]) W with gate = the layer's output y
 *   gate, bias: optional.  scratch: _scratch_bytes; counters: (N + 31) / 32 zeroed 32-bit words (left zeroed).
 * Errors, in this order: a NULL operand is SN_ERR_BAD_ARGUMENT; a size the kernel does not serve (R outside 1..128, K or N below 1:
 * sn_skinny_linear_supported) is SN_ERR_UNSUPPORTED whatever the splits; a ksplit / nsplit that does not fit the size is
 * SN_ERR_BAD_ARGUMENT. */
/* sn_pcrnet_head_forward + sn_qrot_forward as ONE launch (main.py:563-571: twist = model(p0, p1); est_transform.rotate(p0)):
 * y (B,7), v (B,N,3) -> twist (B,7), quat (B,4), qnorm (device scalar, may be NULL), out (B,N,3) = v rotated by quat; and the
 * backward of that pair as one launch: grad_out (B,N,3), grad_twist (B,7), grad_quat (B,4), grad_qnorm (device scalar), each
 * may be NULL -> grad_y (B,7) and, when grad_v != NULL, grad_v (B,N,3).  Bit-identical to the two launches each way. */
int sn_pcrnet_head_rot_forward(int B, int N, const float *y, const float *v, float *twist, float *quat, float *qnorm, float *out,
                               sn_stream_t stream);
int sn_pcrnet_head_rot_backward(int B, int N, const float *y, const float *quat, const float *v, const float *grad_out,
                                const float *grad_twist, const float *grad_quat, const float *grad_qnorm, float *grad_v, float *grad_y,
                                sn_stream_t stream);

/* The pose-error terms of the registration task (registration/src/qdataset.py:62-95 QuaternionTransform.compute_errors, as
 * registration/main.py:579-585 `--loss-type 0` and the evaluation of main.py:364-483 use them) and the per-cloud Chamfer mean of
 * main.py:540-555 / 573-577 for a batch.  (They replace a reference interface; they are declared here because the public header
 * is held at its entry count.)  est, gt: (B,7) rows [quaternion (w,x,y,z) | translation] -- sn_pcrnet_head_*'s twist, sn_batch_assemble's igt.
 *   rot_err[b]   = 2 acos(clamp(2 d^2 - 1, -1, 1)) radians, d = q1 . q2 of the quaternions AS GIVEN (qdataset.py:85).  DEVIATION:
 *                  the clamp -- the reference returns NaN wherever fp32 rounding lifts the argument above 1 (a fifth of all
 *                  self-comparisons of unit quaternions); results differ only there.  A NaN input still gives NaN.
 *   norm_err[b]  = sum_ij (R(q1) R(q2)^T - I)_ij^2, R the rotation matrix of the NORMALISED quaternion q / max(||q||, 1e-12)
 *                  (the arithmetic of kornia's quaternion_to_rotation_matrix, qdataset.py:74-90).
 *   trans_err[b] = (|dt_x| + |dt_y| + |dt_z|) / 3; its batch mean is qdataset.py:93's mean over B x 3.
 *   means (3)    = the batch means of the three, summed in ONE fixed order (thread t of 256 adds clouds t, t + 256, ...; halving
 *                  tree; / B): two runs are bit-identical.  Every output may be NULL; B = 0 is a no-op; any B >= 1 is served.
 * _backward: g_est (B,7), overwritten, of sum_b (g_means[1] / B + g_norm_err[b]) norm_err[b] + (g_means[2] / B + g_trans_err[b])
 *   trans_err[b]; g_means (device, 3 floats), g_norm_err, g_trans_err (B,) may each be NULL.  g_means[0] is NOT read: rot_err is a
 *   metric (the reference never backpropagates it; its derivative is unbounded at zero error).  The quaternion gradient goes
 *   through the normalisation, (g_n - n (n . g_n)) / max(||q||, 1e-12); the translation gradient is sign(dt) / 3 with
 *   sign(0) = 0.  DEVIATION: the reference's sqrt(dt^2) gives NaN at dt = 0.  No gradient flows to gt.
 * sn_chamfer_mean_per_cloud: out[b] = mean(dist1[b, :]) + mean(dist2[b, :]) from sn_chamfer_forward's products (dist1 (B,n1),
 *   dist2 (B,n2)); forward only, one workgroup per cloud, fixed summation order. */
int sn_pose_error_forward(int B, const float *est, const float *gt, float *rot_err, float *norm_err, float *trans_err, float *means,
                          sn_stream_t stream);
int sn_pose_error_backward(int B, const float *est, const float *gt, const float *g_means, const float *g_norm_err,
                           const float *g_trans_err, float *g_est, sn_stream_t stream);
int sn_chamfer_mean_per_cloud(int B, int n1, int n2, const float *dist1, const float *dist2, float *out, sn_stream_t stream);

/* The classification task's loss and prediction terms (classification/models/pointnet_cls.py:117-122 get_loss:
 * tf.nn.sparse_softmax_cross_entropy_with_logits + tf.reduce_mean; classification/evaluate_samplenet.py:237-262: np.argmax of the
 * logits, `correct`, the per-item loss), ONE launch per direction (csrc/cls_terms.hip).  (They replace a reference interface; they
 * are declared here because the public header is held at its entry count.)  logits (B,C) fp32, labels (B,) int32.
 *   ce[b]      = (logf(sum_c expf(x_c - m)) + m) - x_label, m = max_c x_c.
 *   pred[b]    = numpy's argmax: the FIRST maximum (ties to the lowest class); if a logit is NaN, the index of the first NaN.
 *   correct[b] = (pred[b] == labels[b]).
 *   means (2)  = the batch means of ce and of correct.
 * Mapping and summation order: one wave per row, lane l takes the classes l, l + 64, ... ascending (its partial sum starts at 0),
 * the 64 lanes combine by the xor butterfly (offsets 32, 16, .. 1); 16 waves per workgroup, wave w takes rows w, w + 16, ...; with
 * `means` the forward is ONE workgroup: a wave adds its rows' ce ascending from 0, thread 0 adds the 16 wave sums ascending from 0,
 * one division by (float)B; `correct` is counted in integers (exact) and divided once.  No float atomics: two runs are bit-identical.
 * Edge cases: a label outside [0, C) gives ce = NaN and correct = 0 and never reads outside logits; a NaN logit gives ce = NaN; a
 * label whose logit is -inf gives ce = +inf; a row of all -inf gives ce = NaN (pred 0); C = 1 gives ce = 0 exactly; B = 0 is a no-op.
 * Any B >= 1 and any C >= 1 are served (no refused range).  Every output may be NULL.
 * _backward (classification/train_samplenet.py:194-199 differentiates get_loss): g_logits (B,C), OVERWRITTEN,
 *   g_logits[b][c] = (g_means[0] / B + g_ce[b]) * (softmax(x_b)_c - [c == label_b]),
 * the softmax recomputed from the logits (nothing is saved by the forward).  g_means: DEVICE pointer to the upstream of `means`
 * (2 floats); only g_means[0] is read -- g_means[1] is NOT (accuracy is a metric), so a pointer to the one scalar serves as well;
 * g_means and g_ce (B,) may each be NULL (the part is left out).  A bad label gives a NaN row. */
int sn_classification_terms_forward(int B, int C, const float *logits, const int *labels, float *ce, int *pred, int *correct,
                                    float *means, sn_stream_t stream);
int sn_classification_terms_backward(int B, int C, const float *logits, const int *labels, const float *g_means, const float *g_ce,
                                     float *g_logits, sn_stream_t stream);
/* The per-point (segmentation) loss and prediction terms (csrc/seg_terms.hip): torch's F.cross_entropy(weight=, ignore_index=) with
 * reduction 'none' and 'mean', numpy's argmax, and the per-cloud, per-class counts accuracy and IoU are formed from.  The reference
 * has no segmentation code: the yardstick is the fp64 restatement of tests/seg_terms_ref.py.  logits (R,C) fp32 with the C
 * channels contiguous, R = clouds * rows_per_cloud; labels (R,) int32; class_weights (C,) or NULL (every weight 1).
 *   A point is VALID when 0 <= label < C; every other label is IGNORED whatever its value (-100, -1, 255, C, ..): ce = 0, pred is
 *   still written, the point enters no count and no mean and its gradient row is zero.  No label makes the kernels read outside
 *   logits or class_weights.
 *   ce[r]    = (logf(sum_c expf(x_c - m)) + m) - x_label, m = max_c x_c (unweighted).
 *   pred[r]  = numpy's argmax: the FIRST maximum; if a logit is NaN, the index of the first NaN.
 *   cloud_counts[b][c] (clouds,C,3) int32 = (points labelled c, valid points predicted c, valid points with pred == label == c),
 *     exact, OVERWRITTEN (the entry clears it on the stream; the caller clears nothing).
 *   means[0] = sum_valid w_label ce / sum_valid w_label (torch's reduction='mean' with weight=; NaN when no point is valid),
 *   means[1] = correct / valid from integer counts with one division (0 when no point is valid),  means[2] = sum_valid w_label.
 * On a valid row a NaN logit gives ce = NaN, a label whose logit is -inf gives +inf, a row of all -inf gives NaN (pred 0), C = 1
 * gives ce = 0 exactly (sn_classification_terms_forward's rules).  Every output may be NULL: only what is asked for is computed
 * and written.  `means` needs `workspace` (sn_segmentation_terms_workspace_bytes(R, C) bytes, -1 outside the range; no contents
 * are kept between calls): the batch sums are per-workgroup partials in one fixed order, summed in workgroup order by a closing
 * launch on the same stream -- no float atomics, no arrival counter: two runs are bit-identical.  The mapping and the order of
 * every fp32 operation are written at the head of csrc/seg_terms.hip.
 * _backward: g_logits (R,C), OVERWRITTEN,
 *   g_logits[r][c] = (g_means[0] * w_label / means[2] + g_ce[r]) * (softmax(x_r)_c - [c == label_r]),
 * the softmax recomputed (nothing is saved).  means: the forward's (only [2] is read, only with g_means); g_means: DEVICE pointer,
 * only [0] is read, so a pointer to the one scalar serves; g_means and g_ce (R,) may each be NULL (the part is left out).
 * Range: R >= 0, C >= 1, rows_per_cloud >= 1 dividing R, R * C < 2^31; R = 0 is a no-op; anything else is SN_ERR_BAD_ARGUMENT. */
long long sn_segmentation_terms_workspace_bytes(long long R, int C);
int sn_segmentation_terms_forward(long long R, int rows_per_cloud, int C, const float *logits, const int *labels,
                                  const float *class_weights, float *ce, int *pred, int *cloud_counts, float *means, void *workspace,
                                  sn_stream_t stream);
int sn_segmentation_terms_backward(long long R, int C, const float *logits, const int *labels, const float *class_weights,
                                   const float *means, const float *g_means, const float *g_ce, float *g_logits, sn_stream_t stream);
/* sn_nn_matching (samplenet_hip.h) with the two products its kernel computed and dropped: out_idx (B,k) int32 = the indices of the
 * selected points in selection order -- the first occurrences in idx order, then the farthest-point picks: fps_from_given_indices'
 * idx, reconstruction/src/samplenet_pointnet_ae.py:515-533 -- and n_unique (B,) int32 = the number of distinct values of idx[b, :]
 * (classification/evaluate_samplenet.py:227-228, samplenet_pointnet_ae.py:544).  out, out_idx, n_unique may each be NULL; with
 * complete_fps = 0 out_idx is a copy of idx and n_unique is still computed.  Same kernel body, limits (k <= 1024, N <= 8192) and
 * `out` bits as sn_nn_matching. */
int sn_nn_matching_indexed(int B, int N, int k, const float *xyz, int layout, const int *idx, int complete_fps, float *out,
                           int *out_idx, int *n_unique, sn_stream_t stream);
/* A whole cloud ranked by importance: the progressive sampler's inference (classification/infer_samplenet_progressive.py:207-212,
 * reconstruction/src/samplenet_progressive_pointnet_ae.py:490-524).
 * idx (B,k): nearest input point of every generated point, in generation order.  out_idx (B,k): the distinct values of
 * idx[b,:] in order of first occurrence, then farthest-point picks up to k -- fps_from_given_indices
 * (samplenet_progressive_pointnet_ae.py:567-585): float64 ((dx*dx + dy*dy) + dz*dz) never contracted, np.argmax's first
 * maximum (ties to the lowest point index).  out (B,k,3) = xyz[out_idx]; n_unique (B,) = number of distinct values.
 * out / out_idx / n_unique may each be NULL.  1 <= N <= 8192, 1 <= k <= 8192 (k may exceed N: once every distinct point
 * is taken all distances are 0 and index 0 comes again, as in numpy).  idx values are clamped into [0,N): no input makes
 * the kernel read outside xyz.  temp: sn_workspace_bytes("rank_points", B, N, k, 0) bytes, may be 0 / NULL (it is 0 today: a
 * cloud's state lives in its workgroup's LDS).  Where sn_nn_matching_indexed(complete_fps = 1) accepts the shape (k <= 1024) the three
 * outputs are bit-identical to its. */
int sn_rank_points(int B, int N, int k, const float *xyz, int layout, const int *idx, float *temp, float *out, int *out_idx,
                   int *n_unique, sn_stream_t stream);
/* measurement hook: points per lane (1, 2, 4, 8; 0 = chosen by N) of every later sn_rank_points call; returns the previous value,
 * -1 for a bad one.  A value that cannot hold N in 1024 lanes makes the call SN_ERR_UNSUPPORTED.  Outputs do not depend on it. */
int sn_rank_points_set_ppt(int ppt);

/* All-against-all shape retrieval inside one labelled set (the sampler's fourth application, README.md:13, on the classifier's
 * end_points["retrieval_vectors"], classification/models/pointnet_cls.py:111; the reference has no script for it, so this text is
 * the contract, restated in numpy by tests/retrieval_ref.py).  desc (S,n,C) fp32: S descriptor sets over the same n shapes (one per
 * sample size for a progressive sampler); labels (n) int32.  Every shape is a query against the other n - 1:
 *   d(i,j)  = sum_c (a_ic - a_jc)^2 in fp32, from the differences, nothing contracted, in one fixed order: the channels
 *             c = l, l + 64, l + 128, .. are added in ascending order for every l < 64, then the 64 partial sums meet as a balanced
 *             tree of adjacent pairs.  d(i,j) == d(j,i) bit for bit; equal descriptors give exactly +0;
 *   ranking = all j != i ascending by (d(i,j), j): ties to the lower index (numpy's stable argsort without the query);
 *   R = the others with the query's label, H(r) = those among the first r ranks;
 *   ap      = (sum over the relevant ranks r of H(r) / r) / R, accumulated in fp64, rounded once to fp32;
 *   prec[l-1], l = 1..L: H(r) / r (one fp64 division, rounded to fp32) at the smallest r with H(r) >= (l R + L - 1) / L (integer
 *             division: ceil(l R / L)): the precision at recall l / L;
 *   R == 0 (n == 1 included): ap and prec are NaN and n_relevant is 0.
 * Outputs (caller-owned, each may be NULL): ap (S,n), prec (S,n,L), n_relevant (n), order (S,n,n-1) int32, sorted_dist (S,n,n-1).
 * workspace: sn_workspace_bytes("retrieval_metrics", S, n, C, L) bytes, may be 0 / NULL (it is 0 today: a query's keys live in its
 * workgroup's LDS).  One launch, stream-ordered, capturable.  S == 0 or n == 0 is a no-op.  C < 1, L < 1, a negative size or a NULL
 * desc (NULL labels with ap / prec / n_relevant wanted) -> SN_ERR_BAD_ARGUMENT; n > 8192, L > 64 or S > 65535 -> SN_ERR_UNSUPPORTED. */
int sn_retrieval_metrics(int S, int n, int C, const float *desc, const int *labels, int L, float *ap, float *prec, int *n_relevant,
                         int *order, float *sorted_dist, void *workspace, sn_stream_t stream);

/* The progressive sampler's nested prefixes (classification/train_samplenet_progressive.py:157-234) as contiguous tensors in ONE launch:
 * src (B, M, C) of 4-byte elements -> dst[j] (B, sizes[j], C) = src[:, :sizes[j], :] (dst: HOST array of nprefix <= 16 device
 * pointers, NULL entries skipped); and the gradient of that in one launch: out (B, M, C) = sum over j of grads[j] zero-padded to
 * M points, ascending j (NULL entries contribute nothing). */
int sn_prefix_pack(int B, int M, int C, int nprefix, const int *sizes, const void *src, void *const *dst, sn_stream_t stream);
int sn_prefix_scatter_sum(int B, int M, int C, int nprefix, const int *sizes, const float *const *grads, float *out, sn_stream_t stream);
/* Clouds of different sizes as one batch of equal-size clouds for a max-pooling extractor without BatchNorm (PCRNet's PointNetFeatures,
 * registration/models/pcrnet.py:23-46): out[(j B + b), m, :] = src[j][b, m mod sizes[j], :] for m < len (src: HOST array of nclouds <= 16
 * device pointers, cloud j (B, sizes[j], C) fp32); the pooled features of every cloud are unchanged, bit for bit.  _backward: the
 * copies' gradients added onto their originals (grads[j] overwritten; NULL entries skipped). */
int sn_cyclic_pad_cat(int B, int len, int C, int nclouds, const int *sizes, const float *const *src, float *out, sn_stream_t stream);
int sn_cyclic_pad_cat_backward(int B, int len, int C, int nclouds, const int *sizes, const float *grad_out, float *const *grads,
                               sn_stream_t stream);
/* Several evaluations of the registration task term against ONE template in one batch (the progressive sampler's prefixes,
 * classification/train_samplenet_progressive.py:181-216 with registration/main.py:557-577 as the task): rows / clouds [e group, (e+1) group)
 * are evaluation e.
 *   sn_pcrnet_head_rot_*_grouped : sn_pcrnet_head_rot_* on R = E group rows, v = the `group` template clouds (row b rotates v[b % group]),
 *                                  qnorm / grad_qnorm one value per evaluation;
 *   sn_chamfer_mean_loss_*_grouped: mean(dist1) + mean(dist2) per evaluation on clouds padded to n1 points by sn_cyclic_pad_cat, nvalid[e]
 *                                  of them real (HOST array): the copies are not counted forward and get / give no gradient backward.
 * Every number equals the evaluation's own ungrouped call on the unpadded cloud, bit for bit. */
/* sn_chamfer_forward for such a padded batch: only the first q_valid[b / q_group] points (device array) of the smaller cloud of pair b
 * are scanned; the copies' dist / idx stay unwritten, everything else equals sn_chamfer_forward's products. */
int sn_chamfer_forward_valid(int B, int m, const float *xyz_small, int n, const float *xyz_large, const int *q_valid, int q_group,
                             float *dist_small, int *idx_small, float *dist_large, int *idx_large, void *workspace,
                             long long workspace_bytes, sn_stream_t stream);
int sn_pcrnet_head_rot_forward_grouped(int R, int N, int group, const float *y, const float *v, float *twist, float *quat, float *qnorm,
                                       float *out, sn_stream_t stream);
int sn_pcrnet_head_rot_backward_grouped(int R, int N, int group, const float *y, const float *quat, const float *v, const float *grad_out,
                                        const float *grad_twist, const float *grad_quat, const float *grad_qnorm, float *grad_y,
                                        sn_stream_t stream);
int sn_chamfer_mean_loss_forward_grouped(int R, int n1, int n2, int group, int nev, const int *nvalid, const float *dist1,
                                         const float *dist2, float *partial, float *loss, sn_stream_t stream);
int sn_chamfer_mean_loss_backward_grouped(int R, int n1, const float *xyz1, int n2, const float *xyz2, int group, int nev, const int *nvalid,
                                          const int *idx1, const int *idx2, const float *grad_loss, float *grad_xyz1, float *grad_xyz2,
                                          sn_stream_t stream);
/* sigma[0] = max(T^2, min_sigma) (registration/src/soft_projection.py:97-99: the projection loss of get_projection_loss) in one launch;
 * its backward is sn_sigma_grad with the upstream gradient as the single partial. */
int sn_sigma_forward(const float *temperature, float min_sigma, float *sigma, sn_stream_t stream);
/* The simplification losses (samplenet.py:171-181) of the first nterms nested prefixes of the simplified cloud, summed ascending
 * (classification/train_samplenet_progressive.py:204-216), behind one node: dq / iq (B,M) the per-query Chamfer products of the full
 * set, d2 / i2 (S,B,N) sn_prefix_point_minima's products; partial 3 * nterms * B floats, argmax1 nterms * B ints (forward -> backward).
 * Bit-identical to nterms sn_simplification_loss_forward / _backward calls on contiguous copies of the prefixes, added ascending. */
int sn_prefix_simplification_loss_forward(int B, int M, int N, int nterms, const int *sizes, const float *weights, const float *dq,
                                          const float *d2, float *partial, int *argmax1, float *loss, sn_stream_t stream);
int sn_prefix_simplification_loss_backward(int B, int M, int N, int nterms, const int *sizes, const float *weights, const float *samp_pc,
                                           const float *ref_pc, const int *iq, const int *i2, const int *argmax1, const float *grad_loss,
                                           float *grad_samp, sn_stream_t stream);
/* Test hook: the auction's level passes in segments (1, default: the other cloud cut into ranges swept by separate workgroups, partial
 * sums added in ascending order by the last to arrive -- thousands of short workgroups instead of 1.56 waves per SIMD at B = 50) or as
 * one range per workgroup (0); returns the previous setting. */
int sn_emd_set_segments(int on);
/* Test hook: sn_emd_loss_fast on the one-sweep form (1, default: every pair's match value evaluated once for cost, grad1 and grad2;
 * 64 x 64 tiles, tile partials added in ascending order) or on the two order-preserving sweeps of sn_emd_loss (0); returns the
 * previous setting.  Both meet the loss bar (cost 1e-5 of the oracle's). */
int sn_emd_set_sweep2d(int on);
int sn_skinny_linear_supported(int R, int K, int N);
long long sn_skinny_linear_scratch_bytes(int R, int K, int N);
int sn_skinny_linear(int R, int K, int N, const float *x, const float *gate, const float *W, int transposed, const float *bias, int relu,
                     float *out, float *scratch, unsigned *counters, sn_stream_t stream);
/* two-part form: input columns k >= ksplit from x2 (R, K - ksplit) with x (R, ksplit) (x2 NULL: x is (R, K)); output columns n >= nsplit
 * to out2 (R, N - nsplit) with out (R, nsplit) (nsplit 0: out is (R, N)); with nsplit > 0 either output may be NULL.  The trunk's
 * first layer reads the two clouds' feature vectors where they lie and its data gradient hands each cloud its own gradient. */
int sn_skinny_linear2(int R, int K, int N, const float *x, const float *x2, int ksplit, const float *gate, const float *W, int transposed,
                      const float *bias, int relu, float *out, float *out2, int nsplit, float *scratch, unsigned *counters,
                      sn_stream_t stream);
/* Weight gradient of such a layer (a trainable trunk: registration/models/pcrnet.py:62-82 under main.py --train-pcrnet):
 * dW (N, K) = (dy . [gate > 0])^T . [x | x2], db (N, optional) = its column sums; R <= 256 rows, fp32 MFMA, rows in ascending
 * order (deterministic).  gate (R, N, optional): the layer's own output (ReLU mask); x2 / ksplit as in sn_skinny_linear2. */
int sn_skinny_wgrad(int R, int K, int N, const float *x, const float *x2, int ksplit, const float *dy, const float *gate, float *dW,
                    float *db, sn_stream_t stream);
/* Test hook: 64-row blocks per workgroup of the xyz layer's statistics pass inside sn_conv_stack_forward_bn (0 = chosen per call:
 * 1 until the batch is large, then up to 8 -- one pair of atomics per channel and workgroup instead of one per block; the integer
 * totals are the same whatever the grouping).  Returns the previous setting. */
int sn_conv_stack_set_in3_blocks(int blocks);
/* sn_linear_forward for a layer of the FC head above 32 rows (rows = clouds, registration/src/samplenet.py:97-104 at a batch of
 * 64 .. ~1000): no statistics (the head takes two-pass statistics from Z, sn_bn_batch_stats_twopass).  While (R / 32) x (Co / 32)
 * workgroups fit the chip once, the R <= 32 kernel runs row block by row block -- every workgroup's operands in flight at once --
 * instead of the 64 x 64 tile kernel's dependent K chunks (512 x 256 -> 256: 8.8 us instead of 14.8); same products, K summed in
 * four partial chains.  Any other shape: sn_linear_forward's dispatch. */
int sn_linear_forward_rows(int R, int Ci, int Co, const float *ain, const float *coef_prev, const float *W, const float *bias, float *z,
                           sn_stream_t stream);

/* sn_emd_loss (samplenet_hip.h) with the reference op's own exponential -- __expf = v_exp_f32(x log2 e), tf_approxmatch_g.cu:52,97,151 --
 * in the auction and in the cost / gradient sweeps: the form a training loss wants (cost within 1e-5 of the oracle); not
 * bit-identical to the three-call composition, whose match matrix keeps the compensated exponential.  Same arguments / scratch. */
int sn_emd_loss_fast(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *grad1, float *grad2,
                     float *temp, sn_stream_t stream);

/* The Adam update of every parameter of an optimizer group in ONE launch (samplenet_amd/optim.py; registration/main.py:167
 * torch.optim.Adam, classification/train_samplenet.py:194 tf.train.AdamOptimizer).  Replaces no reference C interface.
 *   chunks   device table of nchunks 32-byte entries { float *param; const float *grad; long long moment_offset; int count; int pad }:
 *            workgroup c updates `count` (1 .. sn_adam_chunk_elems()) consecutive elements; a chunk never straddles two tensors;
 *            moment_offset (elements, a multiple of 4) addresses both moment buffers; grad == NULL: the chunk is skipped (parameter
 *            and moments untouched, as torch does for p.grad is None).  param / grad need only 4-byte alignment (16-byte accesses
 *            are used where the address allows them).
 *   exp_avg, exp_avg_sq   the flat fp32 moment buffers (16-byte aligned, distinct)
 *   state    sn_adam_state_bytes() = 64 bytes on the device, 8-byte aligned: { double lr; double beta1^t; double beta2^t; long long t;
 *            unsigned arrival counter (zero between launches); padding }.  The launch reads t, corrects the bias with t + 1 (fp64,
 *            once per workgroup) and its last workgroup to arrive writes t + 1 and the advanced powers: nothing the host passes
 *            changes from step to step, so a captured launch replays as it is.  lr is changed by a stream-ordered write of word 0.
 *   per element (fp32, g1 alone formed in fp64 and rounded once; operation order pinned in csrc/optimizer.hip):
 *            g1 = grad * grad_scale + weight_decay * p,
 *            m' = beta1 m + (1 - beta1) g1, v' = beta2 v + (1 - beta2) g1^2, bc_i = 1 - beta_i^(t+1),
 *            tf_epsilon == 0 (torch): p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
 *            tf_epsilon != 0 (TensorFlow): p' = p - (lr sqrt(bc2) / bc1) m' / (sqrt(v') + eps)
 *   grad_scale folds the 1 / world of a SUM all-reduce into the update (1 when the reducer averages).
 * nchunks == 0 is a no-op that succeeds (the step count does not advance). */
int sn_adam_chunk_elems(void);
long long sn_adam_state_bytes(void);
int sn_adam_update(int nchunks, const void *chunks, float *exp_avg, float *exp_avg_sq, void *state, double beta1, double beta2,
                   double eps, double weight_decay, double grad_scale, int tf_epsilon, sn_stream_t stream);

/* The two other optimizers of registration/main.py:166-171 as ONE launch each: torch.optim.SGD (momentum, dampening, Nesterov; also
 * classification/train_classifier.py:133 tf.train.MomentumOptimizer) and torch.optim.RMSprop (not centered).  Replace no reference C
 * interface.  Chunk table, NULL-gradient rule, alignment rules and the 64-byte state block are sn_adam_update's: word 0 lr, word 3 t,
 * word 4 the arrival counter (zero between launches); words 1 and 2 are neither read nor written.  The last workgroup to arrive writes
 * t + 1 and clears the counter, so a captured launch replays as it is.
 *   momentum_buf   flat fp32 buffer addressed by the table's moment_offset, 16-byte aligned; NULL exactly when momentum == 0 (then
 *                  no buffer is read or written)
 *   square_avg     (RMSprop) flat fp32 buffer, 16-byte aligned, distinct from momentum_buf
 *   per element (fp32, g1 alone formed in fp64 and rounded once; operation order pinned in csrc/optimizer.hip):
 *            g1 = grad * grad_scale + weight_decay * p
 *     SGD:   momentum != 0: b' = g1 when t == 0 (torch's first step: the buffer is a copy of the gradient, dampening ignored), else
 *            b' = momentum b + (1 - dampening) g1;  d = nesterov ? g1 + momentum b' : b';  momentum == 0: d = g1;  p' = p - lr d.
 *            t is ONE count per launch, i.e. per parameter group: it differs from torch's per-parameter "buffer is None" only for a
 *            parameter whose gradient was NULL in the group's first step, and only when dampening != 0.
 *     RMSprop: s' = alpha s + (1 - alpha) g1^2;  q = g1 / (sqrt(s') + eps);  momentum == 0: p' = p - lr q;
 *            else b' = momentum b + q, p' = p - lr b'.
 * Checked before any launch: nchunks >= 0; momentum, dampening, eps, weight_decay >= 0; 0 <= alpha < 1; nesterov needs momentum > 0
 * and dampening == 0; non-null, aligned table / block / buffers.  nchunks == 0 is a no-op that succeeds (the block is not touched). */
int sn_sgd_update(int nchunks, const void *chunks, float *momentum_buf, void *state, double momentum, double dampening,
                  double weight_decay, double grad_scale, int nesterov, sn_stream_t stream);
int sn_rmsprop_update(int nchunks, const void *chunks, float *square_avg, float *momentum_buf, void *state, double alpha, double eps,
                      double weight_decay, double momentum, double grad_scale, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Training batches assembled ON THE DEVICE from an HBM-resident dataset in ONE launch (samplenet_amd/device_data.py; the reference's
 * data side: registration/data/modelnet_loader_torch.py:114-125 ModelNetCls.__getitem__, src/pctransforms.py, src/qdataset.py:133-179
 * QuaternionFixedDataset).  One workgroup of 256 threads per output cloud; no workgroup waits on another.  All arithmetic is fp32,
 * one IEEE operation per operation written below (the unit is built with -ffp-contract=off), no atomics on floats.
 *
 * WHICH ITEM A SLOT HOLDS.  Lset = L * repeat (1 <= Lset < 2^31).  Slot b of the launch sits at the global position
 *     g = position + rank * B + b,      epoch = g / Lset,      item = perm(seed, epoch, g mod Lset),      cloud = item mod L
 * (order == SN_BATCH_ORDER_SEQUENTIAL: item = g mod Lset).  Batches run across epoch ends: there is no "last partial batch" -- the
 * one difference from a DataLoader.  perm is a keyed bijection of [0, Lset): a balanced Feistel network on k bits, k the smallest
 * EVEN number >= 2 with 2^k >= Lset, h = k / 2, mask = 2^h - 1:
 *     (l, r) = (x >> h, x & mask);   four times, i = 0..3:  (l, r) <- (r, l ^ (F(r + rk[i]) & mask));   x' = (l << h) | r
 *     F(v) (32-bit, wrapping):  v ^= v >> 16;  v *= 0x7FEB352D;  v ^= v >> 15;  v *= 0x846CA68B;  v ^= v >> 16
 *     rk[0..3] = the four words of draw(index 0, stream 6, item 0, epoch)
 * applied again while x' >= Lset (cycle walking).  A walk that starts below Lset returns below Lset after at most
 * 2^k - Lset + 1 applications (it can pass through each of the 2^k - Lset values outside the range once), and 2^k < 4 Lset.
 *
 * RANDOM DRAWS.  draw(index, stream, item, epoch) = Philox4x32-10 with counter words (c0, c1, c2, c3) = (index, stream, item,
 * epoch mod 2^32), key (k0, k1) = (seed mod 2^32, seed >> 32), multipliers M0 = 0xD2511F53 (on c0), M1 = 0xCD9E8D57 (on c2), key
 * increments 0x9E3779B9 (k0) and 0xBB67AE85 (k1) between rounds; a round is
 *     (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)).
 * The four output words are x0..x3.  A cloud's content is a function of (seed, epoch, item, dataset, recipe) alone -- not of B, of
 * the slot, of the rank or of the step.
 *     uniform(x)      u = (x >> 8) * 2^-24                                   in [0, 1), exact in fp32
 *     gauss(xa, xb)   u1 = ((xa >> 8) + 1) * 2^-24, u2 = (xb >> 8) * 2^-24,  rad = sqrtf(-2 * logf(u1)),
 *                     (s, c) = sincosf(6.28318530717958647692f * u2),        -> (rad * c, rad * s)
 *     gauss3(x0..x3)  (g0, g1) = gauss(x0, x1), (g2, g3) = gauss(x2, x3); g0, g1, g2 are used, g3 is dropped
 * Streams, j = the point's position in the OUTPUT cloud:
 *     0  sort key        draw(j, 0, ..): x0 = the key of input point j (j < N)
 *     1  jitter          draw(j, 1, ..): gauss3 -> the x, y, z offsets of output point j
 *     2  dropout         draw(j, 2, ..): uniform(x0) = u_j
 *     3  pair noise      draw(j, 3, ..): gauss3 -> the x, y, z noise of point j of p1
 *     4  cloud scalars   draw(0, 4, ..): uniform(x0) scale, uniform(x1) rotation angle, uniform(x2) translation, uniform(x3) dropout ratio
 *     5  perturbation    draw(0, 5, ..): gauss3 -> the angles about x, y, z
 *     6  item order      draw(0, 6, 0, epoch): the Feistel round keys above
 *
 * PIPELINE, in this order; every stage is switched by its recipe field.  v = (x, y, z) of output point j.
 *  1 point order   shuffle_points: the N composites (key_i << 32) | i, i < N, sorted ascending (bitonic sort in LDS, padded to a power
 *                  of two with all-ones sentinels; composites are distinct: no tie rule); output point j is input point
 *                  (composite_j mod 2^32) of the cloud's first N points.  Off: output point j is input point j.  N <= 2048 with the
 *                  shuffle, any N <= P without; else SN_ERR_UNSUPPORTED.
 *  2 unit_cube     per axis lo_c = min, hi_c = max over the N points, e_c = hi_c - lo_c, s = max(e_x, e_y, e_z); v_c = v_c / s;
 *                  m_c = (sum over the points of v_c) / (float)N; v_c = v_c - m_c  (pctransforms.py:162-166).  The sums have one
 *                  fixed order: thread t adds positions t, t + 256, .. ascending, the 64 lanes of a wave combine by the xor tree
 *                  (offsets 32, 16, .. 1), the four wave sums are added in ascending order.  s == 0 divides by zero like the reference.
 *  3 scale         f = scale_lo + u * (scale_hi - scale_lo);  v_c = v_c * f
 *  4 rotate        (s, c) = sincosf(u * 6.28318530717958647692f), a = the unit axis (normalised on the host in fp64, rounded to fp32),
 *                  t = 1 - c,  R[i][j] = (c * [i == j] + s * K[i][j]) + (t * a_i) * a_j  with K = [[0,-az,ay],[az,0,-ax],[-ay,ax,0]];
 *                  v_i = (R[i][0] x + R[i][1] y) + R[i][2] z   (pctransforms.py:12-42, 59-65)
 *  5 perturb       angle_k = min(max(perturb_sigma * g_k, -perturb_clip), perturb_clip), k = x, y, z; Rz Ry Rx applied as three plane
 *                  rotations, about x first: (y, z) <- (c y - s z, s y + c z); about y: (x, z) <- (c x + s z, c z - s x); about z:
 *                  (x, y) <- (c x - s y, s x + c y)   (pctransforms.py:75-96)
 *  6 translate     d = u * (translate_range + translate_range) - translate_range;  v_c = v_c + d  (ONE scalar on all three axes:
 *                  what pctransforms.py:120-127 does)
 *  7 jitter        v_c = v_c + min(max(jitter_std * g_c, -jitter_clip), jitter_clip)
 *  8 dropout       ratio = u * dropout_max;  every point with u_j <= ratio becomes output point 0 (as it stands after stage 7)
 *  9 pair          p1_j = qrot(pair_quat[item], p0_j) with sn_qrot_forward's expression; pair_noise: + pair_noise_std * g_c
 * p0 is the cloud after stage 8.
 *
 * STATE.  `state`: sn_batch_state_bytes() = 64 bytes on the device, 8-byte aligned: { long long position; unsigned arrivals (zero
 * between launches); padding }.  position < 0: every workgroup reads the block's position first, then counts itself as arrived; the
 * LAST to arrive clears the count and adds B * world to the position -- nothing spins, and a replayed graph yields successive
 * batches with no host write.  position >= 0: that position is used and the block is neither read nor written (may be NULL).
 *
 * Arguments: points (L, P, 3) fp32 and labels (L) int64 (needed when out_labels != NULL): the resident set; recipe: HOST memory,
 * read during the call; pair_quat (Lset, 4) as (w, x, y, z), needed for p1 / igt.  Outputs (caller-owned): p0 (B, N, 3) or
 * (B, 3, N) by `layout`; optional p1 (same shape), out_labels (B) int64, igt (B, 7) = the item's quaternion and three zeros,
 * items (B) int32.  Checked on the host before any device work: negative B / N / P / L / repeat < 1, N > P, rank outside [0, world),
 * scale_lo > scale_hi, a negative clip / std / range, dropout_max outside [0, 1), a zero rotation axis, a bad layout or order
 * selector, a NULL required pointer -> SN_ERR_BAD_ARGUMENT.  B == 0 is a no-op that succeeds. */
#define SN_BATCH_ORDER_SHUFFLED 0
#define SN_BATCH_ORDER_SEQUENTIAL 1
typedef struct sn_batch_recipe {
    int order;          /* SN_BATCH_ORDER_* */
    int shuffle_points; /* stage 1 */
    int unit_cube;      /* stage 2 */
    int scale;          /* stage 3 */
    float scale_lo, scale_hi;
    int rotate;         /* stage 4 */
    float axis[3];
    int perturb;        /* stage 5 */
    float perturb_sigma, perturb_clip;
    int translate;      /* stage 6 */
    float translate_range;
    int jitter;         /* stage 7 */
    float jitter_std, jitter_clip;
    int dropout;        /* stage 8 */
    float dropout_max;
    int pair_noise;     /* stage 9: noise on p1 */
    float pair_noise_std;
} sn_batch_recipe;
long long sn_batch_state_bytes(void);
int sn_batch_assemble(int B, int N, int P, int L, int repeat, const float *points, const long long *labels,
                      const sn_batch_recipe *recipe, unsigned long long seed, int rank, int world, long long position, void *state,
                      const float *pair_quat, int layout, float *p0, float *p1, long long *out_labels, float *igt, int *items,
                      sn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Ball-query neighbourhoods and the fused query-and-group of a PointNet++ set abstraction (csrc/ball_query.hip; restated in numpy
 * float32 by tests/ball_ref.py).  For query j and dataset point k, all fp32, every operation rounded once, nothing contracted:
 *     dx = x_query - x_dataset, dy, dz likewise;   d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
 *     SN_BALL_RULE_SQRT     pass = max(sqrtf(d2), 1e-20f) < radius, sqrtf correctly rounded: the reference's rule
 *                           (classification/grouping/tf_grouping_g.cu:24-25, test/query_ball_point.cpp:32-33);
 *     SN_BALL_RULE_SQUARED  pass = d2 < fl(radius * radius): the rule of Pointnet2_PyTorch's ball_query AS RECALLED -- its source
 *                           is not at hand, so this rule is UNPINNED (like knn_cuda's tie order).
 * The rules differ only for pairs at the boundary.  Any float radius is legal: a NaN or a radius <= 0 gives all-empty rows under
 * both rules, and under the reference's rule so does every radius <= 1e-20f.  A NaN distance never passes.
 * Row j of idx holds the FIRST nsample passing dataset indices in ascending order; with 0 < cnt < nsample hits, slots cnt ..
 * nsample-1 repeat the first hit; pts_cnt[j] = min(hits, nsample).  DEVIATION: a row with no hit is written as zeros with
 * pts_cnt[j] = 0 -- the reference leaves such a row unwritten (whatever the buffer held).  nsample has no upper bound.
 * One launch, no workspace, no atomics, deterministic, capturable.  Checked on the host before any device work: a negative size,
 * nsample < 1, an unknown rule / layout / use_xyz, a NULL required pointer, n == 0 with b * m > 0 -> SN_ERR_BAD_ARGUMENT; b == 0
 * or m == 0 is a no-op that succeeds; a launch of more than 2^31 - 1 workgroups (b * m beyond 3e10) -> SN_ERR_UNSUPPORTED. */
#define SN_BALL_RULE_SQRT 0
#define SN_BALL_RULE_SQUARED 1
/* query_ball_point_gpu + queryBallPointLauncher (tf_grouping_g.cu:3-36, 125-128; op shell tf_grouping.cpp:66-100; Python
 * tf_grouping.py:13-28).  xyz1: the dataset, (b,n,3) [SN_LAYOUT_BNC] or (b,3,n) [SN_LAYOUT_BCN] by layout1; xyz2: the queries,
 * (b,m,3) or (b,3,m) by layout2; idx (b,m,nsample) int32; pts_cnt (b,m) int32, may be NULL. */
int sn_ball_query(int b, int n, int m, float radius, int nsample, int rule, const float *xyz1, int layout1, const float *xyz2,
                  int layout2, int *idx, int *pts_cnt, sn_stream_t stream);
/* QueryAndGroup in ONE launch (replaces query_ball_point_gpu + group_point_gpu, tf_grouping_g.cu:3-36, 40-57, and the centre
 * subtraction of the set-abstraction layer around them; Pointnet2_PyTorch's QueryAndGroup.forward).  xyz (b,n,3), new_xyz (b,m,3),
 * features (b,c,n) or NULL with c == 0; out (b, 3 use_xyz + c, m, nsample) channel-major: with use_xyz, channels 0..2 are
 * xyz[idx] - new_xyz[j] (one exact fp32 subtraction each), the remaining c channels are features[:, :, idx].  idx / pts_cnt are
 * written exactly as by sn_ball_query (pts_cnt may be NULL); an empty ball therefore groups point 0.  c == 0 without use_xyz ->
 * SN_ERR_BAD_ARGUMENT.  Bit-identical to sn_ball_query + sn_grouping_operation + the subtraction. */
int sn_ball_group_forward(int b, int n, int m, int c, float radius, int nsample, int rule, int use_xyz, const float *xyz,
                          const float *new_xyz, const float *features, int *idx, int *pts_cnt, float *out, sn_stream_t stream);
/* Its gradient (replaces group_point_grad_gpu, tf_grouping_g.cu:61-78, for both gathered tensors, plus the centre's term).
 * grad_out (b, 3 use_xyz + c, m, nsample) is read where it lies (no slice is copied).  Each output may be NULL; one that is NULL is
 * not touched:
 *   grad_features (b,c,n), grad_xyz (b,n,3): OVERWRITTEN (the caller zeroes nothing), summed with float atomics, so the last bits
 *       depend on arrival order (the contract of sn_grouping_operation_grad's atomic route).  n <= 16384: a workgroup accumulates up
 *       to 16 channels of one cloud as dense rows in LDS (LDS atomics) and stores them; beyond: zero-filled inside, then global
 *       float atomics.  An index outside [0,n) adds to nothing;
 *   grad_new_xyz (b,m,3): grad_new_xyz[b,j,:] = -(sum over s of grad_out[b,0:3,j,s]) in ONE order: lane l of a wave adds slots
 *       s = l, l + 64, .. ascending, the 64 lane sums meet by the xor tree (offsets 32, 16, .. 1), one negation: bit-reproducible.
 * Without use_xyz the two point gradients are zeros.  idx / grad_out may be NULL when m == 0 (the zero-fill still happens). */
int sn_ball_group_backward(int b, int n, int m, int c, int nsample, int use_xyz, const int *idx, const float *grad_out,
                           float *grad_features, float *grad_xyz, float *grad_new_xyz, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * The three nearest known points of every unknown point: the query of a PointNet++ feature-propagation (up-sampling) layer
 * (csrc/feature_propagate.hip; restated in numpy float32 by tests/interp_ref.py).  Stands in for Pointnet2_PyTorch's three_nn.
 * That module's source is NOT at hand: the tie order and the filling with m < 3 are AS RECALLED and UNPINNED (like
 * SN_BALL_RULE_SQUARED above).
 * unknown (b,n,3): the points that receive features; known (b,m,3): the points that carry them.  All fp32, every operation
 * rounded once, nothing contracted.  For unknown j and known k:  dx = u.x - k.x, dy, dz likewise;
 * d2 = ((dx*dx) + (dy*dy)) + (dz*dz).  The three neighbours are the three smallest by (d2, k): strict < in an ascending walk, ties
 * to the lower index (sn_knn's rule).  A NaN (or +inf) d2 is never selected.  With fewer than three selectable points the missing
 * slots hold index 0 and d2 = +inf (an inverse-distance weight of 0).  Indices always lie in [0, m).
 * idx (b,n,3) int32, required; dist2 (b,n,3) the squared distances and dist (b,n,3) = sqrtf(dist2), correctly rounded, what
 * three_nn returns; either may be NULL.  A lane owns an unknown point, the known cloud is staged in LDS in chunks of 1024 points.
 * One launch, no workspace, no atomics, deterministic, capturable.  Checked on the host before any device work: a negative size,
 * m == 0 with b * n > 0, a NULL required pointer -> SN_ERR_BAD_ARGUMENT; b == 0 or n == 0 is a no-op that succeeds; more than
 * 2^31 - 1 workgroups -> SN_ERR_UNSUPPORTED.  n and m are unbounded. */
int sn_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, float *dist, int *idx, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * The gradient of a weighted gather towards its features by INVERTED INDEX (csrc/feature_propagate.hip; restated in numpy by
 * tests/gather_inv_ref.py): the deterministic sum of sn_weighted_gather_backward_ordered (samplenet_hip.h) without its scratch
 * buffer, for the regime of a feature-propagation layer (thousands of queries, hundreds of channels, a small destination cloud).
 * A cloud has n destination rows and ne = m * k entries, entry e = j*k + t being neighbour t of query j; idx[b,e] names the
 * entry's row.  An entry whose index lies outside [0, n) belongs to no row (as in sn_weighted_gather_backward_ordered).
 *
 * sn_gather_invert: idx (b,ne) int32 -> start (b,n+1) int32, order (b,ne) int32, both fully determined and fully overwritten:
 *   start[b,r] = the number of valid entries of cloud b with idx < r (start[b,0] = 0, start[b,n] = the number of valid entries);
 *   order[b, 0 .. start[b,n]) = the valid entry numbers sorted by (idx[e], e) -- a stable sort: row r's list is
 *   order[b, start[b,r] .. start[b,r+1]) and ascends in e; every slot from start[b,n] on holds -1.
 *   One launch, one workgroup of 16 waves per cloud: the counts by integer LDS atomics, 4096 rows at a time (n is not bounded by
 *   LDS), a scan, then a placement that walks the entries in ascending order: a wave owns R consecutive rows, R the smallest power
 *   of two <= 64 with 16 R >= n (so a cloud of up to 1024 rows is shared by all 16 waves in one pass), a lane one row and its
 *   cursor; the wave reads all ne indices once per group of R rows it owns and places, one by one, those that name its rows.  No
 *   workspace but the outputs, no memset, no synchronisation: deterministic, capturable.  idx must not change while the call runs.
 *   BOUND: sn_gather_invert_supported(n, ne) = 1 iff ceil(n / 64) * ne <= 2^26 (and n < 2^31 - 1).  The product is the bound's
 *   DEFINITION, not an exact read count (a wave reads ceil(ceil(n / R) / 16) * ne indices: ne up to n = 1024, about n / 1024 * ne
 *   beyond); it is the bound up to which sn_weighted_gather_backward_ordered's own sum is ordered, so the inverted route exists
 *   exactly where the two can be held bit for bit.  Beyond it the call returns SN_ERR_UNSUPPORTED and leaves the outputs untouched.
 *   (n = 16385 admits ne up to 261 123.)
 *   Checked on the host before any device work, in this order: a negative size -> SN_ERR_BAD_ARGUMENT; b == 0 or n == 0 is a
 *   no-op that succeeds; start NULL, or idx / order NULL with ne > 0 -> SN_ERR_BAD_ARGUMENT; the bound.
 *
 * THE LIST WALK, shared by the three gradients that consume start / order (sn_weighted_gather_backward_inverted here,
 *   sn_group_rows_backward and sn_interp_rows_backward below; csrc/inverse_walk.h holds the row-layout kernels' one body): an output
 *   element of destination row r is the fp32 sum over i in [start[b,r], start[b,r+1]), in that order and starting from +0, of one
 *   term per entry e = order[b,i]; a weighted term is fl(gradient * weights[b,e]), the product rounded, then added; every add is
 *   rounded, nothing is contracted.  A row with no entry receives +0.  On lists of sn_gather_invert the order is ascending entry
 *   number, which is the order of sn_weighted_gather_backward_ordered.  CLAMP AND SKIP: a start outside [0, ne] is clamped and an
 *   entry number outside [0, ne) skipped, so foreign buffers cannot make a walk read elsewhere.  KNOWN LIMIT: lists are not split
 *   (that would change the order), so a launch takes as long as its longest list.  No atomics, no scratch, capturable.
 *
 * sn_weighted_gather_backward_inverted: weights (b,m,k), grad_out (b,c,m), start / order as above -> grad_X (b,c,n), OVERWRITTEN:
 *   grad_X[b,ch,r] = the list walk's sum of fl(grad_out[b,ch,e/k] * weights[b,e]) (ne = m*k).  This is the arithmetic of
 *   sn_weighted_gather_backward_ordered: with start / order from sn_gather_invert on the same idx the two grad_X are BIT-IDENTICAL.
 *   idx itself is not an argument: the lists carry all it says.  The gradient towards the weights stays with
 *   sn_weighted_gather_backward (grad_X = NULL).
 *   One launch: a thread owns one row and 8 channels of it (entry number, query and weight loaded once per entry for the 8
 *   accumulators).
 *   Checked on the host: a negative size, k < 1, m * k beyond 2^31 - 1 -> SN_ERR_BAD_ARGUMENT; b == 0, c == 0 or n == 0 is a no-op
 *   that succeeds; start or grad_X NULL, or weights / grad_out / order NULL with m > 0 -> SN_ERR_BAD_ARGUMENT; more than 2^31 - 1
 *   workgroups (b * ceil(n * ceil(c / 8) / 256)) -> SN_ERR_UNSUPPORTED. */
int sn_gather_invert_supported(int n, int ne);
int sn_gather_invert(int b, int n, int ne, const int *idx, int *start, int *order, sn_stream_t stream);
int sn_weighted_gather_backward_inverted(int b, int c, int n, int m, int k, const float *weights, const float *grad_out,
                                         const int *start, const int *order, float *grad_X, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * A PointNet++ set-abstraction level around the GEMM entries above (csrc/set_abstraction.hip; restated in numpy by
 * tests/group_rows_ref.py): the grouped points in the ROW layout the GEMMs read, the gradient of that gather by inverted index, and
 * a max-pool pair for many small groups.  Together the first two replace query_ball_point_gpu + group_point_gpu +
 * group_point_grad_gpu (tf_grouping_g.cu:3-36, 40-57, 61-78) and the centre subtraction, on that layout.
 *
 * sn_ball_group_rows_forward: xyz (b,n,3), new_xyz (b,m,3), features (b,n,c) ROW-major (channels contiguous) or NULL with c == 0;
 *   rows (b, m, nsample, 3 use_xyz + c): with use_xyz, columns 0..2 of row (j,s) are xyz[idx[j,s]] - new_xyz[j] (one fp32 subtraction
 *   each), then the c feature columns of point idx[j,s].  idx / pts_cnt are written exactly as by sn_ball_query (pts_cnt may be
 *   NULL; an empty ball groups point 0).  Bit-identical to sn_ball_group_forward's output permuted.  One launch, no workspace, no
 *   atomics, capturable.  Checked on the host before any device work, as sn_ball_group_forward: a negative size, nsample < 1, an
 *   unknown rule / use_xyz, c == 0 without use_xyz -> SN_ERR_BAD_ARGUMENT; b == 0 or m == 0 is a no-op that succeeds; n == 0 with
 *   b * m > 0, a NULL required pointer -> SN_ERR_BAD_ARGUMENT; more than 2^31 - 1 workgroups -> SN_ERR_UNSUPPORTED.
 *
 * sn_group_rows_backward: grad_rows (b, m*nsample, 3 use_xyz + c); start (b,n+1) / order (b, m*nsample) from
 *   sn_gather_invert(b, n, m*nsample, idx, ..).  idx itself is not read (the lists carry all it says) and may be NULL.  Each output
 *   may be NULL; one that is NULL is not touched, the others are OVERWRITTEN:
 *   grad_features (b,n,c), grad_xyz (b,n,3): element [b,r,ch] = THE LIST WALK's sum (above; ne = m*nsample) of the unweighted
 *       terms grad_rows[b, e, col].  No atomics, one order: the bits repeat.  Its known limit bites here: point 0 collects every
 *       empty ball;
 *   grad_new_xyz (b,m,3): -(sum over s of grad_rows[b, j*nsample + s, 0:3]) in sn_ball_group_backward's order (lane l adds slots l,
 *       l + 64, .. ascending, the xor tree 32 .. 1, one negation): bit-identical to that entry on the permuted gradient.
 *   Without use_xyz the two point gradients are zeros.  Up to two launches, no workspace, capturable.  Checked on the host: a
 *   negative size, nsample < 1, an unknown use_xyz, c == 0 without use_xyz, m * nsample beyond 2^31 - 1 -> SN_ERR_BAD_ARGUMENT;
 *   b == 0 is a no-op that succeeds; grad_rows NULL with m > 0, or start (order with m > 0) NULL when grad_features / grad_xyz is
 *   asked for -> SN_ERR_BAD_ARGUMENT; more than 2^31 - 1 workgroups -> SN_ERR_UNSUPPORTED.
 *
 * sn_group_pool_forward: sn_pool_forward(B = G, N = S, ..) bit for bit (per channel max or min by the sign of the scale, the FIRST
 *   row wins a tie, pooled = relu(scale * z + shift) as one fmaf), for many small groups: a wave per (group, 64 channels).
 * sn_group_pool_backward: gsel = g * [pooled > 0], bit for bit sn_pool_backward's, and -- unless stats is NULL -- the
 *   BatchNorm-backward partial sums stats [nblk][2][C], nblk = sn_group_pool_stats_blocks(G): block k holds (sum gsel, sum
 *   fl(gsel * zsel)) over groups 64 k .. 64 k + 63, slice q of four adding groups q, q + 4, .. ascending and the four slice sums added
 *   in slice order: the layout sn_bn_backward_coef(nblk, C, R, stats, ..) reduces.  On fixed statistics the caller forms
 *   kcoef = (scale, 0, 0) itself.  Both: one launch, G, S, C >= 1 and non-NULL pointers or SN_ERR_BAD_ARGUMENT. */
int sn_ball_group_rows_forward(int b, int n, int m, int c, float radius, int nsample, int rule, int use_xyz, const float *xyz,
                               const float *new_xyz, const float *features, int *idx, int *pts_cnt, float *rows, sn_stream_t stream);
int sn_group_rows_backward(int b, int n, int m, int c, int nsample, int use_xyz, const int *idx, const int *start, const int *order,
                           const float *grad_rows, float *grad_features, float *grad_xyz, float *grad_new_xyz, sn_stream_t stream);
int sn_group_pool_forward(int G, int S, int C, const float *z, const float *coef, float *pooled, int *argsel, float *zsel,
                          sn_stream_t stream);
int sn_group_pool_stats_blocks(int G);
int sn_group_pool_backward(int G, int C, const float *g, const float *pooled, const float *zsel, float *gsel, float *stats,
                           sn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * A PointNet++ feature-propagation level around the GEMM entries above (csrc/feature_rows.hip; restated in numpy by
 * tests/fp_rows_ref.py): the level's input in the ROW layout the GEMMs read, the gradient of its interpolated part by inverted
 * index, and the backward of the walk's top activation with the top BatchNorm's partial sums.  The query stays sn_three_nn.
 *
 * sn_interp_rows_forward: known_rows (b,m,c2) ROW-major (channels contiguous); skip_rows (b,n,c1) row-major, or NULL with c1 == 0;
 *   idx (b,n,3) int32 and dist2 (b,n,3) as sn_three_nn wrote them; rule 0: PointnetFPModule's 1 / (dist + 1e-8), 1: the TF module's
 *   1 / max(dist^2, 1e-10) (tests/interp_ref.py: SQRT_EPS, SQUARED_CLAMP).  All fp32, every operation rounded once, nothing contracted:
 *     r_t = 1 / (sqrtf(d2_t) + 1e-8f)  or  1 / fmaxf(d2_t, 1e-10f);  norm = (r_0 + r_1) + r_2;  w_t = r_t / norm
 *   (sqrtf and the divisions correctly rounded; an unfilled slot's d2 = +inf gives weight 0).
 *   weights (b,n,3), required (the backward reads it), and rows (b, n, c2 + c1) are fully OVERWRITTEN:
 *     rows[b,j,ch] = ((w_0 * f[i_0,ch]) + (w_1 * f[i_1,ch])) + (w_2 * f[i_2,ch]) for ch < c2, f = known_rows[b], i_t = idx[b,j,t]:
 *       the bits of sn_weighted_gather_forward at k = 3 given these weights;
 *     rows[b,j,c2 + ch] = skip_rows[b,j,ch], copied bit for bit.
 *   An index outside [0, m) is CLAMPED to the nearest of 0 and m - 1: nothing outside the cloud is read (sn_three_nn writes none).
 *   One launch, no workspace, no atomics, capturable.  A group of LG lanes owns an output row, LG the power of two covering
 *   c2 + c1, 64 at most, and walks the row's columns LG at a time; the row's weights are formed once, in front of that walk.
 *   Checked on the host before any device work, in this order: a negative size, an unknown rule, c2 + c1 == 0 ->
 *   SN_ERR_BAD_ARGUMENT; b == 0 or n == 0 is a no-op that succeeds; m == 0 with b * n > 0, a NULL required pointer (known_rows with
 *   c2 > 0, skip_rows with c1 > 0, idx, dist2, weights, rows) -> SN_ERR_BAD_ARGUMENT; more than 2^31 - 1 workgroups
 *   (ceil(b * n / (256 / LG))) -> SN_ERR_UNSUPPORTED.
 *
 * sn_interp_rows_backward: weights (b,n,3) as written above, grad_rows (b, n, c2 + c1); start (b,m+1) / order (b,3n) from
 *   sn_gather_invert(b, m, 3 n, idx, ..) -> grad_known (b,m,c2), OVERWRITTEN:
 *     grad_known[b,r,ch] = THE LIST WALK's sum (above; ne = 3n) of the weighted terms fl(grad_rows[b, e/3, ch] * weights[b,e]).
 *     This is the arithmetic of sn_weighted_gather_backward_inverted: the two are BIT-IDENTICAL on transposed operands.  The skip
 *     features' gradient is the view grad_rows[.., c2:] and needs no kernel; no gradient goes towards the weights, the distances or
 *     the coordinates (sn_three_nn has none).
 *   One launch: a group of LG lanes (the power of two covering c2, 64 at most) owns a row and LG of its columns, four entries'
 *   loads in flight.
 *   Checked on the host, in this order: a negative size, 3 n or c2 + c1 beyond 2^31 - 1 -> SN_ERR_BAD_ARGUMENT; b == 0, m == 0 or
 *   c2 == 0 is a no-op that succeeds; start or grad_known NULL, or weights / grad_rows / order NULL with n > 0 ->
 *   SN_ERR_BAD_ARGUMENT; more than 2^31 - 1 workgroups (ceil(b * m * ceil(c2 / LG) / (256 / LG))) -> SN_ERR_UNSUPPORTED.
 *
 * sn_bn_relu_backward_stats: dy (R, C) = sn_bn_relu_backward(R, C, z, coef, g, with_scale = 0, ..)'s output bit for bit, and in the
 *   same launch the BatchNorm-backward partial sums stats [nblk][2][C], nblk = sn_bn_relu_stats_blocks(R) = ceil(R / 256), both
 *   fully OVERWRITTEN: block k holds (sum dy, sum fl(dy * z)) over rows 256 k .. min(R, 256 k + 256) - 1 of every channel.  With
 *   LR = the power of two covering C / 4, 64 at most, and S = 256 / LR slices: slice q adds the block's rows q, q + S, .. ascending
 *   from +0, then the S slice sums are added in slice order from +0; every add rounded, nothing contracted.  The order depends on
 *   R and C alone, never on the launch or on timing.  The layout is the one sn_bn_backward_coef(nblk, C, R, stats, ..) reduces.
 *   No atomics, no workspace, capturable.  Checked on the host, in this order: a negative size, C % 4 != 0 ->
 *   SN_ERR_BAD_ARGUMENT; R == 0 or C == 0 is a no-op that succeeds; a NULL pointer -> SN_ERR_BAD_ARGUMENT; more than 2^31 - 1
 *   blocks -> SN_ERR_UNSUPPORTED (sn_bn_relu_stats_blocks returns 0 for R < 1 and beyond that bound). */
int sn_interp_rows_forward(int b, int n, int m, int c2, int c1, int rule, const float *known_rows, const float *skip_rows,
                           const int *idx, const float *dist2, float *weights, float *rows, sn_stream_t stream);
int sn_interp_rows_backward(int b, int n, int m, int c2, int c1, const float *weights, const float *grad_rows, const int *start,
                            const int *order, float *grad_known, sn_stream_t stream);
int sn_bn_relu_stats_blocks(long long R);
int sn_bn_relu_backward_stats(long long R, int C, const float *z, const float *coef, const float *g, float *dy, float *stats,
                              sn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SAMPLENET_HIP_INTERNAL_H */

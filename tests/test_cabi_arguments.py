"""Host-side half of the C-ABI contract (no GPU): every geometric entry point of include/samplenet_hip.h refuses a negative
size, a NULL required pointer, an unknown layout selector and an unsupported K / prefix count / matching size with the
documented code and its OWN name in sn_last_error_string(), and treats the documented empty cases as no-ops -- all of it before
any device work.  So do the entries of include/samplenet_hip_internal.h that the task networks share: the skinny FC route
(sn_skinny_linear, sn_skinny_linear2 -- which answer a size they do not serve with UNSUPPORTED --, sn_skinny_wgrad), the per-cloud
transforms, the orthogonality regulariser and sn_bn_relu_*, and the nine entries of the one-batch task evaluation (cyclic padding, the
valid-query Chamfer scan, the grouped Chamfer-mean loss, head + rotation plain and grouped), and the twelve entries of the sampler
step's fused loss (the split pair scans, the step-loss forward / backward, the surface pair, the scalar loss entries), and the five FC-chain entries (tests/test_gpu_fc_chain.py calls them on a device), and the ten per-layer entries of the PointNet MLP (tests/test_gpu_mlp.py calls them on a device), and the five entries and two size queries of the
registration task network's extractor (tests/test_gpu_task_net_direct.py calls them on a device).  The table below is the data; one child process (which sees no GPU, so that a call that slipped through a
missing check comes back as an error code instead of touching a device with the made-up pointers) runs it once."""
import ctypes

import pytest

from cabi_runner import check_case, run_cases

BAD, UNSUP = 10001, 10002
Pp = "PTR"    # a non-NULL (never dereferenced) device pointer
HOSTI = "HOSTI"  # a real host int array {4}: sn_prefix_point_minima reads its prefix sizes on the host
HOSTP = "HOSTP"  # a real host array of ONE non-NULL (never dereferenced) device pointer: sn_cyclic_pad_cat reads its clouds' addresses on the host
# [HOSTI, v0, v1, ...] / [HOSTP, p0, p1, ...]: the same with the values spelled out (a pointer of 0 is NULL)

# entry -> (valid argument list, positions of the sizes, positions of the REQUIRED pointers).  The valid list itself is never
# called: every case breaks one argument of it.  Optional pointers are left NULL in the base.
ENTRIES = {
    "sn_pairscan_forward": ([1, 8, 4, 2, Pp, 0, Pp, 0, Pp, Pp, Pp, Pp, Pp, Pp, Pp, 0, Pp, Pp, 0.0, None], [0, 1, 2, 3], [4, 6, 17]),
    "sn_pairscan_forward_ws": ([1, 8, 4, 2, Pp, 0, Pp, 0, Pp, Pp, Pp, Pp, Pp, Pp, Pp, 0, Pp, Pp, 0.0, None, 0, None], [0, 1, 2, 3],
                               [4, 6, 17]),
    "sn_chamfer_forward": ([1, 8, Pp, 4, Pp, Pp, Pp, Pp, Pp, None], [0, 1, 3], [2, 4]),
    "sn_chamfer_backward": ([1, 8, Pp, 4, Pp, Pp, Pp, Pp, Pp, Pp, Pp, None], [0, 1, 3], [2, 4, 5, 6, 7, 8]),
    "sn_knn": ([1, 8, 4, 2, Pp, 0, Pp, 0, Pp, Pp, None], [0, 1, 2, 3], [4, 6]),
    "sn_soft_weights_forward": ([1, 8, 4, 2, Pp, Pp, Pp, Pp, 0.0, Pp, None], [0, 1, 2, 3], [4, 5, 6, 7, 9]),
    "sn_soft_weights_backward": ([1, 8, 4, 2, Pp, Pp, Pp, Pp, 0.0, None, Pp, None, None, None, None], [0, 1, 2, 3], [4, 5, 6, 7, 10]),
    "sn_soft_weights_backward_ordered": ([1, 8, 4, 2, Pp, Pp, Pp, Pp, 0.0, None, Pp, None, Pp, None, Pp, None], [0, 1, 2, 3],
                                         [4, 5, 6, 7, 10, 12, 14]),
    "sn_weighted_gather_forward": ([1, 3, 8, 4, 2, Pp, Pp, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7, 8]),
    "sn_weighted_gather_backward": ([1, 3, 8, 4, 2, Pp, Pp, Pp, Pp, None, None, None], [0, 1, 2, 3, 4], [5, 6, 7, 8]),
    "sn_weighted_gather_backward_ordered": ([1, 3, 8, 4, 2, Pp, Pp, Pp, Pp, None, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7, 8, 10, 11]),
    "sn_soft_project_backward": ([1, 8, 4, 2, Pp, 0, Pp, 0, Pp, Pp, 0.0, Pp, 0, None, 0, None, None, None], [0, 1, 2, 3],
                                 [4, 6, 8, 9, 11]),
    "sn_soft_project_backward_ordered": ([1, 8, 4, 2, Pp, 0, Pp, 0, Pp, Pp, 0.0, Pp, 0, None, 0, Pp, None, Pp, None], [0, 1, 2, 3],
                                         [4, 6, 8, 9, 11, 15, 17]),
    "sn_sigma_grad": ([2, Pp, Pp, 0.0, Pp, None], [0], [1, 2, 4]),
    "sn_group_point": ([1, 8, 3, 4, 2, Pp, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7]),
    "sn_group_point_grad": ([1, 8, 3, 4, 2, Pp, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7]),
    "sn_grouping_operation": ([1, 3, 8, 4, 2, Pp, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7]),
    "sn_grouping_operation_grad": ([1, 3, 8, 4, 2, Pp, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7]),
    "sn_simplification_loss_forward": ([1, 4, 8, Pp, Pp, 1.0, Pp, Pp, Pp, None], [0, 1, 2], [3, 4, 6, 7, 8]),
    "sn_simplification_loss_backward": ([1, 4, Pp, 8, Pp, Pp, Pp, Pp, 1.0, Pp, Pp, None, 0, None], [0, 1, 3], [2, 4, 5, 6, 7, 9]),
    "sn_chamfer_mean_loss_forward": ([1, 4, 8, Pp, Pp, Pp, Pp, Pp, None], [0, 1, 2], [3, 4, 5, 6, 7]),
    "sn_chamfer_mean_loss_backward": ([1, 4, Pp, 8, Pp, Pp, Pp, Pp, Pp, None, None], [0, 1, 3], [2, 4, 5, 6, 7]),
    "sn_pcrnet_head_forward": ([2, Pp, Pp, None, None, None], [0], [1, 2]),
    "sn_pcrnet_head_backward": ([2, Pp, None, None, None, Pp, None], [0], [1, 5]),
    "sn_qrot_forward": ([1, 8, Pp, Pp, Pp, None], [0, 1], [2, 3, 4]),
    "sn_qrot_backward": ([1, 8, Pp, Pp, Pp, Pp, None, None], [0, 1], [2, 3, 4]),
    "sn_prefix_point_minima": ([1, 8, 4, 1, HOSTI, Pp, Pp, Pp, Pp, None], [0, 1, 2, 3], [4, 5, 6, 7, 8]),
    "sn_nn_matching": ([1, 8, 4, Pp, 0, Pp, 1, Pp, None], [0, 1, 2], [3, 5, 7]),
}
# The entries of include/samplenet_hip_internal.h that the task networks share, under the same rules as ENTRIES (kept apart: ENTRIES
# is the public header's list, which tests/test_gpu_cabi_contract.py walks family by family): the shared FC route's weight gradient,
# the per-cloud transforms (K counts as a size: -1 is as bad as any K outside {3, 64}), the orthogonality regulariser, the
# materialised BatchNorm + ReLU (its R is a long long: cases below)
INTERNAL = {
    "sn_skinny_wgrad": ([4, 8, 8, Pp, None, 0, Pp, None, Pp, None, None], [0, 1, 2], [3, 6, 8]),
    "sn_cloud_transform_forward": ([1, 8, 3, Pp, Pp, Pp, None], [0, 1, 2], [3, 4, 5]),
    "sn_cloud_transform_backward": ([1, 8, 3, Pp, Pp, Pp, Pp, Pp, None], [0, 1, 2], [3, 4, 5]),
    "sn_orthogonality_loss_forward": ([1, 3, Pp, Pp, Pp, None], [0, 1], [2, 3, 4]),
    "sn_orthogonality_loss_backward": ([1, 3, Pp, Pp, Pp, None], [0, 1], [2, 3, 4]),
    "sn_bn_relu_forward": ([2, 8, Pp, Pp, Pp, None], [1], [2, 3, 4]),
    "sn_bn_relu_backward": ([2, 8, Pp, Pp, Pp, 0, Pp, None], [1], [2, 3, 4, 6]),
}
# The one-batch task evaluation (BASELINE configs[4]: every prefix of the progressive sampler as one batch), same rules.  The bases
# hold ONE cloud / evaluation, so that the one-element host arrays above are all an entry may read; the cases past the generic ones
# are spelled out in _task_batch_cases().
TASK_BATCH = {
    # B, len, C, nclouds, sizes, src, out, stream
    "sn_cyclic_pad_cat": ([1, 8, 3, 1, HOSTI, HOSTP, Pp, None], [0, 1, 2, 3], [4, 5, 6]),
    # B, len, C, nclouds, sizes, grad_out, grads, stream
    "sn_cyclic_pad_cat_backward": ([1, 8, 3, 1, HOSTI, Pp, HOSTP, None], [0, 1, 2, 3], [4, 5, 6]),
    # B, m, xyz_small, n, xyz_large, q_valid, q_group, dist_small, idx_small, dist_large, idx_large, workspace, workspace_bytes, stream
    "sn_chamfer_forward_valid": ([2, 4, Pp, 8, Pp, Pp, 1, Pp, Pp, Pp, Pp, None, 0, None], [0, 1, 3, 6], [2, 4, 5, 7, 8, 9, 10]),
    # B, N, y, v, twist, quat, qnorm, out, stream
    "sn_pcrnet_head_rot_forward": ([2, 8, Pp, Pp, Pp, Pp, None, Pp, None], [0, 1], [2, 3, 4, 5, 7]),
    # B, N, y, quat, v, grad_out, grad_twist, grad_quat, grad_qnorm, grad_v, grad_y, stream
    "sn_pcrnet_head_rot_backward": ([2, 8, Pp, Pp, Pp, None, None, None, None, None, Pp, None], [0, 1], [2, 3, 4, 10]),
    # R, N, group, y, v, twist, quat, qnorm, out, stream
    "sn_pcrnet_head_rot_forward_grouped": ([4, 8, 2, Pp, Pp, Pp, Pp, None, Pp, None], [0, 1, 2], [3, 4, 5, 6, 8]),
    # R, N, group, y, quat, v, grad_out, grad_twist, grad_quat, grad_qnorm, grad_y, stream
    "sn_pcrnet_head_rot_backward_grouped": ([4, 8, 2, Pp, Pp, Pp, None, None, None, None, Pp, None], [0, 1, 2], [3, 4, 5, 10]),
    # R, n1, n2, group, nev, nvalid, dist1, dist2, partial, loss, stream
    "sn_chamfer_mean_loss_forward_grouped": ([2, 4, 8, 2, 1, HOSTI, Pp, Pp, Pp, Pp, None], [0, 1, 2, 3, 4], [5, 6, 7, 8, 9]),
    # R, n1, xyz1, n2, xyz2, group, nev, nvalid, idx1, idx2, grad_loss, grad_xyz1, grad_xyz2, stream
    "sn_chamfer_mean_loss_backward_grouped": ([2, 4, Pp, 8, Pp, 2, 1, HOSTI, Pp, Pp, Pp, None, None, None], [0, 1, 3, 5, 6],
                                              [2, 4, 7, 8, 9, 10]),
}
# The sampler step's fused loss entries (include/samplenet_hip_internal.h; tests/test_gpu_step_loss.py calls them on a device), same
# rules.  Every size is >= 1 here (no empty case documented): 0 is refused like -1.  The scan bases are a shape whose queries are
# spread over three workgroups (2 clouds of 8 points, 40 queries), so that a refusal cannot be mistaken for the G <= 1 answer.
STEP_LOSS = {
    # B, N, M, K, P, p_layout, Q, q_layout, knn_idx, dist_q, idx_q, proj, proj_layout, temperature, min_sigma, workspace, workspace_bytes, stream
    "sn_pairscan_forward_partial": ([2, 8, 40, 2, Pp, 0, Pp, 0, Pp, Pp, Pp, Pp, 0, Pp, 0.0, Pp, 1 << 20, None], [0, 1, 2, 3], [4, 6, 13, 15]),
    # B, N, M, K, P, p_layout, fc_z, fc_scale, fc_shift, fc_w, fc_bias, Kfc, q_out, knn_idx, dist_q, idx_q, proj, proj_layout, temperature,
    # min_sigma, workspace, workspace_bytes, stream
    "sn_pairscan_forward_partial_fc": ([2, 8, 40, 2, Pp, 0, Pp, Pp, Pp, Pp, Pp, 8, Pp, Pp, Pp, Pp, Pp, 0, Pp, 0.0, Pp, 1 << 20, None],
                                       [0, 1, 2, 3, 11], [4, 6, 7, 8, 9, 10, 12, 18, 20]),
    # B, N, M, K, P, p_layout, Q, fc_z, fc_scale, fc_shift, fc_w, fc_bias, Kfc, knn_idx, dist_q, idx_q, proj, proj_layout, temperature,
    # min_sigma, colmin_keys, qpart, qmax, stream
    "sn_pairscan_forward_keys": ([2, 8, 40, 2, Pp, 0, Pp, None, None, None, None, None, 0, Pp, Pp, Pp, Pp, 0, Pp, 0.0, Pp, Pp, Pp, None],
                                 [0, 1, 2, 3], [4, 6, 14, 16, 18, 20, 21, 22]),
    # B, M, N, G, dist_q, colmin_ws, proj, temperature, alpha, lmbda, weight, min_sigma, dist_p, idx_p, argmax1, partial, loss, defer_value, stream
    "sn_sampler_step_loss_forward": ([2, 40, 8, 3, Pp, Pp, Pp, Pp, 0.5, 0.5, 1.0, 0.0, Pp, Pp, Pp, Pp, Pp, 0, None], [0, 1, 2, 3],
                                     [4, 5, 6, 7, 12, 13, 14, 15, 16]),
    # B, M, N, dist_q, dist_p, proj, temperature, alpha, lmbda, weight, min_sigma, argmax1, partial, loss, defer_value, stream
    "sn_sampler_step_loss_forward_direct": ([2, 40, 8, Pp, Pp, Pp, Pp, 0.5, 0.5, 1.0, 0.0, Pp, Pp, Pp, 0, None], [0, 1, 2],
                                            [3, 4, 5, 6, 11, 12, 13]),
    # B, N, M, K, P, p_layout, Q, knn_idx, idx_q, idx_p, argmax1, temperature, min_sigma, alpha, lmbda, weight, grad_loss, grad_Q,
    # gsig_scratch, grad_T, deferred_partial, deferred_loss, stream
    "sn_sampler_step_loss_backward": ([2, 8, 40, 2, Pp, 0, Pp, Pp, Pp, Pp, Pp, Pp, 0.0, 0.5, 0.5, 1.0, Pp, Pp, Pp, Pp, None, None, None],
                                      [0, 1, 2, 3], [4, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19]),
    # B, N, M, K, P, p_layout, Q, knn_idx, idx_q, colmin_keys, qpart, qmax, G, temperature, min_sigma, alpha, lmbda, weight, grad_loss, grad_Q,
    # gsig_scratch, grad_T, dpsum, loss, stream, deferred_tail, grad_proj, grad_sigma
    "sn_sampler_step_loss_keys": ([2, 8, 40, 2, Pp, 0, Pp, Pp, Pp, Pp, Pp, Pp, 3, Pp, 0.0, 0.5, 0.5, 1.0, Pp, Pp, Pp, Pp, Pp, Pp, None, None,
                                   None, None], [0, 1, 2, 3, 12], [4, 6, 7, 8, 9, 10, 11, 13, 18, 19, 20, 21, 22, 23]),
    # B, N, M, G, colmin_keys, qpart, qmax, temperature, min_sigma, weight, y_bcn, simp_bnc, dpsum, values, stream
    "sn_surface_values_keys": ([2, 8, 40, 3, Pp, Pp, Pp, Pp, 0.0, 1.0, None, None, Pp, Pp, None], [0, 1, 2, 3], [4, 5, 6, 7, 12, 13]),
    # nproj, g_lsimp, g_sigma, g_proj, scalars, proj_out, stream
    "sn_surface_gather_upstream": ([24, None, None, None, Pp, Pp, None], [0], [4, 5]),
    # nproj, proj, lsimp, temperature, alpha, lmbda, min_sigma, loss, stream
    "sn_sampler_loss_forward": ([24, Pp, Pp, Pp, 0.5, 0.5, 0.0, Pp, None], [0], [1, 2, 3, 7]),
    # nproj, grad_loss, temperature, alpha, lmbda, min_sigma, grad_proj, grad_lsimp, grad_T, stream
    "sn_sampler_loss_backward": ([24, Pp, Pp, 0.5, 0.5, 0.0, Pp, Pp, Pp, None], [0], [1, 2, 6, 7, 8]),
    # temperature, min_sigma, sigma, stream
    "sn_sigma_forward": ([Pp, 0.0, Pp, None], [], [0, 2]),
}
# sn_skinny_linear / sn_skinny_linear2 answer a size they do not serve -- negative ones included -- with UNSUPPORTED (callers ask
# sn_skinny_linear_supported and take another route), so the generic "negative size is a BAD argument" rule above does not fit them:
# entry -> (valid argument list, required pointers); every case is spelled out in _skinny_cases().
SKINNY = {
    # R, K, N, x, gate, W, transposed, bias, relu, out, scratch, counters, stream
    "sn_skinny_linear": ([4, 64, 40, Pp, None, Pp, 0, None, 0, Pp, Pp, Pp, None], [3, 5, 9, 10, 11]),
    # R, K, N, x, x2, ksplit, gate, W, transposed, bias, relu, out, out2, nsplit, scratch, counters, stream
    "sn_skinny_linear2": ([4, 64, 40, Pp, None, 0, None, Pp, 0, None, 0, Pp, None, 0, Pp, Pp, None], [3, 7, 11, 14, 15]),
}


# The five FC-chain entries (csrc/fc_chain.hip).  Their per-layer / per-stage operands are HOST arrays of device pointers, eps / momentum
# host float arrays, Co / Ci / araw host int arrays and bn_rows a host array of long long (spelled as pairs of ints): the bases hold two
# layers (forward, backward) or the three the pool entries serve, so every case is spelled out in _fc_chain_cases().  A row count outside
# 1..32 is a BAD argument; a width or depth the kernels do not serve is UNSUPPORTED (callers ask the `_supported` query first).
_P2, _P3, _F2, _F3 = [HOSTP, 4096, 4096], [HOSTP, 4096, 4096, 4096], [HOSTI, 0, 0], [HOSTI, 0, 0, 0]
_POOL = [4, 64, 5, Pp, Pp, Pp, Pp, Pp, Pp, Pp, None, 1e-5, 0.1, Pp, Pp, Pp, Pp, 256, 3, _P3, _P3, _P3, _P3, None, None, None, _F3, _F3, _P3, _P3,
         Pp, Pp]
_POOL_REQ = [3, 4, 5, 6, 7, 8, 9, 13, 14, 15, 16, 19, 20, 21, 22, 26, 27, 28, 29, 30, 31]
_BWD = [_P2, _P2, _P2, [HOSTI, 4, 0, 4, 0], _P2, _P2, _P2, _P2, None, _P2, [HOSTI, 0, 0], None, None, Pp, Pp, None]
FC_CHAIN = {
    # R, C0, H, nl, a0, W, bias, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, z, coef, xbuf, sync, stream
    "sn_fc_chain_forward": ([4, 128, 256, 2, Pp, _P2, _P2, _P2, _P2, None, None, None, _F2, _F2, _P2, _P2, Pp, Pp, None],
                            [4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17], [5, 6, 7, 8, 14, 15]),
    # B, N, nconv, acc, pool_val, pool_idx, gamma5, beta5, running_mean5, running_var5, num_batches_tracked5, eps5, momentum5, coef5, pooled,
    # argsel, zsel, H, nl, W, bias, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, z, coef, xbuf, sync, stream
    "sn_fc_chain_forward_pool": (_POOL + [None], _POOL_REQ, [19, 20, 21, 22, 28, 29]),
    # ... sync, Co, Wo, bo, gamma_o, beta_o, running_mean_o, running_var_o, num_batches_tracked_o, eps_o, momentum_o, zo, coef_o, y, stream
    "sn_fc_chain_forward_pool_out": (_POOL + [96, Pp, Pp, Pp, Pp, None, None, None, 1e-5, 0.1, Pp, Pp, Pp, None],
                                     _POOL_REQ + [33, 34, 35, 36, 42, 43, 44], [19, 20, 21, 22, 28, 29]),
    # R, ns, Co, Ci, gy, W, zprev, coefprev, bn_rows, dgamma, dbeta, dbias, dW, db_top, aprev, araw, gout, kout, xbuf, sync, stream
    "sn_fc_chain_backward": ([4, 2, [HOSTI, 256, 256], [HOSTI, 256, 128], Pp] + _BWD, [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 18, 19],
                             [5, 6, 7, 9, 10, 12, 14]),
    # R, ns, Co, Ci, gy, zo, coef_o, fixed, dgamma_o, dbeta_o, W, zprev, ... as above
    "sn_fc_chain_backward_obn": ([4, 2, [HOSTI, 256, 256], [HOSTI, 256, 128], Pp, Pp, Pp, 0, Pp, Pp] + _BWD,
                                 [2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 23, 24], [10, 11, 12, 14, 15, 17, 19]),
}

# The ten per-layer entries of the PointNet MLP (csrc/pointnet_mlp.hip, csrc/pointnet_mlp_backward.hip), same rules as ENTRIES: every
# size is >= 1 (0 is refused like -1), dz_mode is 0 (plain), 1 (BatchNorm) or 2 (pool).  The bases sit on the route whose refusals the
# cases past the generic ones name (_mlp_cases()): 64 rows for the tile kernels, 128 / 256 aligned rows for the fused conv entries.
MLP = {
    # R, Ci, Co, ain, coef_prev, W, bias, z, stats, stream
    "sn_linear_forward": ([64, 8, 8, Pp, None, Pp, None, Pp, None, None], [0, 1, 2], [3, 5, 7]),
    # R, Ci, Co, ain, coef_prev, W, bias, z, stream
    "sn_linear_forward_rows": ([64, 8, 8, Pp, None, Pp, None, Pp, None], [0, 1, 2], [3, 5, 7]),
    # R, Ci, Co, ain, coef_prev, W, bias, z, stats, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, coef, stream
    "sn_layer_forward_bn": ([64, 8, 8, Pp, None, Pp, None, Pp, Pp, Pp, Pp, 1e-5, 0.1, None, None, None, Pp, None], [0, 1, 2],
                            [3, 5, 7, 8, 9, 10, 16]),
    # R, Ci, Co, npts, ain, coef_prev, W, bias, z, stats, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, coef,
    # pool_val, pool_idx, pooled, argsel, zsel, stream
    "sn_conv_forward_bn_pool": ([128, 64, 64, 64, Pp, Pp, Pp, None, Pp, Pp, Pp, Pp, 1e-5, 0.1, None, None, None, Pp, Pp, Pp, Pp, Pp, Pp, None],
                                [0, 1, 2, 3], [4, 5, 6, 8, 9, 10, 11, 17, 18, 19, 20, 21, 22]),
    # R, Ci, Co, dz_mode, dy, z, kcoef, gsel, argsel, npts, W, zprev, coef_prev, dyprev, stats, stream
    "sn_linear_dgrad": ([64, 8, 8, 0, Pp, None, None, None, None, 1, Pp, Pp, None, Pp, None, None], [0, 1, 2], [10, 13]),
    # R, Ci, Co, dz_mode, dy, z, kcoef, gsel, argsel, npts, aprev, coef_prev, part, dW, db, stream
    "sn_linear_wgrad": ([64, 8, 8, 0, Pp, None, None, None, None, 1, Pp, None, Pp, Pp, None, None], [0, 1, 2], [10, 12, 13]),
    # R, Ci, Co, dz_mode, dy, z, kcoef, gsel, argsel, npts, W, zprev, coef_prev, dyprev, stats, part, stream
    "sn_conv_backward_partials": ([256, 64, 64, 1, Pp, Pp, Pp, None, None, 64, Pp, Pp, Pp, Pp, Pp, Pp, None], [0, 1, 2],
                                  [4, 5, 6, 10, 11, 12, 13, 14, 15]),
    # R, Ci, Co, dz_mode, dy, z, kcoef, gsel, argsel, npts, W, zprev, coef_prev, dyprev, stats, part, dW, stream
    "sn_linear_backward": ([64, 8, 8, 0, Pp, None, None, None, None, 1, Pp, Pp, None, Pp, None, Pp, Pp, None], [0, 1, 2], [10, 11, 13, 15, 16]),
    # R, Ci, Co, dz_mode, dy, z, kcoef, gsel, argsel, npts, W, zprev, coef_prev, dyprev, stats, part, dW, db, prev_dgamma, prev_dbeta,
    # prev_dbias, prev_kcoef, prev_bn_rows, stream
    "sn_layer_backward": ([64, 8, 8, 0, Pp, None, None, None, None, 1, Pp, Pp, None, Pp, None, Pp, Pp, None, None, None, None, None, 0, None],
                          [0, 1, 2], [10, 11, 13, 16]),
    # R, Ci, Co, dy, z, kcoef, W, zprev, coef_prev, stats, part, dW, prev_dgamma, prev_dbeta, prev_dbias, prev_kcoef, x_in, W_in, b_in, dW_in,
    # stream
    "sn_layer_backward_in3": ([256, 64, 64, Pp, Pp, Pp, Pp, Pp, Pp, Pp, Pp, Pp, Pp, Pp, None, Pp, Pp, Pp, None, Pp, None], [0, 1, 2],
                              [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 19]),
}

# The registration task network's extractor entries (csrc/task_network.hip and sn_linear_forward_maxpool of csrc/pointnet_mlp.hip;
# tests/test_gpu_task_net_direct.py calls them on a device): entry -> (valid argument list, positions of the REQUIRED pointers); optional
# pointers are left NULL in the base.  The two narrow entries and the tile entry refuse a size below 1 as a BAD argument; the wide entry
# and the sparse data gradient answer every size they do not serve -- negative ones included -- with UNSUPPORTED (callers ask their
# `_supported` queries), after the pointer checks: every case is spelled out in _task_net_cases().
TASK_NET = {
    # R, Ci, Co, npts, ain, coef_prev, W, bias, z, keys, pooled, argsel, zsel, keys_cleared, stream
    "sn_linear_forward_maxpool": ([128, 64, 64, 64, Pp, Pp, Pp, None, None, Pp, Pp, None, None, 0, None], [4, 5, 6, 9, 10]),
    # R, Ci, Co, npts, ain, coef_prev, W, bias, z, scratch, pooled, argsel, zsel, wplanes, planes_ready, stream
    "sn_linear_forward_maxpool_wide": ([16384, 64, 512, 64, Pp, None, Pp, None, None, Pp, Pp, None, None, Pp, 0, None], [4, 6, 9, 10, 13]),
    # B, npts, Ci, Co, g, pooled, argsel, W, zprev, coef_prev, dyprev, stream
    "sn_pool_dgrad_sparse": ([1, 8, 8, 8, Pp, Pp, Pp, Pp, None, None, Pp, None], [4, 5, 6, 7, 10]),
    # R, x, W1, b1, W2, b2, W3, b3, W4, b4, wplanes, planes_ready, z1, z2, z3, z4, zero_keys, zero_n, stream
    "sn_pointnet_narrow_forward": ([64, Pp, Pp, None, Pp, None, Pp, None, Pp, None, Pp, 0, None, None, None, Pp, None, 0, None],
                                   [1, 2, 4, 6, 8, 10, 15]),
    # R, dz4, z1, z2, z3, W1, W2, W3, W4, wplanes_t, planes_ready, dx, stream
    "sn_pointnet_narrow_backward": ([64, Pp, Pp, Pp, Pp, Pp, Pp, Pp, Pp, Pp, 0, Pp, None], [1, 2, 3, 4, 5, 6, 7, 8, 9, 11]),
}


def _with(name, changes):
    args = list((ENTRIES.get(name) or INTERNAL.get(name) or TASK_BATCH.get(name) or STEP_LOSS.get(name) or SKINNY.get(name) or FC_CHAIN.get(name)
                 or TASK_NET.get(name) or MLP[name])[0])
    for pos, val in changes.items():
        args[pos] = val
    return args


def _cases():
    out = []  # (id, entry, args, expected code, text the message must contain | None)
    for name, (base, sizes, required) in list(ENTRIES.items()) + list(INTERNAL.items()) + list(TASK_BATCH.items()):
        for pos in sizes:
            out.append(("%s-size%d-negative" % (name, pos), name, _with(name, {pos: -1}), BAD, name))
        for pos in required:
            out.append(("%s-arg%d-null" % (name, pos), name, _with(name, {pos: None}), BAD, name))
    # both gradient outputs NULL: sn_qrot_backward has nothing to compute
    out.append(("sn_qrot_backward-no-output", "sn_qrot_backward", _with("sn_qrot_backward", {5: None, 6: None}), BAD, "sn_qrot_backward"))
    # layout selectors: any value other than 0 / 1 is refused by every entry that takes one
    for name, positions in (("sn_pairscan_forward", (5, 7, 15)), ("sn_pairscan_forward_ws", (5, 7, 15)), ("sn_knn", (5, 7)),
                            ("sn_soft_project_backward", (5, 7, 12, 14)), ("sn_soft_project_backward_ordered", (5, 7, 12, 14)),
                            ("sn_simplification_loss_backward", (12,)), ("sn_nn_matching", (4,))):
        for pos in positions:
            for bad in (2, -1):
                out.append(("%s-selector%d-is-%d" % (name, pos, bad), name, _with(name, {pos: bad}), BAD, name))
    out.append(("simp-bwd-layout1-with-grad_xyz2", "sn_simplification_loss_backward",
                _with("sn_simplification_loss_backward", {12: 1, 11: Pp}), BAD, "grad_xyz2"))
    # K / k limits
    for name in ("sn_pairscan_forward", "sn_pairscan_forward_ws", "sn_knn"):
        out.append((name + "-K65", name, _with(name, {1: 100, 3: 65}), BAD, name))
        out.append((name + "-K>N", name, _with(name, {1: 4, 3: 5}), BAD, name))
    for name in ("sn_soft_weights_forward", "sn_soft_weights_backward", "sn_soft_weights_backward_ordered", "sn_soft_project_backward",
                 "sn_soft_project_backward_ordered"):
        out.append((name + "-k65", name, _with(name, {1: 100, 3: 65}), BAD, name))
        out.append((name + "-k0", name, _with(name, {3: 0}), BAD, name))
    out.append(("sn_knn-k0", "sn_knn", _with("sn_knn", {3: 0}), BAD, "sn_knn"))
    out.append(("pairscan-K0-with-knn-output", "sn_pairscan_forward", _with("sn_pairscan_forward", {3: 0}), BAD, "K must be >= 1"))
    out.append(("pairscan-one-side-empty", "sn_pairscan_forward", _with("sn_pairscan_forward", {2: 0}), BAD, "empty cloud"))
    out.append(("sn_prefix_point_minima-nprefix17", "sn_prefix_point_minima", _with("sn_prefix_point_minima", {3: 17}), BAD,
                "sn_prefix_point_minima"))
    out.append(("sn_prefix_point_minima-last-prefix-not-M", "sn_prefix_point_minima", _with("sn_prefix_point_minima", {2: 5}), BAD,
                "last prefix"))
    out.append(("sn_nn_matching-k1025", "sn_nn_matching", _with("sn_nn_matching", {1: 2000, 2: 1025}), UNSUP, "sn_nn_matching"))
    out.append(("sn_nn_matching-N8193", "sn_nn_matching", _with("sn_nn_matching", {1: 8193}), UNSUP, "sn_nn_matching"))
    out.append(("sn_sigma_grad-nparts0", "sn_sigma_grad", _with("sn_sigma_grad", {0: 0}), BAD, "sn_sigma_grad"))
    for name in ("sn_simplification_loss_forward", "sn_simplification_loss_backward", "sn_chamfer_mean_loss_forward",
                 "sn_chamfer_mean_loss_backward", "sn_pcrnet_head_forward", "sn_pcrnet_head_backward", "sn_prefix_point_minima"):
        out.append((name + "-B0-is-an-error", name, _with(name, {0: 0}), BAD, name))  # (these take B >= 1: no empty case documented)
    # documented empty cases: 0 with every pointer NULL
    nulled = lambda name, ch: [None if a in (Pp, HOSTI) else a for a in _with(name, ch)]
    for name, ch in (("sn_pairscan_forward", {0: 0}), ("sn_pairscan_forward_ws", {0: 0}), ("sn_pairscan_forward", {1: 0, 2: 0, 3: 0}),
                     ("sn_chamfer_forward", {0: 0}), ("sn_chamfer_forward", {1: 0, 3: 0}), ("sn_knn", {0: 0}),
                     ("sn_chamfer_backward", {0: 0}), ("sn_chamfer_backward", {1: 0}), ("sn_chamfer_backward", {3: 0}),
                     ("sn_soft_weights_forward", {0: 0}), ("sn_soft_weights_forward", {2: 0}),
                     ("sn_soft_weights_backward", {0: 0}), ("sn_soft_weights_backward", {2: 0}),
                     ("sn_soft_weights_backward_ordered", {0: 0}), ("sn_soft_weights_backward_ordered", {2: 0}),
                     ("sn_weighted_gather_forward", {0: 0}), ("sn_weighted_gather_forward", {3: 0}), ("sn_weighted_gather_forward", {1: 0}),
                     ("sn_weighted_gather_backward", {0: 0}), ("sn_weighted_gather_backward", {3: 0}),
                     ("sn_weighted_gather_backward_ordered", {0: 0}), ("sn_weighted_gather_backward_ordered", {3: 0}),
                     ("sn_soft_project_backward", {0: 0}), ("sn_soft_project_backward", {2: 0}),
                     ("sn_soft_project_backward_ordered", {0: 0}), ("sn_soft_project_backward_ordered", {2: 0}),
                     ("sn_group_point", {0: 0}), ("sn_group_point", {3: 0}), ("sn_group_point", {4: 0}), ("sn_group_point", {2: 0}),
                     ("sn_group_point_grad", {0: 0}), ("sn_group_point_grad", {1: 0}), ("sn_group_point_grad", {2: 0}),
                     ("sn_grouping_operation", {0: 0}), ("sn_grouping_operation", {3: 0}),
                     ("sn_grouping_operation_grad", {0: 0}), ("sn_grouping_operation_grad", {2: 0}),
                     ("sn_qrot_forward", {0: 0}), ("sn_qrot_forward", {1: 0}), ("sn_qrot_backward", {0: 0}), ("sn_nn_matching", {0: 0})):
        out.append(("%s-empty-%s" % (name, "".join("%d" % p for p in ch)), name, nulled(name, ch), 0, None))
    return (out + _skinny_cases() + _transform_cases(nulled) + _task_batch_cases() + _step_loss_cases() + _fc_chain_cases() + _mlp_cases()
            + _task_net_cases())


def _task_net_cases():
    out = []
    add = lambda cid, name, ch, text=None, code=BAD: out.append(("%s-%s" % (name, cid), name, _with(name, ch), code, text or name))
    for name, (base, required) in TASK_NET.items():
        for pos in required:
            add("arg%d-null" % pos, name, {pos: None})
    tile, wide, sparse, nf, nb = TASK_NET
    for pos in (0, 1, 2, 3):
        add("size%d-negative" % pos, tile, {pos: -1}, "bad size")
        add("size%d-zero" % pos, tile, {pos: 0}, "bad size")
    # shapes the 64 x 64 tiles with one cloud per key do not serve: a single tile, clouds that are no multiple of 64 points or do not
    # divide the rows, ragged channels
    for cid, ch in (("R-64", {0: 64}), ("npts-32", {3: 32}), ("npts-96", {0: 192, 3: 96}), ("R-no-multiple-of-npts", {0: 192, 3: 128}),
                    ("R-no-multiple-of-64", {0: 160, 3: 160}), ("Co-96", {2: 96}), ("Ci-40", {1: 40})):
        add(cid, tile, ch, "needs 64-aligned rows per cloud / channels", UNSUP)
    # the wide entry: fewer than 128 row blocks, rows that are no multiple of 128 / of the cloud, clouds that are no multiple of 32
    # points, an input width other than 64 / 128, fewer than 512 or ragged output channels; a size below 1 is such a shape
    for cid, ch in (("R-16256", {0: 16256}), ("R-16448", {0: 16448}), ("R-no-multiple-of-npts", {3: 96}), ("npts-16", {3: 16}),
                    ("npts-48", {0: 16512, 3: 48}), ("Ci-32", {1: 32}), ("Ci-192", {1: 192}), ("Co-448", {2: 448}), ("Co-544", {2: 544}),
                    ("R-negative", {0: -1}), ("Ci-zero", {1: 0}), ("Co-negative", {2: -1}), ("npts-zero", {3: 0}), ("npts-negative", {3: -32})):
        add(cid, wide, ch, "needs R % 128 == 0", UNSUP)
    add("R-16256-with-null-W", wide, {0: 16256, 6: None})  # (a NULL operand is BAD whatever the shape)
    for pos in (0, 1, 2, 3):
        for v in (0, -1):
            add("size%d-is-%d" % (pos, v), sparse, {pos: v}, "at most 256 points per cloud", UNSUP)
    add("npts-257", sparse, {1: 257}, "at most 256 points per cloud", UNSUP)
    add("npts-257-with-null-g", sparse, {1: 257, 4: None})
    for name in (nf, nb):
        add("R-zero", name, {0: 0})
        add("R-negative", name, {0: -1})
    # z1..z3 of the forward: all three (a backward will read them) or none
    for cid, ch in (("z1-alone", {12: Pp}), ("z2-alone", {13: Pp}), ("z3-alone", {14: Pp}), ("z1-z2", {12: Pp, 13: Pp}), ("z2-z3", {13: Pp, 14: Pp}),
                    ("z1-z3", {12: Pp, 14: Pp})):
        add(cid, nf, ch, "all three or none")
    return out


def _skinny_cases():
    out = []
    for name, (base, required) in SKINNY.items():
        for pos in required:
            out.append(("%s-arg%d-null" % (name, pos), name, _with(name, {pos: None}), BAD, name))
        for pos, vals in ((0, (0, 129, -1)), (1, (0, -1)), (2, (0, -1))):
            for v in vals:
                out.append(("%s-size%d-is-%d" % (name, pos, v), name, _with(name, {pos: v}), UNSUP, name))
    two = "sn_skinny_linear2"
    for cid, ch in (("x2-with-gate", {4: Pp, 5: 8, 6: Pp}), ("ksplit-12", {4: Pp, 5: 12}), ("ksplit-0", {4: Pp, 5: 0}),
                    ("ksplit-K", {4: Pp, 5: 64}), ("ksplit-negative", {4: Pp, 5: -8}), ("ksplit-past-K", {4: Pp, 5: 72}),
                    ("nsplit-negative", {13: -1}), ("nsplit-N", {12: Pp, 13: 40}), ("nsplit-past-N", {12: Pp, 13: 41}),
                    ("nsplit0-out-null", {11: None, 12: Pp}), ("nsplit-both-outputs-null", {11: None, 12: None, 13: 8})):
        out.append((two + "-" + cid, two, _with(two, {**ch}), BAD, two))
    # the documented precedence: a size that is not served is UNSUPPORTED whatever the splits; a NULL operand is BAD whatever the size
    out.append((two + "-R129-with-bad-ksplit", two, _with(two, {0: 129, 4: Pp, 5: 12}), UNSUP, two))
    out.append((two + "-R129-with-bad-nsplit", two, _with(two, {0: 129, 13: -1}), UNSUP, two))
    out.append((two + "-R129-with-null-W", two, _with(two, {0: 129, 7: None}), BAD, two))
    wg = "sn_skinny_wgrad"
    for cid, ch in (("R0", {0: 0}), ("R257", {0: 257}), ("K0", {1: 0}), ("N0", {2: 0}), ("ksplit-0", {4: Pp, 5: 0}),
                    ("ksplit-K", {4: Pp, 5: 8}), ("ksplit-negative", {4: Pp, 5: -1})):
        out.append((wg + "-" + cid, wg, _with(wg, ch), BAD, wg))
    return out


def _task_batch_cases():
    out = []
    add = lambda cid, name, ch, text=None: out.append(("%s-%s" % (name, cid), name, _with(name, ch), BAD, text or name))
    for name, (base, sizes, required) in TASK_BATCH.items():
        for pos in sizes:  # (these take every size >= 1: no empty case documented)
            add("size%d-zero" % pos, name, {pos: 0})
    for name, ppos in (("sn_cyclic_pad_cat", 5), ("sn_cyclic_pad_cat_backward", 6)):
        # 17 clouds: refused before either host array is read (they hold one element)
        add("nclouds17", name, {3: 17})
        add("a-size-of-0", name, {4: [HOSTI, 0]}, "cloud size outside [1, len]")
        add("a-size-above-len", name, {4: [HOSTI, 9]}, "cloud size outside [1, len]")
        add("the-second-size-above-len", name, {3: 2, 4: [HOSTI, 8, 9], ppos: [HOSTP, 4096, 4096]}, "cloud size outside [1, len]")
    add("a-null-cloud", "sn_cyclic_pad_cat", {5: [HOSTP, 0]})  # (forward: every cloud is read; backward: NULL = no gradient wanted)
    add("the-second-cloud-null", "sn_cyclic_pad_cat", {3: 2, 4: [HOSTI, 4, 4], 5: [HOSTP, 4096, 0]})
    fv = "sn_chamfer_forward_valid"
    add("n2049", fv, {3: 2049}, "2048")
    add("m2049-n2049", fv, {1: 2049, 3: 2049}, "2048")
    add("m-above-n", fv, {1: 9}, "m <= n")
    add("q_group-of-0-with-B1", fv, {0: 1, 6: 0})
    hb = "sn_pcrnet_head_rot_backward"
    add("grad_v-without-grad_out", hb, {9: Pp}, "grad_v needs grad_out")
    for name in ("sn_pcrnet_head_rot_forward_grouped", "sn_pcrnet_head_rot_backward_grouped"):
        add("R-no-multiple-of-group", name, {2: 3})
        add("group-above-R", name, {2: 8})
    lf, lb = "sn_chamfer_mean_loss_forward_grouped", "sn_chamfer_mean_loss_backward_grouped"
    for name, gpos in ((lf, 3), (lb, 5)):  # (R, n1 first in both; group, nev, nvalid at gpos, gpos + 1, gpos + 2)
        add("nev17", name, {0: 34, gpos + 1: 17}, "at most 16 evaluations")  # (R = nev * group holds: the count alone is refused)
        add("R-is-not-nev-times-group", name, {0: 3}, "R = nev * group")
        add("R-is-not-nev-times-group-2", name, {0: 4, gpos: 2, gpos + 1: 1}, "R = nev * group")
        add("R-no-multiple-of-group", name, {0: 3, gpos: 2, gpos + 1: 2, gpos + 2: [HOSTI, 4, 4]}, "R = nev * group")
        add("nvalid-0", name, {gpos + 2: [HOSTI, 0]}, "valid points outside [1, n1]")
        add("nvalid-n1-plus-1", name, {gpos + 2: [HOSTI, 5]}, "valid points outside [1, n1]")
        add("nvalid-negative", name, {gpos + 2: [HOSTI, -1]}, "valid points outside [1, n1]")
        add("the-last-nvalid-n1-plus-1", name, {0: 6, gpos + 1: 3, gpos + 2: [HOSTI, 4, 1, 5]}, "valid points outside [1, n1]")
    add("n1-2049", lb, {1: 2049}, "2048")
    add("n2-2049", lb, {3: 2049}, "2048")
    return out


def _step_loss_cases():
    out = []
    add = lambda cid, name, ch, text=None, code=BAD: out.append(("%s-%s" % (name, cid), name, _with(name, ch), code, text or name))
    for name, (base, sizes, required) in STEP_LOSS.items():
        for pos in sizes:
            add("size%d-negative" % pos, name, {pos: -1})
            add("size%d-zero" % pos, name, {pos: 0})
        for pos in required:
            add("arg%d-null" % pos, name, {pos: None})
    scans = ("sn_pairscan_forward_partial", "sn_pairscan_forward_partial_fc", "sn_pairscan_forward_keys")
    for name in scans + ("sn_sampler_step_loss_backward", "sn_sampler_step_loss_keys"):
        add("K65", name, {1: 100, 3: 65})
        for bad in (2, -1):
            add("p_layout-is-%d" % bad, name, {5: bad})
    for name in scans:
        add("K-above-N", name, {3: 9})
    for bad in (2, -1):
        add("q_layout-is-%d" % bad, scans[0], {7: bad})
    # the layout refusal: the backward entries take the reference cloud as (B,N,3) only
    for name in ("sn_sampler_step_loss_backward", "sn_sampler_step_loss_keys"):
        add("P-channel-major", name, {5: 1}, "(B,N,3)")
    add("deferred_loss-without-partials", "sn_sampler_step_loss_backward", {21: Pp}, "deferred")
    add("N2049", "sn_sampler_step_loss_keys", {1: 2049}, "N <= 2048", UNSUP)
    # Kfc: a multiple of 4, at least 4
    for kfc in (0, 2, 6, 261):
        add("Kfc%d" % kfc, scans[1], {11: kfc}, "multiple of 4")
        add("Kfc%d" % kfc, scans[2], {7: Pp, 8: Pp, 9: Pp, 10: Pp, 11: Pp, 12: kfc}, "bad fc operands")
    for pos in (7, 8, 9, 11):
        add("fc_w-without-arg%d" % pos, scans[2], {**{q: Pp for q in (7, 8, 9, 10, 11)}, 12: 8, pos: None}, "bad fc operands")
    # the partial scans check the workspace before any device work (these bases spread a cloud over 3 workgroups: 2 * 3 * 8 keys)
    for name, pos in ((scans[0], 16), (scans[1], 21)):
        add("workspace-one-byte-short", name, {pos: 2 * 3 * 8 * 8 - 1}, "workspace too small")
        add("workspace-of-0-bytes", name, {pos: 0}, "workspace too small")
    # a shape that runs as one workgroup per cloud is UNSUPPORTED, whatever the workspace
    for name in scans:
        add("one-workgroup-per-cloud", name, {2: 4}, "one workgroup per cloud", UNSUP)
    add("simp_bnc-without-y_bcn", "sn_surface_values_keys", {11: Pp})
    return out


def _fc_chain_cases():
    out = []
    add = lambda cid, name, ch, text=None, code=BAD: out.append(("%s-%s" % (name, cid), name, _with(name, ch), code, text or name))
    for name, (base, required, arrays) in FC_CHAIN.items():
        for pos in required:
            add("arg%d-null" % pos, name, {pos: None})
        for pos in arrays:  # a NULL inside a per-layer / per-stage host array, in its last place
            add("arg%d-holds-a-null" % pos, name, {pos: base[pos][:-1] + [0]}, "null layer pointer" if "forward" in name else "null stage pointer")
        for r in (0, -1, 33):
            add("rows-%d" % r, name, {0: r})
    fw, fp, fo, bw, bo = FC_CHAIN
    for cid, ch in (("C0-96", {1: 96}), ("C0-512", {1: 512}), ("H-128", {2: 128}), ("nl-1", {3: 1}), ("nl-5", {3: 5}),
                    ("nl-4-needs-too-much-LDS", {3: 4})):
        add(cid, fw, ch, "shape not supported", UNSUP)
    for name in (fp, fo):
        for cid, ch in (("N-32", {1: 32}), ("N-96", {1: 96}), ("H-128", {17: 128}), ("nl-2", {18: 2})):
            add(cid, name, ch, "shape not supported", UNSUP)
        add("N-negative", name, {1: -1})
        add("nconv-1", name, {2: 1})
    for co in (0, 16, 48, 288):
        add("Co-%d" % co, fo, {32: co}, "shape not supported", UNSUP)
    # running_mean[l] given while running_var[l] is NULL: the kernel would read through the NULL
    for name, (rm, rv) in ((fw, (9, 10)), (fp, (23, 24)), (fo, (23, 24))):
        n = len(FC_CHAIN[name][0][rm - 4]) - 1  # (the W array sits four places in front: as many layers)
        full, last_null, only_last = [HOSTP] + [4096] * n, [HOSTP] + [4096] * (n - 1) + [0], [HOSTP] + [0] * (n - 1) + [4096]
        add("running_mean-without-the-running_var-array", name, {rm: full}, "running_mean without running_var")
        add("running_mean-with-a-null-running_var", name, {rm: full, rv: last_null}, "running_mean without running_var")
        add("the-last-running_mean-alone", name, {rm: only_last, rv: last_null}, "running_mean without running_var")
    add("running_mean_o-without-running_var_o", fo, {37: Pp}, "running_mean without running_var")
    for name in (bw, bo):
        for cid, ch in (("Co-96", {2: [HOSTI, 96, 256]}), ("Co-320", {2: [HOSTI, 320, 256]}), ("Ci-48", {3: [HOSTI, 256, 48]}),
                        ("Ci-288", {3: [HOSTI, 256, 288]}), ("inner-Ci-128", {2: [HOSTI, 256, 128], 3: [HOSTI, 128, 128]}),
                        ("Co-is-not-the-Ci-above", {2: [HOSTI, 256, 128]}), ("ns-1", {1: 1}), ("ns-6", {1: 6}), ("ns-negative", {1: -1})):
            add(cid, name, ch, "shape not supported", UNSUP)
    return out


def _mlp_cases():
    out = []
    add = lambda cid, name, ch, text=None, code=BAD: out.append(("%s-%s" % (name, cid), name, _with(name, ch), code, text or name))
    for name, (base, sizes, required) in MLP.items():
        for pos in sizes:
            add("size%d-negative" % pos, name, {pos: -1})
            add("size%d-zero" % pos, name, {pos: 0})
        for pos in required:
            add("arg%d-null" % pos, name, {pos: None})
    for name in ("sn_linear_dgrad", "sn_linear_wgrad", "sn_linear_backward", "sn_layer_backward"):
        for bad in (-1, 3):
            add("dz_mode-is-%d" % bad, name, {3: bad}, "bad dz_mode")
    cp, lb = "sn_conv_backward_partials", "sn_layer_backward"
    for bad in (-1, 0, 3):  # (the fused kernel serves the BatchNorm and the pool form only)
        add("dz_mode-is-%d" % bad, cp, {3: bad}, "bad dz_mode")
    add("pool-without-gsel", cp, {3: 2, 8: Pp}, "missing gradient source")
    add("pool-without-argsel", cp, {3: 2, 7: Pp}, "missing gradient source")
    # shapes the fused backward kernel does not serve: fewer than 256 rows, other channel counts, a pool over clouds that are no
    # multiple of 64 points
    for cid, ch in (("R-255", {0: 255}), ("R-64", {0: 64}), ("Ci-192", {1: 192}), ("Ci-128-Co-64", {1: 128}), ("Co-40", {2: 40}),
                    ("pool-npts-48", {3: 2, 7: Pp, 8: Pp, 9: 48}), ("pool-npts-0", {3: 2, 7: Pp, 8: Pp, 9: 0})):
        add(cid, cp, ch, "shape not served by the fused kernel", UNSUP)
    fp = "sn_conv_forward_bn_pool"
    for cid, ch in (("R-64", {0: 64}), ("R-130", {0: 130}), ("npts-32", {3: 32}), ("npts-96", {0: 192, 3: 96}), ("R-no-multiple-of-npts", {0: 192, 3: 128}),
                    ("Co-96", {2: 96}), ("Ci-40", {1: 40})):
        add(cid, fp, ch, "needs 64-aligned rows / points / channels", UNSUP)
    # the layer below has a BatchNorm (coef_prev): its outputs are required, the statistics scratch above 32 rows only
    with_bn = {12: Pp, 14: Pp, 18: Pp, 19: Pp, 21: Pp}
    for cid, pos in (("prev_dgamma", 18), ("prev_dbeta", 19), ("prev_kcoef", 21), ("stats", 14)):
        add("coef_prev-without-" + cid, lb, {**with_bn, pos: None}, "previous-layer BatchNorm outputs missing")
    add("coef_prev-without-prev_dgamma-at-32-rows", lb, {**with_bn, 0: 32, 14: None, 18: None}, "previous-layer BatchNorm outputs missing")
    add("prev_bn_rows-at-33-rows", lb, {0: 33, 22: 5}, "prev_bn_rows > 0")
    add("prev_bn_rows-at-64-rows-with-coef_prev", lb, {**with_bn, 22: 4096}, "prev_bn_rows > 0")
    add("no-scratch-above-32-rows", lb, {0: 33, 15: None}, "scratch missing")
    in3 = "sn_layer_backward_in3"
    for cid, ch in (("R-255", {0: 255}), ("Ci-128", {1: 128}), ("Co-128", {2: 128})):
        add(cid, in3, ch, "shape not supported by the input-layer variant")
    return out


def _transform_cases(nulled):
    out = []
    tf, tb, of, ob = "sn_cloud_transform_forward", "sn_cloud_transform_backward", "sn_orthogonality_loss_forward", "sn_orthogonality_loss_backward"
    for name, kpos in ((tf, 2), (tb, 2), (of, 1), (ob, 1)):
        for k in (0, 1, 2, 4, 63, 65):
            out.append(("%s-K%d" % (name, k), name, _with(name, {kpos: k}), BAD, "K must be 3 or 64"))
    # B > 65535: the transform kernels put the cloud on the grid's second dimension, which ends there; the orthogonality kernels put it on
    # the first and document no such limit, so there is no such case for them
    for name in (tf, tb):
        out.append((name + "-B65536", name, _with(name, {0: 65536}), BAD, "65535"))
    # sn_cloud_transform_backward: an output's other operand is required only with that output
    out.append((tb + "-dX-without-T", tb, _with(tb, {4: None, 7: None}), BAD, tb))
    out.append((tb + "-dT-without-X", tb, _with(tb, {3: None, 6: None}), BAD, tb))
    out.append((tb + "-no-output-checks-dY", tb, _with(tb, {5: None, 6: None, 7: None}), BAD, tb))
    out.append((tb + "-no-output-launches-nothing", tb, _with(tb, {3: None, 4: None, 6: None, 7: None}), 0, None))
    for name in ("sn_bn_relu_forward", "sn_bn_relu_backward"):
        out.append((name + "-R-negative", name, _with(name, {0: -1}), BAD, name))
        for c in (1, 2, 6, 63):
            out.append(("%s-C%d" % (name, c), name, _with(name, {1: c}), BAD, "multiple of 4"))
    for name, ch in ((tf, {0: 0}), (tf, {1: 0}), (tb, {0: 0}), (of, {0: 0}), (ob, {0: 0}), ("sn_bn_relu_forward", {0: 0}),
                     ("sn_bn_relu_forward", {1: 0}), ("sn_bn_relu_backward", {0: 0}), ("sn_bn_relu_backward", {1: 0})):
        out.append(("%s-empty-%s" % (name, "".join("%d" % p for p in ch)), name, nulled(name, ch), 0, None))
    return out


CASES = _cases()
IN_SCOPE = sorted(ENTRIES) + sorted(INTERNAL) + sorted(TASK_BATCH) + sorted(STEP_LOSS) + sorted(SKINNY) + sorted(FC_CHAIN) + sorted(MLP) + ["sn_pairscan_workspace_bytes", "sn_soft_bwd_splits", "sn_skinny_linear_supported",
                                               "sn_skinny_linear_scratch_bytes"] + sorted(TASK_NET) + [
                                                   "sn_linear_forward_maxpool_wide_supported", "sn_linear_forward_maxpool_wide_scratch_bytes"]


@pytest.fixture(scope="module")
def results():
    return run_cases(CASES)


def test_the_table_walks_every_entry_in_scope():
    from samplenet_amd import _lib

    for name, (base, sizes, required) in list(ENTRIES.items()) + list(INTERNAL.items()) + list(TASK_BATCH.items()) + list(STEP_LOSS.items()) + list(MLP.items()):
        proto = _lib.PROTOTYPES[name]
        assert len(base) == len(proto), name
        for pos, ty in enumerate(proto):
            if pos in sizes:
                assert ty is ctypes.c_int, (name, pos)
            if pos in required or base[pos] in (Pp, HOSTI, HOSTP):
                assert ty is ctypes.c_void_p, (name, pos)
            if ty is ctypes.c_void_p:
                assert base[pos] in (Pp, HOSTI, HOSTP, None), (name, pos)
    for name, (base, required) in SKINNY.items():
        proto = _lib.PROTOTYPES[name]
        assert len(base) == len(proto) and proto[:3] == [ctypes.c_int] * 3, name
        for pos, ty in enumerate(proto):
            assert (ty is ctypes.c_void_p) == (base[pos] in (Pp, None)), (name, pos)
            assert pos not in required or base[pos] == Pp, (name, pos)
    for name, (base, required) in TASK_NET.items():
        proto = _lib.PROTOTYPES[name]
        assert len(base) == len(proto), name
        for pos, ty in enumerate(proto[:-1]):  # (the last is the stream)
            assert (ty is ctypes.c_void_p) == (base[pos] in (Pp, None)), (name, pos)
            assert (pos in required) == (base[pos] == Pp), (name, pos)
    for name, (base, required, arrays) in FC_CHAIN.items():
        proto = _lib.PROTOTYPES[name]
        assert len(base) == len(proto) and set(arrays) <= set(required), name
        for pos, ty in enumerate(proto):
            is_ptr = base[pos] is None or base[pos] == Pp or isinstance(base[pos], list)
            assert (ty is ctypes.c_void_p) == is_ptr, (name, pos)
            assert pos not in required or base[pos] is not None, (name, pos)
            assert pos not in arrays or base[pos][0] == HOSTP, (name, pos)
    assert not [n for n in IN_SCOPE if n not in _lib.PROTOTYPES]
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_table(results, case):
    check_case(results, case)


def test_size_queries():
    """sn_pairscan_workspace_bytes / sn_soft_bwd_splits are pure host functions: the documented shape of their answers."""
    from samplenet_amd._lib import lib

    assert lib.sn_pairscan_workspace_bytes(32, 4100, 64) == 0  # the multi-chunk scan takes no scratch
    assert lib.sn_pairscan_workspace_bytes(1024, 1024, 64) == 0  # the batch alone fills the chip: one workgroup per cloud
    for B, N, M in ((1, 1, 1), (1, 64, 64), (32, 1024, 64), (17, 2048, 2100), (512, 1024, 64), (513, 1024, 64)):
        wb = lib.sn_pairscan_workspace_bytes(B, N, M)
        assert wb >= 0 and wb % 8 == 0 and wb <= 8 * B * N * min(M, 512)
    assert lib.sn_pairscan_workspace_bytes(32, 1024, 64) == 32 * 16 * 1024 * 8
    for b, m in ((1, 1), (1, 64), (32, 64), (2048, 64), (1, 5000), (0, 4)):
        s = lib.sn_soft_bwd_splits(b, m)
        assert 1 <= s <= max(1, (m + 3) // 4)
    assert lib.sn_soft_bwd_splits(32, 64) == 16 and lib.sn_soft_bwd_splits(1, 64) == 16 and lib.sn_soft_bwd_splits(2048, 64) == 1


# (K, N) -> K slices of csrc/task_network.hip's skinny_plan, evaluated by hand: one slice, scalar and vector operand loads, partial
# batches of the eight-at-a-time slice sum (9, 17, 25), slices of 2 and 4 k-steps (584, 1024, 2048, 4096)
SKINNY_SLICES = {(1, 1): 1, (7, 5): 1, (61, 33): 1, (64, 7): 1, (72, 40): 2, (130, 100): 3, (200, 64): 4, (576, 33): 9, (584, 70): 5,
                 (1088, 20): 17, (1600, 3): 25, (1024, 512): 8, (2048, 1024): 8, (4096, 64): 16}


def test_skinny_size_queries():
    """sn_skinny_linear_supported / _scratch_bytes are pure host functions: 1..128 rows, K and N at least 1; the scratch is
    slices x 32-column tiles x row tiles (1, 2 or 4 tiles of 32 rows) x 4096 bytes."""
    from samplenet_amd._lib import lib

    for R, K, N, ok in ((1, 1, 1, 1), (128, 4096, 6144, 1), (0, 8, 8, 0), (129, 8, 8, 0), (-1, 8, 8, 0), (4, 0, 8, 0), (4, 8, 0, 0),
                        (4, -1, 8, 0), (4, 8, -1, 0)):
        assert lib.sn_skinny_linear_supported(R, K, N) == ok, (R, K, N)
    for (K, N), slices in SKINNY_SLICES.items():
        for R in (1, 5, 31, 32, 33, 64, 65, 97, 128):
            rt = 1 if R <= 32 else 2 if R <= 64 else 4
            assert lib.sn_skinny_linear_scratch_bytes(R, K, N) == slices * ((N + 31) // 32) * rt * 4096, (R, K, N)

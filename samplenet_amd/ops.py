"""Functional layer: torch.autograd.Functions over the C ABI of libsamplenet_hip.so.

Host-side plumbing only -- allocation of outputs with torch, stream / device selection, autograd
bookkeeping.  All arithmetic happens in the HIP kernels (samplenet_amd/csrc).  Every function
requires CUDA(HIP) tensors and raises otherwise: there is no CPU path in the product.
"""
from typing import NamedTuple

import torch

from ._lib import check, lib, ptr, stream_of

BNC, BCN = 0, 1  # SN_LAYOUT_*


def _stream(t):
    return stream_of(t)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("samplenet_amd ops run on the GPU only (got a %s tensor); no CPU fallback exists" % t.device)


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    return t.contiguous()


# --------------------------------------------------------------------------------------------- Chamfer
def chamfer_forward_impl(xyz1, xyz2):
    """xyz1 (B,n,3), xyz2 (B,m,3) -> contiguous inputs, dist1 (B,n), idx1, dist2 (B,m), idx2 (one launch)."""
    _need_gpu(xyz1, xyz2)
    xyz1, xyz2 = _f32c(xyz1), _f32c(xyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dist1 = torch.empty(b, n, device=xyz1.device, dtype=torch.float32)
    dist2 = torch.empty(b, m, device=xyz1.device, dtype=torch.float32)
    idx1 = torch.empty(b, n, device=xyz1.device, dtype=torch.int32)
    idx2 = torch.empty(b, m, device=xyz1.device, dtype=torch.int32)
    with torch.cuda.device(xyz1.device):
        # sn_chamfer_forward's own role choice (lanes own the larger set), through the workspace form of the scan: with
        # scratch for partial per-point minima the queries of a cloud spread over several workgroups -- at small batches the
        # plain launcher signature (no scratch argument, as the reference's) leaves one workgroup per cloud: 32 of 256 CUs
        if m >= n:
            N, M, P, Q, dq, iq, dp, ip = m, n, xyz2, xyz1, dist1, idx1, dist2, idx2
        else:
            N, M, P, Q, dq, iq, dp, ip = n, m, xyz1, xyz2, dist2, idx2, dist1, idx1
        wsb = lib.sn_pairscan_workspace_bytes(b, N, M) if (b > 0 and N > 0 and M > 0) else 0
        if wsb > 0:
            ws = torch.empty(wsb // 8, device=xyz1.device, dtype=torch.int64)
            check(lib.sn_pairscan_forward_ws(b, N, M, 0, ptr(P), BNC, ptr(Q), BNC, None, None, ptr(dq), ptr(iq), ptr(dp), ptr(ip),
                                             None, 0, None, None, 0.0, ptr(ws), wsb, _stream(xyz1)), "sn_pairscan_forward_ws")
        else:
            check(lib.sn_chamfer_forward(b, n, ptr(xyz1), m, ptr(xyz2), ptr(dist1), ptr(idx1), ptr(dist2), ptr(idx2),
                                         _stream(xyz1)), "sn_chamfer_forward")
    return xyz1, xyz2, dist1, idx1, dist2, idx2


def chamfer_backward_impl(xyz1, xyz2, idx1, idx2, graddist1, graddist2, need1=True, need2=True):
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    graddist1, graddist2 = graddist1.contiguous(), graddist2.contiguous()
    g1 = torch.empty_like(xyz1) if need1 else None
    g2 = torch.empty_like(xyz2) if need2 else None
    with torch.cuda.device(xyz1.device):
        check(lib.sn_chamfer_backward(b, n, ptr(xyz1), m, ptr(xyz2), ptr(graddist1), ptr(idx1), ptr(graddist2),
                                      ptr(idx2), ptr(g1), ptr(g2), _stream(xyz1)), "sn_chamfer_backward")
    return g1, g2


class ChamferDistanceFunction(torch.autograd.Function):
    """Four-output form: dist1 (B,n), dist2 (B,m), idx1, idx2 (indices non-differentiable)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1, xyz2, dist1, idx1, dist2, idx2 = chamfer_forward_impl(xyz1, xyz2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, graddist1, graddist2, _gi1, _gi2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        return chamfer_backward_impl(xyz1, xyz2, idx1, idx2, graddist1, graddist2, ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1])


class ChamferMeanLossFunction(torch.autograd.Function):
    """mean(dist1) + mean(dist2) of (xyz1, xyz2) as ONE differentiable scalar -- the Chamfer term of the registration task loss
    (registration/main.py:573-577): scan, fused reduction, and a backward with implicit upstream gradients (no per-point
    gradient tensors, no mean / add / expand / div launches)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1, xyz2, dist1, idx1, dist2, idx2 = chamfer_forward_impl(xyz1, xyz2)
        B, n1 = dist1.shape
        n2 = dist2.shape[1]
        dev = dist1.device
        partial = torch.empty(B * 3, device=dev, dtype=torch.float32)
        argmax1 = torch.empty(B, device=dev, dtype=torch.int32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            check(lib.sn_chamfer_mean_loss_forward(B, n1, n2, ptr(dist1), ptr(dist2), ptr(partial), ptr(argmax1), ptr(loss),
                                                   _stream(dist1)), "sn_chamfer_mean_loss_forward")
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        B, n1, _ = xyz1.shape
        n2 = xyz2.shape[1]
        g1 = torch.empty_like(xyz1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(xyz2) if ctx.needs_input_grad[1] else None
        gl = grad_loss.contiguous().float()
        with torch.cuda.device(xyz1.device):
            check(lib.sn_chamfer_mean_loss_backward(B, n1, ptr(xyz1), n2, ptr(xyz2), ptr(idx1), ptr(idx2), ptr(gl), ptr(g1), ptr(g2),
                                                    _stream(xyz1)), "sn_chamfer_mean_loss_backward")
        return g1, g2


_QVALID = {}  # (n1, n2, valid counts, device) -> the counts on the device (made outside captures; constants of the graphs that use them)


class ChamferMeanLossGroupedFunction(torch.autograd.Function):
    """chamfer_mean_loss for E evaluations in one batch: xyz1 (E G, n1, 3) clouds padded to n1 points by cyclic_pad_cat, nvalid[e] real
    points in evaluation e's G clouds; xyz2 (E G, n2, 3) -> losses (E,), each equal -- bit for bit, gradients included -- to
    chamfer_mean_loss(xyz1[e G:(e+1) G, :nvalid[e]], xyz2[e G:(e+1) G]).  One scan + two reduction launches forward, two backward."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, group, nvalid):
        import ctypes

        _need_gpu(xyz1, xyz2)
        n1, n2, R = xyz1.shape[1], xyz2.shape[1], xyz1.shape[0]
        key = (n1, n2, tuple(int(v) for v in nvalid), xyz1.device)
        qv = _QVALID.get(key)
        if qv is None and n1 <= n2 <= 2048 and not torch.cuda.is_current_stream_capturing():
            qv = _QVALID[key] = torch.tensor(list(key[2]), device=xyz1.device, dtype=torch.int32)
        if qv is not None:
            # the scan walks the valid queries only (the copies' own products are read by nobody)
            xyz1, xyz2 = _f32c(xyz1), _f32c(xyz2)
            dev = xyz1.device
            dist1 = torch.empty(R, n1, device=dev, dtype=torch.float32)
            dist2 = torch.empty(R, n2, device=dev, dtype=torch.float32)
            idx1 = torch.empty(R, n1, device=dev, dtype=torch.int32)
            idx2 = torch.empty(R, n2, device=dev, dtype=torch.int32)
            wsb = lib.sn_pairscan_workspace_bytes(R, n2, n1)
            ws = torch.empty(max(wsb, 8) // 8, device=dev, dtype=torch.int64)
            with torch.cuda.device(dev):
                check(lib.sn_chamfer_forward_valid(R, n1, ptr(xyz1), n2, ptr(xyz2), ptr(qv), int(group), ptr(dist1), ptr(idx1), ptr(dist2),
                                                   ptr(idx2), ptr(ws), wsb, _stream(xyz1)), "sn_chamfer_forward_valid")
        else:
            xyz1, xyz2, dist1, idx1, dist2, idx2 = chamfer_forward_impl(xyz1, xyz2)
        E = len(nvalid)
        dev = dist1.device
        partial = torch.empty(R * 2, device=dev, dtype=torch.float32)
        loss = torch.empty(E, device=dev, dtype=torch.float32)
        nv = (ctypes.c_int * E)(*[int(v) for v in nvalid])
        with torch.cuda.device(dev):
            check(lib.sn_chamfer_mean_loss_forward_grouped(R, n1, n2, int(group), E, nv, ptr(dist1), ptr(dist2), ptr(partial), ptr(loss),
                                                           _stream(dist1)), "sn_chamfer_mean_loss_forward_grouped")
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.cfg = (int(group), E, nv)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        group, E, nv = ctx.cfg
        R, n1, _ = xyz1.shape
        n2 = xyz2.shape[1]
        g1 = torch.empty_like(xyz1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(xyz2) if ctx.needs_input_grad[1] else None
        gl = grad_loss.contiguous().float()
        with torch.cuda.device(xyz1.device):
            check(lib.sn_chamfer_mean_loss_backward_grouped(R, n1, ptr(xyz1), n2, ptr(xyz2), group, E, nv, ptr(idx1), ptr(idx2), ptr(gl),
                                                            ptr(g1), ptr(g2), _stream(xyz1)), "sn_chamfer_mean_loss_backward_grouped")
        return g1, g2, None, None


def chamfer_mean_loss_grouped(xyz1, xyz2, group, nvalid):
    return ChamferMeanLossGroupedFunction.apply(xyz1, xyz2, group, nvalid)


def chamfer_mean_loss(xyz1, xyz2):
    return ChamferMeanLossFunction.apply(xyz1, xyz2)


def chamfer_distance(xyz1, xyz2, return_idx=False):
    d1, d2, i1, i2 = ChamferDistanceFunction.apply(xyz1, xyz2)
    return (d1, d2, i1, i2) if return_idx else (d1, d2)


def prefix_point_minima(ref_pc, samp_pc, sizes):
    """Nearest simplified point of every input point for each nested prefix samp_pc[:, :s] (one launch, no gradient):
    ref_pc (B,N,3), samp_pc (B,M,3), sizes ascending with sizes[-1] == M -> dist (S,B,N) float32, idx (S,B,N) int32."""
    import ctypes

    _need_gpu(ref_pc, samp_pc)
    P, Q = _f32c(ref_pc.detach()), _f32c(samp_pc.detach())
    B, N, _ = P.shape
    M = Q.shape[1]
    S = len(sizes)
    dist = torch.empty(S, B, N, device=P.device, dtype=torch.float32)
    idx = torch.empty(S, B, N, device=P.device, dtype=torch.int32)
    arr = (ctypes.c_int * S)(*[int(v) for v in sizes])
    with torch.cuda.device(P.device):
        check(lib.sn_prefix_point_minima(B, N, M, S, arr, ptr(P), ptr(Q), ptr(dist), ptr(idx), _stream(P)), "sn_prefix_point_minima")
    return dist, idx


class PrefixPackFunction(torch.autograd.Function):
    """prefixes[j] = t[:, :sizes[j], :] as CONTIGUOUS tensors, all in one launch; backward: the sum of the prefixes' gradients
    (zero-padded), ascending prefix order, in one launch (sn_prefix_pack / sn_prefix_scatter_sum).  t (B, M, C) fp32 / int32."""

    @staticmethod
    def forward(ctx, t, *sizes):
        import ctypes

        _need_gpu(t)
        src = t.contiguous()
        B, M, C = src.shape
        S = len(sizes)
        outs = [torch.empty(B, int(s), C, device=src.device, dtype=src.dtype) for s in sizes]
        with torch.cuda.device(src.device):
            check(lib.sn_prefix_pack(B, M, C, S, (ctypes.c_int * S)(*[int(s) for s in sizes]), ptr(src),
                                     (ctypes.c_void_p * S)(*[ptr(o) for o in outs]), _stream(src)), "sn_prefix_pack")
        ctx.shape, ctx.sizes = (B, M, C), tuple(int(s) for s in sizes)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        import ctypes

        B, M, C = ctx.shape
        S = len(ctx.sizes)
        if all(g is None for g in grads):
            return (None,) * (1 + S)
        gs = [(_f32c(g) if g is not None else None) for g in grads]
        like = next(g for g in gs if g is not None)
        out = torch.empty(B, M, C, device=like.device, dtype=torch.float32)
        with torch.cuda.device(like.device):
            check(lib.sn_prefix_scatter_sum(B, M, C, S, (ctypes.c_int * S)(*ctx.sizes), (ctypes.c_void_p * S)(*[ptr(g) for g in gs]),
                                            ptr(out), _stream(like)), "sn_prefix_scatter_sum")
        return (out,) + (None,) * S


class CyclicPadCatFunction(torch.autograd.Function):
    """clouds (B, s_j, C) of different sizes -> (E B, len, C), every cloud repeated cyclically up to len = max s_j points (one launch
    each way: sn_cyclic_pad_cat / _backward).  For a BatchNorm-free max-pooling extractor the padded batch gives every cloud's features
    unchanged -- E evaluations as one pass."""

    @staticmethod
    def forward(ctx, *clouds):
        import ctypes

        _need_gpu(*clouds)
        cs = [_f32c(c) for c in clouds]
        B, _, C = cs[0].shape
        E = len(cs)
        sizes = [int(c.shape[1]) for c in cs]
        P = max(sizes)
        out = torch.empty(E * B, P, C, device=cs[0].device, dtype=torch.float32)
        with torch.cuda.device(out.device):
            check(lib.sn_cyclic_pad_cat(B, P, C, E, (ctypes.c_int * E)(*sizes), (ctypes.c_void_p * E)(*[ptr(c) for c in cs]), ptr(out),
                                        _stream(out)), "sn_cyclic_pad_cat")
        ctx.cfg = (B, P, C, tuple(sizes))
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes

        B, P, C, sizes = ctx.cfg
        E = len(sizes)
        g = _f32c(g)
        outs = [torch.empty(B, s, C, device=g.device, dtype=torch.float32) if need else None
                for s, need in zip(sizes, ctx.needs_input_grad)]
        with torch.cuda.device(g.device):
            check(lib.sn_cyclic_pad_cat_backward(B, P, C, E, (ctypes.c_int * E)(*sizes), ptr(g),
                                                 (ctypes.c_void_p * E)(*[ptr(o) for o in outs]), _stream(g)), "sn_cyclic_pad_cat_backward")
        return tuple(outs)


def cyclic_pad_cat(clouds):
    return CyclicPadCatFunction.apply(*clouds)


def prefix_pack(t, sizes):
    """[t[:, :s, :].contiguous() for s in sizes] in one launch (and one for the backward).  t (B, M, C) or (B, M): fp32 / int32."""
    if t.dim() == 2:
        return [o.squeeze(2) for o in PrefixPackFunction.apply(t.unsqueeze(2), *sizes)]
    return list(PrefixPackFunction.apply(t, *sizes))


# --------------------------------------------------------------------------------------------- kNN
def knn(k, ref, query, ref_layout=BCN, query_layout=BCN, return_dist=True):
    """K nearest `ref` points of every `query` point (no gradient).

    ref (B,3,N) / query (B,3,M) for BCN, (B,N,3) / (B,M,3) for BNC.
    Returns idx (B,M,K) int32 and squared distances (B,M,K), ascending by (distance, index).
    """
    _need_gpu(ref, query)
    ref, query = _f32c(ref.detach()), _f32c(query.detach())
    B = ref.shape[0]
    N = ref.shape[2] if ref_layout == BCN else ref.shape[1]
    M = query.shape[2] if query_layout == BCN else query.shape[1]
    idx = torch.empty(B, M, k, device=ref.device, dtype=torch.int32)
    dist = torch.empty(B, M, k, device=ref.device, dtype=torch.float32) if return_dist else None
    with torch.cuda.device(ref.device):
        check(lib.sn_knn(B, N, M, k, ptr(ref), ref_layout, ptr(query), query_layout, ptr(idx), ptr(dist), _stream(ref)),
              "sn_knn")
    return idx, dist


def nn_matching(xyz, idx, k, complete_fps=True, layout=BNC):
    """Device-side sputils.nn_matching (sputils.py:31-41): xyz (B,N,3) [BNC] or (B,3,N) [BCN], idx (B,k) -> (B,k,3) float32.
    Same points as the numpy routine (float64 distances, first-maximum argmax, first-occurrence unique)."""
    _need_gpu(xyz, idx)
    xyz = _f32c(xyz.detach())
    idx = idx.detach().reshape(idx.shape[0], -1).contiguous().int()
    B = xyz.shape[0]
    N = xyz.shape[1] if layout == BNC else xyz.shape[2]
    if idx.shape[1] != k:
        raise ValueError("nn_matching: idx must hold k indices per cloud")
    out = torch.empty(B, k, 3, device=xyz.device, dtype=torch.float32)
    with torch.cuda.device(xyz.device):
        check(lib.sn_nn_matching(B, N, k, ptr(xyz), layout, ptr(idx), 1 if complete_fps else 0, ptr(out), _stream(xyz)),
              "sn_nn_matching")
    return out


def nn_matching_indexed(xyz, idx, k, complete_fps=True, layout=BNC):
    """nn_matching with the indices it selected: -> (points (B,k,3) float32, out_idx (B,k) int32, n_unique (B,) int32).
    out_idx: the first occurrences of idx in order, then the farthest-point picks (fps_from_given_indices' idx,
    samplenet_pointnet_ae.py:515-533; idx itself with complete_fps=False); n_unique: the distinct values of idx[b, :]
    (evaluate_samplenet.py:227-228).  points is bit-identical to nn_matching's and equals xyz[out_idx].  One launch."""
    _need_gpu(xyz, idx)
    xyz = _f32c(xyz.detach())
    idx = idx.detach().reshape(idx.shape[0], -1).contiguous().int()
    B = xyz.shape[0]
    N = xyz.shape[1] if layout == BNC else xyz.shape[2]
    if idx.shape[1] != k:
        raise ValueError("nn_matching_indexed: idx must hold k indices per cloud")
    out = torch.empty(B, k, 3, device=xyz.device, dtype=torch.float32)
    out_idx = torch.empty(B, k, device=xyz.device, dtype=torch.int32)
    n_unique = torch.empty(B, device=xyz.device, dtype=torch.int32)
    with torch.cuda.device(xyz.device):
        check(lib.sn_nn_matching_indexed(B, N, k, ptr(xyz), layout, ptr(idx), 1 if complete_fps else 0, ptr(out), ptr(out_idx),
                                         ptr(n_unique), _stream(xyz)), "sn_nn_matching_indexed")
    return out, out_idx, n_unique


def rank_points(xyz, idx, k=None, layout=BNC):
    """A whole cloud re-ordered by importance (the progressive sampler's inference, samplenet_progressive_pointnet_ae.py:490-524,
    546-600): xyz (B,N,3) [BNC] or (B,3,N) [BCN], idx (B,k) nearest input point of every generated point in generation order ->
    (points (B,k,3) float32, order (B,k) int32, n_unique (B,) int32).  order: the distinct values of idx in order of first
    occurrence, then farthest-point picks up to k (float64 distances, first maximum); points = xyz[order]; n_unique: the distinct
    values of idx[b, :].  k defaults to idx's width; N, k <= 8192 (sn_rank_points); every prefix order[:, :s] is the sample of
    size s.  One launch, no synchronisation, no gradient."""
    _need_gpu(xyz, idx)
    xyz = _f32c(xyz.detach())
    idx = idx.detach().reshape(idx.shape[0], -1).contiguous().int()
    B = xyz.shape[0]
    N = xyz.shape[1] if layout == BNC else xyz.shape[2]
    if k is None:
        k = idx.shape[1]
    if idx.shape[1] != k:
        raise ValueError("rank_points: idx must hold k indices per cloud")
    out = torch.empty(B, k, 3, device=xyz.device, dtype=torch.float32)
    order = torch.empty(B, k, device=xyz.device, dtype=torch.int32)
    n_unique = torch.empty(B, device=xyz.device, dtype=torch.int32)
    with torch.cuda.device(xyz.device):
        check(lib.sn_rank_points(B, N, k, ptr(xyz), layout, ptr(idx), None, ptr(out), ptr(order), ptr(n_unique), _stream(xyz)),
              "sn_rank_points")
    return out, order, n_unique


def retrieval_metrics(desc, labels, levels=20, return_order=False):
    """All-against-all retrieval inside one labelled set (sn_retrieval_metrics): desc (n,C) or (S,n,C) float32 descriptors -- S sets
    over the same n shapes --, labels (n,) integers -> (ap (S,n) float32, prec (S,n,levels) float32, n_relevant (n,) int32) and, with
    return_order, (order (S,n,n-1) int32, sorted_dist (S,n,n-1) float32); without the leading S for a 2-D desc.  Every shape queries the
    other n - 1, ranked by squared L2 distance (ties to the lower index); ap: the average precision, prec[l-1]: the precision at
    recall l / levels, both NaN for a query whose label no other shape carries.  n <= 8192, levels <= 64.  One launch, no
    synchronisation, no gradient."""
    _need_gpu(desc, labels)
    desc = _f32c(desc.detach())
    flat = desc.dim() == 2
    if flat:
        desc = desc.unsqueeze(0)
    if desc.dim() != 3:
        raise ValueError("retrieval_metrics: desc must be (n,C) or (S,n,C), got %s" % (tuple(desc.shape),))
    S, n, C = desc.shape
    labels = labels.detach().reshape(-1).contiguous().int()
    if labels.numel() != n:
        raise ValueError("retrieval_metrics: labels must hold one entry per shape")
    levels, m = int(levels), max(n - 1, 0)
    dev = desc.device
    ap = torch.empty(S, n, device=dev, dtype=torch.float32)
    prec = torch.empty(S, n, levels, device=dev, dtype=torch.float32)
    n_relevant = torch.empty(n, device=dev, dtype=torch.int32)
    order = torch.empty(S, n, m, device=dev, dtype=torch.int32) if return_order else None
    sorted_dist = torch.empty(S, n, m, device=dev, dtype=torch.float32) if return_order else None
    wsb = lib.sn_workspace_bytes(b"retrieval_metrics", S, n, C, levels)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8) if wsb > 0 else None
    with torch.cuda.device(dev):
        check(lib.sn_retrieval_metrics(S, n, C, ptr(desc), ptr(labels), levels, ptr(ap), ptr(prec), ptr(n_relevant), ptr(order),
                                       ptr(sorted_dist), ptr(ws), _stream(desc)), "sn_retrieval_metrics")
    out = (ap, prec, n_relevant) + ((order, sorted_dist) if return_order else ())
    return tuple(t[0] if flat and t is not n_relevant else t for t in out)


def furthest_point_sample(xyz, npoint, layout=BNC):
    """Farthest-point sampling (no gradient): xyz (B,N,3) [BNC] or (B,3,N) [BCN] -> idx (B,npoint) int32.

    idx[:, 0] = 0; each later pick is the point farthest from those picked so far (fp32 squared distances, ties to the lowest
    index; include/samplenet_hip.h).  pointnet2_utils.furthest_point_sample (registration/src/fps.py:35) and the TF op
    farthest_point_sample(npoint, inp) (reconstruction/external/sampling/tf_sampling.py:65-75) with layout=BNC."""
    _need_gpu(xyz)
    xyz = _f32c(xyz.detach())
    if xyz.dim() != 3 or xyz.shape[2 if layout == BNC else 1] != 3:
        raise ValueError("furthest_point_sample: xyz must be (B,N,3) for BNC or (B,3,N) for BCN, got %s" % (tuple(xyz.shape),))
    B = xyz.shape[0]
    N = xyz.shape[1] if layout == BNC else xyz.shape[2]
    idx = torch.empty(B, npoint, device=xyz.device, dtype=torch.int32)
    # the running minima live in registers unless the streaming path runs (then B*N floats)
    wsb = lib.sn_workspace_bytes(b"furthest_point_sample", B, N, npoint, 0) if B > 0 and npoint > 0 else 0
    temp = torch.empty(wsb // 4, device=xyz.device, dtype=torch.float32) if wsb > 0 else None
    with torch.cuda.device(xyz.device):
        check(lib.sn_furthest_point_sample(B, N, npoint, ptr(xyz), layout, ptr(temp), ptr(idx), _stream(xyz)),
              "sn_furthest_point_sample")
    return idx


def emd_matching(full_pc, gen_pc):
    """Device-side `emd_matching` of the TF sampler (classification/models/samplenet_model.py:152-167, the same three steps
    as reconstruction/src/samplenet_pointnet_ae.py:111-116): match = approx_match(full_pc, gen_pc) (B,k,N); every generated
    point takes the input point it is matched to most strongly (argmax over the N inputs, first maximum); repeats are
    dropped in first-occurrence order and the set is completed to k points by farthest-point sampling (sn_nn_matching).
    full_pc (B,N,3), gen_pc (B,k,3) -> (B,k,3) points of full_pc.  Nothing leaves the GPU."""
    _need_gpu(full_pc, gen_pc)
    k = gen_pc.shape[1]
    match = approx_match(full_pc, gen_pc)          # (B, k, N)
    idx = torch.argmax(match, dim=2).int()         # first maximum, as tf.argmax / numpy
    return nn_matching(full_pc, idx, k, complete_fps=True)


# --------------------------------------------------------------------------------------------- gather ops
class GroupPointFunction(torch.autograd.Function):
    """points (B,n,c), idx (B,m,ns) int32 -> (B,m,ns,c)   [tf_grouping.py:46-61]"""

    @staticmethod
    def forward(ctx, points, idx):
        _need_gpu(points, idx)
        points, idx = _f32c(points), idx.contiguous().int()
        b, n, c = points.shape
        _, m, ns = idx.shape
        out = torch.empty(b, m, ns, c, device=points.device, dtype=torch.float32)
        with torch.cuda.device(points.device):
            check(lib.sn_group_point(b, n, c, m, ns, ptr(points), ptr(idx), ptr(out), _stream(points)), "sn_group_point")
        ctx.save_for_backward(idx)
        ctx.shape = (b, n, c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        b, n, c = ctx.shape
        _, m, ns = idx.shape
        grad_out = grad_out.contiguous()
        g = torch.empty(b, n, c, device=grad_out.device, dtype=torch.float32)
        with torch.cuda.device(grad_out.device):
            check(lib.sn_group_point_grad(b, n, c, m, ns, ptr(grad_out), ptr(idx), ptr(g), _stream(grad_out)),
                  "sn_group_point_grad")
        return g, None


class GroupingOperationFunction(torch.autograd.Function):
    """features (B,C,N), idx (B,npoint,nsample) int32 -> (B,C,npoint,nsample)   [pointnet2 grouping_operation]"""

    @staticmethod
    def forward(ctx, features, idx):
        _need_gpu(features, idx)
        features, idx = _f32c(features), idx.contiguous().int()
        b, c, n = features.shape
        _, m, ns = idx.shape
        out = torch.empty(b, c, m, ns, device=features.device, dtype=torch.float32)
        with torch.cuda.device(features.device):
            check(lib.sn_grouping_operation(b, c, n, m, ns, ptr(features), ptr(idx), ptr(out), _stream(features)),
                  "sn_grouping_operation")
        ctx.save_for_backward(idx)
        ctx.shape = (b, c, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        b, c, n = ctx.shape
        _, m, ns = idx.shape
        grad_out = grad_out.contiguous()
        g = torch.empty(b, c, n, device=grad_out.device, dtype=torch.float32)
        with torch.cuda.device(grad_out.device):
            check(lib.sn_grouping_operation_grad(b, c, n, m, ns, ptr(grad_out), ptr(idx), ptr(g), _stream(grad_out)),
                  "sn_grouping_operation_grad")
        return g, None


group_point = GroupPointFunction.apply
grouping_operation = GroupingOperationFunction.apply


def gather_operation(features, idx):
    """features (B,C,N), idx (B,npoint) int32 -> (B,C,npoint), differentiable w.r.t. features  [pointnet2 gather_operation,
    registration/src/fps.py:39, random_sampling.py:42]: grouping_operation with one sample per point."""
    return GroupingOperationFunction.apply(features, idx.unsqueeze(-1)).squeeze(-1)


# --------------------------------------------------------------------------------------------- ball query
BALL_RULES = {"sqrt": 0, "squared": 1}  # SN_BALL_RULE_*


def _ball_rule(rule):
    if rule not in BALL_RULES:
        raise ValueError("ball query rule must be 'sqrt' or 'squared', got %r" % (rule,))
    return BALL_RULES[rule]


def ball_query(radius, nsample, xyz, new_xyz, rule="sqrt", layout=BNC, xyz_layout=None):
    """Radius neighbourhoods (no gradient): the FIRST nsample points of `xyz` (ascending index) inside the ball of every point of
    `new_xyz`; short rows repeat their first hit, an empty ball gives a row of zeros with count 0 (sn_ball_query).

    new_xyz (B,M,3) [BNC] or (B,3,M) [BCN] by `layout`; xyz (B,N,3) or (B,3,N) by `xyz_layout` (default: `layout`).
    rule "sqrt": max(sqrt(d2), 1e-20) < radius, the reference's; "squared": d2 < radius * radius (unpinned).
    Returns idx (B,M,nsample) int32 and pts_cnt (B,M) int32."""
    rule = _ball_rule(rule)
    _need_gpu(xyz, new_xyz)
    xyz_layout = layout if xyz_layout is None else xyz_layout
    xyz, new_xyz = _f32c(xyz.detach()), _f32c(new_xyz.detach())
    for t, lay, name in ((xyz, xyz_layout, "xyz"), (new_xyz, layout, "new_xyz")):
        if t.dim() != 3 or t.shape[2 if lay == BNC else 1] != 3:
            raise ValueError("ball_query: %s must be (B,N,3) for BNC or (B,3,N) for BCN, got %s" % (name, tuple(t.shape)))
    B = xyz.shape[0]
    N = xyz.shape[1] if xyz_layout == BNC else xyz.shape[2]
    M = new_xyz.shape[1] if layout == BNC else new_xyz.shape[2]
    idx = torch.empty(B, M, nsample, device=xyz.device, dtype=torch.int32)
    cnt = torch.empty(B, M, device=xyz.device, dtype=torch.int32)
    with torch.cuda.device(xyz.device):
        check(lib.sn_ball_query(B, N, M, float(radius), nsample, rule, ptr(xyz), xyz_layout, ptr(new_xyz), layout, ptr(idx), ptr(cnt),
                                _stream(xyz)), "sn_ball_query")
    return idx, cnt


def query_ball_point(radius, nsample, xyz1, xyz2):
    """The TF op of classification/grouping/tf_grouping.py:13-28: xyz1 (B,N,3) dataset, xyz2 (B,M,3) queries ->
    (idx (B,M,nsample) int32, pts_cnt (B,M) int32), the reference's comparison (rule "sqrt")."""
    return ball_query(radius, nsample, xyz1, xyz2, rule="sqrt", layout=BNC)


class BallGroupFunction(torch.autograd.Function):
    """xyz (B,N,3), new_xyz (B,M,3), features (B,C,N) or None -> out (B, 3 use_xyz + C, M, nsample), idx, pts_cnt: the ball query,
    the two gathers and the centre subtraction in one launch (sn_ball_group_forward); sn_ball_group_backward gives the three gradients."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, radius, nsample, use_xyz, rule):
        _need_gpu(xyz, new_xyz, features)
        xyz, new_xyz = _f32c(xyz), _f32c(new_xyz)
        features = None if features is None else _f32c(features)
        if xyz.dim() != 3 or xyz.shape[2] != 3 or new_xyz.dim() != 3 or new_xyz.shape[2] != 3:
            raise ValueError("ball_group: xyz must be (B,N,3) and new_xyz (B,M,3)")
        b, n, _ = xyz.shape
        m = new_xyz.shape[1]
        c = 0 if features is None else features.shape[1]
        if features is not None and (features.dim() != 3 or features.shape[0] != b or features.shape[2] != n):
            raise ValueError("ball_group: features must be (B,C,N)")
        u = 1 if use_xyz else 0
        out = torch.empty(b, 3 * u + c, m, nsample, device=xyz.device, dtype=torch.float32)
        idx = torch.empty(b, m, nsample, device=xyz.device, dtype=torch.int32)
        cnt = torch.empty(b, m, device=xyz.device, dtype=torch.int32)
        with torch.cuda.device(xyz.device):
            check(lib.sn_ball_group_forward(b, n, m, c, float(radius), nsample, rule, u, ptr(xyz), ptr(new_xyz), ptr(features), ptr(idx),
                                            ptr(cnt), ptr(out), _stream(xyz)), "sn_ball_group_forward")
        ctx.save_for_backward(idx)
        ctx.dims = (b, n, m, c, nsample, u)
        ctx.mark_non_differentiable(idx, cnt)
        return out, idx, cnt

    @staticmethod
    def backward(ctx, grad_out, _gi, _gc):
        (idx,) = ctx.saved_tensors
        b, n, m, c, ns, u = ctx.dims
        grad_out = _f32c(grad_out)
        dev = grad_out.device
        need_xyz, need_new, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and c > 0
        gx = torch.empty(b, n, 3, device=dev, dtype=torch.float32) if need_xyz else None
        gn = torch.empty(b, m, 3, device=dev, dtype=torch.float32) if need_new else None
        gf = torch.empty(b, c, n, device=dev, dtype=torch.float32) if need_f else None
        with torch.cuda.device(dev):
            check(lib.sn_ball_group_backward(b, n, m, c, ns, u, ptr(idx), ptr(grad_out), ptr(gf), ptr(gx), ptr(gn), _stream(grad_out)),
                  "sn_ball_group_backward")
        return gx, gn, gf, None, None, None, None


def ball_group(radius, nsample, xyz, new_xyz, features=None, use_xyz=True, rule="squared", return_idx=False):
    """QueryAndGroup as one differentiable op: xyz (B,N,3), new_xyz (B,M,3), features (B,C,N) or None ->
    (B, 3 use_xyz + C, M, nsample): with use_xyz the first three channels are xyz[idx] - new_xyz, then features[:, :, idx], idx the
    ball query's rows (ops.ball_query).  Gradients reach features, xyz and new_xyz where each requires one (the indices are constants).
    return_idx: also the indices (B,M,nsample) int32 and the counts (B,M) int32."""
    if features is None and not use_xyz:
        raise ValueError("ball_group: nothing to group (features is None and use_xyz is False)")
    out, idx, cnt = BallGroupFunction.apply(xyz, new_xyz, features, radius, nsample, bool(use_xyz), _ball_rule(rule))
    return (out, idx, cnt) if return_idx else out


# --------------------------------------------------------------------------------------------- feature propagation
def _one_device(who, *ts):
    devs = {t.device for t in ts if t is not None}
    if len(devs) > 1:
        raise ValueError("%s: all tensors must live on one device, got %s" % (who, sorted(str(d) for d in devs)))


def _two_clouds(who, unknown, known):
    _one_device(who, unknown, known)
    if unknown.dim() != 3 or unknown.shape[2] != 3 or known.dim() != 3 or known.shape[2] != 3 or known.shape[0] != unknown.shape[0]:
        raise ValueError("%s: unknown must be (B,n,3) and known (B,m,3), got %s and %s" % (who, tuple(unknown.shape), tuple(known.shape)))
    if known.shape[1] == 0 and unknown.shape[0] * unknown.shape[1] > 0:
        raise ValueError("%s: the known cloud is empty" % who)


def three_nn(unknown, known, return_dist2=False):
    """The three nearest `known` points of every `unknown` point (no gradient): unknown (B,n,3), known (B,m,3) ->
    dist (B,n,3), the distances themselves (square roots, as Pointnet2_PyTorch's three_nn returns), and idx (B,n,3) int32,
    ascending by (squared distance, index); with m < 3 the missing slots hold index 0 and an infinite distance (sn_three_nn).
    return_dist2: -> (dist2, idx), the squared distances in place of their roots: what ops.interp_rows reads."""
    _need_gpu(unknown, known)
    unknown, known = _f32c(unknown.detach()), _f32c(known.detach())
    _two_clouds("three_nn", unknown, known)
    b, n, _ = unknown.shape
    dist = torch.empty(b, n, 3, device=unknown.device, dtype=torch.float32)
    idx = torch.empty(b, n, 3, device=unknown.device, dtype=torch.int32)
    d2, d = (dist, None) if return_dist2 else (None, dist)
    with torch.cuda.device(unknown.device):
        check(lib.sn_three_nn(b, n, known.shape[1], ptr(unknown), ptr(known), ptr(d2), ptr(d), ptr(idx), _stream(unknown)), "sn_three_nn")
    return dist, idx


class GatherInverse(NamedTuple):
    """The inverted index of a gather (sn_gather_invert): row r of cloud b is named by the entries order[b, start[b,r] : start[b,r+1]],
    ascending; order is -1 from start[b,-1] on."""
    start: torch.Tensor  # (B, n+1) int32
    order: torch.Tensor  # (B, ne) int32


def gather_invert_supported(n, ne):
    """Whether sn_gather_invert serves n destination rows and ne entries per cloud (ceil(n / 64) * ne <= 2^26)."""
    return 0 <= n < 2 ** 31 and 0 <= ne < 2 ** 31 and bool(lib.sn_gather_invert_supported(n, ne))


def gather_invert(idx, n):
    """idx (B,m,k) or (B,ne), int32 (or int64, converted), naming rows of an n-row destination -> GatherInverse(start, order): per
    destination row the entries e = j*k + t that name it, in ascending order (an index outside [0,n) belongs to no row).  It depends
    on idx alone: build it once for an idx that serves several three_interpolate calls and pass it as their inverse=."""
    _need_gpu(idx)
    if idx.dim() not in (2, 3) or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("gather_invert: idx must be (B,m,k) or (B,ne), int32 or int64, got %s %s" % (tuple(idx.shape), idx.dtype))
    idx = idx.detach().contiguous().int()
    b, ne, n = idx.shape[0], idx.shape[1] * (idx.shape[2] if idx.dim() == 3 else 1), int(n)
    if not gather_invert_supported(n, ne):
        raise ValueError("gather_invert: n = %d rows with %d entries per cloud is beyond sn_gather_invert_supported" % (n, ne))
    if n == 0:  # no row: no entry is valid (the entry itself is a no-op here)
        return GatherInverse(torch.zeros(b, 1, device=idx.device, dtype=torch.int32), torch.full((b, ne), -1, device=idx.device, dtype=torch.int32))
    start = torch.empty(b, n + 1, device=idx.device, dtype=torch.int32)
    order = torch.empty(b, ne, device=idx.device, dtype=torch.int32)
    with torch.cuda.device(idx.device):
        check(lib.sn_gather_invert(b, n, ne, ptr(idx), ptr(start), ptr(order), _stream(idx)), "sn_gather_invert")
    return GatherInverse(start, order)


def _inverse_arg(who, inverse, b, n, ne, like):
    """The inverse= of `who`, checked against b clouds of n destination rows and ne entries on `like`'s device -> (start, order);
    (None, None) for None."""
    if inverse is None:
        return None, None
    start, order = inverse
    if not gather_invert_supported(n, ne):
        raise ValueError("%s: m = %d with %d entries per cloud is beyond sn_gather_invert_supported: no inverse exists "
                         "for it (leave inverse=None for the ordered route)" % (who, n, ne))
    for t, shape, name in ((start, (b, n + 1), "start"), (order, (b, ne), "order")):
        if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("%s: inverse.%s must be contiguous int32 %s (ops.gather_invert(idx, %d)), got %s %s"
                             % (who, name, shape, n, tuple(t.shape), t.dtype))
    _one_device(who, like, start, order)
    return start, order


def _backward_inverse(idx, n, start=None, order=None):
    """The lists a backward by inverted index walks: the pair its forward was given, else one built now (sn_gather_invert), else --
    beyond gather_invert_supported -- None, and the node takes its own fallback route."""
    if start is not None:
        return start, order
    if not gather_invert_supported(n, idx.shape[1:].numel()):
        return None
    return gather_invert(idx, n)


class ThreeInterpolateFunction(torch.autograd.Function):
    """WeightedGatherFunction's forward; the gradient towards the features by inverted index (sn_gather_invert +
    sn_weighted_gather_backward_inverted: the bits of the ordered route, without its (B,C,M,K) scratch buffer).  start / order: a
    GatherInverse of idx the caller built, or None (built in backward).  Beyond sn_gather_invert_supported: the ordered route."""

    @staticmethod
    def forward(ctx, X, idx, w, start, order):
        X, idx, w = _f32c(X), idx.contiguous().int(), _f32c(w)
        B, C, N = X.shape
        _, M, K = idx.shape
        out = torch.empty(B, C, M, device=X.device, dtype=torch.float32)
        with torch.cuda.device(X.device):
            check(lib.sn_weighted_gather_forward(B, C, N, M, K, ptr(X), ptr(idx), ptr(w), ptr(out), _stream(X)),
                  "sn_weighted_gather_forward")
        ctx.save_for_backward(X, idx, w, start, order)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        X, idx, w, start, order = ctx.saved_tensors
        B, C, N = X.shape
        _, M, K = idx.shape
        grad_out = grad_out.contiguous()
        need_X, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        gX = torch.empty_like(X) if need_X else None
        gw = torch.empty_like(w) if need_w else None
        with torch.cuda.device(X.device):
            inverse = _backward_inverse(idx, N, start, order) if need_X else None
            if need_X and inverse is None:
                scratch = torch.empty(B * C * M * K, device=X.device, dtype=torch.float32)
                check(lib.sn_weighted_gather_backward_ordered(B, C, N, M, K, ptr(X), ptr(idx), ptr(w), ptr(grad_out), ptr(gw),
                                                              ptr(gX), ptr(scratch), _stream(X)), "sn_weighted_gather_backward_ordered")
                return gX, None, gw, None, None
            if need_X:
                check(lib.sn_weighted_gather_backward_inverted(B, C, N, M, K, ptr(w), ptr(grad_out), ptr(inverse[0]), ptr(inverse[1]),
                                                               ptr(gX), _stream(X)), "sn_weighted_gather_backward_inverted")
            if need_w:
                check(lib.sn_weighted_gather_backward(B, C, N, M, K, ptr(X), ptr(idx), ptr(w), ptr(grad_out), ptr(gw), None,
                                                      _stream(X)), "sn_weighted_gather_backward")
        return gX, None, gw, None, None


def three_interpolate(features, idx, weight, inverse=None):
    """features (B,C,m), idx (B,n,3) int32, weight (B,n,3) -> (B,C,n): sum_t weight[:, :, t] * features[:, :, idx[:, :, t]]
    (gradients to features and weight).  The gradient towards the features is the deterministic ordered sum, taken by inverted
    index; inverse: what ops.gather_invert(idx, m) returned for THIS idx (nothing else: a pair built by hand is checked for shape and
    type only, and the gradient then follows whatever lists it holds), for a caller that reuses one idx; without it every backward
    builds the inversion anew.  Beyond ops.gather_invert_supported(m, 3 n) the gradient takes the ordered route and no inverse exists."""
    _need_gpu(features, idx, weight)
    if features.dim() != 3 or idx.dim() != 3 or idx.shape[2] != 3 or tuple(weight.shape) != tuple(idx.shape) or idx.shape[0] != features.shape[0]:
        raise ValueError("three_interpolate: features must be (B,C,m), idx and weight (B,n,3)")
    if idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("three_interpolate: idx must be int32 (or int64, converted), got %s" % idx.dtype)
    _one_device("three_interpolate", features, idx, weight)
    start, order = _inverse_arg("three_interpolate", inverse, features.shape[0], features.shape[2], idx.shape[1] * 3, features)
    return ThreeInterpolateFunction.apply(features, idx, weight, start, order)


INTERP_RULES = {"sqrt_eps": 0, "squared_clamp": 1}  # sn_interp_rows_forward's rule


class InterpRowsFunction(torch.autograd.Function):
    """known_rows (B,m,C2), skip_rows (B,n,C1) or None, both row-major, idx / dist2 (B,n,3) of sn_three_nn -> rows (B,n,C2+C1)
    (sn_interp_rows_forward).  Backward: towards known_rows by inverted index (sn_gather_invert + sn_interp_rows_backward; beyond
    sn_gather_invert_supported the ordered route on the transposed slice, the same bits), towards skip_rows the view
    grad_rows[..., C2:].  No gradient goes towards the weights, the distances or the coordinates: three_nn has none and the module's
    weights carry none."""

    @staticmethod
    def forward(ctx, known_rows, skip_rows, idx, dist2, rule, start, order):
        known_rows, dist2 = _f32c(known_rows), _f32c(dist2)
        skip_rows = None if skip_rows is None else _f32c(skip_rows)
        idx = idx.contiguous().int()
        b, m, c2 = known_rows.shape
        n = idx.shape[1]
        c1 = 0 if skip_rows is None else skip_rows.shape[2]
        weights = torch.empty(b, n, 3, device=known_rows.device, dtype=torch.float32)
        rows = torch.empty(b, n, c2 + c1, device=known_rows.device, dtype=torch.float32)
        with torch.cuda.device(known_rows.device):
            check(lib.sn_interp_rows_forward(b, n, m, c2, c1, rule, ptr(known_rows), ptr(skip_rows), ptr(idx), ptr(dist2), ptr(weights),
                                             ptr(rows), _stream(known_rows)), "sn_interp_rows_forward")
        ctx.save_for_backward(known_rows, idx, weights, start, order)
        ctx.dims = (b, n, m, c2, c1)
        return rows

    @staticmethod
    def backward(ctx, grad_rows):
        known_rows, idx, weights, start, order = ctx.saved_tensors
        b, n, m, c2, c1 = ctx.dims
        grad_rows = _f32c(grad_rows)
        dev = grad_rows.device
        gk = None
        gs = grad_rows[..., c2:] if c1 > 0 and ctx.needs_input_grad[1] else None
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(dev):
                st = _stream(grad_rows)
                inverse = _backward_inverse(idx, m, start, order)
                if inverse is None:
                    # the ordered route reads and writes channel-major: the transposed slice in, the transposed gradient out
                    g = grad_rows[..., :c2].transpose(1, 2).contiguous()
                    X = known_rows.transpose(1, 2).contiguous()
                    gX = torch.empty(b, c2, m, device=dev, dtype=torch.float32)
                    scratch = torch.empty(b * c2 * n * 3, device=dev, dtype=torch.float32)
                    check(lib.sn_weighted_gather_backward_ordered(b, c2, m, n, 3, ptr(X), ptr(idx), ptr(weights), ptr(g), None, ptr(gX),
                                                                  ptr(scratch), st), "sn_weighted_gather_backward_ordered")
                    gk = gX.transpose(1, 2).contiguous()
                else:
                    start, order = inverse
                    gk = torch.empty(b, m, c2, device=dev, dtype=torch.float32)
                    check(lib.sn_interp_rows_backward(b, n, m, c2, c1, ptr(weights), ptr(grad_rows), ptr(start), ptr(order), ptr(gk), st),
                          "sn_interp_rows_backward")
        return gk, gs, None, None, None, None, None


def interp_rows(known_rows, skip_rows, idx, dist2, rule="sqrt_eps", inverse=None):
    """The input of a feature-propagation level in the row layout the GEMM entries read, in one launch: known_rows (B,m,C2) and
    skip_rows (B,n,C1) or None, both ROW-major (channels contiguous), idx (B,n,3) int32 and dist2 (B,n,3) from
    ops.three_nn(.., return_dist2=True) -> rows (B, n, C2 + C1): columns 0 .. C2-1 the inverse-distance interpolation of the three
    neighbours' rows (rule "sqrt_eps": weights 1 / (dist + 1e-8), PointnetFPModule's; "squared_clamp": 1 / max(dist^2, 1e-10),
    normalised over the three), bit for bit ops.three_interpolate on these weights, then the C1 skip columns copied.
    Differentiable towards known_rows (the deterministic ordered sum by inverted index; inverse: ops.gather_invert(idx, m) of THIS
    idx for a caller that reuses it, else every backward builds it; beyond ops.gather_invert_supported(m, 3 n) the ordered route
    serves and no inverse exists) and towards skip_rows (a view of the incoming gradient).  No gradient goes towards the weights,
    the distances or the coordinates: three_nn has none and the module's weights carry none."""
    _need_gpu(known_rows, skip_rows, idx, dist2)
    if rule not in INTERP_RULES:
        raise ValueError("interp_rows: rule must be one of %s, got %r" % (sorted(INTERP_RULES), rule))
    if known_rows.dim() != 3 or idx.dim() != 3 or idx.shape[2] != 3 or tuple(dist2.shape) != tuple(idx.shape) or idx.shape[0] != known_rows.shape[0]:
        raise ValueError("interp_rows: known_rows must be (B,m,C2), idx and dist2 (B,n,3)")
    if idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("interp_rows: idx must be int32 (or int64, converted), got %s" % idx.dtype)
    b, m, c2 = known_rows.shape
    n = idx.shape[1]
    if skip_rows is not None and (skip_rows.dim() != 3 or skip_rows.shape[0] != b or skip_rows.shape[1] != n):
        raise ValueError("interp_rows: skip_rows must be (B,n,C1), got %s" % (tuple(skip_rows.shape),))
    if skip_rows is not None and skip_rows.shape[2] == 0:
        skip_rows = None
    if c2 + (0 if skip_rows is None else skip_rows.shape[2]) == 0:
        raise ValueError("interp_rows: no output column (C2 + C1 == 0)")
    if m == 0 and b * n > 0:
        raise ValueError("interp_rows: the known cloud is empty")
    _one_device("interp_rows", known_rows, skip_rows, idx, dist2)
    start, order = _inverse_arg("interp_rows", inverse, b, m, n * 3, known_rows)
    return InterpRowsFunction.apply(known_rows, skip_rows, idx, dist2, INTERP_RULES[rule], start, order)


# --------------------------------------------------------------------------------------------- set abstraction: row-layout grouping
class BallGroupRowsFunction(torch.autograd.Function):
    """xyz (B,N,3), new_xyz (B,M,3), features (B,N,C) row-major or None -> rows (B, M, nsample, 3 use_xyz + C), idx, pts_cnt
    (sn_ball_group_rows_forward).  Backward: sn_gather_invert + sn_group_rows_backward, only the outputs that need a gradient;
    beyond sn_gather_invert_supported the gradient is permuted to channel-major for sn_ball_group_backward (float atomics)."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, radius, nsample, use_xyz, rule):
        _need_gpu(xyz, new_xyz, features)
        xyz, new_xyz = _f32c(xyz), _f32c(new_xyz)
        features = None if features is None else _f32c(features)
        if xyz.dim() != 3 or xyz.shape[2] != 3 or new_xyz.dim() != 3 or new_xyz.shape[2] != 3 or new_xyz.shape[0] != xyz.shape[0]:
            raise ValueError("ball_group_rows: xyz must be (B,N,3) and new_xyz (B,M,3)")
        b, n, _ = xyz.shape
        m = new_xyz.shape[1]
        if features is not None and (features.dim() != 3 or features.shape[0] != b or features.shape[1] != n):
            raise ValueError("ball_group_rows: features_bnc must be (B,N,C)")
        c = 0 if features is None else features.shape[2]
        u = 1 if use_xyz else 0
        rows = torch.empty(b, m, nsample, 3 * u + c, device=xyz.device, dtype=torch.float32)
        idx = torch.empty(b, m, nsample, device=xyz.device, dtype=torch.int32)
        cnt = torch.empty(b, m, device=xyz.device, dtype=torch.int32)
        with torch.cuda.device(xyz.device):
            check(lib.sn_ball_group_rows_forward(b, n, m, c, float(radius), nsample, rule, u, ptr(xyz), ptr(new_xyz), ptr(features),
                                                 ptr(idx), ptr(cnt), ptr(rows), _stream(xyz)), "sn_ball_group_rows_forward")
        ctx.save_for_backward(idx)
        ctx.dims = (b, n, m, c, nsample, u)
        ctx.mark_non_differentiable(idx, cnt)
        return rows, idx, cnt

    @staticmethod
    def backward(ctx, grad_rows, _gi, _gc):
        (idx,) = ctx.saved_tensors
        b, n, m, c, ns, u = ctx.dims
        grad_rows = _f32c(grad_rows)
        dev = grad_rows.device
        need_xyz, need_new, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and c > 0
        gx = torch.empty(b, n, 3, device=dev, dtype=torch.float32) if need_xyz else None
        gn = torch.empty(b, m, 3, device=dev, dtype=torch.float32) if need_new else None
        with torch.cuda.device(dev):
            st = _stream(grad_rows)
            # the lists are built only for the outputs that are sums over them ((need_xyz and u) or need_f)
            inverse = _backward_inverse(idx, n) if (need_xyz and u) or need_f else None
            if inverse is None and (need_xyz or need_f) and not gather_invert_supported(n, m * ns):
                # the atomic route: sn_ball_group_backward reads channel-major and writes (B,C,N)
                g = grad_rows.permute(0, 3, 1, 2).contiguous()
                gf = torch.empty(b, c, n, device=dev, dtype=torch.float32) if need_f else None
                check(lib.sn_ball_group_backward(b, n, m, c, ns, u, ptr(idx), ptr(g), ptr(gf), ptr(gx), ptr(gn), st),
                      "sn_ball_group_backward")
                return gx, gn, (gf.transpose(1, 2).contiguous() if need_f else None), None, None, None, None
            gf = torch.empty(b, n, c, device=dev, dtype=torch.float32) if need_f else None
            start, order = inverse or (None, None)
            check(lib.sn_group_rows_backward(b, n, m, c, ns, u, ptr(idx), ptr(start), ptr(order), ptr(grad_rows), ptr(gf), ptr(gx),
                                             ptr(gn), st), "sn_group_rows_backward")
        return gx, gn, gf, None, None, None, None


def ball_group_rows(radius, nsample, xyz, new_xyz, features_bnc=None, use_xyz=True, rule="squared", return_idx=False):
    """QueryAndGroup in the row layout the GEMM entries read: xyz (B,N,3), new_xyz (B,M,3), features_bnc (B,N,C) ROW-major or None
    -> rows (B, M, nsample, 3 use_xyz + C): with use_xyz the first three columns are xyz[idx] - new_xyz, then the C feature columns
    of point idx, idx the ball query's rows (ops.ball_query) -- ops.ball_group's tensor permuted, bit for bit, in one launch.
    Gradients reach features_bnc, xyz and new_xyz where each requires one.  Within ops.gather_invert_supported(N, M * nsample) the
    gradients towards features_bnc and xyz are DETERMINISTIC: per point the sum over the slots that name it in ascending slot order,
    by inverted index (a launch takes as long as its longest list; point 0 collects every empty ball).  Beyond that bound they take
    sn_ball_group_backward's route on the permuted gradient, which sums with float atomics (last bits depend on arrival order).
    The gradient towards new_xyz has one order on both routes.  return_idx: also the indices (B,M,nsample) and counts (B,M)."""
    if features_bnc is None and not use_xyz:
        raise ValueError("ball_group_rows: nothing to group (features_bnc is None and use_xyz is False)")
    rows, idx, cnt = BallGroupRowsFunction.apply(xyz, new_xyz, features_bnc, radius, nsample, bool(use_xyz), _ball_rule(rule))
    return (rows, idx, cnt) if return_idx else rows


# --------------------------------------------------------------------------------------------- SoftProjection
def _grad_temperature(gsig, temperature, min_sigma):
    """d loss / dT from the d loss / d sigma partials (one tiny kernel): sigma = max(T^2, min_sigma), with torch.max's
    even split of the gradient on an exact tie."""
    T = temperature.detach().float().reshape(1)
    gT = torch.empty(1, device=gsig.device, dtype=torch.float32)
    with torch.cuda.device(gsig.device):
        check(lib.sn_sigma_grad(gsig.numel(), ptr(gsig), ptr(T), float(min_sigma), ptr(gT), _stream(gsig)), "sn_sigma_grad")
    return gT.reshape(temperature.shape)


class SigmaFunction(torch.autograd.Function):
    """sigma = max(T^2, min_sigma) of the one-element temperature (soft_projection.py:97-99) -- what get_projection_loss returns -- as
    one launch each way (torch: pow + maximum, and seven launches of their backwards); the same bits, torch.max's even split on a tie."""

    @staticmethod
    def forward(ctx, temperature, min_sigma):
        _need_gpu(temperature)
        T = temperature.detach().float().reshape(1)
        out = torch.empty(1, device=T.device, dtype=torch.float32)
        with torch.cuda.device(T.device):
            check(lib.sn_sigma_forward(ptr(T), float(min_sigma), ptr(out), _stream(T)), "sn_sigma_forward")
        ctx.save_for_backward(temperature)
        ctx.min_sigma = float(min_sigma)
        return out.reshape(temperature.shape)

    @staticmethod
    def backward(ctx, g):
        (temperature,) = ctx.saved_tensors
        return _grad_temperature(_f32c(g).reshape(1), temperature, ctx.min_sigma), None


class SoftProjectFunction(torch.autograd.Function):
    """Fused SoftProjection.project (soft_projection.py:138-152): kNN + softmax weights + weighted sum
    in ONE kernel (sn_pairscan_forward), optionally together with both Chamfer directions between the
    query cloud and the point cloud (the sampler's simplification loss reuses them).

    forward(point_cloud, query_cloud (B,3,M), temperature (scalar tensor), min_sigma, K, want_chamfer,
            p_layout=BCN, out_layout=BCN)
      point_cloud: (B,3,N) for BCN or (B,N,3) for BNC (the kernels read either layout: no transposed copy)
      -> proj (B,3,M) for BCN / (B,M,3) for BNC, idx (B,M,K) [, dist_q (B,M), idx_q, dist_p (B,N), idx_p]
    """

    @staticmethod
    def forward(ctx, point_cloud, query_cloud, temperature, min_sigma, K, want_chamfer, p_layout=BCN, out_layout=BCN):
        _need_gpu(point_cloud, query_cloud, temperature)
        P, Q = _f32c(point_cloud), _f32c(query_cloud)
        B = P.shape[0]
        N = P.shape[2] if p_layout == BCN else P.shape[1]
        M = Q.shape[2]
        dev = P.device
        proj = torch.empty((B, 3, M) if out_layout == BCN else (B, M, 3), device=dev, dtype=torch.float32)
        idx = torch.empty(B, M, K, device=dev, dtype=torch.int32)
        dq = iq = dp = ip = None
        if want_chamfer:
            dq = torch.empty(B, M, device=dev, dtype=torch.float32)
            iq = torch.empty(B, M, device=dev, dtype=torch.int32)
            dp = torch.empty(B, N, device=dev, dtype=torch.float32)
            ip = torch.empty(B, N, device=dev, dtype=torch.int32)
        T = temperature.detach().float().reshape(1)
        wsb = lib.sn_pairscan_workspace_bytes(B, N, M) if want_chamfer else 0
        ws = torch.empty(wsb // 8, device=dev, dtype=torch.int64) if wsb else None
        with torch.cuda.device(dev):
            check(lib.sn_pairscan_forward_ws(B, N, M, K, ptr(P), p_layout, ptr(Q), BCN, ptr(idx), None, ptr(dq), ptr(iq),
                                             ptr(dp), ptr(ip), ptr(proj), out_layout, None, ptr(T), float(min_sigma), ptr(ws),
                                             wsb, _stream(P)), "sn_pairscan_forward_ws")
        ctx.save_for_backward(P, Q, idx, temperature)
        ctx.min_sigma = float(min_sigma)
        ctx.K, ctx.N, ctx.p_layout, ctx.out_layout = K, N, p_layout, out_layout
        ctx.set_materialize_grads(False)  # no zero tensors for the (non-differentiable) index / distance outputs
        ctx.mark_non_differentiable(idx)
        if want_chamfer:
            ctx.mark_non_differentiable(dq, iq, dp, ip)  # their gradient is taken by the loss functions below
            return proj, idx, dq, iq, dp, ip
        return proj, idx

    @staticmethod
    def backward(ctx, grad_proj, *_unused):
        if grad_proj is None:
            return (None,) * 8
        P, Q, idx, temperature = ctx.saved_tensors
        B, N, M = P.shape[0], ctx.N, Q.shape[2]
        dev = P.device
        grad_proj = grad_proj.contiguous()
        gQ = torch.empty_like(Q)
        gsig = torch.empty(B * lib.sn_soft_bwd_splits(B, M), device=dev, dtype=torch.float32)
        T = temperature.detach().float().reshape(1)
        gP = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                # gradient towards the point cloud: contributions stored per (query, neighbour), summed per point in the
                # reference's order (deterministic; no atomics, no zero fill)
                gP = torch.empty_like(P)
                scratch = torch.empty(B * M * ctx.K * 3, device=dev, dtype=torch.float32)
                check(lib.sn_soft_project_backward_ordered(B, N, M, ctx.K, ptr(P), ctx.p_layout, ptr(Q), BCN, ptr(idx), ptr(T),
                                                           ctx.min_sigma, ptr(grad_proj), ctx.out_layout, ptr(gQ), BCN, ptr(gP),
                                                           ptr(gsig), ptr(scratch), _stream(P)), "sn_soft_project_backward_ordered")
            else:
                check(lib.sn_soft_project_backward(B, N, M, ctx.K, ptr(P), ctx.p_layout, ptr(Q), BCN, ptr(idx), ptr(T),
                                                   ctx.min_sigma, ptr(grad_proj), ctx.out_layout, ptr(gQ), BCN, None, ptr(gsig),
                                                   _stream(P)), "sn_soft_project_backward")
        gT = None
        if ctx.needs_input_grad[2]:
            gT = _grad_temperature(gsig, temperature, ctx.min_sigma)
        return gP, (gQ if ctx.needs_input_grad[1] else None), gT, None, None, None, None, None


class SoftWeightsFunction(torch.autograd.Function):
    """w (B,M,K) = softmax_k(-|P[idx]-Q|^2 / sigma)   (soft_projection.py:92-95,110,128,143)"""

    @staticmethod
    def forward(ctx, P, Q, idx, temperature, min_sigma):
        _need_gpu(P, Q, idx, temperature)
        P, Q, idx = _f32c(P), _f32c(Q), idx.contiguous().int()
        B, _, N = P.shape
        M = Q.shape[2]
        K = idx.shape[2]
        w = torch.empty(B, M, K, device=P.device, dtype=torch.float32)
        T = temperature.detach().float().reshape(1)
        with torch.cuda.device(P.device):
            check(lib.sn_soft_weights_forward(B, N, M, K, ptr(P), ptr(Q), ptr(idx), ptr(T), float(min_sigma), ptr(w),
                                              _stream(P)), "sn_soft_weights_forward")
        ctx.save_for_backward(P, Q, idx, temperature, w)
        ctx.min_sigma = float(min_sigma)
        return w

    @staticmethod
    def backward(ctx, grad_w):
        P, Q, idx, temperature, w = ctx.saved_tensors
        B, _, N = P.shape
        M = Q.shape[2]
        K = idx.shape[2]
        grad_w = grad_w.contiguous()
        gQ = torch.empty_like(Q)
        gsig = torch.empty(B * lib.sn_soft_bwd_splits(B, M), device=P.device, dtype=torch.float32)
        T = temperature.detach().float().reshape(1)
        gP = None
        with torch.cuda.device(P.device):
            if ctx.needs_input_grad[0]:
                gP = torch.empty_like(P)
                scratch = torch.empty(B * M * K * 3, device=P.device, dtype=torch.float32)
                check(lib.sn_soft_weights_backward_ordered(B, N, M, K, ptr(P), ptr(Q), ptr(idx), ptr(T), ctx.min_sigma, ptr(w),
                                                           ptr(grad_w), ptr(gQ), ptr(gP), ptr(gsig), ptr(scratch), _stream(P)),
                      "sn_soft_weights_backward_ordered")
            else:
                check(lib.sn_soft_weights_backward(B, N, M, K, ptr(P), ptr(Q), ptr(idx), ptr(T), ctx.min_sigma, ptr(w),
                                                   ptr(grad_w), ptr(gQ), None, ptr(gsig), _stream(P)),
                      "sn_soft_weights_backward")
        gT = None
        if ctx.needs_input_grad[3]:
            gT = _grad_temperature(gsig, temperature, ctx.min_sigma)
        return gP, (gQ if ctx.needs_input_grad[1] else None), None, gT, None


class WeightedGatherFunction(torch.autograd.Function):
    """out (B,C,M) = sum_k w[:, :, k] * X[:, :, idx[:, :, k]]   (soft_projection.py:113-118,131-134,148-151)"""

    @staticmethod
    def forward(ctx, X, idx, w):
        _need_gpu(X, idx, w)
        X, idx, w = _f32c(X), idx.contiguous().int(), _f32c(w)
        B, C, N = X.shape
        _, M, K = idx.shape
        out = torch.empty(B, C, M, device=X.device, dtype=torch.float32)
        with torch.cuda.device(X.device):
            check(lib.sn_weighted_gather_forward(B, C, N, M, K, ptr(X), ptr(idx), ptr(w), ptr(out), _stream(X)),
                  "sn_weighted_gather_forward")
        ctx.save_for_backward(X, idx, w)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        X, idx, w = ctx.saved_tensors
        B, C, N = X.shape
        _, M, K = idx.shape
        grad_out = grad_out.contiguous()
        gw = torch.empty_like(w) if ctx.needs_input_grad[2] else None
        gX = None
        with torch.cuda.device(X.device):
            if ctx.needs_input_grad[0]:  # (ordered sum per point: deterministic, see sn_soft_project_backward_ordered)
                gX = torch.empty_like(X)
                scratch = torch.empty(B * C * M * K, device=X.device, dtype=torch.float32)
                check(lib.sn_weighted_gather_backward_ordered(B, C, N, M, K, ptr(X), ptr(idx), ptr(w), ptr(grad_out), ptr(gw),
                                                              ptr(gX), ptr(scratch), _stream(X)), "sn_weighted_gather_backward_ordered")
            else:
                check(lib.sn_weighted_gather_backward(B, C, N, M, K, ptr(X), ptr(idx), ptr(w), ptr(grad_out), ptr(gw), None,
                                                      _stream(X)), "sn_weighted_gather_backward")
        return gX, None, gw


class ChamferFromScanFunction(torch.autograd.Function):
    """Autograd node for Chamfer distances that were produced by a previous pair scan.

    forward(xyz1 (B,n,3), xyz2 (B,m,3), dist1, idx1, dist2, idx2) -> dist1, dist2 (no kernel launch);
    backward = sn_chamfer_backward.  Used by SampleNet.get_simplification_loss when the sampler's own
    forward pass already scanned the same pair of clouds (one distance matrix instead of three).
    """

    @staticmethod
    def forward(ctx, xyz1, xyz2, dist1, idx1, dist2, idx2):
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        return dist1.clone(), dist2.clone()

    @staticmethod
    def backward(ctx, graddist1, graddist2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        g1, g2 = chamfer_backward_impl(xyz1.contiguous(), xyz2.contiguous(), idx1, idx2, graddist1, graddist2,
                                       ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return g1, g2, None, None, None, None


class SimplificationLossFunction(torch.autograd.Function):
    """loss = mean(dist1) + mean_b(max_m dist1) + weight * mean(dist2)   (samplenet.py:171-181) from the Chamfer products
    of (samp_pc, ref_pc); backward = Chamfer backward with the implicit upstream gradients, one launch per input.
    samp_layout: BNC (B,M,3) or BCN (B,3,M) -- the latter lets the loss hang directly off the FC head's output."""

    @staticmethod
    def forward(ctx, samp_pc, ref_pc, dist1, idx1, dist2, idx2, weight, samp_layout=BNC):
        _need_gpu(samp_pc, ref_pc, dist1, dist2)
        B, M = dist1.shape
        N = dist2.shape[1]
        dev = dist1.device
        partial = torch.empty(B * 3, device=dev, dtype=torch.float32)
        argmax1 = torch.empty(B, device=dev, dtype=torch.int32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            check(lib.sn_simplification_loss_forward(B, M, N, ptr(dist1), ptr(dist2), float(weight), ptr(partial),
                                                     ptr(argmax1), ptr(loss), _stream(dist1)), "sn_simplification_loss_forward")
        ctx.save_for_backward(samp_pc, ref_pc, idx1, idx2, argmax1)
        ctx.weight = float(weight)
        ctx.samp_layout = samp_layout
        if samp_layout != BNC and ref_pc.requires_grad:
            raise ValueError("SimplificationLossFunction: a (B,3,M) sampled cloud needs a constant reference cloud")
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        samp_pc, ref_pc, idx1, idx2, argmax1 = ctx.saved_tensors
        x1, x2 = samp_pc.contiguous(), ref_pc.contiguous()
        B, N = x2.shape[0], x2.shape[1]
        M = idx1.shape[1]
        g1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        gl = grad_loss.contiguous().float()
        with torch.cuda.device(x1.device):
            check(lib.sn_simplification_loss_backward(B, M, ptr(x1), N, ptr(x2), ptr(idx1), ptr(idx2), ptr(argmax1), ctx.weight,
                                                      ptr(gl), ptr(g1), ptr(g2), ctx.samp_layout, _stream(x1)),
                  "sn_simplification_loss_backward")
        return g1, g2, None, None, None, None, None, None


class PrefixSimplificationLossFunction(torch.autograd.Function):
    """sum over the first len(sizes) nested prefixes of SimplificationLossFunction(samp_pc[:, :s], ref_pc, dist1[:, :s], idx1[:, :s],
    dist2[p], idx2[p], weights[p]) -- the progressive sampler's loss (classification/train_samplenet_progressive.py:204-216) --
    as ONE node: two launches forward, one backward, no copies of the prefixes; bit-identical to the separate terms added ascending.
    samp_pc (B,M,3), ref_pc (B,N,3) [constant], dist1 / idx1 (B,M), dist2 / idx2 (S,B,N) from prefix_point_minima."""

    @staticmethod
    def forward(ctx, samp_pc, ref_pc, dist1, idx1, dist2, idx2, sizes, weights):
        import ctypes

        _need_gpu(samp_pc, ref_pc, dist1, dist2)
        B, M = dist1.shape
        N = dist2.shape[2]
        P = len(sizes)
        dev = dist1.device
        partial = torch.empty(P * B * 3, device=dev, dtype=torch.float32)
        argmax1 = torch.empty(P * B, device=dev, dtype=torch.int32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        cs, cw = (ctypes.c_int * P)(*[int(v) for v in sizes]), (ctypes.c_float * P)(*[float(w) for w in weights])
        d1, d2 = _f32c(dist1), _f32c(dist2)
        with torch.cuda.device(dev):
            check(lib.sn_prefix_simplification_loss_forward(B, M, N, P, cs, cw, ptr(d1), ptr(d2), ptr(partial), ptr(argmax1), ptr(loss),
                                                            _stream(d1)), "sn_prefix_simplification_loss_forward")
        ctx.save_for_backward(samp_pc, ref_pc, idx1, idx2, argmax1)
        ctx.cfg = (cs, cw, P)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        samp_pc, ref_pc, idx1, idx2, argmax1 = ctx.saved_tensors
        cs, cw, P = ctx.cfg
        x1, x2 = _f32c(samp_pc), _f32c(ref_pc)
        B, M, _ = x1.shape
        N = x2.shape[1]
        g1 = torch.empty_like(x1)
        gl = grad_loss.contiguous().float()
        with torch.cuda.device(x1.device):
            check(lib.sn_prefix_simplification_loss_backward(B, M, N, P, cs, cw, ptr(x1), ptr(x2), ptr(idx1.contiguous()),
                                                             ptr(idx2.contiguous()), ptr(argmax1), ptr(gl), ptr(g1), _stream(x1)),
                  "sn_prefix_simplification_loss_backward")
        return g1, None, None, None, None, None, None, None


class SamplerLossFunction(torch.autograd.Function):
    """L = alpha * L_simp + lmbda * max(T^2, min_sigma) + mean(proj): the sampler's loss as registration/main.py:507-531
    composes it, with mean(proj) standing in for the task loss.  One kernel forward, one backward."""

    @staticmethod
    def forward(ctx, lsimp, temperature, proj, alpha, lmbda, min_sigma):
        _need_gpu(lsimp, temperature, proj)
        proj = _f32c(proj)
        T = temperature.detach().float().reshape(1)
        ls = lsimp.detach().float().reshape(1)
        loss = torch.empty((), device=proj.device, dtype=torch.float32)
        with torch.cuda.device(proj.device):
            check(lib.sn_sampler_loss_forward(proj.numel(), ptr(proj), ptr(ls), ptr(T), float(alpha), float(lmbda),
                                              float(min_sigma), ptr(loss), _stream(proj)), "sn_sampler_loss_forward")
        ctx.save_for_backward(temperature)
        ctx.cfg = (float(alpha), float(lmbda), float(min_sigma), tuple(proj.shape), lsimp.shape)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (temperature,) = ctx.saved_tensors
        alpha, lmbda, min_sigma, pshape, lshape = ctx.cfg
        dev = grad_loss.device
        gproj = torch.empty(pshape, device=dev, dtype=torch.float32)
        gls = torch.empty(1, device=dev, dtype=torch.float32)
        gT = torch.empty(1, device=dev, dtype=torch.float32)
        gl = grad_loss.contiguous().float().reshape(1)
        T = temperature.detach().float().reshape(1)
        with torch.cuda.device(dev):
            check(lib.sn_sampler_loss_backward(gproj.numel(), ptr(gl), ptr(T), alpha, lmbda, min_sigma, ptr(gproj), ptr(gls),
                                               ptr(gT), _stream(gl)), "sn_sampler_loss_backward")
        return gls.reshape(lshape), gT.reshape(temperature.shape), gproj, None, None, None


class StepCfg(NamedTuple):
    """The step loss's constants, as step_loss_backward takes them."""

    K: int
    min_sigma: float
    alpha: float
    lmbda: float
    weight: float


class StepLossState:
    """What step_loss_forward hands to step_loss_backward.  idx (B,M,K): the kNN indices; idx_q (B,M) / idx_p (B,N): the nearest
    point of every query / the nearest query of every point; argmax1 (B,).  deferred: (partial, loss) when the backward's first
    launch writes the loss value, else (None, None).  Keys mode (the per-point minima stay in the caller's key table, the
    backward produces idx_p / argmax1 itself: both None here): keys, qpart, qmax and G, the scan workgroups per cloud; None
    on the other routes."""

    __slots__ = ("idx", "idx_q", "idx_p", "argmax1", "deferred", "keys", "qpart", "qmax", "G")

    def __init__(self, idx, idx_q, idx_p, argmax1, deferred, keys=None, qpart=None, qmax=None, G=None):
        self.idx, self.idx_q, self.idx_p, self.argmax1, self.deferred = idx, idx_q, idx_p, argmax1, deferred
        self.keys, self.qpart, self.qmax, self.G = keys, qpart, qmax, G

    @property
    def keys_mode(self):
        return self.keys is not None


def scan_splits(B, N, M):
    """Scan workgroups per cloud (pairscan_ysplit): 1 = the one-workgroup-per-cloud scan finishes the per-point minima itself
    (batches that fill the chip, and every N > 2048); above 1 a cloud's per-point minima are combined behind the scan."""
    return lib.sn_pairscan_colmin_splits(B, N, M)


def keys_step_possible(B, N, M):
    """True when the batch can run the keys-mode step: clouds split over workgroups, N within the key table's bound, and the
    test hook fused_step.KEYS_LOSS left on."""
    from . import fused_step

    return bool(fused_step.KEYS_LOSS and N <= 2048 and scan_splits(B, N, M) > 1)


class SamplerStepLossFunction(torch.autograd.Function):
    """The whole loss side of the sampler's training step behind ONE autograd node (engine fast path):
        simp = y (B,3,M) from the FC head;  proj = SoftProjection(x, simp)                       (soft_projection.py:138-152)
        L = alpha * simplification_loss(x, simp) + lmbda * sigma + mean(proj)                    (main.py:507-531)
    forward : pair scan (per-point minima left as partials) -> per-cloud reduction -> combine     = 3 launches
    backward: Chamfer backward (implicit gradients) -> soft-projection backward (+=) -> grad_T    = 3 launches
    Same numbers as SoftProjectFunction + SimplificationLossFunction + SamplerLossFunction composed by autograd.
    t_sink: optional tensor the temperature gradient is written into (p.grad view of a flat bucket); then no gradient is
    returned for the temperature."""

    @staticmethod
    def forward(ctx, y_bcn, x_bnc, temperature, K, min_sigma, alpha, lmbda, weight, t_sink=None, defer_value=False):
        _need_gpu(y_bcn, x_bnc, temperature)
        y, x = _f32c(y_bcn), _f32c(x_bnc)
        with torch.cuda.device(y.device):
            loss, proj, state = step_loss_forward(x, y, None, temperature, K, min_sigma, alpha, lmbda, weight, defer_value)
        ctx.save_for_backward(x, y, temperature, state.idx, state.idx_q, state.idx_p, state.argmax1)
        ctx.deferred = state.deferred
        ctx.cfg = StepCfg(K, float(min_sigma), float(alpha), float(lmbda), float(weight))
        ctx.t_sink = t_sink
        ctx.mark_non_differentiable(proj)
        ctx.set_materialize_grads(False)
        return loss[0], proj

    @staticmethod
    def backward(ctx, grad_loss, _gproj=None):
        x, y, temperature, idx, iq, ip, argmax1 = ctx.saved_tensors
        if grad_loss is None:
            return (None,) * 10
        with torch.cuda.device(y.device):
            state = StepLossState(idx, iq, ip, argmax1, ctx.deferred)
            gQ, gT, _ = step_loss_backward(x, y, temperature, state, ctx.cfg, grad_loss, ctx.t_sink)
        g_temp = None
        if ctx.t_sink is None and ctx.needs_input_grad[2]:
            g_temp = gT.reshape(temperature.shape)
        return (gQ if ctx.needs_input_grad[0] else None), None, g_temp, None, None, None, None, None, None, None


def step_loss_forward(x, y, fc, temperature, K, min_sigma, alpha, lmbda, weight, defer_value, keys=None, proj_out=None):
    """Forward launches of the sampler step's loss side (SamplerStepLossFunction / fused_step.SamplerStepFunction).
    x (B,N,3), y (B,3,M): the simplified cloud -- read when fc is None, otherwise WRITTEN by the pair scan from
    fc = (z3 (B,Kfc), coef3 (>=2*Kfc: scale | shift), W4 (3M,Kfc), b4 (3M)).  Caller holds the device guard.
    -> loss (2,), proj (B,M,3), state (a StepLossState).
    keys (needs N <= 2048; the backward must follow): zeroed (B*N) int64 table; only the pair scan runs here, the per-point
    minima are combined in the table and the loss value is produced by the backward's launches (sn_sampler_step_loss_keys).
    proj_out: a preallocated contiguous (B,M,3) fp32 tensor for the projected cloud (the captured surface's output block)."""
    B, _, M = y.shape
    N = x.shape[1]
    dev = y.device
    G = scan_splits(B, N, M)
    if G <= 1 and (fc is not None or keys is not None):
        raise ValueError("fc4 inside the scan / the keys-mode step need a batch small enough for split clouds")
    proj = proj_out if proj_out is not None else torch.empty(B, M, 3, device=dev, dtype=torch.float32)
    idx = torch.empty(B, M, K, device=dev, dtype=torch.int32)
    dq = torch.empty(B, M, device=dev, dtype=torch.float32)
    iq = torch.empty(B, M, device=dev, dtype=torch.int32)
    dp = torch.empty(B, N, device=dev, dtype=torch.float32)
    ip = torch.empty(B, N, device=dev, dtype=torch.int32)
    argmax1 = torch.empty(B, device=dev, dtype=torch.int32)
    if G <= 1:
        # the batch fills the chip with one workgroup per cloud: the scan finishes dist_p / idx_p itself (no partial key sets);
        # per-cloud loss partials in parallel, then the clouds in order -- the backward is the same fused launch
        partial = torch.empty(B * 4, device=dev, dtype=torch.float32)
        loss = torch.empty(2, device=dev, dtype=torch.float32)
        T = temperature.detach().float().reshape(1)
        wsb = lib.sn_pairscan_workspace_bytes(B, N, M)
        wsd = torch.empty(wsb // 8, device=dev, dtype=torch.int64) if wsb else None
        st = _stream(y)
        check(lib.sn_pairscan_forward_ws(B, N, M, K, ptr(x), BNC, ptr(y), BCN, ptr(idx), None, ptr(dq), ptr(iq), ptr(dp), ptr(ip),
                                         ptr(proj), BNC, None, ptr(T), float(min_sigma), ptr(wsd), wsb, st), "sn_pairscan_forward_ws")
        check(lib.sn_sampler_step_loss_forward_direct(B, M, N, ptr(dq), ptr(dp), ptr(proj), ptr(T), float(alpha), float(lmbda),
                                                      float(weight), float(min_sigma), ptr(argmax1), ptr(partial), ptr(loss),
                                                      1 if defer_value else 0, st), "sn_sampler_step_loss_forward_direct")
        return loss, proj, StepLossState(idx, iq, ip, argmax1, (partial, loss) if defer_value else (None, None))
    ws = torch.empty(B * G * N, device=dev, dtype=torch.int64)
    partial = torch.empty(B * 4, device=dev, dtype=torch.float32)
    loss = torch.empty(2, device=dev, dtype=torch.float32)
    T = temperature.detach().float().reshape(1)
    st = _stream(y)
    if keys is not None:
        # keys mode: the scan combines the per-point minima in place (atomicMax on inverted keys in the caller's persistent,
        # zeroed table) -- no partial key sets, nothing between the scan and the backward (sn_sampler_step_loss_keys)
        qpart = torch.empty(B * G * 2, device=dev, dtype=torch.float32)
        qmax = torch.empty(B * G, device=dev, dtype=torch.int64)
        z3, coef3, W4, b4 = fc if fc is not None else (None, None, None, None)
        Kfc = z3.shape[1] if fc is not None else 0
        check(lib.sn_pairscan_forward_keys(B, N, M, K, ptr(x), BNC, ptr(y), ptr(z3), ptr(coef3),
                                           (coef3.data_ptr() + 4 * Kfc) if fc is not None else None, ptr(W4), ptr(b4), Kfc,
                                           ptr(idx), ptr(dq), ptr(iq), ptr(proj), BNC, ptr(T), float(min_sigma), ptr(keys),
                                           ptr(qpart), ptr(qmax), st), "sn_pairscan_forward_keys")
        return loss, proj, StepLossState(idx, iq, None, None, (partial, loss), keys, qpart, qmax, G)
    if fc is None:
        check(lib.sn_pairscan_forward_partial(B, N, M, K, ptr(x), BNC, ptr(y), BCN, ptr(idx), ptr(dq), ptr(iq), ptr(proj), BNC,
                                              ptr(T), float(min_sigma), ptr(ws), ws.numel() * 8, st),
              "sn_pairscan_forward_partial")
    else:
        z3, coef3, W4, b4 = fc
        Kfc = z3.shape[1]
        check(lib.sn_pairscan_forward_partial_fc(B, N, M, K, ptr(x), BNC, ptr(z3), ptr(coef3), coef3.data_ptr() + 4 * Kfc,
                                                 ptr(W4), ptr(b4), Kfc, ptr(y), ptr(idx), ptr(dq), ptr(iq), ptr(proj), BNC,
                                                 ptr(T), float(min_sigma), ptr(ws), ws.numel() * 8, st),
              "sn_pairscan_forward_partial_fc")
    check(lib.sn_sampler_step_loss_forward(B, M, N, G, ptr(dq), ptr(ws), ptr(proj), ptr(T), float(alpha), float(lmbda),
                                           float(weight), float(min_sigma), ptr(dp), ptr(ip), ptr(argmax1), ptr(partial),
                                           ptr(loss), 1 if defer_value else 0, st), "sn_sampler_step_loss_forward")
    # defer_value: the loss VALUE is written by the backward's first launch (engine: backward always follows)
    return loss, proj, StepLossState(idx, iq, ip, argmax1, (partial, loss) if defer_value else (None, None))


def step_loss_backward(x, y, temperature, state, cfg, grad_loss, t_sink, deferred_tail=None, grad_proj=None, grad_sigma=None):
    """Backward launches of the sampler step's loss side -> (grad_Q (B,3,M), grad_T (1,), keep).  Caller holds the device guard.
    state: step_loss_forward's StepLossState; cfg: a StepCfg.  keep: the scratch a deferred tail still reads -- the caller holds
    it until that launch (the closing kernel of the conv backward) is enqueued -- or None.
    grad_proj (B,M,3), keys mode only: gradient of an outside task loss w.r.t. the projected points; the step's own loss then
    has no mean(proj) term (None: that stand-in term is part of the loss, its gradient implicit).
    grad_sigma (1,), keys mode only: upstream gradient of sigma as an output of its own (the drop-in surface); the direct term of
    grad_T is then grad_sigma * d sigma / dT instead of lmbda * grad_loss * d sigma / dT."""
    dpart, dloss = state.deferred
    K, min_sigma, alpha, lmbda, weight = cfg
    B, _, M = y.shape
    N = x.shape[1]
    dev = y.device
    gQ = torch.empty_like(y)
    gsig = torch.empty(B * lib.sn_soft_bwd_splits(B, M), device=dev, dtype=torch.float32)
    gT = t_sink if t_sink is not None else torch.empty(1, device=dev, dtype=torch.float32)
    gl = grad_loss.contiguous().float().reshape(1)
    T = temperature.detach().float().reshape(1)
    if state.keys_mode:
        check(lib.sn_sampler_step_loss_keys(B, N, M, K, ptr(x), BNC, ptr(y), ptr(state.idx), ptr(state.idx_q), ptr(state.keys),
                                            ptr(state.qpart), ptr(state.qmax), state.G, ptr(T), min_sigma, alpha, lmbda, weight,
                                            ptr(gl), ptr(gQ), ptr(gsig), ptr(gT), ptr(dpart), ptr(dloss), _stream(y), deferred_tail, ptr(grad_proj), ptr(grad_sigma)),
              "sn_sampler_step_loss_keys")
        # the deferred launch (closing kernel of the conv backward) still reads these: the caller keeps them until then
        return gQ, gT, ((gsig, gl, T) if deferred_tail is not None else None)
    if grad_proj is not None or grad_sigma is not None:
        raise ValueError("step_loss_backward: an explicit grad_proj / grad_sigma needs the keys-mode step")
    check(lib.sn_sampler_step_loss_backward(B, N, M, K, ptr(x), BNC, ptr(y), ptr(state.idx), ptr(state.idx_q), ptr(state.idx_p),
                                            ptr(state.argmax1), ptr(T), min_sigma, alpha, lmbda, weight, ptr(gl), ptr(gQ),
                                            ptr(gsig), ptr(gT), ptr(dpart), ptr(dloss), _stream(y)), "sn_sampler_step_loss_backward")
    return gQ, gT, None


# --------------------------------------------------------------------------------------------- EMD
def approx_match(xyz1, xyz2):
    """xyz1 (B,n,3), xyz2 (B,m,3) -> match (B,m,n); no gradient (tf_approxmatch.py:13-24)."""
    _need_gpu(xyz1, xyz2)
    xyz1, xyz2 = _f32c(xyz1.detach()), _f32c(xyz2.detach())
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    match = torch.empty(b, m, n, device=xyz1.device, dtype=torch.float32)
    ws = torch.empty(max(1, lib.sn_workspace_bytes(b"approxmatch", b, n, m, 0) // 4), device=xyz1.device, dtype=torch.float32)
    with torch.cuda.device(xyz1.device):
        check(lib.sn_approxmatch(b, n, m, ptr(xyz1), ptr(xyz2), ptr(match), ptr(ws), _stream(xyz1)), "sn_approxmatch")
    return match


class MatchCostFunction(torch.autograd.Function):
    """cost (B,) = sum match * distance; gradient to xyz1 / xyz2 with match constant (tf_approxmatch.py:34-64)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, match):
        _need_gpu(xyz1, xyz2, match)
        xyz1, xyz2, match = _f32c(xyz1), _f32c(xyz2), _f32c(match)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        cost = torch.empty(b, device=xyz1.device, dtype=torch.float32)
        ws = torch.empty(max(1, lib.sn_workspace_bytes(b"matchcost", b, n, m, 0) // 4), device=xyz1.device, dtype=torch.float32)
        with torch.cuda.device(xyz1.device):
            check(lib.sn_matchcost(b, n, m, ptr(xyz1), ptr(xyz2), ptr(match), ptr(cost), ptr(ws), _stream(xyz1)), "sn_matchcost")
        ctx.save_for_backward(xyz1, xyz2, match)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        xyz1, xyz2, match = ctx.saved_tensors
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        g1 = torch.empty_like(xyz1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(xyz2) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(xyz1.device):
            check(lib.sn_matchcost_grad(b, n, m, ptr(xyz1), ptr(xyz2), ptr(match), ptr(g1), ptr(g2), _stream(xyz1)),
                  "sn_matchcost_grad")
        gc = grad_cost.reshape(b, 1, 1)
        return (g1 * gc if g1 is not None else None), (g2 * gc if g2 is not None else None), None


match_cost = MatchCostFunction.apply


class EmdLossFunction(torch.autograd.Function):
    """cost (B,) = match_cost(xyz1, xyz2, approx_match(xyz1, xyz2)) in one call, WITHOUT the (B,m,n) match matrix
    (sn_emd_loss / sn_emd_loss_fast): forward runs the auction and the cost / gradient sweep(s) -- the default form ONE sweep that
    evaluates every pair's match value once for cost and both gradients, the exact form two order-preserving ones --; backward
    scales the saved gradients (match is a constant of the gradient, tf_approxmatch.py:54-64).
    exact=False (default): the reference op's own exponential (__expf = v_exp_f32(x log2 e), tf_approxmatch_g.cu:52,97,151) -- the
    cost within 1e-5 of the oracle; exact=True: the compensated exponential of approx_match -- cost and the xyz1 gradient bit for
    bit those of match_cost(approx_match(...))."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, exact=False):
        _need_gpu(xyz1, xyz2)
        x1, x2 = _f32c(xyz1), _f32c(xyz2)
        b, n, _ = x1.shape
        m = x2.shape[1]
        cost = torch.empty(b, device=x1.device, dtype=torch.float32)
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g1 = torch.empty_like(x1) if need1 else None
        g2 = torch.empty_like(x2) if need2 else None
        # (measured and not kept, round 5: the batch split into 2..8 independent chains of clouds on side streams, to keep the
        #  chip full across the 21 dependent launches of 1600 equal waves on 1024 SIMDs -- 3.19 -> 4.5 .. 9.0 ms: launches of
        #  different streams did not overlap on this stack)
        fn = lib.sn_emd_loss if exact else lib.sn_emd_loss_fast
        ws = torch.empty(max(1, lib.sn_workspace_bytes(b"emd_loss", b, n, m, 0) // 4), device=x1.device, dtype=torch.float32)
        with torch.cuda.device(x1.device):
            check(fn(b, n, m, ptr(x1), ptr(x2), ptr(cost), ptr(g1), ptr(g2), ptr(ws), _stream(x1)), "sn_emd_loss" if exact else "sn_emd_loss_fast")
        ctx.save_for_backward(g1, g2)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        g1, g2 = ctx.saved_tensors
        gc = grad_cost.reshape(-1, 1, 1)
        return (g1 * gc if g1 is not None else None), (g2 * gc if g2 is not None else None), None


def emd_loss(xyz1, xyz2, exact=False):
    """EMD loss without the match matrix.  DEFAULT (exact=False, since round 5): the reference GPU op's own exponential (__expf) --
    the cost within 1e-5 of match_cost(approx_match(...)), gradients within 1e-4 of their norm / 2e-3 of their scale per component
    (they follow the transport plan, whose entries the reference itself only pins to 1e-2 between its CPU and GPU ops).
    exact=True: cost and the xyz1 gradient bit for bit those of the three-call composition, ~1.3x slower."""
    return EmdLossFunction.apply(xyz1, xyz2, exact)


# --------------------------------------------------------------------------------------------- pose-error terms
class PoseErrorFunction(torch.autograd.Function):
    """est, gt (B,7) rows [quaternion (w,x,y,z) | translation] -> rot_err, norm_err, trans_err (B,) and their batch means (3,)
    (registration/src/qdataset.py:62-95 compute_errors) -- sn_pose_error_forward / _backward, one launch each way.  rot_err and
    component 0 of the means are metrics: non-differentiable.  No gradient flows to gt."""

    @staticmethod
    def forward(ctx, est, gt):
        _need_gpu(est, gt)
        est, gt = _f32c(est), _f32c(gt)
        if est.dim() != 2 or est.shape[1] != 7 or gt.shape != est.shape:
            raise ValueError("pose_errors: est and gt must both be (B,7), got %s and %s" % (tuple(est.shape), tuple(gt.shape)))
        B = est.shape[0]
        e = lambda *shape: torch.empty(shape, device=est.device, dtype=torch.float32)  # noqa: E731
        rot, nrm, trn, means = e(B), e(B), e(B), e(3)
        with torch.cuda.device(est.device):
            check(lib.sn_pose_error_forward(B, ptr(est), ptr(gt), ptr(rot), ptr(nrm), ptr(trn), ptr(means), _stream(est)),
                  "sn_pose_error_forward")
        ctx.save_for_backward(est, gt)
        ctx.mark_non_differentiable(rot)
        ctx.set_materialize_grads(False)
        return rot, nrm, trn, means

    @staticmethod
    def backward(ctx, _g_rot, g_nrm, g_trn, g_means):
        est, gt = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        if g_nrm is None and g_trn is None and g_means is None:
            return torch.zeros_like(est), None
        c = lambda g: None if g is None else g.contiguous().float()  # noqa: E731
        g_nrm, g_trn, g_means = c(g_nrm), c(g_trn), c(g_means)
        g_est = torch.empty_like(est)
        with torch.cuda.device(est.device):
            check(lib.sn_pose_error_backward(est.shape[0], ptr(est), ptr(gt), ptr(g_means), ptr(g_nrm), ptr(g_trn), ptr(g_est),
                                             _stream(est)), "sn_pose_error_backward")
        return g_est, None


def pose_errors(est, gt):
    """Per-cloud (rot_err [radians], norm_err, trans_err), each (B,), of the poses est against gt ((B,7) rows
    [quaternion (w,x,y,z) | translation]); differentiable in norm_err and trans_err with respect to est."""
    return PoseErrorFunction.apply(est, gt.detach())[:3]


_POSE_ZERO = {}  # device -> a (1,) zero (made outside captures; a constant of the graphs that use it)


class PoseErrorMeansFunction(torch.autograd.Function):
    """est, gt (B,7) -> the batch means rot_err, norm_err, trans_err as three 0-d tensors (compute_errors' return, qdataset.py:95):
    one sn_pose_error_forward launch.  Backward: the (3,) upstream vector of sn_pose_error_backward is put together by ONE cat
    launch from the scalars autograd hands over (a missing one is a cached zero), then the one backward launch."""

    @staticmethod
    def forward(ctx, est, gt):
        _need_gpu(est, gt)
        est, gt = _f32c(est), _f32c(gt)
        if est.dim() != 2 or est.shape[1] != 7 or gt.shape != est.shape:
            raise ValueError("pose errors: est and gt must both be (B,7), got %s and %s" % (tuple(est.shape), tuple(gt.shape)))
        means = torch.empty(3, device=est.device, dtype=torch.float32)
        with torch.cuda.device(est.device):
            check(lib.sn_pose_error_forward(est.shape[0], ptr(est), ptr(gt), None, None, None, ptr(means), _stream(est)),
                  "sn_pose_error_forward")
        ctx.save_for_backward(est, gt)
        ctx.set_materialize_grads(False)
        rot, nrm, trn = means.unbind(0)
        ctx.mark_non_differentiable(rot)
        return rot, nrm, trn

    @staticmethod
    def backward(ctx, _g_rot, g_nrm, g_trn):
        est, gt = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        if g_nrm is None and g_trn is None:
            return torch.zeros_like(est), None
        zero = _POSE_ZERO.get(est.device)
        if zero is None:
            zero = torch.zeros(1, device=est.device, dtype=torch.float32)
            if not torch.cuda.is_current_stream_capturing():
                _POSE_ZERO[est.device] = zero
        one = lambda g: zero if g is None else g.reshape(1).float()  # noqa: E731
        g_means = torch.cat((zero, one(g_nrm), one(g_trn)))  # (component 0 is not read)
        g_est = torch.empty_like(est)
        with torch.cuda.device(est.device):
            check(lib.sn_pose_error_backward(est.shape[0], ptr(est), ptr(gt), ptr(g_means), None, None, ptr(g_est), _stream(est)),
                  "sn_pose_error_backward")
        return g_est, None


def pose_error_means(est, gt):
    """The batch means (rot_err, norm_err, trans_err) as 0-d tensors -- compute_errors' return (qdataset.py:95); rot_err is a
    metric: non-differentiable."""
    return PoseErrorMeansFunction.apply(est, gt.detach())


def chamfer_mean_per_cloud(xyz1, xyz2):
    """mean_n d(xyz1[b] -> xyz2[b]) + mean_m d(xyz2[b] -> xyz1[b]) for every cloud pair, (B,): the Chamfer term of
    registration/main.py:573-577 / 549-554 per item of a batch (forward only: the scan + one reduction launch)."""
    with torch.no_grad():
        _x1, _x2, dist1, _i1, dist2, _i2 = chamfer_forward_impl(xyz1, xyz2)
        B, n1 = dist1.shape
        out = torch.empty(B, device=dist1.device, dtype=torch.float32)
        with torch.cuda.device(dist1.device):
            check(lib.sn_chamfer_mean_per_cloud(B, n1, dist2.shape[1], ptr(dist1), ptr(dist2), ptr(out), _stream(dist1)),
                  "sn_chamfer_mean_per_cloud")
    return out


# --------------------------------------------------------------------------------------------- classification terms
class ClassificationTermsFunction(torch.autograd.Function):
    """logits (B,C), labels (B,) -> ce (B,), pred (B,) int32, correct (B,) int32, means (2,) = the batch means of ce and correct
    (pointnet_cls.py:117-122, evaluate_samplenet.py:237-262) -- sn_classification_terms_forward / _backward, one launch each way.
    Gradients flow to the logits through ce and means[0]; means[1] (accuracy) is a metric: its upstream component is not read."""

    @staticmethod
    def forward(ctx, logits, labels):
        _need_gpu(logits, labels)
        logits = _f32c(logits)
        if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
            raise ValueError("classification_terms: logits (B,C) and labels (B,), got %s and %s" % (tuple(logits.shape), tuple(labels.shape)))
        labels = labels.contiguous().int()
        B, C = logits.shape
        ce = torch.empty(B, device=logits.device, dtype=torch.float32)
        pred = torch.empty(B, device=logits.device, dtype=torch.int32)
        correct = torch.empty(B, device=logits.device, dtype=torch.int32)
        means = torch.empty(2, device=logits.device, dtype=torch.float32)
        with torch.cuda.device(logits.device):
            check(lib.sn_classification_terms_forward(B, C, ptr(logits), ptr(labels), ptr(ce), ptr(pred), ptr(correct), ptr(means),
                                                      _stream(logits)), "sn_classification_terms_forward")
        ctx.save_for_backward(logits, labels)
        ctx.mark_non_differentiable(pred, correct)
        ctx.set_materialize_grads(False)
        return ce, pred, correct, means

    @staticmethod
    def backward(ctx, g_ce, _g_pred, _g_correct, g_means):
        logits, labels = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        if g_ce is None and g_means is None:
            return torch.zeros_like(logits), None
        c = lambda g: None if g is None else g.contiguous().float()  # noqa: E731
        g_ce, g_means = c(g_ce), c(g_means)
        g_logits = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            check(lib.sn_classification_terms_backward(logits.shape[0], logits.shape[1], ptr(logits), ptr(labels), ptr(g_means),
                                                       ptr(g_ce), ptr(g_logits), _stream(logits)), "sn_classification_terms_backward")
        return g_logits, None


def classification_terms(logits, labels):
    """-> (ce (B,), pred (B,) int32, correct (B,) int32, means (2,)): the per-item softmax cross-entropy, numpy's argmax of the
    logits, pred == label, and the batch means (loss, accuracy); differentiable in ce and means[0] with respect to the logits."""
    return ClassificationTermsFunction.apply(logits, labels.detach())


class ClassificationMeanLossFunction(torch.autograd.Function):
    """logits (B,C), labels (B,) -> the batch mean of the softmax cross-entropy as a 0-d tensor (pointnet_cls.py:117-122): means[0] of
    sn_classification_terms_forward with no per-item output, and sn_classification_terms_backward with the upstream SCALAR itself as
    g_means (the entry reads g_means[0] only) -- one launch each way, nothing in between (selecting means[0] of classification_terms
    costs a zero-fill and a copy in the backward)."""

    @staticmethod
    def forward(ctx, logits, labels):
        _need_gpu(logits, labels)
        logits = _f32c(logits)
        if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
            raise ValueError("classification_mean_loss: logits (B,C) and labels (B,), got %s and %s" % (tuple(logits.shape), tuple(labels.shape)))
        labels = labels.contiguous().int()
        means = torch.empty(2, device=logits.device, dtype=torch.float32)
        with torch.cuda.device(logits.device):
            check(lib.sn_classification_terms_forward(logits.shape[0], logits.shape[1], ptr(logits), ptr(labels), None, None, None,
                                                      ptr(means), _stream(logits)), "sn_classification_terms_forward")
        ctx.save_for_backward(logits, labels)
        return means[0]

    @staticmethod
    def backward(ctx, g):
        logits, labels = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        g = g.contiguous().float()
        g_logits = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            check(lib.sn_classification_terms_backward(logits.shape[0], logits.shape[1], ptr(logits), ptr(labels), ptr(g), None,
                                                       ptr(g_logits), _stream(logits)), "sn_classification_terms_backward")
        return g_logits, None


def classification_mean_loss(logits, labels):
    """classification_terms' means[0] alone, as a 0-d tensor differentiable in the logits: what classification_loss(fused=True) adds
    its regulariser to."""
    return ClassificationMeanLossFunction.apply(logits, labels.detach())


# --------------------------------------------------------------------------------------------- segmentation terms
def _seg_rows(logits, labels, who):
    """-> (rows (B,N,C) float32 contiguous, transposed): logits given as (B,N,C), or as (B,C,N) when that is a transposed view of
    contiguous (B,N,C) rows -- taken without a copy either way (pointnet2_modules._rows_of's rule)."""
    if logits.dim() != 3 or labels.dim() != 2:
        raise ValueError("%s: logits (B,N,C) or (B,C,N) and labels (B,N), got %s and %s" % (who, tuple(logits.shape), tuple(labels.shape)))
    if logits.dtype != torch.float32:
        logits = logits.float()
    as_given = tuple(logits.shape[:2]) == tuple(labels.shape)
    flipped = (logits.shape[0], logits.shape[2]) == tuple(labels.shape)
    if as_given and (logits.is_contiguous() or not flipped or not logits.transpose(1, 2).is_contiguous()):
        return logits.contiguous(), False
    if flipped:
        return logits.transpose(1, 2).contiguous(), True
    raise ValueError("%s: logits %s do not go with labels %s" % (who, tuple(logits.shape), tuple(labels.shape)))


def _seg_weights(class_weights, rows, who):
    if class_weights is None:
        return None
    _need_gpu(class_weights)
    if class_weights.dim() != 1 or class_weights.shape[0] != rows.shape[2]:
        raise ValueError("%s: class_weights must be (%d,), got %s" % (who, rows.shape[2], tuple(class_weights.shape)))
    return class_weights.detach().contiguous().float()


def _seg_forward(rows, labels, weights, ce, pred, counts, means):
    B, N, C = rows.shape
    work = None
    if means is not None:
        work = torch.empty(max(1, lib.sn_segmentation_terms_workspace_bytes(B * N, C)), device=rows.device, dtype=torch.uint8)
    with torch.cuda.device(rows.device):
        check(lib.sn_segmentation_terms_forward(B * N, max(N, 1), C, ptr(rows), ptr(labels), ptr(weights), ptr(ce), ptr(pred), ptr(counts),
                                                ptr(means), ptr(work), _stream(rows)), "sn_segmentation_terms_forward")


def _seg_backward(rows, labels, weights, means, g_means, g_ce):
    B, N, C = rows.shape
    g_rows = torch.empty_like(rows)
    with torch.cuda.device(rows.device):
        check(lib.sn_segmentation_terms_backward(B * N, C, ptr(rows), ptr(labels), ptr(weights), ptr(means), ptr(g_means), ptr(g_ce),
                                                 ptr(g_rows), _stream(rows)), "sn_segmentation_terms_backward")
    return g_rows


class SegmentationTermsFunction(torch.autograd.Function):
    """logits (B,N,C) [or the (B,C,N) transposed view], labels (B,N), class_weights (C,) or None -> ce (B,N), pred (B,N) int32,
    cloud_counts (B,C,3) int32, means (3,) -- sn_segmentation_terms_forward (the terms and the closing sum) / _backward, one launch.
    Gradients flow to the logits through ce and means[0]; means[1] and means[2] are not differentiated."""

    @staticmethod
    def forward(ctx, logits, labels, class_weights):
        _need_gpu(logits, labels)
        rows, flipped = _seg_rows(logits, labels, "segmentation_terms")
        weights = _seg_weights(class_weights, rows, "segmentation_terms")
        labels = labels.contiguous().int()
        B, N, C = rows.shape
        ce = torch.empty(B, N, device=rows.device, dtype=torch.float32)
        pred = torch.empty(B, N, device=rows.device, dtype=torch.int32)
        counts = torch.empty(B, C, 3, device=rows.device, dtype=torch.int32)
        means = torch.empty(3, device=rows.device, dtype=torch.float32)
        _seg_forward(rows, labels, weights, ce, pred, counts, means)
        ctx.save_for_backward(rows, labels, weights, means)
        ctx.flipped = flipped
        ctx.mark_non_differentiable(pred, counts)
        ctx.set_materialize_grads(False)
        return ce, pred, counts, means

    @staticmethod
    def backward(ctx, g_ce, _g_pred, _g_counts, g_means):
        rows, labels, weights, means = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        if g_ce is None and g_means is None:
            g_rows = torch.zeros_like(rows)
        else:
            c = lambda g: None if g is None else g.contiguous().float()  # noqa: E731
            g_rows = _seg_backward(rows, labels, weights, means, c(g_means), c(g_ce))
        return (g_rows.transpose(1, 2) if ctx.flipped else g_rows), None, None


def segmentation_terms(logits, labels, class_weights=None):
    """-> (ce (B,N), pred (B,N) int32, cloud_counts (B,C,3) int32, means (3,)): the per-point softmax cross-entropy (0 on an ignored
    point: any label outside [0, C)), numpy's argmax of the logits, per cloud and class the counts (labelled, predicted, correct) over
    the valid points, and (the weighted mean loss of F.cross_entropy(weight=), correct / valid, the sum of the valid points' weights).
    logits: (B,N,C), or (B,C,N) when that is a transposed view of (B,N,C) rows (no copy).  Differentiable in ce and means[0] with
    respect to the logits."""
    return SegmentationTermsFunction.apply(logits, labels.detach(), class_weights)


class SegmentationMeanLossFunction(torch.autograd.Function):
    """segmentation_terms' means[0] alone as a 0-d tensor: the forward with no per-point output, and the backward with the upstream
    SCALAR itself as g_means -- ClassificationMeanLossFunction's twin."""

    @staticmethod
    def forward(ctx, logits, labels, class_weights):
        _need_gpu(logits, labels)
        rows, flipped = _seg_rows(logits, labels, "segmentation_mean_loss")
        weights = _seg_weights(class_weights, rows, "segmentation_mean_loss")
        labels = labels.contiguous().int()
        means = torch.empty(3, device=rows.device, dtype=torch.float32)
        _seg_forward(rows, labels, weights, None, None, None, means)
        ctx.save_for_backward(rows, labels, weights, means)
        ctx.flipped = flipped
        return means[0]

    @staticmethod
    def backward(ctx, g):
        rows, labels, weights, means = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g_rows = _seg_backward(rows, labels, weights, means, g.contiguous().float(), None)
        return (g_rows.transpose(1, 2) if ctx.flipped else g_rows), None, None


def segmentation_mean_loss(logits, labels, class_weights=None):
    """segmentation_terms' means[0] alone, as a 0-d tensor differentiable in the logits: what segmentation_loss(fused=True) returns."""
    return SegmentationMeanLossFunction.apply(logits, labels.detach(), class_weights)

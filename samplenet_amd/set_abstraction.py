"""The shared MLP and max-pool of a PointNet++ set-abstraction level on the HIP GEMM walk.

    grouped rows (G, S, Ci), channels contiguous  ->  relu(bn(conv_1x1(.))) x L  ->  max over the S rows of a group  ->  (G, Co)

with G = B * npoint groups of S = nsample rows (ops.ball_group_rows writes them in this layout), or G = B, S = N for a group-all level.
The layers run on pointnet.py's layer-by-layer walk (_conv_stack_fwd, _conv_stack_bwd: the GEMM entries with fused BatchNorm of the
sampler's own head), differentiable towards the rows (input_grad=True) and, in training mode, the parameters.  The pool is one of two
pairs, picked by group_pool_route(G, S): sn_group_pool_forward / sn_group_pool_backward + sn_bn_backward_coef (a wave per group and
64 channels: many small groups), or sn_pool_forward / sn_pool_backward_bn (a workgroup per group: few large groups).  The forward
outputs of the two are bit-identical; their BatchNorm-backward sums differ in order, each fixed.

The layer records are built from the Conv2d / BatchNorm2d modules of the pointnet2 stand-in's shared_mlp: a (Co, Ci, 1, 1) weight has
the memory of (Co, Ci).  With a BatchNorm the conv has no bias: the GEMMs get NULL, and the walk's bias-gradient outputs (the sum of
dZ, which the kernels write in any case) land in scratch tensors handed over as its sink.
BatchNorm follows torch: .train() = batch statistics and a running-statistics update, .eval() = running statistics; weight gradients
need training mode.  No float atomics anywhere on this route.  Capturing the node's backward in a graph is not supported."""
import torch

from . import pointnet
from ._lib import check, lib, ptr, stream_of

_EVAL_WGRAD = ("samplenet_amd.set_abstraction: weight gradients need training mode (.train()); an eval-mode module is differentiated "
               "w.r.t. its input only -- freeze it with requires_grad_(False)")

# Test hook: None = group_pool_route's rule, True / False = that pair wherever it is legal.
FORCE_GROUP_POOL = None


def group_pool_route(G, S):
    """True: the group-pool pair serves (G groups, S rows each).  The rule is what tools/sa_bench.py's pool table supports
    (profiles/sa/sa_bench.txt): the new pair where it won by more than the larger spread."""
    if FORCE_GROUP_POOL is not None:
        return bool(FORCE_GROUP_POOL)
    return S <= 128 and G >= 256


def layer_records(mlp):
    """pointnet._Layer records of a shared_mlp Sequential whose every layer has a BatchNorm, named by their state-dict prefixes."""
    out = []
    for j, m in enumerate(mlp):
        if getattr(m, "bn", None) is None or m.conv.bias is not None or m.conv.kernel_size != (1, 1):
            raise ValueError("set_abstraction: the fused route needs 1 x 1 convolutions without bias, each followed by a BatchNorm")
        out.append(pointnet._Layer("%d.conv" % j, m.conv, "%d.bn" % j, m.bn))
    return out


def fused_supported(mlp):
    """The walk's backward starts at a pooled top layer and ends at a first layer below it: two layers at least, each with BatchNorm."""
    return len(mlp) >= 2 and all(getattr(m, "bn", None) is not None for m in mlp)


def _params(layers):
    return [L.W for L in layers] + [p for L in layers for p in (L.bn.weight, L.bn.bias)]


def _param_names(layers):
    return [L.name + ".weight" for L in layers] + [L.bn_name + k for L in layers for k in (".weight", ".bias")]


class _SetAbstractionFunction(torch.autograd.Function):
    """rows (G, S, Ci) -> pooled (G, Co), argsel (G, Co) int32: the shared MLP and the max over every group's rows."""

    @staticmethod
    def forward(ctx, layers, training, group_pool, rows, *params):
        G, S, _ = rows.shape
        Co = layers[-1].Co
        with torch.cuda.device(rows.device):
            pooled, argsel, zsel = pointnet._pool_bufs(G, Co, rows)
            zc, cc = pointnet._conv_stack_fwd(layers, rows, training, None)
            fn, name = (lib.sn_group_pool_forward, "sn_group_pool_forward") if group_pool else (lib.sn_pool_forward, "sn_pool_forward")
            check(fn(G, S, Co, ptr(zc[-1]), ptr(cc[-1]), ptr(pooled), ptr(argsel), ptr(zsel), stream_of(rows)), name)
        ctx.layers, ctx.training, ctx.group_pool = layers, bool(training), bool(group_pool)
        ctx.saved = {"x": rows, "B": G, "N": S, "zc": zc, "cc": cc, "pooled": pooled, "argsel": argsel, "zsel": zsel}
        ctx.mark_non_differentiable(argsel)
        return pooled, argsel

    @staticmethod
    def backward(ctx, g, _ga):
        layers, saved = ctx.layers, ctx.saved
        fixed = not ctx.training
        trainable = any(ctx.needs_input_grad[4:])
        if trainable and fixed:
            raise RuntimeError(_EVAL_WGRAD)
        g = g.contiguous().float()
        top = layers[-1]
        G, S, C = saved["B"], saved["N"], top.Co
        grads = {}
        with torch.cuda.device(g.device):
            # the convs have no bias: the kernels' bias-gradient outputs go to scratch
            sink = {L.name + ".bias": torch.empty(L.Co, device=g.device, dtype=torch.float32) for L in layers}
            if ctx.group_pool:
                coef = saved["cc"][-1]
                gsel = torch.empty(G, C, device=g.device, dtype=torch.float32)
                nblk = lib.sn_group_pool_stats_blocks(G)
                stats = None if fixed else torch.empty(nblk, 2, C, device=g.device, dtype=torch.float32)
                check(lib.sn_group_pool_backward(G, C, ptr(g), ptr(saved["pooled"]), ptr(saved["zsel"]), ptr(gsel), ptr(stats),
                                                 stream_of(g)), "sn_group_pool_backward")
                if fixed:
                    kcoef = torch.zeros(3, C, device=g.device, dtype=torch.float32)
                    kcoef[0].copy_(coef[0])
                else:
                    dgam, dbet, _, kcoef = pointnet._bn_bwd(top, G * S, stats, nblk, coef, sink, top.bn_name, top.name)
                    grads[top.bn_name + ".weight"], grads[top.bn_name + ".bias"] = dgam, dbet
            else:
                gsel, kcoef = pointnet._pool_bwd_bn(top, saved, g, fixed, sink, grads)
            gx = pointnet._conv_stack_bwd(layers, saved, gsel, kcoef, fixed, grads, sink=sink, wgrads=not fixed,
                                          input_grad=ctx.needs_input_grad[3])
        out = [None] * (3 * len(layers))
        if trainable:
            out = [grads[n] if ctx.needs_input_grad[4 + j] else None for j, n in enumerate(_param_names(layers))]
        return (None, None, None, None if gx is None else gx.view(saved["x"].shape)) + tuple(out)


def grouped_mlp_max(mlp, rows, return_argsel=False):
    """rows (G, S, Ci) float32 on the GPU, mlp a shared_mlp Sequential (fused_supported) -> (G, mlp[-1] width): relu(bn(conv)) per
    layer on every row, then the max over each group's S rows.  mlp.training selects batch or running statistics."""
    if not rows.is_cuda:
        raise RuntimeError("samplenet_amd.set_abstraction runs on the GPU only (got a %s tensor); no CPU fallback exists" % rows.device)
    if not fused_supported(mlp):
        raise ValueError("set_abstraction: the fused route needs at least two layers, each with a BatchNorm")
    layers = layer_records(mlp)
    if rows.dim() != 3 or rows.shape[2] != layers[0].Ci or rows.shape[0] * rows.shape[1] == 0:
        raise ValueError("set_abstraction: rows must be (G, S, %d) with G, S >= 1, got %s" % (layers[0].Ci, tuple(rows.shape)))
    G, S, _ = rows.shape
    pooled, argsel = _SetAbstractionFunction.apply(layers, mlp.training, group_pool_route(G, S), rows.contiguous().float(), *_params(layers))
    return (pooled, argsel) if return_argsel else pooled

"""The one autograd node of "relu(bn(conv_1x1(.))) x L on rows, then a max over each group of rows": the shell around pointnet.py's
layer-by-layer walk (_conv_stack_fwd, _pool_bwd_bn, _conv_stack_bwd) that the classifier's stacks, the autoencoder's encoder and the
set-abstraction MLP share.  What the callers do differently is a StackSpec, nothing else:

                     pool           owner (one-call forward)   walk_wgrads             eval_wgrad_error
    classifier       POINTS / NONE  None                       a parameter asks        raises
    autoencoder      POINTS         the module (CONV_STACK)    a parameter asks        None: fixed statistics, allowed
    set abstraction  POINTS/GROUPS  None                       the module is training  raises
    feature propag.  ROWS           None                       the module is training  raises

A layer without a bias (L.b is None) gets NULL in the GEMMs and a scratch entry in the walk's sink for the bias-gradient output the
kernels write in any case.  Parameters: pointnet.stack_params(layers), gradients returned in that order.
"""
from collections import namedtuple

import torch

from . import pointnet
from ._lib import check, lib, ptr, stream_of

# pool: the max over a group's rows and its backward
POOL_POINTS = "points"  # sn_pool_forward / sn_pool_backward_bn (a workgroup per group)
POOL_GROUPS = "groups"  # sn_group_pool_forward / sn_group_pool_backward + sn_bn_backward_coef (a wave per group and 64 channels)
POOL_NONE = "none"      # the activated rows themselves: sn_bn_relu_forward / _backward, torch sums for the top BatchNorm
POOL_ROWS = "rows"      # POOL_NONE's forward; backward: sn_bn_relu_backward_stats, dY and the top BatchNorm's sums in one launch
# walk_wgrads: when the backward walk is the one that also forms weight gradients
WGRADS_ASKED = "asked"        # a parameter asks for a gradient
WGRADS_TRAINING = "training"  # the forward ran on batch statistics, frozen parameters or not

StackSpec = namedtuple("StackSpec", "layers training pool owner walk_wgrads eval_wgrad_error")
# layers: pointnet._Layer records.  owner: the module that keeps the one-call forward's persistent accumulator (_fx_acc), None =
# never the one-call route.  eval_wgrad_error: raised when an eval-mode stack's parameters ask for a gradient, None = allowed.

_WGRAD_NEEDS_TRAINING = ("samplenet_amd.%s: weight gradients need training mode (.train()); an eval-mode %s is differentiated "
                     "w.r.t. its input only -- freeze it with requires_grad_(False)")


def eval_wgrad_error(module, noun):
    return _WGRAD_NEEDS_TRAINING % (module, noun)


class _ConvStackFunction(torch.autograd.Function):
    """x (G, S, Ci) -> (pooled (G, Co), argsel (G, Co) int32), or (activated rows (G, S, Co), None) without a pool.  Differentiable
    w.r.t. x and the layers' parameters."""

    @staticmethod
    def forward(ctx, spec, x, *params):
        layers, training = spec.layers, spec.training
        G, S, _ = x.shape
        top = layers[-1]
        Co = top.Co
        saved = {"x": x, "B": G, "N": S}
        argsel = None
        with torch.cuda.device(x.device):
            if spec.pool in (POOL_NONE, POOL_ROWS):
                saved["zc"], saved["cc"] = pointnet._conv_stack_fwd(layers, x, training, None)
                out = torch.empty(G, S, Co, device=x.device, dtype=torch.float32)
                check(lib.sn_bn_relu_forward(G * S, Co, ptr(saved["zc"][-1]), ptr(saved["cc"][-1]), ptr(out), stream_of(x)),
                      "sn_bn_relu_forward")
            else:
                out, argsel, zsel = pointnet._pool_bufs(G, Co, x)
                saved.update(pooled=out, argsel=argsel, zsel=zsel)
                fuse = (spec.owner is not None and training and G * S > 64 and S % 64 == 0 and Co % 64 == 0 and top.Ci % 64 == 0
                        and pointnet._conv_stack_fx(spec.owner, layers, x, G, S, saved, out, argsel, zsel))
                if fuse:
                    if any(ctx.needs_input_grad):
                        # the per-layer backward reads the xyz layer's output, which the one-call stack may not have kept: rebuilt
                        # here, in the forward, so that a differentiated step issues its launches in one fixed order (nothing when
                        # no gradient is asked)
                        pointnet._z1(layers, saved)
                elif spec.pool == POOL_POINTS:
                    saved["zc"], saved["cc"] = pointnet._conv_stack_fwd(layers, x, training, (out, argsel, zsel))
                else:
                    zc, cc = saved["zc"], saved["cc"] = pointnet._conv_stack_fwd(layers, x, training, None)
                    check(lib.sn_group_pool_forward(G, S, Co, ptr(zc[-1]), ptr(cc[-1]), ptr(out), ptr(argsel), ptr(zsel), stream_of(x)),
                          "sn_group_pool_forward")
                ctx.mark_non_differentiable(argsel)
        ctx.spec, ctx.saved = spec, saved
        return out, argsel

    @staticmethod
    def backward(ctx, g, _ga):
        spec, saved = ctx.spec, ctx.saved
        layers = spec.layers
        fixed = not spec.training
        trainable = any(ctx.needs_input_grad[2:])
        if trainable and fixed and spec.eval_wgrad_error is not None:
            raise RuntimeError(spec.eval_wgrad_error)
        g = g.contiguous().float()
        top = layers[-1]
        G, S, C = saved["B"], saved["N"], top.Co
        R = G * S
        grads = {}
        gsel = dy = None
        with torch.cuda.device(g.device):
            # a conv without bias: the kernels' bias-gradient output goes to scratch
            sink = {L.name + ".bias": torch.empty(L.Co, device=g.device, dtype=torch.float32) for L in layers if L.b is None}
            if spec.pool == POOL_POINTS:
                gsel, kcoef = pointnet._pool_bwd_bn(top, saved, g, fixed, sink, grads)
            else:
                z, coef = saved["zc"][-1], saved["cc"][-1]
                if spec.pool == POOL_GROUPS:
                    gsel = torch.empty(G, C, device=g.device, dtype=torch.float32)
                    nblk = lib.sn_group_pool_stats_blocks(G)
                    stats = None if fixed else torch.empty(nblk, 2, C, device=g.device, dtype=torch.float32)
                    check(lib.sn_group_pool_backward(G, C, ptr(g), ptr(saved["pooled"]), ptr(saved["zsel"]), ptr(gsel), ptr(stats),
                                                     stream_of(g)), "sn_group_pool_backward")
                elif spec.pool == POOL_ROWS and not fixed:
                    dy = torch.empty(R, C, device=g.device, dtype=torch.float32)
                    nblk = lib.sn_bn_relu_stats_blocks(R)
                    stats = torch.empty(nblk, 2, C, device=g.device, dtype=torch.float32)
                    check(lib.sn_bn_relu_backward_stats(R, C, ptr(z), ptr(coef), ptr(g), ptr(dy), ptr(stats), stream_of(g)),
                          "sn_bn_relu_backward_stats")
                else:
                    dy = torch.empty(R, C, device=g.device, dtype=torch.float32)
                    check(lib.sn_bn_relu_backward(R, C, ptr(z), ptr(coef), ptr(g), 0, ptr(dy), stream_of(g)), "sn_bn_relu_backward")
                    if not fixed:  # (POOL_NONE)
                        # (sum dY, sum dY Z) of the top BatchNorm as ONE block of partials; training mode need not be fast
                        stats, nblk = torch.stack((dy.sum(0), (dy * z).sum(0))).view(1, 2, C).contiguous(), 1
                if fixed:
                    kcoef = pointnet._fixed_kcoef(coef)
                else:
                    dgam, dbet, dbias, kcoef = pointnet._bn_bwd(top, R, stats, nblk, coef, sink, top.bn_name, top.name)
                    grads[top.bn_name + ".weight"], grads[top.bn_name + ".bias"], grads[top.name + ".bias"] = dgam, dbet, dbias
            wgrads = trainable if spec.walk_wgrads == WGRADS_ASKED else not fixed
            gx = pointnet._conv_stack_bwd(layers, saved, gsel, kcoef, fixed, grads, sink=sink, wgrads=wgrads,
                                          input_grad=ctx.needs_input_grad[1], dy_top=dy)
        out = [None] * (len(ctx.needs_input_grad) - 2)
        if trainable:
            out = [grads[n] if ctx.needs_input_grad[2 + j] else None for j, n in enumerate(pointnet.stack_param_names(layers))]
        return (None, None if gx is None else gx.view(saved["x"].shape)) + tuple(out)


def conv_stack(spec, x):
    """-> (out, argsel) of the node on x (G, S, Ci) float32 contiguous."""
    return _ConvStackFunction.apply(spec, x, *pointnet.stack_params(spec.layers))

"""The shared MLP and max-pool of a PointNet++ set-abstraction level on the HIP GEMM walk.

    grouped rows (G, S, Ci), channels contiguous  ->  relu(bn(conv_1x1(.))) x L  ->  max over the S rows of a group  ->  (G, Co)

with G = B * npoint groups of S = nsample rows (ops.ball_group_rows writes them in this layout), or G = B, S = N for a group-all level.
The layers run on stack_node.py's node around pointnet.py's layer-by-layer walk (the GEMM entries with fused BatchNorm of the
sampler's own head), differentiable towards the rows (input_grad=True) and, in training mode, the parameters.  The pool is one of two
pairs, picked by group_pool_route(G, S): sn_group_pool_forward / sn_group_pool_backward + sn_bn_backward_coef (a wave per group and
64 channels: many small groups), or sn_pool_forward / sn_pool_backward_bn (a workgroup per group: few large groups).  The forward
outputs of the two are bit-identical; their BatchNorm-backward sums differ in order, each fixed.

The layer records are built from the Conv2d / BatchNorm2d modules of the pointnet2 stand-in's shared_mlp: a (Co, Ci, 1, 1) weight has
the memory of (Co, Ci).  With a BatchNorm the conv has no bias: the GEMMs get NULL, and the walk's bias-gradient outputs (the sum of
dZ, which the kernels write in any case) land in scratch tensors handed over as its sink.
BatchNorm follows torch: .train() = batch statistics and a running-statistics update, .eval() = running statistics; weight gradients
need training mode.  No float atomics anywhere on this route.  Capturing the node's backward in a graph is not supported."""
from . import pointnet, stack_node

_WGRAD_NEEDS_TRAINING = stack_node.eval_wgrad_error("set_abstraction", "module")

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
    # (walks with weight gradients whenever the module is in training mode, frozen or not)
    spec = stack_node.StackSpec(layers, mlp.training, stack_node.POOL_GROUPS if group_pool_route(G, S) else stack_node.POOL_POINTS, None,
                                stack_node.WGRADS_TRAINING, _WGRAD_NEEDS_TRAINING)
    pooled, argsel = stack_node.conv_stack(spec, rows.contiguous().float())
    return (pooled, argsel) if return_argsel else pooled

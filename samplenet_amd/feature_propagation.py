"""The shared MLP of a PointNet++ feature-propagation (up-sampling) level on the HIP GEMM walk: set_abstraction.py's twin.

    rows (B, n, Ci), channels contiguous  ->  relu(bn(conv_1x1(.))) x L  ->  (B, n, Co)

ops.interp_rows writes the rows in this layout (the three-neighbour interpolation of the known features beside the skip features).
The layers run on stack_node.py's node around pointnet.py's layer-by-layer walk, without a pool (POOL_ROWS): the activated rows of
the top layer are the output, and the backward takes dY and the top BatchNorm's partial sums from one launch
(sn_bn_relu_backward_stats) before the walk goes down.  Differentiable towards the rows and, in training mode, the parameters.
BatchNorm follows torch: .train() = batch statistics and a running-statistics update, .eval() = running statistics; weight gradients
need training mode.  No float atomics anywhere on this route.  Capturing the node's backward in a graph is not supported."""
from . import stack_node
from .set_abstraction import layer_records

_WGRAD_NEEDS_TRAINING = stack_node.eval_wgrad_error("feature_propagation", "module")


def fused_supported(mlp):
    """The walk's backward starts at a top layer and ends at a first layer below it: two layers at least, each with BatchNorm; the
    top activation's kernels move four channels at a time, so the top width is a multiple of 4."""
    return (len(mlp) >= 2 and all(getattr(m, "bn", None) is not None for m in mlp) and mlp[-1].conv.out_channels % 4 == 0)


def propagate_mlp(mlp, rows):
    """rows (B, n, Ci) float32 on the GPU, mlp a shared_mlp Sequential (fused_supported) -> (B, n, mlp[-1] width): relu(bn(conv)) per
    layer on every row.  mlp.training selects batch or running statistics."""
    if not rows.is_cuda:
        raise RuntimeError("samplenet_amd.feature_propagation runs on the GPU only (got a %s tensor); no CPU fallback exists" % rows.device)
    if not fused_supported(mlp):
        raise ValueError("feature_propagation: the fused route needs at least two layers, each with a BatchNorm, and a top width that "
                         "is a multiple of 4")
    layers = layer_records(mlp)
    if rows.dim() != 3 or rows.shape[2] != layers[0].Ci or rows.shape[0] * rows.shape[1] == 0:
        raise ValueError("feature_propagation: rows must be (B, n, %d) with B, n >= 1, got %s" % (layers[0].Ci, tuple(rows.shape)))
    # (walks with weight gradients whenever the module is in training mode, frozen or not)
    spec = stack_node.StackSpec(layers, mlp.training, stack_node.POOL_ROWS, None, stack_node.WGRADS_TRAINING, _WGRAD_NEEDS_TRAINING)
    return stack_node.conv_stack(spec, rows.contiguous().float())[0]

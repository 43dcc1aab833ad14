"""The feature-propagation module of Pointnet2_PyTorch's pointnet2_modules, on the kernels of libsamplenet_hip.so:

    PointnetFPModule(mlp, bn=True)(unknown (B,n,3), known (B,m,3), unknow_feats (B,C1,n) or None, known_feats (B,C2,m))
        -> (B, mlp[-1], n)

forward reads as the original's: three_nn (sn_three_nn), the inverse-distance weights 1 / (dist + 1e-8) normalised over the three
neighbours as torch operations, three_interpolate (sn_weighted_gather_forward at k = 3; the features' gradient by inverted index,
ops.ThreeInterpolateFunction) and torch.cat with the skip features; the
shared MLP behind them is plain torch: per layer a 1 x 1 Conv2d (with a bias only without BatchNorm), BatchNorm2d, ReLU, applied on
unsqueeze(-1).  The original's sources are not at hand: the state_dict key names of `self.mlp` ("<i>.conv.weight",
"<i>.bn.weight", ..), the weight expression and the tie order of the query (pointnet2_utils) are AS RECALLED and UNPINNED.
PointnetSAModule and the multi-scale grouping modules are not provided."""
import torch
from torch import nn

from .... import ops


class _ConvBnRelu(nn.Sequential):
    def __init__(self, cin, cout, bn):
        super().__init__()
        self.add_module("conv", nn.Conv2d(cin, cout, kernel_size=1, bias=not bn))
        if bn:
            self.add_module("bn", nn.BatchNorm2d(cout))
        self.add_module("activation", nn.ReLU(inplace=True))


def shared_mlp(sizes, bn=True):
    """sizes [c0, c1, ..] -> Sequential of 1 x 1 Conv2d (+ BatchNorm2d) + ReLU layers c0 -> c1 -> .."""
    return nn.Sequential(*[_ConvBnRelu(sizes[i], sizes[i + 1], bn) for i in range(len(sizes) - 1)])


class PointnetFPModule(nn.Module):
    """Propagates the features of a sparse (known) cloud to a dense (unknown) one.  mlp: the layer widths, mlp[0] = C2 + C1."""

    def __init__(self, mlp, bn=True):
        super().__init__()
        self.mlp = shared_mlp(list(mlp), bn=bn)

    def forward(self, unknown, known, unknow_feats, known_feats):
        if known is not None:
            dist, idx = ops.three_nn(unknown, known)
            dist_recip = 1.0 / (dist + 1e-8)
            weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
            interpolated = ops.three_interpolate(known_feats, idx, weight)
            new_features = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        else:
            interpolated = known_feats.expand(*(tuple(known_feats.shape[:2]) + (unknown.shape[1],)))
            new_features = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        return self.mlp(new_features.unsqueeze(-1)).squeeze(-1)

"""The modules of Pointnet2_PyTorch's pointnet2_modules, on the kernels of libsamplenet_hip.so:

    PointnetFPModule(mlp, bn=True, fused=False)(unknown (B,n,3), known (B,m,3), unknow_feats (B,C1,n) or None, known_feats (B,C2,m))
        -> (B, mlp[-1], n)
    PointnetSAModuleMSG(npoint, radii, nsamples, mlps, bn=True, use_xyz=True)(xyz (B,N,3), features (B,C,N) or None)
        -> (new_xyz (B,npoint,3), new_features (B, sum of mlp[-1], npoint))
    PointnetSAModule(mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True): one scale; npoint=None groups the whole
        cloud (GroupAll) and returns new_xyz = None

PointnetFPModule.forward reads as the original's: three_nn (sn_three_nn), the inverse-distance weights 1 / (dist + 1e-8) normalised
over the three neighbours as torch operations, three_interpolate (sn_weighted_gather_forward at k = 3; the features' gradient by
inverted index, ops.ThreeInterpolateFunction) and torch.cat with the skip features; the shared MLP behind them is plain torch: per
layer a 1 x 1 Conv2d (with a bias only without BatchNorm), BatchNorm2d, ReLU, applied on unsqueeze(-1).  That is the default
route; fused=True (opt-in) runs the level in the row layout on ops.interp_rows and the HIP GEMM walk
(samplenet_amd.feature_propagation).

The set-abstraction modules sample their centres with ops.furthest_point_sample, gather them (differentiable towards xyz), group
every ball in the ROW layout (ops.ball_group_rows: one launch, a deterministic gradient by inverted index) and run the shared MLP
and the max over each group on the HIP GEMM walk (samplenet_amd.set_abstraction).  With bn=False, with a one-layer MLP, or when
forward is called with fused=False -- the keyword kept as the test hook and yardstick -- they run the composition a user would
write around this file: QueryAndGroup / GroupAll, the torch shared MLP and F.max_pool2d.

The original's sources are not at hand: the constructor arguments, the members `groupers` / `mlps`, the state_dict key names
("mlp.<i>.conv.weight", "mlps.<s>.<i>.conv.weight", "mlps.<s>.<i>.bn.*"), `spec[0] += 3` with use_xyz, the weight expression and
the tie order of the queries (pointnet2_utils) are AS RECALLED and UNPINNED."""
import torch
import torch.nn.functional as F
from torch import nn

from .... import feature_propagation, ops, set_abstraction
from . import pointnet2_utils


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
    """Propagates the features of a sparse (known) cloud to a dense (unknown) one.  mlp: the layer widths, mlp[0] = C2 + C1.
    fused (the constructor's default, or forward's keyword): with a known cloud and feature_propagation.fused_supported(self.mlp) the
    level runs in the row layout -- sn_three_nn, ops.interp_rows (weights, interpolation and skip columns in one launch, a
    deterministic gradient by inverted index) and the shared MLP on the HIP GEMM walk -- and returns (B, mlp[-1], n) as a transposed
    VIEW of the walk's (B, n, mlp[-1]) rows, which the next fused level reads without a copy (.contiguous() gives channel-major
    memory).  No gradient goes towards the coordinates on either route.  Anything else runs the default route."""

    def __init__(self, mlp, bn=True, fused=False):
        super().__init__()
        self.mlp = shared_mlp(list(mlp), bn=bn)
        self.fused = bool(fused)

    def forward(self, unknown, known, unknow_feats, known_feats, fused=None):
        fused = self.fused if fused is None else fused
        if fused and known is not None and feature_propagation.fused_supported(self.mlp):
            dist2, idx = ops.three_nn(unknown, known, return_dist2=True)
            rows = ops.interp_rows(_rows_of(known_feats), None if unknow_feats is None else _rows_of(unknow_feats), idx, dist2)
            return feature_propagation.propagate_mlp(self.mlp, rows).transpose(1, 2)
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


def _rows_of(features):
    """features (B,C,N) -> (B,N,C) contiguous: no copy when the argument is a transposed view of a contiguous (B,N,C) tensor."""
    t = features.transpose(1, 2)
    return t if t.is_contiguous() else t.contiguous()


class PointnetSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping: npoint centres by farthest-point sampling, per scale a ball of radii[i] with
    nsamples[i] slots, the shared MLP mlps[i] (widths; mlps[i][0] = C, raised by 3 with use_xyz) and the max over the ball; the
    scales' features are concatenated.  npoint=None: one group holding the whole cloud per scale (radii / nsamples are not read)."""

    def __init__(self, npoint, radii, nsamples, mlps, bn=True, use_xyz=True):
        super().__init__()
        if not len(radii) == len(nsamples) == len(mlps):
            raise ValueError("PointnetSAModuleMSG: radii, nsamples and mlps must have one entry per scale")
        self.npoint, self.use_xyz, self.bn = npoint, use_xyz, bn
        self.groupers, self.mlps = nn.ModuleList(), nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            spec = list(spec)
            if use_xyz:
                spec[0] += 3
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            self.mlps.append(shared_mlp(spec, bn=bn))

    def forward(self, xyz, features=None, fused=True):
        new_xyz = None
        if self.npoint is not None:
            fps = ops.furthest_point_sample(xyz, self.npoint)
            new_xyz = ops.gather_operation(xyz.transpose(1, 2).contiguous(), fps).transpose(1, 2).contiguous()
        if features is None and not self.use_xyz:
            raise ValueError("Cannot have not features and not use xyz as a feature!")
        if not (fused and all(set_abstraction.fused_supported(m) for m in self.mlps)):
            outs = []
            for grouper, mlp in zip(self.groupers, self.mlps):
                new = mlp(grouper(xyz, new_xyz, features))                       # (B, C', npoint, nsample)
                outs.append(F.max_pool2d(new, kernel_size=[1, new.size(3)]).squeeze(-1))
            return new_xyz, torch.cat(outs, dim=1)
        B = xyz.shape[0]
        rows_f = None if features is None else _rows_of(features)               # (B,N,C) for every scale
        outs = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            if self.npoint is None:
                parts = ([xyz] if self.use_xyz else []) + ([] if rows_f is None else [rows_f])
                rows = parts[0] if len(parts) == 1 else torch.cat(parts, dim=2)  # (B, N, 3 + C): G = B groups of S = N rows
            else:
                rows = ops.ball_group_rows(grouper.radius, grouper.nsample, xyz, new_xyz, rows_f, use_xyz=self.use_xyz, rule="squared")
                rows = rows.view(B * self.npoint, grouper.nsample, rows.shape[3])
            outs.append(set_abstraction.grouped_mlp_max(mlp, rows).view(B, -1, mlp[-1].conv.out_channels))
        pooled = outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)           # (B, npoint, C')
        return new_xyz, pooled.transpose(1, 2).contiguous()


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction at one scale; npoint=None groups the whole cloud."""

    def __init__(self, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True):
        super().__init__(npoint, [radius], [nsample], [mlp], bn=bn, use_xyz=use_xyz)

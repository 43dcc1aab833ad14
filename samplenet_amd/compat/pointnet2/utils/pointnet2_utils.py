"""The functions of Pointnet2_PyTorch's pointnet2_utils that the reference calls, and the grouping half of that module a
PointNet++-style task network imports beside them, on the kernels of libsamplenet_hip.so:

    grouping_operation(features (B,C,N), idx (B,npoint,nsample) int32) -> (B,C,npoint,nsample)   soft_projection.py:8,86,88
    furthest_point_sample(xyz (B,N,3), npoint) -> idx (B,npoint) int32, no gradient             fps.py:4,35
    gather_operation(features (B,C,N), idx (B,npoint) int32) -> (B,C,npoint)                    fps.py:5,39; random_sampling.py:4,42
    ball_query(radius, nsample, xyz (B,N,3), new_xyz (B,npoint,3)) -> idx (B,npoint,nsample) int32, no gradient
    QueryAndGroup(radius, nsample, use_xyz=True)(xyz, new_xyz, features (B,C,N) or None) -> (B,3+C,npoint,nsample)
    GroupAll(use_xyz=True)(xyz, new_xyz, features (B,C,N) or None) -> (B,3+C,1,N)
    three_nn(unknown (B,n,3), known (B,m,3)) -> dist (B,n,3), idx (B,n,3) int32, no gradient
    three_interpolate(features (B,C,m), idx (B,n,3) int32, weight (B,n,3)) -> (B,C,n)

grouping_operation and gather_operation are differentiable w.r.t. features; QueryAndGroup w.r.t. features, xyz and new_xyz.
ball_query and QueryAndGroup compare d2 < radius^2 (ops' "squared" rule: that module's comparison as recalled, its source not being
at hand -- the reference's own TF op, ops.query_ball_point, compares sqrt(d2) < radius; the two differ only on the boundary).  A
ball with no point in it gives a row of zeros here (point 0 is grouped); short rows repeat their first hit.
three_nn returns the three smallest distances (square roots) ascending by (squared distance, index), ties to the lower index; with
fewer than three known points the missing slots hold index 0 and an infinite distance.  That module's source not being at hand,
the tie order and that filling are as recalled, unpinned.  three_interpolate is differentiable w.r.t. features and weight; the
feature-propagation module on top of the two, PointnetFPModule, lives in pointnet2_modules."""
import torch
from torch import nn

from .... import ops


def grouping_operation(features, idx):
    return ops.grouping_operation(features, idx)


def furthest_point_sample(xyz, npoint):
    return ops.furthest_point_sample(xyz, npoint, ops.BNC)


def gather_operation(features, idx):
    return ops.gather_operation(features, idx)


def ball_query(radius, nsample, xyz, new_xyz):
    return ops.ball_query(radius, nsample, xyz, new_xyz, rule="squared", layout=ops.BNC)[0]


class QueryAndGroup(nn.Module):
    """Groups the points of every ball: one launch forward (ops.ball_group)."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        if features is None and not self.use_xyz:
            raise ValueError("Cannot have not features and not use xyz as a feature!")
        return ops.ball_group(self.radius, self.nsample, xyz, new_xyz, features, use_xyz=self.use_xyz, rule="squared")


class GroupAll(nn.Module):
    """One group holding the whole cloud (plain tensor ops: a transpose and a concatenation)."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)  # (B,3,1,N)
        if features is None:
            return grouped_xyz
        grouped_features = features.unsqueeze(2)        # (B,C,1,N)
        return torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features


def three_nn(unknown, known):
    return ops.three_nn(unknown, known)


def three_interpolate(features, idx, weight):
    return ops.three_interpolate(features, idx, weight)

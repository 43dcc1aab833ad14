"""The functions of Pointnet2_PyTorch's pointnet2_utils that the reference calls, on the kernels of libsamplenet_hip.so:

    grouping_operation(features (B,C,N), idx (B,npoint,nsample) int32) -> (B,C,npoint,nsample)   soft_projection.py:8,86,88
    furthest_point_sample(xyz (B,N,3), npoint) -> idx (B,npoint) int32, no gradient             fps.py:4,35
    gather_operation(features (B,C,N), idx (B,npoint) int32) -> (B,C,npoint)                    fps.py:5,39; random_sampling.py:4,42

grouping_operation and gather_operation are differentiable w.r.t. features."""
from .... import ops


def grouping_operation(features, idx):
    return ops.grouping_operation(features, idx)


def furthest_point_sample(xyz, npoint):
    return ops.furthest_point_sample(xyz, npoint, ops.BNC)


def gather_operation(features, idx):
    return ops.gather_operation(features, idx)

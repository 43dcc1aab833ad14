"""FPSSampler / RandomSampler -- drop-ins for registration/src/fps.py and random_sampling.py, the non-learned baselines of
`registration/main.py --sampler fps|random` (main.py:279-287).

Same constructor, `.name`, shape checks and torch RNG calls (order and devices) as the reference classes, so a seeded run
picks the same points.  Underneath: ops.furthest_point_sample (sampling.hip) and the gather kernels of soft_projection.hip.
Two deliberate differences:
  * FPS reads a `bnc` cloud in place through the kernel's layout argument, and a `bnc` cloud is gathered without a
    transposed copy (ops.group_point);
  * input_shape="bcn": the reference hands the (B,3,N) tensor to an op that reads (B,N,3), and its `permute` shuffles the
    channel axis.  Here the N points of the channel-major cloud are sampled, permuted along the point axis.
"""
import warnings

import torch
import torch.nn as nn

from . import ops


def _check_shapes(who, input_shape, output_shape):
    if input_shape not in ["bcn", "bnc"]:
        raise ValueError("allowed shape are 'bcn' (batch * channels * num_in_points), 'bnc' ")
    if output_shape not in ["bcn", "bnc"]:
        raise ValueError("allowed shape are 'bcn' (batch * channels * num_in_points), 'bnc' ")
    if input_shape != output_shape:
        warnings.warn("%s: input_shape is different to output_shape." % who)


def _gather(x, idx, input_shape, output_shape):
    """The points idx (B,M) of x in input_shape -> (B,M,3) or (B,3,M) in output_shape; differentiable w.r.t. x."""
    if input_shape == "bnc":
        y = ops.group_point(x, idx.unsqueeze(-1)).squeeze(2)  # (B,M,3)
        return y if output_shape == "bnc" else y.permute(0, 2, 1).contiguous()
    y = ops.gather_operation(x, idx)  # (B,3,M)
    return y if output_shape == "bcn" else y.permute(0, 2, 1).contiguous()


class FPSSampler(nn.Module):
    def __init__(self, num_out_points, permute, input_shape="bcn", output_shape="bcn"):
        super().__init__()
        self.num_out_points = num_out_points
        self.permute = permute
        self.name = "fps"
        _check_shapes("FPS", input_shape, output_shape)
        self.input_shape = input_shape
        self.output_shape = output_shape

    def forward(self, x: torch.Tensor):
        bnc = self.input_shape == "bnc"
        if self.permute:  # one torch.randperm(N) on the default device, as fps.py:31-33
            N = x.shape[1] if bnc else x.shape[2]
            x = x[:, torch.randperm(N), :] if bnc else x[:, :, torch.randperm(N)]
        idx = ops.furthest_point_sample(x, self.num_out_points, ops.BNC if bnc else ops.BCN)
        return _gather(x, idx, self.input_shape, self.output_shape)


class RandomSampler(nn.Module):
    def __init__(self, num_out_points, input_shape="bcn", output_shape="bcn"):
        super().__init__()
        self.num_out_points = num_out_points
        self.name = "random"
        _check_shapes("RandomSampler", input_shape, output_shape)
        self.input_shape = input_shape
        self.output_shape = output_shape

    def forward(self, x: torch.Tensor):
        B = x.shape[0]
        N = x.shape[1] if self.input_shape == "bnc" else x.shape[2]
        idx = torch.zeros(B, self.num_out_points, dtype=torch.int32, device=x.device)
        for i in range(B):  # one randperm per cloud on x's device, as random_sampling.py:33-40
            idx[i] = torch.randperm(N, dtype=torch.int32, device=x.device)[: self.num_out_points]
        return _gather(x, idx, self.input_shape, self.output_shape)

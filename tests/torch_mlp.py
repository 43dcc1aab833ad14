"""Test helper: the sampler's feature extractor through plain torch.nn modules (the reference's own op chain,
registration/src/samplenet.py:90-104) on the SAME parameters -- the fp32 / fp64 yardstick the HIP MLP kernels are compared
with.  Lives in tests/ on purpose: the product module has no torch route.  Also here: the sampler variants' constructor
arguments, the accuracy bar against fp64 that the parity tests share, and one whole training step of the sampler in plain
torch."""
import copy

import torch
import torch.nn.functional as F

from samplenet_amd import SampleNet

VARIANTS = {
    # reconstruction/src/samplers.py:23-38 (+ soft_projection.py:51-54): wider conv stack, two FC layers without BatchNorm
    "reconstruction": dict(conv_widths=(64, 128, 128, 256), fc_widths=(256, 256), fc_batchnorm=False, temperature_floor=1e-2,
                           min_sigma=0.0),
    # classification/models/samplenet_model.py:30-108: registration widths + BatchNorm on the last FC layer
    "classification": dict(last_fc_batchnorm=True, min_sigma=0.0),
}


class TorchMLPSampleNet(SampleNet):
    def _features(self, x, x_bnc=None):
        y = x
        for i in range(1, 6):
            y = F.relu(getattr(self, "bn%d" % i)(getattr(self, "conv%d" % i)(y)))
        y = y.max(dim=2).values  # (B, bottleneck)
        nfc = self.num_fc_layers
        for i in range(1, nfc):
            y = getattr(self, "fc%d" % i)(y)
            bn = getattr(self, "bn_fc%d" % i, None)
            y = F.relu(bn(y) if bn is not None else y)
        y = getattr(self, "fc%d" % nfc)(y)
        bn = getattr(self, "bn_fc%d" % nfc, None)  # classification variant: BatchNorm on the head's output
        if bn is not None:
            y = bn(y)
        return y.view(-1, 3, self.num_out_points)


def torch_mlp_copy(net):
    """Deep copy of a SampleNet whose feature extractor runs through torch.nn (gradients through autograd)."""
    ref = copy.deepcopy(net)
    ref.__class__ = TorchMLPSampleNet
    ref.use_hip_mlp = False
    ref.__dict__.pop("_grad_sink", None)
    return ref


# ------------------------------------------------------------------------------------------ the bar against fp64
def rel(a, b):
    """|a - b| / |b| in double (Frobenius norms)."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def fp64_floor(B):
    """Floor of the bar: BatchNorm over a batch of only a handful of clouds in the FC head amplifies fp32 summation-order
    noise (~3e-4 there)."""
    return 2e-4 if B >= 16 else 6e-4


def fp64_bar(B, err_torch32):
    """ONE bar for a HIP result against the fp64 run of the same network: as close to it as torch's own fp32 path is
    (factor 2), or within fp64_floor(B) -- torch-fp32 itself drifts up to a few 1e-2 from fp64 on some shapes, so it cannot
    serve as the only yardstick."""
    return max(fp64_floor(B), 2 * err_torch32)


def bias_before_batchnorm(net, name):
    """For a parameter whose exact training-mode gradient is 0: the name of the weight whose gradient norm scales its bound;
    None for every other parameter.  A bias in front of a batch-statistics BatchNorm (conv1..5; fc_i followed by bn_fc_i, the
    classification sampler's output layer included): fp64 gives ~1e-12, fp32 holds rounding noise.  bn5.bias likewise when
    fc1 carries a BatchNorm: sum_b of the pooled-feature gradient, which fc1's batch-BatchNorm makes vanish over the batch
    wherever the pooled feature is positive."""
    if not name.endswith(".bias"):
        return None
    layer = name[: -len(".bias")]
    if layer.startswith("conv") or (layer.startswith("fc") and getattr(net, "bn_" + layer, None) is not None):
        return layer + ".weight"
    if layer == "bn5" and getattr(net, "bn_fc1", None) is not None:
        return "bn5.weight"
    return None


# ------------------------------------------------------------------------------------------ one training step
def projection_sigma(project):
    """The variant's sigma rule in plain torch: max(T^2, min_sigma) (registration/src/soft_projection.py:97-99), or
    max(max(T, floor)^2, min_sigma) for the reconstruction sampler (reconstruction/src/soft_projection.py:51-54)."""
    T = project._temperature
    if project._temperature_floor is not None:
        t = torch.clamp(T, min=project._temperature_floor)
        return torch.clamp(t * t, min=project._min_sigma_f)
    return torch.max(T ** 2, torch.tensor(project._min_sigma_f, dtype=T.dtype, device=T.device))


def sampler_step_reference(ref, x, alpha, lmbda, gamma, delta, idx=None):
    """One training step of the sampler in plain torch, in the dtype of `ref` (a torch_mlp_copy; .double() for fp64):
        y    = head(x)                                              samplenet.py:90-104
        proj = softmax-weighted mean of the K nearest input points  soft_projection.py:92-152 (brute-force kNN)
        loss = alpha * L_simp + lmbda * sigma + mean(proj)          main.py:507-531, mean(proj) standing in for the task
    with L_simp = mean(d12) + mean_b(max_m d12) + (gamma + delta M) mean(d21) over squared nearest distances (samplenet.py:
    174-181).  x (B,N,3).  idx (B,M,K): neighbour sets to project onto instead of this run's own kNN (near-ties).
    Returns dict(loss, y (B,3,M), proj (B,M,3), idx (B,M,K), ascending by distance where this run chose them)."""
    x = x.to(ref.project._temperature.dtype)
    y = ref._features(x.permute(0, 2, 1))
    q = y.permute(0, 2, 1)  # (B,M,3)
    d = ((q.unsqueeze(2) - x.unsqueeze(1)) ** 2).sum(-1)  # (B,M,N) squared distances as differences (no cancellation)
    B, M, N = d.shape
    K = ref.project._group_size
    if idx is None:
        idx = d.detach().topk(K, dim=2, largest=False).indices
    grouped = x[torch.arange(B, device=x.device)[:, None, None], idx]  # (B,M,K,3)
    sigma = projection_sigma(ref.project)
    w = torch.softmax(-((grouped - q.unsqueeze(2)) ** 2).sum(-1) / sigma, dim=2)
    proj = (grouped * w.unsqueeze(-1)).sum(2)
    d12, d21 = d.min(dim=2).values, d.min(dim=1).values
    lsimp = d12.mean() + d12.max(dim=1).values.mean() + (gamma + delta * M) * d21.mean()
    loss = alpha * lsimp + lmbda * sigma + proj.mean()
    return dict(loss=loss, y=y, proj=proj, idx=idx)

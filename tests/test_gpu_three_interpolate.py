"""The layers over sn_three_nn on the device: the pointnet2 stand-in's three_nn / three_interpolate and PointnetFPModule.

three_interpolate (WeightedGatherFunction at k = 3: ascending t from +0, product then sum) bit for bit the numpy float32
three-term sum; its gradient towards the features, a deterministic ordered sum, within (contributions to that known point + 1) *
2^-24 * sum|w g| of float64, towards the weights within c2 * 2^-24 * sum|g f|.  The module's weights are torch's elementwise
1 / (dist + 1e-8) over torch.sum, whose order over three terms is torch's own: within the counted 9 units of 2^-24 of float64.
PointnetFPModule: the tensor the module hands to its MLP (a forward pre-hook) against float64 on the forced indices, 9 units for
the weights, 1 per product, 2 for the sum: 12 * 2^-24 * sum|w f|, the skip channels bit for bit; its backward on the gradient that
arrives at exactly that tensor (a tensor hook): the skip gradient is that gradient's slice exactly, the features' gradient within
the counted bound with no other term; and the whole module against a torch-only twin with the same parameters, known=None too."""
import copy

import numpy as np
import pytest
import torch

import interp_ref as R
from cabi_ref import bits as _bits

pytestmark = pytest.mark.gpu

U = R.U
SHAPE = (2, 257, 65, 16, 1)


def case(recipe):
    u, k = R.make_case(SHAPE, recipe)
    kf, uf, g = R.make_feats(SHAPE)
    idx, d2 = R.three_nn(u, k)
    return u, k, kf, uf, g, idx, d2


def dev(a):
    return torch.tensor(a, device="cuda")


def _within(got, ref, k, sab, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = k * U * sab
    print("%s: worst error / bound %.3g" % (what, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), what


def _module_weights(dist):
    """the weights as PointnetFPModule.forward computes them"""
    dist_recip = 1.0 / (dist + 1e-8)
    return dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)


@pytest.mark.parametrize("recipe", ["rand", "lattice", "dup"])
def test_compat_three_nn_and_three_interpolate(recipe):
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    b, n, m, c2, c1 = SHAPE
    u, k, kf, uf, g, idx_np, d2 = case(recipe)
    dist, idx = PU.three_nn(dev(u), dev(k))
    assert np.array_equal(idx.cpu().numpy(), idx_np) and np.array_equal(_bits(dist.cpu().numpy()), _bits(np.sqrt(d2)))
    weight = _module_weights(dist).requires_grad_(True)
    w64 = R.weights64(d2, R.SQRT_EPS)
    assert (np.abs(weight.detach().cpu().numpy() - w64) <= R.WEIGHT_BOUND[R.SQRT_EPS] * w64).all()
    dkf = dev(kf).requires_grad_(True)
    out = PU.three_interpolate(dkf, idx, weight)
    wn = weight.detach().cpu().numpy()
    assert out.shape == (b, c2, n) and np.array_equal(_bits(out.detach().cpu().numpy()), _bits(R.interpolate(kf, idx_np, wn)))
    assert torch.equal(PU.three_interpolate(dkf.detach(), idx.long(), weight.detach()), out.detach())   # int64 indices are converted
    out.backward(dev(g)[:, :c2].contiguous())
    ref, ab, mult = R.backward64(m, c2, idx_np, wn, g)
    _within(dkf.grad.cpu().numpy(), ref, mult[:, None, :] + 1, ab, "three_interpolate towards features")
    f = R._gather(kf.astype(np.float64), idx_np)
    terms = g[:, :c2, :, None].astype(np.float64) * f
    _within(weight.grad.cpu().numpy(), terms.sum(1), c2, np.abs(terms).sum(1), "three_interpolate towards the weights")
    for bad in (lambda: PU.three_interpolate(dkf, idx[:, :, :2], weight), lambda: PU.three_interpolate(dkf, idx.float(), weight),
                lambda: PU.three_interpolate(dkf[:1], idx, weight)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("bn", [True, False])
def test_fp_module_against_float64_and_a_torch_twin(bn):
    from samplenet_amd.compat.pointnet2.utils.pointnet2_modules import PointnetFPModule

    b, n, m, c2, c1 = SHAPE
    u, k, kf, uf, _, idx_np, d2 = case("lattice")
    torch.manual_seed(5)
    fp = PointnetFPModule([c2 + c1, 8, 4], bn=bn).cuda()
    twin = copy.deepcopy(fp.mlp)
    dkf, duf = dev(kf).requires_grad_(True), dev(uf).requires_grad_(True)
    seen = {}

    def pre(_module, args):   # what the module itself hands to its MLP, and the gradient that comes back to exactly that tensor
        seen["input"] = args[0].detach().clone()
        args[0].register_hook(lambda grad: seen.__setitem__("grad", grad.detach().clone()))

    hook = fp.mlp.register_forward_pre_hook(pre)
    out = fp(dev(u), dev(k), duf, dkf)
    hook.remove()
    assert out.shape == (b, 4, n) and seen["input"].shape == (b, c2 + c1, n, 1)
    feats = seen["input"][..., 0]
    # the module's own MLP input against float64 on the forced indices: 12 units of sum|w f|; the skip channels are copies
    w64 = R.weights64(d2, R.SQRT_EPS)
    ref_in, ab_in = R.interpolate64(kf, idx_np, w64), R.interpolate64(np.abs(kf), idx_np, w64)
    _within(feats[:, :c2].cpu().numpy(), ref_in, R.WEIGHT_BOUND[R.SQRT_EPS] / U + 3, ab_in, "the MLP's input")
    assert np.array_equal(_bits(feats[:, c2:].cpu().numpy()), _bits(uf))
    # the twin: the same weights expression, torch.gather, three products and two sums, the same MLP parameters
    rkf, ruf = dev(kf).requires_grad_(True), dev(uf).requires_grad_(True)
    wm = _module_weights(dev(np.sqrt(d2)))
    li = dev(idx_np).long().view(b, 1, n * 3).expand(b, c2, n * 3)
    f = torch.gather(rkf, 2, li).view(b, c2, n, 3)
    w = wm[:, None]
    tfeats = torch.cat([((w[..., 0] * f[..., 0]) + (w[..., 1] * f[..., 1])) + (w[..., 2] * f[..., 2]), ruf], 1)
    assert torch.equal(tfeats.detach().view(torch.int32), feats.view(torch.int32))   # the two MLPs see the same bits
    ref = twin(tfeats.unsqueeze(-1)).squeeze(-1)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-6)   # (the MLP's library convolutions may pick another algorithm per call)
    wt = torch.randn(b, 4, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    (out * wt).sum().backward()
    (ref * wt).sum().backward()
    gin = seen["grad"][..., 0]
    assert torch.equal(duf.grad, gin[:, c2:])   # exactly the slice of the gradient that arrived
    g64, ab, mult = R.backward64(m, c2, idx_np, wm.cpu().numpy(), gin.cpu().numpy())
    _within(dkf.grad.cpu().numpy(), g64, mult[:, None, :] + 1, ab, "PointnetFPModule towards known_feats")
    assert torch.allclose(duf.grad, ruf.grad, rtol=1e-4, atol=1e-6) and torch.allclose(dkf.grad, rkf.grad, rtol=1e-3, atol=1e-4)
    for (name, p), q in zip(fp.mlp.named_parameters(), twin.parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-3, atol=1e-5), name
    # known is None: known_feats (B,C2,1) expanded over n and concatenated (plain torch)
    one = dev(kf)[:, :, :1].contiguous()
    got = fp(dev(u), None, dev(uf), one)
    want = twin(torch.cat([one.expand(b, c2, n), dev(uf)], 1).unsqueeze(-1)).squeeze(-1)
    assert got.shape == (b, 4, n) and torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    # no skip features
    assert fp.mlp[0].conv.in_channels == c2 + c1 and PointnetFPModule([c2, 4], bn=bn).cuda()(dev(u), dev(k), None, dev(kf)).shape == (b, 4, n)

"""The classification task network (samplenet_amd/classifier.py) and its per-cloud transform kernels (csrc/cloud_transform.hip) on
the GPU against the torch restatement of the reference's lines (tests/torch_cls.py) and torch.bmm evaluated in fp64.  The reference
is TensorFlow: there is no reference run and no golden file.

Yardsticks.  Integer-valued operands whose sums stay below 2^24: equality with fp64, bit for bit (derived, no tolerance).
Real-valued operands of the transform kernels: no further from fp64 than twice torch.bmm's fp32 run of the same inputs, or within
TRANSFORM_FLOOR.  Forward values of the network (tests/test_gpu_mlp.py:743-749): twice torch's fp32 error, or 2e-4 (2e-3 below 16
clouds).  Gradient handed to the input cloud, relative to its norm: twice torch's fp32 error or IN_GRAD_FLOOR of that mode and shape.  Weight gradients and
the whole step (test_gpu_mlp.py:750-756): 5e-3 (1e-1 below 16 clouds) of the gradient's norm plus 1e-5 of the largest norm.

The floors are the WORST error of torch fp32 against fp64 over 16 seeds per shape, measured on an MI355X with
tools/cls_floors.py (the code under test takes no part in it; profiles/cls/floors.txt holds the run):

    transform K = 3   (32,64) 1.51e-07  (32,1024) 4.99e-07  (3,100) 1.55e-07  (1,2500) 9.03e-07   -> floor 9.03e-07
    transform K = 64  (32,64) 4.99e-07  (32,1024) 5.53e-07  (3,100) 4.70e-07  (1,2500) 2.34e-06   -> floor 2.34e-06
    input gradient, eval   (32,64) 3.43e-02  (32,1024) 8.22e-03  (3,64) 9.08e-07  (5,100) 4.11e-04  (50,64) 3.96e-03   -> floor 3.43e-02
    input gradient, train  (32,64) 2.56e-02  (32,1024) 5.84e-03  (3,64) 1.84e-04  (5,100) 7.21e-03  (50,64) 7.80e-03   -> floor 2.56e-02
    input gradient, basic model, eval  (32,64) 3.02e-03  (32,1024) 6.53e-06  (3,64) 4.85e-07  (5,100) 4.42e-07  (50,64) 3.72e-03   -> floor 3.72e-03
        (input gradient: where fp32 and fp64 pick different points in a max over the points -- the network has three such pools --
         the gradient moves by 1e-4 .. 3e-2 of its norm on that seed, otherwise it sits near 1e-6)
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from torch_cls import torch_classification_loss, torch_cls_copy  # noqa: E402

pytestmark = pytest.mark.gpu

# max |fp32 bmm - fp64| relative to max |fp64|, worst of 16 seeds and of the three products (Y, dX, dT), per K
TRANSFORM_FLOOR = {3: 9.03e-7, 64: 2.34e-6}
# per mode and shape (B, N), the table above
IN_GRAD_FLOOR = {
    "eval": {(32, 64): 3.43e-2, (32, 1024): 8.22e-3, (3, 64): 9.08e-7, (5, 100): 4.11e-4, (50, 64): 3.96e-3},
    "train": {(32, 64): 2.56e-2, (32, 1024): 5.84e-3, (3, 64): 1.84e-4, (5, 100): 7.21e-3, (50, 64): 7.80e-3},
    "basic-eval": {(32, 64): 3.02e-3, (32, 1024): 6.53e-6, (3, 64): 4.85e-7, (5, 100): 4.42e-7, (50, 64): 3.72e-3},
}


def _floor(B):
    return 2e-4 if B >= 16 else 2e-3


def _gfloor(B):
    return 5e-3 if B >= 16 else 1e-1


def _transform(x, t, dy, want_dx=True, want_dt=True):
    from samplenet_amd._lib import check, lib, ptr, stream_of

    B, N, K = x.shape
    y = torch.empty_like(x)
    dx = torch.full_like(x, float("nan")) if want_dx else None
    dt = torch.full_like(t, float("nan")) if want_dt else None  # dT is overwritten, not accumulated
    check(lib.sn_cloud_transform_forward(B, N, K, ptr(x), ptr(t), ptr(y), stream_of(x)))
    check(lib.sn_cloud_transform_backward(B, N, K, ptr(x), ptr(t), ptr(dy), ptr(dx), ptr(dt), stream_of(x)))
    return y, dx, dt


def _bmm64(x, t, dy):
    x, t, dy = x.double(), t.double(), dy.double()
    return torch.bmm(x, t), torch.bmm(dy, t.transpose(1, 2)), torch.bmm(x.transpose(1, 2), dy)


@pytest.mark.parametrize("K", [64, 3])
@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("N", [1, 64, 100, 1024, 2500])
def test_transform_kernels_exact_on_integers_and_deterministic(B, N, K):
    """Item 1: |values| <= 8 and N <= 2500: every sum is an integer below 2500 * 64 < 2^24, so Y, dX, dT equal fp64 bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(B * 10007 + N * 3 + K)
    x, t, dy = (torch.randint(-8, 9, s, device="cuda", generator=g).float() for s in ((B, N, K), (B, K, K), (B, N, K)))
    got = _transform(x, t, dy)
    for name, a, w in zip(("Y", "dX", "dT"), got, _bmm64(x, t, dy)):
        assert torch.equal(a, w.float()), (name, float((a.double() - w).abs().max()))
    again = _transform(x, t, dy)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # either gradient alone (the other pointer NULL)
    assert torch.equal(_transform(x, t, dy, want_dt=False)[1], got[1]) and torch.equal(_transform(x, t, dy, want_dx=False)[2], got[2])


@pytest.mark.parametrize("K", [64, 3])
@pytest.mark.parametrize("B,N", [(32, 64), (32, 1024), (3, 100), (1, 2500)])
def test_transform_kernels_real_data_vs_fp64(B, N, K):
    """Item 2."""
    for seed in range(3):
        g = torch.Generator(device="cuda").manual_seed(seed * 977 + B + N + K)
        x = torch.rand(B, N, K, device="cuda", generator=g) - 0.5
        t = torch.randn(B, K, K, device="cuda", generator=g)
        dy = torch.randn(B, N, K, device="cuda", generator=g)
        want = _bmm64(x, t, dy)
        ref = (torch.bmm(x, t), torch.bmm(dy, t.transpose(1, 2)), torch.bmm(x.transpose(1, 2), dy))
        for name, a, r, w in zip(("Y", "dX", "dT"), _transform(x, t, dy), ref, want):
            s = float(w.abs().max())
            e_hip, e_ref = float((a.double() - w).abs().max()) / s, float((r.double() - w).abs().max()) / s
            print("transform", name, B, N, K, seed, "e_hip %.3e e_ref %.3e" % (e_hip, e_ref))
            assert e_hip <= max(TRANSFORM_FLOOR[K], 2 * e_ref), (name, e_hip, e_ref)


def _ortho64(t):
    t = t.double().requires_grad_(True)
    d = torch.bmm(t, t.transpose(1, 2)) - torch.eye(t.shape[1], dtype=torch.float64, device=t.device)
    loss = 0.5 * (d * d).sum()
    (g,) = torch.autograd.grad(loss, t)
    return loss.detach(), g


@pytest.mark.parametrize("K", [64, 3])
def test_orthogonality_loss(K):
    """Item 3: value and gradient against fp64; exactly 0 with zero gradient at T = I; integer T exact (sparse entries in
    {-1, 0, 1}: T T^T - I is integer, the sum of its squares stays below 2^24 -- asserted on the fp64 value -- and the gradient
    entries are integers of at most 6 * 64 * 64).  Real T: fp32 chains of K products and sums of K * K squares (a 256-leaf tree
    over chains of K * K / 256): 4 (K + 32) 2^-24 of the value / of the largest gradient entry covers both with the factor 2 of
    the square."""
    from samplenet_amd.classifier import orthogonality_loss

    B = 5
    eye = torch.eye(K, device="cuda").expand(B, K, K).contiguous().requires_grad_(True)
    loss = orthogonality_loss(eye)
    loss.backward()
    assert float(loss) == 0.0 and not bool(eye.grad.any())
    g = torch.Generator(device="cuda").manual_seed(K)
    ti = (torch.randint(-1, 2, (3, K, K), device="cuda", generator=g) * (torch.rand(3, K, K, device="cuda", generator=g) < 0.125)).float()
    ti.requires_grad_(True)
    loss = orthogonality_loss(ti)
    (3.0 * loss).backward()
    w_loss, w_grad = _ortho64(ti.detach())
    assert float(w_loss) < 2 ** 24
    assert float(loss) == float(w_loss) and torch.equal(ti.grad, (3.0 * w_grad).float())
    t = (torch.eye(K, device="cuda") + 0.1 * torch.randn(B, K, K, device="cuda", generator=g)).requires_grad_(True)
    loss = orthogonality_loss(t)
    loss.backward()
    w_loss, w_grad = _ortho64(t.detach())
    tol = 4 * (K + 32) * 2.0 ** -24
    print("ortho", K, abs(float(loss) - float(w_loss)) / float(w_loss), float((t.grad.double() - w_grad).abs().max()) / float(w_grad.abs().max()))
    assert abs(float(loss) - float(w_loss)) <= tol * float(w_loss)
    assert float((t.grad.double() - w_grad).abs().max()) <= tol * float(w_grad.abs().max())


def _clouds(B, N):
    """Clouds that differ from each other as shapes do (own extent and offset per cloud).  Uniform clouds of one size pool to nearly
    the same feature vector; a BatchNorm behind the max-pool then divides by sqrt(eps) and every later figure measures that
    amplification instead of the code."""
    return (torch.rand(B, N, 3, device="cuda") - 0.5) * (0.5 + torch.rand(B, 1, 3, device="cuda")) + 0.2 * torch.randn(B, 1, 3, device="cuda")


def _make(seed, mode="eval", frozen=True, basic=False, dropout=0.3):
    """A classifier with perturbed BatchNorm parameters and NON-ZERO final T-Net weights (with the construction values every
    transform is the identity and the gradient path through the T-Nets is multiplied by zero weights), whose running statistics
    then come from one training pass of the torch restatement over 64 clouds -- statistics that fit the weights, as a trained
    checkpoint's do -- and are perturbed relative to their own scale (test_gpu_autoencoder._make's perturbation, which assumes
    unit-variance features, in units of each channel's standard deviation)."""
    from samplenet_amd import PointNetCls, PointNetClsBasic

    torch.manual_seed(seed)
    net = (PointNetClsBasic if basic else PointNetCls)(dropout=dropout).cuda()
    with torch.no_grad():
        if not basic:
            net.transform_net1.transform.weight.normal_(0, 0.005)
            net.transform_net2.transform.weight.normal_(0, 0.002)
        for n, p in net.named_parameters():
            if "bn" in n:
                p.add_(0.1 * torch.randn_like(p))
        # the pooled layer well above the ReLU's zero: a channel that is negative at every point of a cloud pools to a tie at 0
        # and says nothing about which point was selected (the critical-set check leaves ties out and caps their share)
        net.bn5.bias.add_(1.0)
        cal = torch_cls_copy(net.state_dict(), basic=basic, dropout=0.0, device="cuda").train()
        for m in cal.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.momentum = 1.0
        cal(_clouds(64, 128))
        net.load_state_dict({k: v for k, v in cal.state_dict().items() if "running_" in k}, strict=False)
        bufs = dict(net.named_buffers())
        for n, b in bufs.items():
            if "running_mean" in n:
                b.add_(0.05 * torch.randn_like(b) * bufs[n.replace("running_mean", "running_var")].sqrt())
        for n, b in bufs.items():
            if "running_var" in n:
                b.mul_(0.5 + torch.rand_like(b))
    net.train(mode == "train")
    if frozen:
        for p in net.parameters():
            p.requires_grad_(False)
    return net


def _refs(net, mode, basic=False, dropout=0.3):
    sd = net.state_dict()
    kw = dict(basic=basic, dropout=dropout, device="cuda")
    r32 = torch_cls_copy(sd, **kw).train(mode == "train")
    r64 = torch_cls_copy(sd, dtype=torch.float64, **kw).train(mode == "train")
    for r in (r32, r64):
        for p, q in zip(r.parameters(), net.parameters()):
            p.requires_grad_(q.requires_grad)
    return r32, r64


def _forward_case(B, N, mode, basic=False):
    net = _make(B * 7 + N, mode, basic=basic, dropout=0.0)
    r32, r64 = _refs(net, mode, basic, 0.0)
    x = _clouds(B, N).requires_grad_(True)
    w = torch.randn(B, 40, device="cuda")
    y, ep = net(x)
    assert y.shape == (B, 40) and bool(torch.isfinite(y).all())
    (y * w).sum().backward()
    x32 = x.detach().clone().requires_grad_(True)
    y32, ep32 = r32(x32)
    (y32 * w).sum().backward()
    x64 = x.detach().double().requires_grad_(True)
    y64, ep64 = r64(x64)
    (y64 * w.double()).sum().backward()
    keys = ["GFV", "retrieval_vectors"] + ([] if basic else ["transform"])
    assert set(ep) == set(keys + ["critical_set_idx"])
    for name, a, r, t in [("logits", y, y32, y64)] + [(k, ep[k], ep32[k], ep64[k]) for k in keys]:
        assert a.shape == t.shape, name
        e_hip, e_ref = float((a.double() - t).abs().max()), float((r.double() - t).abs().max())
        print("forward", name, B, N, mode, "e_hip %.3e e_ref %.3e" % (e_hip, e_ref))
        assert e_hip <= max(_floor(B), 2 * e_ref), (name, e_hip, e_ref)
    # critical set: the fp64 argmax wherever the fp64 top two values of a channel differ by more than the forward floor
    top2 = ep64["pre_pool"].topk(min(2, N), dim=2)[0]
    clear = (top2[..., 0] - top2[..., -1] > _floor(B)) if N > 1 else torch.ones_like(top2[..., 0], dtype=torch.bool)
    share = 1.0 - float(clear.double().mean())
    print("critical_set", B, N, mode, "left out %.4f (pooled to zero: %.4f)" % (share, float((top2[..., 0] <= 0).double().mean())))
    assert share <= 0.01, share
    idx = ep["critical_set_idx"]
    assert idx.shape == (B, 1024) and not idx.dtype.is_floating_point
    assert torch.equal(idx.long()[clear], ep64["critical_set_idx"][clear])
    gn = float(x64.grad.norm())
    g_hip, g_ref = float((x.grad.double() - x64.grad).norm()) / gn, float((x32.grad.double() - x64.grad).norm()) / gn
    print("dgrad", B, N, mode, "g_hip %.3e g_ref %.3e" % (g_hip, g_ref))
    assert g_hip <= max(IN_GRAD_FLOOR["basic-" + mode if basic else mode][(B, N)], 2 * g_ref), (g_hip, g_ref)


@pytest.mark.parametrize("B,N", [(32, 64), (32, 1024), (3, 64), (5, 100), (50, 64)])
def test_frozen_eval_network_vs_fp64(B, N):
    """Item 4 (the hot path): logits, every end_points entry and the gradient to the input cloud."""
    _forward_case(B, N, "eval")


@pytest.mark.parametrize("B,N", [(32, 64), (50, 64), (5, 100)])
def test_frozen_eval_network_on_the_layer_walk(B, N, monkeypatch):
    """The SKINNY_HEADS hook: the frozen eval-mode FC heads on sn_linear_forward / sn_linear_dgrad (the route of batch statistics
    and trainable weights) meet the same bars as the sn_skinny_linear composition."""
    from samplenet_amd import classifier

    monkeypatch.setattr(classifier, "SKINNY_HEADS", False)
    _forward_case(B, N, "eval")


def test_more_than_128_clouds_run_in_row_blocks():
    """sn_skinny_linear serves at most 128 rows; a larger batch runs its heads in row blocks."""
    net = _make(4, "eval")
    _, r64 = _refs(net, "eval")
    x = _clouds(130, 64)
    y, _ = net(x)
    with torch.no_grad():
        y64, _ = r64(x.double())
    assert float((y.double() - y64).abs().max()) <= _floor(130)


@pytest.mark.parametrize("B,N", [(32, 64), (5, 100)])
def test_frozen_network_on_batch_statistics_vs_fp64(B, N):
    """The frozen network in training mode (batch statistics, dropout probability 0 for the comparison)."""
    _forward_case(B, N, "train")


@pytest.mark.parametrize("B,N", [(32, 64), (5, 100)])
def test_basic_model_vs_fp64(B, N):
    """Item 6: PointNetClsBasic."""
    _forward_case(B, N, "eval", basic=True)


@pytest.mark.parametrize("B,N", [(32, 64), (8, 1024), (3, 64)])
def test_trainable_network_gradients_and_running_statistics(B, N):
    """Item 5: every parameter gradient and the running statistics after one training step, dropout probability 0."""
    net = _make(11 + B, "train", frozen=False, dropout=0.0)
    r32, r64 = _refs(net, "train", dropout=0.0)
    x = _clouds(B, N)
    w = torch.randn(B, 40, device="cuda")
    lab = torch.randint(0, 40, (B,), device="cuda")
    from samplenet_amd import classification_loss

    y, ep = net(x)
    ((y * w).sum() + classification_loss(y, lab, ep, 0.01)).backward()
    y32, ep32 = r32(x)
    ((y32 * w).sum() + torch_classification_loss(y32, lab, ep32, 0.01)).backward()
    y64, ep64 = r64(x.double())
    ((y64 * w.double()).sum() + torch_classification_loss(y64, lab, ep64, 0.01)).backward()
    g64 = {n: p.grad for n, p in r64.named_parameters()}
    g32 = {n: p.grad for n, p in r32.named_parameters()}
    gmax = max(float(g.norm()) for g in g64.values())
    assert set(dict(net.named_parameters())) == set(g64)
    for n, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        e_hip, e_ref = float((p.grad.double() - g64[n]).norm()), float((g32[n].double() - g64[n]).norm())
        print("wgrad", B, N, n, "e_hip %.3e e_ref %.3e norm %.3e" % (e_hip, e_ref, float(g64[n].norm())))
        assert e_hip <= max(_gfloor(B) * float(g64[n].norm()) + 1e-5 * gmax, 2 * e_ref), (n, e_hip, e_ref)
    b64, b32 = dict(r64.named_buffers()), dict(r32.named_buffers())
    for n, b in net.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(b64[n]) == 1, n
        else:
            e_hip, e_ref = float((b.double() - b64[n]).abs().max()), float((b32[n].double() - b64[n]).abs().max())
            print("buffer", B, N, n, "e_hip %.3e e_ref %.3e max %.3e" % (e_hip, e_ref, float(b64[n].abs().max())))
            assert e_hip <= 1e-5 * max(1.0, float(b64[n].abs().max())), n


def test_eval_mode_weight_gradients_are_refused():
    net = _make(3, "eval", frozen=False)
    y, _ = net(_clouds(4, 64))
    with pytest.raises(RuntimeError):
        y.sum().backward()


def test_dropout_in_training_mode(monkeypatch):
    """Item 5, dropout on: the fraction of zeros within 4 sigma of 0.3, kept activations scaled by 1 / 0.7.  Read off the basic
    model, whose only dropout sits on the returned vectors (two passes on batch statistics see the same activations in front of
    it), and off both masks of the full model where they are applied."""
    B = 32
    x = _clouds(B, 64)
    nb = _make(6, "train", basic=True)
    _, eb = nb(x)
    nb.dropout = 0.0
    _, eb0 = nb(x)
    h, h0 = eb["retrieval_vectors"], eb0["retrieval_vectors"]
    live = h0 > 0
    n = int(live.sum())
    zeros = int((h[live] == 0).sum())
    print("dropout", n, zeros, zeros / n)
    assert abs(zeros - 0.3 * n) <= 4 * (n * 0.3 * 0.7) ** 0.5
    kept = live & (h != 0)
    assert float((h[kept] - h0[kept] / 0.7).abs().max()) <= 2.0 ** -22 * float(h0.abs().max())  # one fp32 division by 0.7
    # the full model: both masks, read where they are applied (the values behind fc1 are not returned)
    from samplenet_amd import classifier

    seen = []
    real = classifier.F.dropout

    def spy(h, p, training):
        out = real(h, p, training)
        seen.append((h.detach().clone(), out.detach().clone(), p, training))
        return out

    net = _make(5, "train")  # (before the spy: _make's calibration pass calls the same torch function)
    monkeypatch.setattr(classifier.F, "dropout", spy)
    _, ep = net(x)
    assert [tuple(a.shape) for a, _, _, _ in seen] == [(B, 1, 512), (B, 256)]
    for h0, h, p, training in seen:
        assert p == 0.3 and training
        live = h0 > 0
        n, zeros = int(live.sum()), int((h[live] == 0).sum())
        print("dropout", tuple(h.shape), n, zeros, zeros / n)
        assert abs(zeros - 0.3 * n) <= 4 * (n * 0.3 * 0.7) ** 0.5
        kept = live & (h != 0)
        assert float((h[kept] - h0[kept] / 0.7).abs().max()) <= 2.0 ** -22 * float(h0.abs().max())
    assert torch.equal(ep["retrieval_vectors"], seen[1][1])


@pytest.mark.parametrize("basic", [False, True])
def test_classification_loss_vs_fp64(basic):
    """Item 7: with the transform term (reg_weight large enough to matter) and without it (basic model / reg_weight 0)."""
    from samplenet_amd import classification_loss

    B = 32
    net = _make(17, "eval", basic=basic)
    r32, r64 = _refs(net, "eval", basic)
    x = _clouds(B, 64).requires_grad_(True)
    lab = torch.randint(0, 40, (B,), device="cuda")
    x32 = x.detach().clone().requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    for rw in (0.001, 0.5, 0.0):
        x.grad = x32.grad = x64.grad = None
        y, ep = net(x)
        loss = classification_loss(y, lab, ep, rw)
        loss.backward()
        y32, ep32 = r32(x32)
        l32 = torch_classification_loss(y32, lab, ep32, rw)
        l32.backward()
        y64, ep64 = r64(x64)
        want = torch_classification_loss(y64, lab, ep64, rw)
        want.backward()
        e_hip, e_ref = abs(float(loss) - float(want)), abs(float(l32) - float(want))
        print("loss", basic, rw, float(loss), float(want), "e_hip %.3e e_ref %.3e" % (e_hip, e_ref))
        assert e_hip <= max(1e-5 * max(1.0, abs(float(want))), 2 * e_ref)
        gn = float(x64.grad.norm())
        g_hip, g_ref = float((x.grad.double() - x64.grad).norm()) / gn, float((x32.grad.double() - x64.grad).norm()) / gn
        print("loss dgrad", basic, rw, "g_hip %.3e g_ref %.3e" % (g_hip, g_ref))
        assert g_hip <= max(IN_GRAD_FLOOR["basic-eval" if basic else "eval"][(B, 64)], 2 * g_ref), (g_hip, g_ref)


def _sampler(seed=0):
    from samplenet_amd import SampleNet

    torch.manual_seed(100 + seed)
    return SampleNet(64, 128, group_size=7, input_shape="bnc", output_shape="bnc", last_fc_batchnorm=True, min_sigma=0.0).cuda().train()


def _cls_step(net, task, loss_fn, x, lab):
    simp, proj = net(x)
    y, ep = task(proj)
    loss = loss_fn(y, lab, ep) + 30 * net.get_simplification_loss(x, simp, 64, 1, 0) + net.get_projection_loss()
    loss.backward()
    return loss.detach()


@pytest.mark.parametrize("B", [32, 4])
def test_classification_step_vs_torch_classifier(B):
    """Item 8: classification sampler (K = 7, BatchNorm on the head's output) -> projected points -> frozen PointNetCls ->
    classification_loss + 30 simplification + projection -> sampler gradients, with PointNetCls and with its torch restatement
    behind the SAME sampler."""
    from samplenet_amd import classification_loss

    cls = _make(21, "eval")
    ref = torch_cls_copy(copy.deepcopy(cls.state_dict()), device="cuda").eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    net_a = _sampler()
    net_b = copy.deepcopy(net_a)
    x = _clouds(B, 1024)
    lab = torch.randint(0, 40, (B,), device="cuda")
    la = _cls_step(net_a, cls, classification_loss, x, lab)
    lb = _cls_step(net_b, ref, torch_classification_loss, x, lab)
    print("step", B, float(la), float(lb))
    assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb))), (float(la), float(lb))
    gb = {n: p.grad for n, p in net_b.named_parameters()}
    gmax = max(float(g.norm()) for g in gb.values())
    for n, p in net_a.named_parameters():
        assert p.grad is not None, n
        assert float((p.grad - gb[n]).norm()) <= _gfloor(B) * float(gb[n].norm()) + 1e-5 * gmax, n


@pytest.mark.parametrize("B", [4, 32])
def test_captured_step_is_bit_identical_to_eager_and_sees_weight_updates(B):
    """Item 9: the step of item 8 as a task_loss of engine.SamplerTrainStep (alpha = 30, lmbda = 1), captured and eager, on fresh
    inputs: the same bits over four replays; an in-place change of classifier weights is seen by the next replay."""
    from samplenet_amd import classification_loss
    from samplenet_amd.engine import SamplerTrainStep

    cls = _make(31, "eval")
    net_g = _sampler()
    net_e = copy.deepcopy(net_g)
    xs = [_clouds(B, 1024) for _ in range(5)]
    xs[3] = xs[2]
    labs = [torch.randint(0, 40, (B,), device="cuda") for _ in range(5)]
    labs[3] = labs[2]
    lab = torch.empty_like(labs[0])  # caller-owned device tensor: the captured graph reads it where it lies

    def task(proj):
        y, ep = cls(proj)
        return classification_loss(y, lab, ep)

    sd0 = copy.deepcopy(net_g.state_dict())
    step_g = SamplerTrainStep(net_g, xs[0], alpha=30.0, lmbda=1.0, task_loss=task, use_graph=True)
    net_g.load_state_dict(sd0)
    step_e = SamplerTrainStep(net_e, xs[0], alpha=30.0, lmbda=1.0, task_loss=task, use_graph=False)

    def run(step, net, x):
        loss = step(x).clone()
        torch.cuda.synchronize()
        return loss, {n: p.grad.clone() for n, p in net.named_parameters()}

    for i, x in enumerate(xs):
        if i == 3:
            with torch.no_grad():
                cls.fc3.bias.add_(0.25)
                cls.conv1.weight.mul_(1.5)
                cls.transform_net2.transform.weight.mul_(0.5)
        lab.copy_(labs[i])
        for p in net_e.parameters():
            p.grad = None
        le, ge = run(step_e, net_e, x)
        lg, gg = run(step_g, net_g, x)
        assert torch.equal(le, lg), (i, float(le), float(lg))
        for n in ge:
            assert torch.equal(ge[n], gg[n]), (i, n)
        if i == 3:
            assert not torch.equal(lg, last[0]) and any(not torch.equal(gg[n], last[1][n]) for n in gg)
        last = (lg, gg)

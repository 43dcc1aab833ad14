"""The sampler head (PointNet feature extractor + FC head on the HIP kernels, routed by samplenet_amd/pointnet.py) against the
same network in fp64 across the reference's whole range of num_out_points (2 .. 1024: registration/src/sputils.py:51,
classification/train_samplenet.py:42) and across the routing limits of forward_impl / _last_layer / backward_impl -- batch
(<= 32, 33 .. 64, above), N % 64 (fused pool), output width (the chain's output stage and backward: Co % 32 / % 64, <= 256),
bottleneck width (chain, one-call conv stack), row-block tiles against the CU count, train / eval -- and the whole training
step (engine fast path and module surface) against a plain-torch step in fp64 at the edge M.

Every case names the C entry points it exists to reach; the test fails when a route is not taken (pointnet.check sees each
entry point's name once per call), so an edit of the table cannot silently drop a route."""
import copy

import numpy as np
import pytest
import torch

from torch_mlp import VARIANTS, bias_before_batchnorm, fp64_bar, fp64_floor, rel, sampler_step_reference, torch_mlp_copy

pytestmark = pytest.mark.gpu


def _sampler(M, bneck, variant, shape, seed, K=8, temperature=1.0):
    from samplenet_amd import SampleNet

    torch.manual_seed(seed)
    net = SampleNet(M, bneck, group_size=K, initial_temperature=temperature, input_shape=shape, output_shape=shape,
                    **VARIANTS.get(variant, {})).cuda()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if "bn" in n:
                p.add_(0.2 * torch.randn_like(p))
        net.bn3.weight[:5] *= -1.0  # negative BatchNorm scales: the max-pool must then select the minimum
        net.bn5.weight[:7] *= -1.0
    return net


@pytest.fixture
def routes(monkeypatch):
    """Names of the C entry points pointnet.py called (each call goes through pointnet.check with its name)."""
    from samplenet_amd import pointnet

    called = []
    real = pointnet.check

    def spy(rc, what=""):
        called.append(what)
        return real(rc, what)

    monkeypatch.setattr(pointnet, "check", spy)
    return called


# Entry points every case of a kind reaches anyway; the tables below name the ones each case exists for.
CONV_FX = ("sn_conv_stack_forward_bn",)
CONV_FX_B = ("sn_conv_stack_backward",)
EVAL = ("sn_linear_forward", "sn_bn_eval_coef", "sn_pool_forward")


def _case(cid, M, B, N, bneck, variant, shape, train, evl, why, seed=0):
    return pytest.param(M, B, N, bneck, variant, shape, tuple(train), tuple(evl), seed, id=cid)


# (M, B, N, bottleneck, variant, layout, entry points of the training forward + backward, of the eval forward; why)
HEAD_CASES = [
    _case("cls-M2-B2", 2, 2, 1024, 128, "classification", "bnc",
          CONV_FX + ("sn_fc_chain_forward_pool", "sn_layer_forward_bn_out", "sn_bn_output_backward", "sn_layer_backward") + CONV_FX_B,
          EVAL + ("sn_bn_output_forward",),
          "Co = 6: the reference's minimum M, 3M % 4 != 0; chain output stage and backward chain refused"),
    _case("cls-M5-B33", 5, 33, 1024, 128, "classification", "bcn",
          CONV_FX + ("sn_layer_forward_bn", "sn_linear_forward_rows", "sn_bn_output_forward", "sn_bn_output_backward",
                     "sn_layer_backward", "sn_pool_backward_bn") + CONV_FX_B,
          EVAL + ("sn_bn_output_forward",),
          "Co = 15 above 32 clouds: the output BatchNorm on its own launch in training mode"),
    _case("cls-M2-B65", 2, 65, 1024, 128, "classification", "bnc",
          CONV_FX + ("sn_linear_forward_rows", "sn_bn_batch_stats_twopass", "sn_bn_output_forward", "sn_bn_output_backward",
                     "sn_layer_backward", "sn_pool_backward_bn") + CONV_FX_B,
          EVAL + ("sn_bn_output_forward",),
          "Co = 6 above 64 clouds: two-pass statistics in the hidden layers"),
    _case("cls-M32-B32", 32, 32, 1024, 128, "classification", "bnc",
          CONV_FX + ("sn_fc_chain_forward_pool_out", "sn_bn_output_backward", "sn_layer_backward") + CONV_FX_B,
          EVAL + ("sn_bn_output_forward",),
          "Co = 96: the chain's output stage allowed (Co % 32), its backward not (Co % 64)"),
    _case("cls-M64-B16", 64, 16, 1024, 128, "classification", "bcn",
          CONV_FX + ("sn_fc_chain_forward_pool_out", "sn_fc_chain_backward_obn") + CONV_FX_B,
          EVAL + ("sn_bn_output_forward",),
          "default M: output stage and the backward chain opened by the output BatchNorm"),
    _case("reg-M64-B32", 64, 32, 1024, 128, "registration", "bnc",
          CONV_FX + ("sn_fc_chain_forward_pool", "sn_linear_forward", "sn_fc_chain_backward") + CONV_FX_B, EVAL,
          "the benchmark's shape: every fused route"),
    _case("reg-M86-B32", 86, 32, 1024, 128, "registration", "bcn",
          CONV_FX + ("sn_fc_chain_forward_pool", "sn_linear_forward", "sn_layer_backward") + CONV_FX_B, EVAL,
          "Co = 258: just past the 256-wide backward chain"),
    _case("cls-M128-B64", 128, 64, 1024, 128, "classification", "bnc",
          CONV_FX + ("sn_layer_forward_bn", "sn_linear_forward_rows", "sn_bn_output_forward", "sn_bn_output_backward",
                     "sn_layer_backward", "sn_pool_backward_bn") + CONV_FX_B,
          EVAL + ("sn_bn_output_forward",),
          "Co = 384 at 64 clouds: 33 .. 64-row BatchNorm layers, row-tiled output layer"),
    _case("reg-M1024-B64", 1024, 64, 1024, 128, "registration", "bnc",
          CONV_FX + ("sn_layer_forward_bn", "sn_linear_forward_rows", "sn_layer_backward", "sn_pool_backward_bn") + CONV_FX_B,
          EVAL + ("sn_linear_forward_rows",),
          "Co = 3072, M = N: 2 x 96 = 192 row-block tiles <= 256 CUs (row-tiled output layer)"),
    _case("reg-M1024-B65", 1024, 65, 1024, 128, "registration", "bcn",
          CONV_FX + ("sn_linear_forward_rows", "sn_bn_batch_stats_twopass", "sn_layer_backward", "sn_pool_backward_bn") + CONV_FX_B,
          EVAL + ("sn_linear_forward_rows",),
          "Co = 3072: 3 x 96 = 288 tiles > 256 CUs (the 64-row tile kernel), two-pass statistics"),
    _case("reg-M1000-B4", 1000, 4, 1024, 128, "registration", "bnc",
          CONV_FX + ("sn_fc_chain_forward_pool", "sn_linear_forward", "sn_layer_backward") + CONV_FX_B, EVAL,
          "Co = 3000, near-complete farthest-point completion in eval"),
    _case("reg-M64-B200", 64, 200, 1024, 128, "registration", "bnc",
          CONV_FX + ("sn_linear_forward_rows", "sn_bn_batch_stats_twopass", "sn_layer_backward", "sn_pool_backward_bn") + CONV_FX_B,
          EVAL + ("sn_linear_forward_rows",),
          "200 clouds"),
    _case("reg-N1000-B4", 64, 4, 1000, 128, "registration", "bnc",
          ("sn_layer_forward_bn", "sn_pool_forward", "sn_fc_chain_forward", "sn_linear_forward", "sn_fc_chain_backward",
           "sn_layer_backward", "sn_layer_backward_in3"), EVAL,
          "N % 64 != 0: per-layer conv stack, separate max-pool, chain without its pool stage"),
    _case("reg-N64-B2-bneck64", 64, 2, 64, 64, "registration", "bcn",
          CONV_FX + ("sn_fc_chain_forward", "sn_fc_chain_backward", "sn_layer_backward", "sn_linear_wgrad"), EVAL,
          "128 rows: one-call conv stack forward, per-layer backward without the closed-form input layer"),
    _case("reg-N2048-bneck256", 64, 16, 2048, 256, "registration", "bnc",
          ("sn_layer_forward_bn", "sn_conv_forward_bn_pool", "sn_fc_chain_forward", "sn_fc_chain_backward", "sn_layer_backward",
           "sn_layer_backward_in3"), EVAL,
          "bottleneck 256: no one-call conv stack, fused pool on the last conv layer"),
    _case("reg-bneck100-B16", 32, 16, 1024, 100, "registration", "bnc",
          ("sn_layer_forward_bn", "sn_pool_forward", "sn_linear_forward", "sn_layer_backward", "sn_layer_backward_in3"), EVAL,
          "bottleneck 100 (not a multiple of 64): no fused pool, no chain",
          # (under seed 0 the fp64 run takes another max-pool branch than an fp32 run: conv1.weight moves by 8e-3 in both
          #  fp32 implementations alike, and the bar has no alternative from 16 clouds up)
          seed=1),
    _case("reg-bneck1024-B4", 64, 4, 1024, 1024, "registration", "bcn",
          ("sn_layer_forward_bn", "sn_conv_forward_bn_pool", "sn_linear_forward", "sn_layer_backward", "sn_layer_backward_in3"),
          EVAL, "bottleneck 1024: fc1 on 1024 inputs"),
    _case("rec-M64-B8-N2048", 64, 8, 2048, 128, "reconstruction", "bnc",
          CONV_FX + ("sn_linear_forward", "sn_layer_backward", "sn_linear_wgrad"), EVAL,
          "reconstruction sampler: wide conv stack, FC head without BatchNorm"),
    _case("rec-M5-B40", 5, 40, 1024, 128, "reconstruction", "bcn",
          CONV_FX + ("sn_linear_forward_rows", "sn_layer_backward", "sn_pool_backward_bn", "sn_linear_wgrad"),
          EVAL + ("sn_linear_forward_rows",),
          "reconstruction sampler, Co = 15 above 32 clouds"),
]


def _grad_check(hip, ref, ref64, B, what):
    """Every parameter gradient of the HIP module against the fp64 module: the bar of fp64_bar (below 16 clouds a max-pool /
    ReLU near-tie may resolve differently in one fp32 implementation than in fp64: then the two fp32 runs agree within 1e-1);
    biases whose exact gradient is 0 hold rounding noise only."""
    wnorm = {n: float(p.grad.norm()) for n, p in ref64.named_parameters() if p.grad is not None}
    for (n, ph), (_, pr), (_, pd) in zip(hip.named_parameters(), ref.named_parameters(), ref64.named_parameters()):
        if pd.grad is None:
            continue
        assert ph.grad is not None, (what, n)
        zero = bias_before_batchnorm(ref64, n)
        if zero is not None:
            assert float(ph.grad.double().norm()) <= 1e-3 * wnorm[zero] + 1e-6, (what, n)
            continue
        nd = float(pd.grad.norm())
        err_h, err_r = rel(ph.grad, pd.grad), rel(pr.grad, pd.grad)
        err_hr = float((ph.grad.double() - pr.grad.double()).norm()) / nd
        if B >= 16:
            assert err_h <= fp64_bar(B, err_r), (what, n, err_h, err_r, err_hr)
        else:
            assert err_h <= fp64_bar(B, err_r) or err_hr <= 1e-1, (what, n, err_h, err_r, err_hr)


def _output_check(h, r, d, B, what):
    e_h, e_r = rel(h, d), rel(r, d)
    if B >= 16:
        assert e_h <= fp64_bar(B, e_r), (what, e_h, e_r)
    else:
        assert e_h <= fp64_bar(B, e_r) or rel(h, r) < fp64_floor(B), (what, e_h, e_r)


def _missing(called, expected):
    return sorted(set(expected) - set(called))


@pytest.mark.parametrize("M,B,N,bneck,variant,shape,train_routes,eval_routes,seed", HEAD_CASES)
def test_head_vs_fp64_across_routes(routes, M, B, N, bneck, variant, shape, train_routes, eval_routes, seed):
    """Training mode: head output, every parameter gradient under a random upstream gradient, running statistics and
    num_batches_tracked against torch_mlp_copy(net).double().  Eval mode (after that training forward moved the running
    statistics): head output against the fp64 module, and SampleNet.forward's matched cloud against sputils.nn_matching
    (numpy) of the HIP head output's nearest input points.  Both passes must reach the case's entry points."""
    from samplenet_amd import ops, sputils

    hip = _sampler(M, bneck, variant, shape, seed=M * 131 + B * 7 + N + bneck + 1000 * seed).train()
    ref = torch_mlp_copy(hip)
    ref64 = copy.deepcopy(ref).double()
    x_bnc = torch.rand(B, N, 3, device="cuda") - 0.5
    x = x_bnc if shape == "bnc" else x_bnc.permute(0, 2, 1).contiguous()
    xb = x_bnc.permute(0, 2, 1)  # (B,3,N) view

    # ---- training mode
    y_h = hip._features(xb, x_bnc)
    y_r = ref._features(xb)
    y_d = ref64._features(xb.double())
    assert y_h.shape == (B, 3, M)
    _output_check(y_h, y_r, y_d, B, "train output")
    g = torch.randn_like(y_r)
    (y_h * g).sum().backward()
    (y_r * g).sum().backward()
    (y_d * g.double()).sum().backward()
    torch.cuda.synchronize()
    assert not _missing(routes, train_routes), ("training routes not taken", _missing(routes, train_routes), sorted(set(routes)))
    _grad_check(hip, ref, ref64, B, "train")
    for (n, bh), (_, bd) in zip(hip.named_buffers(), ref64.named_buffers()):
        if bh.dtype == torch.long:
            assert int(bh) == int(bd) == 1, n
        else:
            assert torch.allclose(bh.double(), bd, rtol=1e-4, atol=1e-5), n
    del y_h, y_r, y_d, g
    for net in (hip, ref, ref64):
        net.zero_grad(set_to_none=True)

    # ---- eval mode (running statistics)
    routes.clear()
    for net in (hip, ref, ref64):
        net.eval()
    with torch.no_grad():
        e_h = hip._features(xb, x_bnc)
        e_r = ref._features(xb)
        e_d = ref64._features(xb.double())
        torch.cuda.synchronize()
        assert not _missing(routes, eval_routes), ("eval routes not taken", _missing(routes, eval_routes), sorted(set(routes)))
        _output_check(e_h, e_r, e_d, B, "eval output")
        simp, match = hip(x)
        y = simp if shape == "bcn" else simp.permute(0, 2, 1)  # (B,3,M)
        assert torch.equal(y, e_h)
        # the nearest input point of every generated point: the HIP kNN's pick must be a nearest point in fp64 (ties up to
        # fp32 rounding of the squared distances); the matching is then checked on exactly those picks
        idx = ops.knn(1, xb.contiguous(), y.contiguous(), ops.BCN, ops.BCN, return_dist=False)[0][:, :, 0].long()  # (B,M)
        d64 = ((y.double().permute(0, 2, 1).unsqueeze(2) - x_bnc.double().unsqueeze(1)) ** 2).sum(-1)  # (B,M,N)
        picked = d64.gather(2, idx.unsqueeze(2)).squeeze(2)
        assert float((picked - d64.min(dim=2).values).max()) <= 1e-6 * max(1.0, float(d64.max())), "kNN(1) is not a nearest point"
        del d64
        want = sputils.nn_matching(x_bnc.cpu().numpy(), idx.cpu().numpy(), M, complete_fps=True)  # (B,M,3) float64
        got = match if shape == "bnc" else match.permute(0, 2, 1)
        assert got.shape == (B, M, 3)
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want)


# ------------------------------------------------------------------------------------------ the whole training step
STEP = dict(alpha=0.5, lmbda=0.1, gamma=1.0, delta=0.01)


def _same_sets(a, b):
    return (a.sort(dim=2).values == b.sort(dim=2).values).all(dim=2)  # (B,M) True where the K-sets agree


@pytest.mark.parametrize("M,variant,N,seed", [(2, "registration", 1024, 0), (5, "registration", 1024, 0),
                                              (1024, "registration", 1024, 0), (2, "classification", 1024, 0),
                                              (5, "classification", 1024, 0),
                                              # (seed 0: a max-pool near-tie -- both fp32 runs drift from fp64 on conv1.weight)
                                              (1024, "classification", 1024, 1), (64, "reconstruction", 2048, 0)])
def test_training_step_vs_fp64(M, variant, N, seed):
    """One sampler training step -- head, soft projection, alpha L_simp + lmbda sigma + mean(proj), backward -- through the
    engine's fast path (SamplerTrainStep, use_graph=False) and through the module surface (net(x), the loss getters,
    backward) against sampler_step_reference in fp64 (torch's fp32 run of it is the yardstick of the bar): loss within 1e-5
    relative, simplified and projected cloud, every parameter gradient and the temperature gradient within fp64_bar."""
    from samplenet_amd import ops
    from samplenet_amd.engine import SamplerTrainStep

    B, K = 16, 8
    net0 = _sampler(M, 128, variant, "bnc", seed=M * 17 + N + len(variant) + 1000 * seed, K=K, temperature=0.2).train()
    x = torch.rand(B, N, 3, device="cuda")  # a cloud in the unit cube: mean(proj) keeps the loss O(1)

    def run_reference(idx_hip):
        """fp64 and fp32 reference steps (each on a module of its own: the gradients land on its parameters), projecting onto
        the fp64 run's own neighbour sets -- except where the HIP run's set differs from them (a near-tie at the K-th
        neighbour): there onto the HIP run's indices, so that both sides project onto the same points."""
        m64, m32 = torch_mlp_copy(net0).double(), torch_mlp_copy(net0)
        r64 = sampler_step_reference(m64, x, **STEP)
        same = _same_sets(r64["idx"], idx_hip)
        if not bool(same.all()):
            idx = torch.where(same.unsqueeze(2), r64["idx"], idx_hip)
            m64 = torch_mlp_copy(net0).double()
            r64 = sampler_step_reference(m64, x, idx=idx, **STEP)
        r32 = sampler_step_reference(m32, x, idx=r64["idx"], **STEP)
        r64["loss"].backward()
        r32["loss"].backward()
        return r64, m64, r32, m32

    # engine fast path: fc4 inside the pair scan where the architecture allows it
    net_e = copy.deepcopy(net0)
    step = SamplerTrainStep(net_e, x, use_graph=False, **STEP)
    loss_e = step(x)
    y_e, proj_e = step.outputs  # (B,3,M), (B,M,3)
    # module surface
    net_m = copy.deepcopy(net0)
    simp, proj_m = net_m(x)
    loss_m = (STEP["alpha"] * net_m.get_simplification_loss(x, simp, M, STEP["gamma"], STEP["delta"])
              + STEP["lmbda"] * net_m.get_projection_loss() + proj_m.mean())
    loss_m.backward()
    y_m = simp.permute(0, 2, 1)

    for what, net, loss, y, proj in (("engine", net_e, loss_e, y_e, proj_e), ("module", net_m, loss_m, y_m, proj_m)):
        idx_hip = ops.knn(K, x, y.detach().contiguous(), ops.BNC, ops.BCN, return_dist=False)[0].long()  # (B,M,K)
        r64, m64, r32, m32 = run_reference(idx_hip)
        l64 = float(r64["loss"])
        assert abs(float(loss) - l64) <= 1e-5 * abs(l64), (what, float(loss), l64)
        for name, h, r, d in (("simplified", y, r32["y"], r64["y"]), ("projected", proj, r32["proj"], r64["proj"])):
            e_h, e_r = rel(h, d), rel(r, d)
            assert e_h <= fp64_bar(B, e_r), (what, name, e_h, e_r)
        wnorm = {n: float(p.grad.norm()) for n, p in m64.named_parameters() if p.grad is not None}
        for (n, ph), (_, pr), (_, pd) in zip(net.named_parameters(), m32.named_parameters(), m64.named_parameters()):
            assert ph.grad is not None and pd.grad is not None, (what, n)
            zero = bias_before_batchnorm(m64, n)
            if zero is not None:
                assert float(ph.grad.double().norm()) <= 1e-3 * wnorm[zero] + 1e-6, (what, n)
                continue
            e_h, e_r = rel(ph.grad, pd.grad), rel(pr.grad, pd.grad)
            assert e_h <= fp64_bar(B, e_r), (what, n, e_h, e_r)  # (n = project._temperature: the temperature gradient)
        del r64, m64, r32, m32
        torch.cuda.empty_cache()

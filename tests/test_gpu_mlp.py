"""GPU parity of the hand-written MFMA PointNet MLP (samplenet_amd/csrc/pointnet_mlp.hip, pointnet_mlp_backward.hip, fc_chain.hip, task_network.hip) against the plain
PyTorch fp32 modules of the same network (the reference's own op chain, samplenet.py:90-104) on the same
weights and inputs: outputs, BatchNorm running statistics, and the gradient of every parameter."""
import copy

import numpy as np
import pytest
import torch

from torch_mlp import VARIANTS, fp64_bar, fp64_floor, rel as _rel, torch_mlp_copy

pytestmark = pytest.mark.gpu


def _pair(B, N, M, K, bneck, shape, seed=0):
    from samplenet_amd import SampleNet

    torch.manual_seed(seed)
    hip = SampleNet(M, bneck, group_size=K, input_shape=shape, output_shape=shape).cuda()
    with torch.no_grad():
        for n, p in hip.named_parameters():
            if "bn" in n:
                p.add_(0.2 * torch.randn_like(p))
        hip.bn3.weight[:5] *= -1.0  # negative BatchNorm scale: the fused max-pool must then select the minimum
        hip.bn5.weight[:7] *= -1.0
    ref = torch_mlp_copy(hip)
    x = torch.rand(B, N, 3, device="cuda") - 0.5
    if shape == "bcn":
        x = x.permute(0, 2, 1).contiguous()
    return hip, ref, x


def _acc_sums_zero(acc, nlayers=5, channels=None):
    """The statistics accumulators at the head of the conv stack's persistent scratch are zero between calls (behind them:
    the forward's split-weight planes, scratch).  channels: the stack's widths (a layer above 128 channels doubles the region)."""
    import ctypes

    from samplenet_amd._lib import lib

    ch = (ctypes.c_int * (nlayers + 1))(*channels) if channels is not None else None
    n = lib.sn_conv_stack_acc_sum_elems(nlayers, ch)
    assert 0 < n <= acc.numel()
    return int(acc[:n].abs().max()) == 0


CFGS = [(4, 1024, 64, 8, 128, "bnc"), (3, 96, 12, 5, 32, "bcn"), (32, 1024, 64, 8, 128, "bnc"), (6, 130, 7, 4, 40, "bnc"),
        (70, 64, 16, 4, 128, "bnc"), (33, 1024, 64, 8, 128, "bnc"), (48, 512, 32, 8, 64, "bnc"),
        # exactly 64 rows in the FC head: the combined backward's statistics partials are one TileBig block where
        # sn_linear_stats_blocks counts two TileSmall blocks (round 4: the BatchNorm-backward sums read an unwritten block)
        # (shapes are picked where neither fp32 run takes another max-pool / ReLU branch than the fp64 run under this seed: at
        #  (128, 128) the HIP run does -- 6e-4 on the conv gradients --, at (128, 256) torch's own fp32 run does -- 4e-3)
        (64, 256, 64, 8, 128, "bnc"), (96, 128, 32, 8, 128, "bnc"),
        # a bottleneck that is a multiple of 64 but not a power of two: fc1 outside the chain, on the register-direct R <= 32 kernel
        # (the LDS-staged one needs Ci / 4 to divide its 256 threads; it was dispatched here and returned wrong rows until round 4)
        (8, 256, 16, 4, 192, "bnc"), (40, 128, 16, 4, 192, "bnc")]


@pytest.mark.parametrize("cfg", CFGS)
def test_mlp_forward_backward_vs_torch(cfg):
    """Three implementations of the same network on the same weights / inputs: the HIP kernels (fp32 MFMA), the torch
    fp32 modules (MIOpen / rocBLAS) and the torch fp64 modules.  Bar: the HIP result is as close to the fp64 result as
    torch's own fp32 path is (factor 2), or within 2e-4 -- torch-fp32 itself drifts up to a few 1e-2 from fp64 on some
    shapes (measured: conv1.weight at B=33), so it cannot serve as the only yardstick.  Where the fp64 run takes a
    different max-pool / ReLU branch than both fp32 runs, the two fp32 runs are compared with each other instead."""
    B, N, M, K, bneck, shape = cfg
    hip, ref, x = _pair(*cfg)
    ref64 = copy.deepcopy(ref).double()
    for net in (hip, ref, ref64):
        net.train()
    xb = x if shape == "bcn" else x.permute(0, 2, 1)
    y_h = hip._features(xb, x if shape == "bnc" else None)
    y_r = ref._features(xb)
    y_d = ref64._features(xb.double())
    assert y_h.shape == y_r.shape == (B, 3, M)
    e_h, e_r = _rel(y_h.detach(), y_d.detach()), _rel(y_r.detach(), y_d.detach())
    # BatchNorm over a batch of only 3-6 samples in the FC head amplifies fp32 summation-order noise (~3e-4 there)
    floor = fp64_floor(B)
    if B >= 16:  # ONE bar: as close to the fp64 run as torch's own fp32 path (factor 2), floor 2e-4
        assert e_h <= fp64_bar(B, e_r), (e_h, e_r)
    else:
        assert e_h <= fp64_bar(B, e_r) or _rel(y_h.detach(), y_r.detach()) < floor, (e_h, e_r)
    g = torch.randn_like(y_r)
    (y_h * g).sum().backward()
    (y_r * g).sum().backward()
    (y_d * g.double()).sum().backward()
    wnorm = {n: float(p.grad.norm()) for n, p in ref64.named_parameters() if p.grad is not None}
    for (n, ph), (_, pr), (_, pd) in zip(hip.named_parameters(), ref.named_parameters(), ref64.named_parameters()):
        if n.startswith("project"):
            continue
        if (n.endswith(".bias") and not n.startswith(("bn", "fc4"))) or n == "bn5.bias":
            # a bias in front of a BatchNorm: the true gradient is exactly 0 (fp64 gives ~1e-12); fp32 holds rounding
            # noise.  bn5.bias likewise: sum_b of the pooled-feature gradient, which fc1's batch-BatchNorm makes
            # vanish over the batch wherever the pooled feature is positive.
            assert float(ph.grad.double().norm()) <= 1e-3 * wnorm[n.replace(".bias", ".weight")] + 1e-6, n
            continue
        nd = float(pd.grad.norm())
        err_h = float((ph.grad.double() - pd.grad).norm()) / nd
        err_r = float((pr.grad.double() - pd.grad).norm()) / nd
        err_hr = float((ph.grad.double() - pr.grad.double()).norm()) / nd
        # B < 16: a near-tie in the max-pool can resolve to a different point in one fp32 implementation than in the other
        # (and than in fp64); the gradient routed through it then moves early-layer gradients by a few per cent.
        if B >= 16:  # ONE bar (no alternative): twice torch-fp32's own distance from the fp64 gradient, floor 2e-4
            assert err_h <= fp64_bar(B, err_r), (n, err_h, err_r, err_hr)
        else:
            assert err_h <= fp64_bar(B, err_r) or err_hr <= 1e-1, (n, err_h, err_r, err_hr)
    for (n, bh), (_, bd) in zip(hip.named_buffers(), ref64.named_buffers()):
        if bh.dtype == torch.long:
            assert int(bh) == int(bd) == 1, n
        else:
            assert torch.allclose(bh.double(), bd, rtol=1e-4, atol=1e-5), n


def test_mlp_eval_mode_vs_torch():
    hip, ref, x = _pair(5, 256, 16, 4, 64, "bnc")
    for net in (hip, ref):
        net.train()
        with torch.no_grad():
            net._features(x.permute(0, 2, 1), x if net.use_hip_mlp else None)  # populate running statistics
        net.eval()
    with torch.no_grad():
        y_h = hip._features(x.permute(0, 2, 1), x)
        y_r = ref._features(x.permute(0, 2, 1))
    assert _rel(y_h, y_r) < 1e-4


def test_linear_kernels_exact_small_integers():
    """MFMA fragment / tile indexing check that is transpose-detecting: small-integer operands make every
    product and sum exact in fp32, so the three GEMM kernels must match an integer reference bit-for-bit."""
    from samplenet_amd._lib import check, lib, ptr

    g = torch.Generator(device="cuda").manual_seed(3)
    st = torch.cuda.current_stream().cuda_stream
    # (the 64-aligned shapes take the split-bf16 path of the conv layers: small integers are exact in bf16 as well)
    # ((32, 192, 256) .. (16, 448, 96): input widths that are multiples of 64 but not powers of two -- the LDS-staged R <= 32 kernel
    #  stages a row with Ci / 4 threads, which must divide 256: those widths returned wrong outputs until round 4)
    for (R, Ci, Co) in [(300, 24, 40), (32, 128, 256), (1000, 3, 64), (129, 64, 128), (64, 256, 36), (4096, 128, 128),
                        (1024, 64, 64), (640, 64, 128), (32, 192, 256), (20, 320, 64), (32, 384, 128), (16, 448, 96), (7, 512, 64)]:
        A = torch.randint(-4, 5, (R, Ci), device="cuda", generator=g).float()
        W = torch.randint(-4, 5, (Co, Ci), device="cuda", generator=g).float()
        b = torch.randint(-4, 5, (Co,), device="cuda", generator=g).float()
        Z = torch.empty(R, Co, device="cuda")
        nblk = lib.sn_linear_stats_blocks(R)
        stats = torch.empty(nblk, 2, Co, device="cuda")
        check(lib.sn_linear_forward(R, Ci, Co, ptr(A), None, ptr(W), ptr(b), ptr(Z), ptr(stats), st))
        Zr = A.double() @ W.double().t() + b.double()
        assert torch.equal(Z.double(), Zr), (R, Ci, Co)
        assert torch.equal(stats.double().sum(0)[0], Zr.sum(0)) and torch.equal(stats.double().sum(0)[1], (Zr * Zr).sum(0))
        dZ = torch.randint(-3, 4, (R, Co), device="cuda", generator=g).float()
        dA = torch.empty(R, Ci, device="cuda")
        check(lib.sn_linear_dgrad(R, Ci, Co, 0, ptr(dZ), None, None, None, None, 1, ptr(W), None, None, ptr(dA), None, st))
        assert torch.equal(dA.double(), dZ.double() @ W.double())
        ns = lib.sn_linear_wgrad_splits(R, Ci, Co, 1)
        part = torch.empty(ns * Co * (Ci + 1), device="cuda")
        dW, db = torch.empty(Co, Ci, device="cuda"), torch.empty(Co, device="cuda")
        check(lib.sn_linear_wgrad(R, Ci, Co, 0, ptr(dZ), None, None, None, None, 1, ptr(A), None, ptr(part), ptr(dW), ptr(db), st))
        assert torch.equal(dW.double(), dZ.double().t() @ A.double())
        assert torch.equal(db.double(), dZ.double().sum(0))


@pytest.mark.parametrize("R,Ci,Co", [(512, 256, 256), (512, 128, 256), (100, 256, 192), (40, 64, 250), (1000, 256, 256), (33, 512, 64),
                                      (128, 256, 256), (2048, 256, 256), (48, 192, 256), (100, 384, 64)])
@pytest.mark.parametrize("act", [False, True])
def test_row_tiled_layer_forward_exact_small_integers(R, Ci, Co, act):
    """A layer of the FC head above 32 rows, no statistics requested (the caller takes two-pass statistics from Z): while
    (R / 32) x (Co / 32) workgroups fit the chip, sn_linear_forward_rows runs the R <= 32 kernel row block by row block (all of K in flight per
    workgroup) instead of the 64 x 64 tile kernel.  Small-integer operands (and a power-of-two BatchNorm scale) make every product and
    sum exact: the result must equal the integer reference bit for bit at ragged rows / columns too ((2048, 256, 256) is past the
    chip-filling bound and takes the tile kernel: same bar)."""
    from samplenet_amd._lib import check, lib, ptr

    g = torch.Generator(device="cuda").manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    A = torch.randint(-4, 5, (R, Ci), device="cuda", generator=g).float()
    W = torch.randint(-4, 5, (Co, Ci), device="cuda", generator=g).float()
    b = torch.randint(-4, 5, (Co,), device="cuda", generator=g).float()
    coef = None
    Ain = A.double()
    if act:  # relu(scale * a + shift) with scale in {1, 2, -1}, integer shifts
        sc = torch.tensor([1.0, 2.0, -1.0], device="cuda")[torch.randint(0, 3, (Ci,), device="cuda", generator=g)]
        sh = torch.randint(-2, 3, (Ci,), device="cuda", generator=g).float()
        coef = torch.stack([sc, sh, torch.zeros(Ci, device="cuda"), torch.ones(Ci, device="cuda")]).contiguous()
        Ain = torch.relu(A.double() * sc.double() + sh.double())
    Z = torch.full((R + 1, Co), -7.0, device="cuda")  # one guard row behind the output
    check(lib.sn_linear_forward_rows(R, Ci, Co, ptr(A), ptr(coef) if act else None, ptr(W), ptr(b), ptr(Z), st))
    Zr = Ain @ W.double().t() + b.double()
    assert torch.equal(Z[:R].double(), Zr), (R, Ci, Co)
    assert bool((Z[R] == -7.0).all())


@pytest.mark.parametrize("R,Ci,Co", [(50, 256, 256), (33, 128, 256), (64, 256, 192), (40, 64, 250), (50, 192, 128), (20, 192, 256)])
@pytest.mark.parametrize("act", [False, True])
def test_layer_forward_with_batchnorm_on_33_to_64_rows(R, Ci, Co, act):
    """sn_layer_forward_bn on 33 .. 64 rows: both 32-row halves in one workgroup, the BatchNorm finalised in the epilogue (two-pass
    variance over all rows in registers) -- no statistics launch.  Integer operands: Z exact; coefficients and running statistics
    against a float64 evaluation of torch.nn.BatchNorm1d's training-mode formulas (1e-6 relative)."""
    from samplenet_amd._lib import check, lib, ptr

    g = torch.Generator(device="cuda").manual_seed(R * 7 + Ci + Co)
    st = torch.cuda.current_stream().cuda_stream
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, device="cuda", generator=g).float()  # noqa: E731
    A, W, b = ri(-4, 5, R, Ci), ri(-4, 5, Co, Ci), ri(-4, 5, Co)
    coefp, Ain = None, A.double()
    if act:
        sc = torch.tensor([1.0, 2.0, -1.0], device="cuda")[torch.randint(0, 3, (Ci,), device="cuda", generator=g)]
        sh = ri(-2, 3, Ci)
        coefp = torch.stack([sc, sh, torch.zeros(Ci, device="cuda"), torch.ones(Ci, device="cuda")]).contiguous()
        Ain = torch.relu(A.double() * sc.double() + sh.double())
    gamma, beta = torch.rand(Co, device="cuda", generator=g) + 0.5, torch.randn(Co, device="cuda", generator=g)
    rm, rv = torch.randn(Co, device="cuda", generator=g), torch.rand(Co, device="cuda", generator=g) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    Z = torch.full((R + 1, Co), -7.0, device="cuda")
    coef = torch.empty(4, Co, device="cuda")
    stats = torch.empty(lib.sn_linear_stats_blocks(R), 2, Co, device="cuda")
    eps, mom = 1e-5, 0.1
    check(lib.sn_layer_forward_bn(R, Ci, Co, ptr(A), ptr(coefp), ptr(W), ptr(b), ptr(Z), ptr(stats), ptr(gamma), ptr(beta), eps, mom,
                                  ptr(rm), ptr(rv), ptr(nbt), ptr(coef), st))
    Zr = Ain @ W.double().t() + b.double()
    assert torch.equal(Z[:R].double(), Zr) and bool((Z[R] == -7.0).all()) and int(nbt) == 1
    mean, var = Zr.mean(0), Zr.var(0, unbiased=False)
    invstd = (var + eps).rsqrt()
    ref = torch.stack([gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd, mean, invstd])
    assert float((coef.double() - ref).abs().max() / ref.abs().max()) <= 1e-6
    assert torch.allclose(rm.double(), 0.9 * rm0.double() + 0.1 * mean, rtol=1e-6, atol=1e-6)
    assert torch.allclose(rv.double(), 0.9 * rv0.double() + 0.1 * Zr.var(0, unbiased=True), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("R,Ci,Co", [(50, 256, 256), (33, 128, 256), (96, 256, 192), (100, 256, 256), (192, 256, 256), (500, 128, 64),
                                      (70, 40, 72)])
@pytest.mark.parametrize("bn", [False, True])
def test_row_blocked_layer_backward_exact_small_integers(R, Ci, Co, bn):
    """A layer's backward on 33 .. 512 rows that are not whole 64-row blocks (and the small multiples of 64): ONE launch of the
    R <= 32 kernels row block by row block (rows_bwd_kernel) instead of guarded tiles + split-K partials + a reduction launch.
    Small-integer operands make everything exact: data gradient with the ReLU mask of the layer below, weight gradient over ALL rows,
    the BatchNorm-backward sums as one partial per 64 rows -- bit for bit against the integer reference; dZ = k1 dY + k2 Z + k3 with
    power-of-two coefficients in the bn case."""
    from samplenet_amd._lib import check, lib, ptr

    g = torch.Generator(device="cuda").manual_seed(R + Ci + Co)
    st = torch.cuda.current_stream().cuda_stream
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, device="cuda", generator=g).float()  # noqa: E731
    dy, W, zprev = ri(-3, 4, R, Co), ri(-4, 5, Co, Ci), ri(-4, 5, R, Ci)
    sc = torch.tensor([1.0, 2.0, -1.0], device="cuda")[torch.randint(0, 3, (Ci,), device="cuda", generator=g)]
    sh = ri(-2, 3, Ci)
    coefp = torch.stack([sc, sh, torch.zeros(Ci, device="cuda"), torch.ones(Ci, device="cuda")]).contiguous()
    z = kc = None
    dz = dy.double()
    if bn:
        z = ri(-3, 4, R, Co)
        kc = torch.stack([torch.tensor([1.0, 2.0, 0.5], device="cuda")[torch.randint(0, 3, (Co,), device="cuda", generator=g)],
                          torch.tensor([0.0, 1.0, -0.5], device="cuda")[torch.randint(0, 3, (Co,), device="cuda", generator=g)],
                          ri(-2, 3, Co)]).contiguous()
        dz = kc[0].double() * dy.double() + kc[1].double() * z.double() + kc[2].double()
    nblk = (R + 63) // 64
    dyprev = torch.full((R + 1, Ci), -7.0, device="cuda")
    stats = torch.full((lib.sn_linear_stats_blocks(R) + 1, 2, Ci), -7.0, device="cuda")
    nsplit = lib.sn_linear_wgrad_splits(R, Ci, Co, 0)
    part = torch.empty(nsplit * Co * Ci, device="cuda")
    dW = torch.full((Co + 1, Ci), -7.0, device="cuda")
    check(lib.sn_linear_backward(R, Ci, Co, 1 if bn else 0, ptr(dy), ptr(z), ptr(kc), None, None, 1, ptr(W), ptr(zprev), ptr(coefp),
                                 ptr(dyprev), ptr(stats), ptr(part), ptr(dW), st))
    act = zprev.double() * sc.double() + sh.double()
    ref_dy = (dz @ W.double()) * (act > 0)
    assert torch.equal(dyprev[:R].double(), ref_dy) and bool((dyprev[R] == -7.0).all())
    assert torch.equal(dW[:Co].double(), dz.t() @ torch.relu(act)) and bool((dW[Co] == -7.0).all())
    s = stats[:nblk].double().sum(0)
    assert torch.equal(s[0], ref_dy.sum(0)) and torch.equal(s[1], (ref_dy * zprev.double()).sum(0))
    assert bool((stats[nblk:] == -7.0).all())  # exactly ceil(R / 64) partial blocks


@pytest.mark.parametrize("R,Ci,Co", [(4096, 128, 128), (2048, 64, 128), (1024, 64, 64)])
def test_split_bf16_products_are_fp32_accurate(R, Ci, Co):
    """The conv-layer GEMMs run on the bf16 matrix cores with every fp32 operand split into three bf16 terms and six
    products per K = 16 (gemm_tile_bx3): against the fp64 product of the same fp32 inputs the error must stay at the fp32
    level -- within 4e-7 of sum |a b| per element, mean no worse than 1.5x the error of torch's own fp32 GEMM -- for
    activation-like (non-negative, offset) and gradient-like (tiny, signed) operands."""
    from samplenet_amd._lib import check, lib, ptr

    g = torch.Generator(device="cuda").manual_seed(R + Ci)
    st = torch.cuda.current_stream().cuda_stream
    for kind in ("activation", "gradient"):
        if kind == "activation":
            A = (torch.rand(R, Ci, device="cuda", generator=g) * 6.0 - 2.5).clamp_min(0.0)
        else:
            A = (torch.rand(R, Ci, device="cuda", generator=g) * 2.0 - 1.0) * 1e-3
        W = (torch.rand(Co, Ci, device="cuda", generator=g) * 2.0 - 1.0) * 0.2
        Z = torch.empty(R, Co, device="cuda")
        check(lib.sn_linear_forward(R, Ci, Co, ptr(A), None, ptr(W), None, ptr(Z), None, st))
        ref = A.double() @ W.double().t()
        mag = A.double().abs() @ W.double().abs().t()
        ours = ((Z.double() - ref).abs() / mag)
        theirs = (((A @ W.t()).double() - ref).abs() / mag)
        assert float(ours.max()) <= max(4e-7, 2.0 * float(theirs.max())), (kind, float(ours.max()), float(theirs.max()))
        assert float(ours.mean()) <= 1.5 * float(theirs.mean()) + 1e-9, (kind, float(ours.mean()), float(theirs.mean()))


@pytest.mark.parametrize("shape", [(64, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("mode,B,npts", [(1, 5, 512), (1, 1, 1000), (1, 75, 512), (2, 5, 512), (2, 33, 1024), (2, 3, 320)])
def test_fused_conv_backward_exact_small_integers(shape, mode, B, npts):
    """sn_linear_backward on the shapes served by conv_bwd_fused_kernel (persistent workgroups, dgrad + wgrad from one
    LDS tile, W in registers): integer operands make every product and sum exact, so dYprev, the BatchNorm-backward
    sums and dW must equal the float64 reference bit-for-bit -- for one tile per workgroup, several, a ragged last
    tile, and both dZ modes (dense dY; dY scattered from the max-pool selection)."""
    from samplenet_amd._lib import check, lib, ptr

    Ci, Co = shape
    R = B * npts
    g = torch.Generator(device="cuda").manual_seed(R + Ci + 7 * Co + mode)

    def ri(lo, hi, *size):
        return torch.randint(lo, hi + 1, size, device="cuda", generator=g).float()

    z, zprev, W = ri(-1, 1, R, Co), ri(-2, 2, R, Ci), ri(-1, 1, Co, Ci)
    kcoef = torch.stack([ri(1, 2, Co), ri(-1, 1, Co), ri(0, 1, Co)]).contiguous()
    coefp = torch.zeros(4, Ci, device="cuda")
    coefp[0], coefp[1] = ri(-1, 2, Ci), ri(-1, 1, Ci)
    dy = gsel = argsel = None
    if mode == 1:
        dy = ri(-1, 1, R, Co)
        dyd = dy.double()
    else:
        gsel = ri(-3, 3, B, Co)
        argsel = torch.randint(0, npts, (B, Co), device="cuda", generator=g, dtype=torch.int32)
        dyd = torch.zeros(B, npts, Co, device="cuda", dtype=torch.float64)
        dyd.scatter_(1, argsel.long().unsqueeze(1), gsel.double().unsqueeze(1))
        dyd = dyd.reshape(R, Co)
    dZ = kcoef[0].double() * dyd + kcoef[1].double() * z.double() + kcoef[2].double()
    pre = coefp[0].double() * zprev.double() + coefp[1].double()
    ref_dyp = (pre > 0) * (dZ @ W.double())
    ref_dW = dZ.t() @ pre.clamp_min(0)
    dyprev = torch.empty(R, Ci, device="cuda")
    stats = torch.zeros(lib.sn_linear_stats_blocks(R), 2, Ci, device="cuda")
    ns = lib.sn_linear_wgrad_splits(R, Ci, Co, 0)
    part = torch.empty(ns * Co * Ci, device="cuda")
    dW = torch.empty(Co, Ci, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    check(lib.sn_linear_backward(R, Ci, Co, mode, ptr(dy), ptr(z), ptr(kcoef), ptr(gsel), ptr(argsel), npts, ptr(W), ptr(zprev),
                                 ptr(coefp), ptr(dyprev), ptr(stats), ptr(part), ptr(dW), st), "sn_linear_backward")
    assert torch.equal(dyprev.double(), ref_dyp)
    assert torch.equal(dW.double(), ref_dW)
    assert torch.equal(stats.double().sum(0)[0], ref_dyp.sum(0))
    assert torch.equal(stats.double().sum(0)[1], (ref_dyp * zprev.double()).sum(0))


@pytest.mark.parametrize("B,N", [(32, 1024), (5, 320), (2, 64)])
def test_fused_pooling_equals_separate_pass(B, N):
    """The max-pool folded into the last conv layer (per-block max / min in the GEMM epilogue, pick in the BatchNorm
    finalisation: sn_conv_forward_bn_pool) returns bit-for-bit what the separate pass over the layer's output does
    (sn_layer_forward_bn + sn_pool_forward): pooled values, the selected row of every (cloud, channel) -- first row on
    ties -- its pre-BN value, the BatchNorm coefficients and the running statistics."""
    import copy

    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B * 7 + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn5.weight[::3] *= -1.0  # negative BatchNorm scales: the pool must pick the minimum there
    net_b = copy.deepcopy(net_a)
    x = torch.rand(B, N, 3, device="cuda") - 0.5
    x[:, N // 2:N // 2 + 8] = x[:, :8]  # duplicated points: exact ties in every channel
    old, old_fx = pointnet.FUSE_POOL, pointnet.FX_STATS
    try:
        pointnet.FX_STATS = False  # (the fixed-point statistics chain has its own test below)
        pointnet.FUSE_POOL = True
        ya, sa = pointnet.forward_impl(net_a, x.contiguous(), True)
        pointnet.FUSE_POOL = False
        yb, sb = pointnet.forward_impl(net_b, x.contiguous(), True)
    finally:
        pointnet.FUSE_POOL, pointnet.FX_STATS = old, old_fx
    for k in ("pooled", "argsel", "zsel"):
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(sa["cc"][4], sb["cc"][4])
    assert torch.equal(ya, yb)
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        assert torch.equal(ba, bb), n


@pytest.mark.parametrize("B,N", [(32, 1024), (5, 320), (2, 64), (48, 512)])
def test_fixed_point_statistics_chain(B, N):
    """sn_conv_stack_forward_bn (batch statistics as 64-bit fixed-point sums via integer atomics, each layer finalising the
    BatchNorm of its input; 6 launches for the conv stack) against the per-layer path (partials + bn_finalize launches):
    BatchNorm coefficients and running statistics within 1e-6 relative, layer outputs within 1e-5, same pooled points;
    and bit-for-bit reproducible from run to run (integer accumulation does not depend on the arrival order), with the
    persistent accumulators left at zero."""
    import copy

    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B * 3 + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn2.weight[::3] *= -1.0
        net_a.bn5.weight[::5] *= -1.0
    net_b, net_c = copy.deepcopy(net_a), copy.deepcopy(net_a)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).contiguous()
    old = pointnet.FX_STATS
    try:
        pointnet.FX_STATS = True
        ya, sa = pointnet.forward_impl(net_a, x, True)
        assert hasattr(net_a, "_fx_acc") and _acc_sums_zero(net_a._fx_acc)
        yc, sc = pointnet.forward_impl(net_c, x, True)
        pointnet.FX_STATS = False
        yb, sb = pointnet.forward_impl(net_b, x, True)
    finally:
        pointnet.FX_STATS = old
    assert not hasattr(net_b, "_fx_acc")
    # (the one-call stack does not materialise the xyz layer's activation where sn_conv_stack_z1_free_supported: Z1_FREE)
    assert (sa["zc"][0] is None) == (B * N >= 64 * 44)
    for l in range(5):
        assert torch.equal(sa["cc"][l], sc["cc"][l]), l  # run-to-run
        assert torch.allclose(sa["cc"][l], sb["cc"][l], rtol=2e-6, atol=1e-7), l
        if l > 0 or sa["zc"][0] is not None:
            assert torch.equal(sa["zc"][l], sc["zc"][l]), l
            assert _rel(sa["zc"][l], sb["zc"][l]) <= 1e-5, l
    assert torch.equal(ya, yc) and torch.equal(sa["argsel"], sc["argsel"])
    assert float((sa["argsel"] == sb["argsel"]).float().mean()) >= 0.995
    assert _rel(sa["pooled"], sb["pooled"]) <= 1e-5 and _rel(ya, yb) <= 1e-4
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        if ba.dtype == torch.long:
            assert int(ba) == int(bb), n
        else:
            assert torch.allclose(ba, bb, rtol=2e-6, atol=1e-8), n
    # a second step on the same module: accumulators were left clean
    pointnet.FX_STATS, keep = True, pointnet.FX_STATS
    try:
        y2, s2 = pointnet.forward_impl(net_a, x, True)
    finally:
        pointnet.FX_STATS = keep
    assert torch.equal(s2["zc"][4], sa["zc"][4]) and torch.equal(s2["cc"][4][:2], sa["cc"][4][:2])


@pytest.mark.parametrize("B,N", [(50, 2048), (32, 1024), (9, 640), (6, 320)])
def test_fixed_point_statistics_chain_256_channels(B, N):
    """The reconstruction sampler's conv stack (reconstruction/src/samplers.py:23-38: 3-64-128-128-256-bottleneck) on the one-call
    statistics chain (two accumulator blocks per layer, K = 256 on the pre-split weight planes, two 128-column
    blocks for the 256-wide layer) against the per-layer launches: as test_fixed_point_statistics_chain.  (6, 320): too few
    64-row blocks to carry the weight split -- the per-layer route must run, and does."""
    from samplenet_amd import SampleNet, pointnet
    from samplenet_amd._lib import lib
    import ctypes

    torch.manual_seed(B * 5 + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc", conv_widths=(64, 128, 128, 256), fc_widths=(256, 256),
                      fc_batchnorm=False, temperature_floor=1e-2, min_sigma=0.0).cuda().train()
    with torch.no_grad():
        net_a.bn2.weight[::3] *= -1.0
        net_a.bn4.weight[::7] *= -1.0
        net_a.bn5.weight[::5] *= -1.0
    net_b, net_c = copy.deepcopy(net_a), copy.deepcopy(net_a)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).contiguous()
    chans = (ctypes.c_int * 6)(3, 64, 128, 128, 256, 128)
    wide = bool(lib.sn_conv_stack_forward_supported(B, N, 5, chans))
    assert wide == (B * N // 64 >= 88)
    old = pointnet.FX_STATS
    try:
        pointnet.FX_STATS = True
        ya, sa = pointnet.forward_impl(net_a, x, True)
        yc, sc = pointnet.forward_impl(net_c, x, True)
        pointnet.FX_STATS = False
        yb, sb = pointnet.forward_impl(net_b, x, True)
    finally:
        pointnet.FX_STATS = old
    assert hasattr(net_a, "_fx_acc") == wide
    if wide:  # (two accumulator blocks per layer in this layout)
        assert _acc_sums_zero(net_a._fx_acc, 5, (3, 64, 128, 128, 256, 128))
    for l in range(5):
        assert torch.equal(sa["cc"][l], sc["cc"][l]), l  # run-to-run
        assert torch.allclose(sa["cc"][l], sb["cc"][l], rtol=2e-6, atol=1e-7), l
        assert torch.equal(sa["zc"][l], sc["zc"][l]), l
        assert _rel(sa["zc"][l], sb["zc"][l]) <= 1e-5, l
    assert torch.equal(ya, yc) and torch.equal(sa["argsel"], sc["argsel"])
    assert float((sa["argsel"] == sb["argsel"]).float().mean()) >= 0.995
    assert _rel(sa["pooled"], sb["pooled"]) <= 1e-5 and _rel(ya, yb) <= 1e-4
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        if ba.dtype == torch.long:
            assert int(ba) == int(bb), n
        else:
            assert torch.allclose(ba, bb, rtol=2e-6, atol=1e-8), n
    y2, s2 = pointnet.forward_impl(net_a, x, True)  # a second step on the same module: accumulators were left clean
    assert torch.equal(s2["zc"][4], sa["zc"][4]) and torch.equal(s2["cc"][4][:2], sa["cc"][4][:2])


@pytest.mark.parametrize("B,N", [(32, 1024), (5, 320), (3, 330)])
def test_first_activation_rebuilt_from_the_cloud(B, N):
    """Z1_FREE: the xyz layer runs as a statistics-only pass and conv2's forward / backward rebuild its activation from the
    cloud with the same expression -- every output, every BatchNorm buffer and every gradient is bit-identical to the run that
    writes and re-reads the 8 MB tensor; the per-layer backward (which needs the tensor) materialises it on demand."""
    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn1.weight[::4] *= -1.0
        net_a.bn1.bias.add_(0.1 * torch.randn_like(net_a.bn1.bias))
    net_b, net_c = copy.deepcopy(net_a), copy.deepcopy(net_a)
    x = ((torch.rand(B, N, 3, device="cuda") - 0.5) * torch.tensor([1.0, 0.6, 1.4], device="cuda") + 0.05).contiguous()
    g = torch.randn(B, 3, 64, device="cuda")
    old, old_fx = pointnet.Z1_FREE, pointnet.FX_STATS
    try:
        pointnet.Z1_FREE = True
        ya = net_a._features(x.permute(0, 2, 1), x)
        (ya * g).sum().backward()
        yc = net_c._features(x.permute(0, 2, 1), x)
        pointnet.FX_STATS = False  # backward through the per-layer entries: needs Z1
        (yc * g).sum().backward()
        pointnet.FX_STATS = True
        pointnet.Z1_FREE = False
        yb = net_b._features(x.permute(0, 2, 1), x)
        (yb * g).sum().backward()
    finally:
        pointnet.Z1_FREE, pointnet.FX_STATS = old, old_fx
    assert torch.equal(ya, yb) and torch.equal(yc, yb)
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        assert torch.equal(ba, bb), n
    gc = dict(net_c.named_parameters())
    gmax = max(float(p.grad.norm()) for n, p in net_b.named_parameters() if p.grad is not None)
    for (n, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        if n.startswith("project"):
            continue
        assert torch.equal(pa.grad, pb.grad), n
        # the per-layer backward of the third run rebuilt the tensor with the xyz kernel: same operands as the stack's kernels
        floor = 2e-5 if (n.endswith(".bias") and n.startswith(("conv", "fc1", "fc2", "fc3"))) else 1e-6
        assert float((gc[n].grad - pb.grad).norm()) <= 1e-4 * float(pb.grad.norm()) + floor * gmax, n


@pytest.mark.parametrize("scale", [3.0e3, 2.0e5, 1.0e-4])
def test_fixed_point_statistics_range(scale):
    """The fixed-point accumulators are exact over the whole fp32 range that matters: unnormalised clouds (coordinates in
    the thousands: block sums beyond 2^18 take the split lo / hi path), tiny ones (sums far below 1), and gradients scaled
    accordingly -- forward coefficients and all gradients still agree with the partial-sum path; a non-finite input poisons
    the statistics (NaN BatchNorm coefficients -> NaN output, never a wrapped sum), and the step after it is clean."""
    import copy

    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(17)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    net_b = copy.deepcopy(net_a)
    x = ((torch.rand(8, 512, 3, device="cuda") - 0.5) * scale).contiguous()
    g = torch.randn(8, 3, 64, device="cuda") * (1.0 / scale)
    old = pointnet.FX_STATS
    try:
        pointnet.FX_STATS = True
        ya = net_a._features(x.permute(0, 2, 1), x)
        (ya * g).sum().backward()
        pointnet.FX_STATS = False
        yb = net_b._features(x.permute(0, 2, 1), x)
        (yb * g).sum().backward()
    finally:
        pointnet.FX_STATS = old
    assert torch.isfinite(ya).all() and _rel(ya, yb) <= 1e-4
    for l in (1, 2, 3, 4, 5):
        ra, rb = getattr(net_a, "bn%d" % l).running_var, getattr(net_b, "bn%d" % l).running_var
        assert torch.allclose(ra, rb, rtol=2e-6, atol=0), l
    gb = {n: p.grad for n, p in net_b.named_parameters() if p.grad is not None}
    gmax = max(float(v.norm()) for v in gb.values())
    for n, p in net_a.named_parameters():
        if not n.startswith("project"):
            # (a bias in front of a BatchNorm has a zero gradient: what both paths return is the rounding noise of a
            #  cancellation, a few 1e-6 of the largest gradient at these scales)
            floor = 2e-5 if (n.endswith(".bias") and n.startswith(("conv", "fc1", "fc2", "fc3"))) else 1e-6
            assert float((p.grad - gb[n]).norm()) <= 1e-4 * float(gb[n].norm()) + floor * gmax, n
    # poison: a non-finite coordinate -> NaN output, accumulators clean for the next step
    xbad = x.clone()
    xbad[0, 0, 0] = float("inf")
    old = pointnet.FX_STATS
    try:
        pointnet.FX_STATS = True
        with torch.no_grad():
            ybad = net_a._features(xbad.permute(0, 2, 1), xbad)
            assert torch.isnan(ybad).any()  # NaN coefficients + NaN-propagating ReLU: loud, as torch's own modules
            assert not torch.isfinite(net_a.bn1.running_mean).all() or not torch.isfinite(net_a.bn1.running_var).all()
            net_a.load_state_dict(net_b.state_dict())  # the poisoned step wrote NaN running statistics
            net_c = copy.deepcopy(net_b)
            y2 = net_a._features(x.permute(0, 2, 1), x)
            pointnet.FX_STATS = False
            y3 = net_c._features(x.permute(0, 2, 1), x)
    finally:
        pointnet.FX_STATS = old
    assert torch.isfinite(y2).all() and _rel(y2, y3) <= 1e-4


@pytest.mark.parametrize("B,N", [(32, 1024), (5, 320), (3, 330), (33, 1024)])
def test_input_layer_weight_gradient_closed_form(B, N):
    """conv1's weight gradient taken out of conv2's fused backward (three extra per-channel sums + the moments of x,
    combined in double: sn_layer_backward_in3) against the separate pass over dY1 (sn_layer_backward + sn_linear_wgrad):
    conv1.weight within 2e-5 of its norm (different summation order, same cancellation), every other gradient bit-equal
    (the dgrad / wgrad arithmetic of conv2 is unchanged).  R = B*N both a multiple of the 64-row tile and not."""
    import copy

    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn1.weight[::4] *= -1.0
        net_a.bn1.bias.add_(0.1 * torch.randn_like(net_a.bn1.bias))
    net_b = copy.deepcopy(net_a)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5) * torch.tensor([1.0, 0.6, 1.4], device="cuda") + 0.05
    from samplenet_amd._lib import lib
    assert lib.sn_layer_backward_in3_stats_floats(B * N, 64, 64) > 0
    g = torch.randn(B, 3, 64, device="cuda")
    old, old_fx = pointnet.IN3_CLOSED_FORM, pointnet.FX_STATS
    try:
        pointnet.FX_STATS = False  # per-layer entries on both sides (the one-call stack has its own test below)
        pointnet.IN3_CLOSED_FORM = True
        (net_a._features(x.permute(0, 2, 1), x) * g).sum().backward()
        pointnet.IN3_CLOSED_FORM = False
        (net_b._features(x.permute(0, 2, 1), x) * g).sum().backward()
    finally:
        pointnet.IN3_CLOSED_FORM, pointnet.FX_STATS = old, old_fx
    for (n, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        if n.startswith("project"):
            continue
        if n == "conv1.weight":
            assert _rel(pa.grad, pb.grad) <= 2e-5, (n, _rel(pa.grad, pb.grad))
        else:
            assert torch.equal(pa.grad, pb.grad), n


@pytest.mark.parametrize("B,N", [(32, 1024), (5, 320), (33, 1024), (4, 64)])
def test_conv_stack_one_call_backward(B, N):
    """sn_conv_stack_forward_bn + sn_conv_stack_backward (5 + 5 launches, statistics as fixed-point atomics, one closing
    reduction of all weight-gradient partials) against the per-layer entries (partials + reduction launches): every
    gradient within 1e-4 of its norm (+ noise floor for the zero-gradient biases), bit-for-bit reproducible from run to
    run, persistent accumulators left at zero."""
    import copy

    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B * 5 + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn3.weight[::4] *= -1.0
    net_b, net_c = copy.deepcopy(net_a), copy.deepcopy(net_a)
    x = torch.rand(B, N, 3, device="cuda") - 0.5
    g = torch.randn(B, 3, 64, device="cuda")
    old = pointnet.FX_STATS
    try:
        pointnet.FX_STATS = True
        (net_a._features(x.permute(0, 2, 1), x) * g).sum().backward()
        (net_c._features(x.permute(0, 2, 1), x) * g).sum().backward()
        pointnet.FX_STATS = False
        (net_b._features(x.permute(0, 2, 1), x) * g).sum().backward()
    finally:
        pointnet.FX_STATS = old
    assert hasattr(net_a, "_fx_acc_b") and _acc_sums_zero(net_a._fx_acc_b) and _acc_sums_zero(net_a._fx_acc)
    gb = {n: p.grad for n, p in net_b.named_parameters() if p.grad is not None}
    gmax = max(float(v.norm()) for v in gb.values())
    gc = dict(net_c.named_parameters())
    for n, p in net_a.named_parameters():
        if n.startswith("project"):
            continue
        assert torch.equal(p.grad, gc[n].grad), n  # run to run
        assert float((p.grad - gb[n]).norm()) <= 1e-4 * float(gb[n].norm()) + 1e-6 * gmax, n


@pytest.mark.parametrize("B,N,shape", [(4, 1024, "bcn"), (3, 64, "bnc"), (2, 200, "bcn")])
def test_task_network_features_vs_torch(B, N, shape):
    """samplenet_amd.task_features.PointNetFeatures (rows a12 / f1: registration/models/pcrnet.py:8-41 -- five 1x1 convs with
    ReLU, no BatchNorm, max over points, bottleneck 1024) against the same module on torch.nn: forward 1e-5, gradient to
    the input cloud (the path the sampler's task loss takes) and to the weights within fp32 GEMM rounding."""
    import torch.nn.functional as F

    from samplenet_amd.task_features import PointNetFeatures

    torch.manual_seed(N)
    net = PointNetFeatures(1024, shape).cuda()
    x = (torch.rand(B, 3, N, device="cuda") - 0.5) if shape == "bcn" else (torch.rand(B, N, 3, device="cuda") - 0.5)
    x.requires_grad_(True)
    y = net(x)
    assert y.shape == (B, 1024)
    xr = x.detach().clone().requires_grad_(True)
    h = xr if shape == "bcn" else xr.permute(0, 2, 1)
    for conv in (net.conv1, net.conv2, net.conv3, net.conv4, net.conv5):
        h = F.relu(conv(h))
    yr = torch.max(h, 2)[0]
    assert torch.allclose(y, yr, rtol=1e-5, atol=1e-6)
    w = torch.randn_like(y)
    params = [net.conv1.weight, net.conv3.weight, net.conv5.weight, net.conv5.bias]
    got = torch.autograd.grad((y * w).sum(), [x] + params)
    want = torch.autograd.grad((yr * w).sum(), [xr] + params)
    for a, b in zip(got, want):
        scale = float(b.abs().max()) + 1e-12
        assert float((a.reshape(b.shape) - b).abs().max()) <= 2e-4 * scale


def test_pcrnet_task_loss_matches_reference(golden):
    """Row f1: the registration task network and the Chamfer term of its loss (registration/models/pcrnet.py:44-82,
    main.py:557-577 with --loss-type 1) against the REFERENCE modules run on CPU (tests/golden/make_golden.py:golden_pcrnet:
    reference PCRNet + reference qrot + the reference's own compiled Chamfer): same default-initialised weights (checked by
    checksum), twist / pre-normalised quaternion / loss within 1e-5, the gradient that flows back to the (sampled) template
    cloud and the weight gradients within 2e-4 of their norms."""
    from samplenet_amd.task_features import PCRNet, pcrnet_chamfer_loss

    g = golden("pcrnet_reference.npz")
    torch.manual_seed(21)
    model = PCRNet(bottleneck_size=256, input_shape="bnc")
    for n, p in model.named_parameters():
        assert abs(float(p.detach().double().abs().sum()) - float(g["w_" + n.replace(".", "_")])) <= 1e-9 * max(1.0, float(g["w_" + n.replace(".", "_")])), n
    model = model.cuda()
    p0 = torch.from_numpy(g["p0"]).cuda().requires_grad_(True)
    p1 = torch.from_numpy(g["p1"]).cuda()
    loss, qnorm, twist = pcrnet_chamfer_loss(model, p0, p1)
    assert torch.allclose(twist.detach().cpu(), torch.from_numpy(g["twist"]), rtol=1e-5, atol=1e-6)
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    assert abs(float(qnorm) - float(g["qnorm"])) <= 1e-5 * max(1.0, abs(float(g["qnorm"])))
    loss.backward()
    assert _rel(p0.grad.cpu(), torch.from_numpy(g["grad_p0"])) <= 2e-4
    for n, p in model.named_parameters():
        key = "g_" + n.replace(".", "_")
        if key in g.files:
            assert _rel(p.grad.cpu(), torch.from_numpy(g[key])) <= 2e-4, n


@pytest.mark.parametrize("variant", ["reconstruction", "classification"])
@pytest.mark.parametrize("B,N,M,K", [(32, 1024, 64, 8), (50, 2048, 64, 16), (6, 320, 32, 5)])
def test_sampler_variants_vs_torch(variant, B, N, M, K):
    """The TF packages' sampler architectures (SURVEY C4 / config #4 sampler) through the same HIP kernels: head output,
    every parameter gradient and the whole module step (projection + losses + temperature gradient with the variant's
    sigma rule) against the torch.nn op chain on the same weights."""
    from samplenet_amd import SampleNet

    torch.manual_seed(B + N)
    net = SampleNet(M, 128, group_size=K, initial_temperature=0.5, input_shape="bnc", output_shape="bnc", **VARIANTS[variant]).cuda().train()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if "bn" in n:
                p.add_(0.1 * torch.randn_like(p))
    ref = torch_mlp_copy(net).train()
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}  # (before the step moves the running statistics)
    x = torch.rand(B, N, 3, device="cuda") - 0.5

    def step(m, xx):
        simp, proj = m(xx)
        return 0.01 * m.get_simplification_loss(xx, simp, M, 1, 0.01) + 0.01 * m.get_projection_loss() + proj.mean(), simp

    la, sa = step(net, x)
    lb, sb = step(ref, x)
    la.backward(), lb.backward()
    # yardstick: the same network in fp64 -- the HIP head must be as close to it as torch's fp32 path is (x2), or within the floor
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        ref64.load_state_dict({k: v.double() for k, v in sd0.items()})
        y64 = ref64._features(x.double().permute(0, 2, 1)).permute(0, 2, 1)
    e_hip, e_ref = float((sa.double() - y64).abs().max()), float((sb.double() - y64).abs().max())
    assert e_hip <= max(2e-4 if B >= 16 else 2e-3, 2 * e_ref), (e_hip, e_ref)
    assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb)))
    gb = {n: p.grad for n, p in ref.named_parameters()}
    gmax = max(float(g.norm()) for g in gb.values())
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        assert float((p.grad - gb[n]).norm()) <= (5e-3 if B >= 16 else 1e-1) * float(gb[n].norm()) + 1e-5 * gmax, n
    assert set(dict(net.named_parameters())) == set(gb)
    # sigma rule of the variant
    if variant == "reconstruction":
        with torch.no_grad():
            net.project._temperature.fill_(-0.3)
        assert abs(float(net.get_projection_loss()) - 1e-4) < 1e-9  # max(T, 1e-2)^2


@pytest.mark.parametrize("B,Ci,Co", [(32, 256, 192), (7, 256, 96), (1, 128, 48), (33, 256, 192), (200, 256, 192), (32, 192, 60)])
@pytest.mark.parametrize("training", [True, False])
def test_output_batchnorm_kernels_vs_torch(B, Ci, Co, training):
    """The classification sampler's output layer -- Linear then BatchNorm1d WITHOUT activation (classification/models/
    samplenet_model.py:100-108) -- through pointnet._last_layer / backward_impl's first stage (sn_layer_forward_bn_out up to 32 rows
    and power-of-two widths, sn_linear_forward_rows + sn_bn_output_forward otherwise; sn_bn_output_backward) against torch in fp64:
    output, running statistics, dZ, dgamma, dbeta -- batch statistics (training) and running statistics (eval)."""
    from samplenet_amd import pointnet
    from samplenet_amd._lib import check, lib, ptr, stream_of

    if B == 1 and training:
        pytest.skip("torch refuses one row in training mode (the kernel normalises it to beta)")
    torch.manual_seed(B * 7 + Co)
    lin = torch.nn.Linear(Ci, Co).cuda()
    bn = torch.nn.BatchNorm1d(Co).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(Co) * 0.5 + 1.0), bn.bias.copy_(torch.randn(Co) * 0.3)
        bn.running_mean.copy_(torch.randn(Co) * 0.1), bn.running_var.copy_(torch.rand(Co) + 0.5)
    bn.train(training)
    ref_lin, ref_bn = copy.deepcopy(lin).double(), copy.deepcopy(bn).double()
    a = torch.randn(B, Ci, device="cuda")
    gy = torch.randn(B, Co, device="cuda")
    L = pointnet._Layer("fc4", lin, "bn_fc4", None)
    saved = {}
    y = pointnet._last_layer(B, L, ("bn_fc4", bn), a, None, training, saved)
    a64 = a.double().requires_grad_(True)
    z64 = ref_lin(a64)
    z64.retain_grad()
    y64 = ref_bn(z64)
    y64.backward(gy.double())
    assert float((y.double() - y64).abs().max()) <= 2e-5 * max(1.0, float(y64.abs().max()))
    assert torch.allclose(bn.running_mean.double(), ref_bn.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.running_var.double(), ref_bn.running_var, rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked)
    assert saved["out_fixed"] == (not training)
    dz, dg, db = torch.empty(B, Co, device="cuda"), torch.empty(Co, device="cuda"), torch.empty(Co, device="cuda")
    check(lib.sn_bn_output_backward(B, Co, 0 if training else 1, ptr(gy), ptr(saved["z_out"]), ptr(saved["c_out"]), ptr(dz), ptr(dg),
                                    ptr(db), stream_of(gy)), "sn_bn_output_backward")
    for got, want in ((dz, z64.grad), (dg, ref_bn.weight.grad), (db, ref_bn.bias.grad)):
        assert float((got.double() - want).norm()) <= 2e-5 * float(want.norm()) + 1e-6
    # deterministic
    dz2 = torch.empty_like(dz)
    check(lib.sn_bn_output_backward(B, Co, 0 if training else 1, ptr(gy), ptr(saved["z_out"]), ptr(saved["c_out"]), ptr(dz2), ptr(dg),
                                    ptr(db), stream_of(gy)), "sn_bn_output_backward")
    assert torch.equal(dz, dz2)


@pytest.mark.parametrize("B,M", [(32, 64), (5, 32), (17, 64)])
def test_fc_chain_output_stage_equals_the_separate_output_layer(B, M):
    """sn_fc_chain_forward_pool_out (the classification sampler's output layer + BatchNorm as the LAST STAGE of the forward FC
    chain) against the chain without it + sn_layer_forward_bn_out: hidden layers bit-identical (the added hand-off of the last
    hidden layer changes no arithmetic), the output layer's pre-BN values bit-identical (same K split and summation order), its
    BatchNorm coefficients / the head's output / running statistics within 2 ulp-level tolerances (fp32 1/sqrt with host-side
    reciprocals in the chain, as its hidden layers), the backward's gradients accordingly; repeated calls, error word clear."""
    from samplenet_amd import SampleNet, pointnet
    from samplenet_amd._lib import lib

    torch.manual_seed(B + M)
    net_a = SampleNet(M, 128, group_size=4, input_shape="bnc", output_shape="bnc", last_fc_batchnorm=True, min_sigma=0.0).cuda().train()
    with torch.no_grad():
        net_a.bn_fc4.weight.copy_(torch.rand_like(net_a.bn_fc4.weight) + 0.5), net_a.bn_fc4.bias.normal_(0, 0.2)
    net_b = copy.deepcopy(net_a)
    orig = lib.sn_fc_chain_forward_pool_out_supported
    for it in range(3):
        x = (torch.rand(B, 256, 3, device="cuda") - 0.5).contiguous()
        ya, sa = pointnet.forward_impl(net_a, x, True, use_plan=False)
        assert "y_out" in sa and ya is sa["y_out"]
        try:  # the same module with the output stage refused: chain + separate output layer launch
            lib.sn_fc_chain_forward_pool_out_supported = lambda *a: 0
            yb, sb = pointnet.forward_impl(net_b, x, True, use_plan=False)
        finally:
            lib.sn_fc_chain_forward_pool_out_supported = orig
        assert "y_out" not in sb and "z_out" in sb
        for l in range(3):
            assert torch.equal(sa["zf"][l], sb["zf"][l]) and torch.equal(sa["cf"][l], sb["cf"][l]), (it, l)
        assert torch.equal(sa["z_out"], sb["z_out"]), it
        assert torch.allclose(sa["c_out"], sb["c_out"], rtol=3e-6, atol=1e-7), it
        assert torch.allclose(ya, yb, rtol=1e-5, atol=2e-6), it
        gy = torch.randn(B, 3 * M, device="cuda")
        ga = pointnet.backward_impl(net_a, sa, gy)  # (the output BatchNorm's backward opens the FC chain's backward launch)
        orig_b = pointnet._fc_chain_bwd
        try:  # reference: the stand-alone sn_bn_output_backward launch in front of the chain
            def plain(net, convs, fcs, saved, grad_y, sink, grads, fixed, obn=None):
                if obn is None:
                    return orig_b(net, convs, fcs, saved, grad_y, sink, grads, fixed)
                return False
            pointnet._fc_chain_bwd = plain
            gb = pointnet.backward_impl(net_b, sb, gy)
        finally:
            pointnet._fc_chain_bwd = orig_b
        gmax = max(float(v.norm()) for v in gb.values())
        for n in gb:
            # (a bias in front of a BatchNorm has a zero gradient up to rounding noise of the size 1e-6 gmax: absolute floor)
            assert float((ga[n] - gb[n]).norm()) <= 2e-5 * float(gb[n].norm()) + 1e-5 * gmax, (it, n)
    for (n, a), (_, b) in zip(net_a.named_buffers(), net_b.named_buffers()):
        assert torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-7), n
    assert pointnet.chain_error_words(net_a) == (0, 0)


@pytest.mark.parametrize("B,bneck", [(32, 128), (4, 128), (17, 256), (32, 64)])
def test_fc_chain_forward_equals_per_layer_launches(B, bneck):
    """sn_fc_chain_forward (the FC head's three BatchNorm + ReLU layers as ONE launch, activations handed between the
    resident workgroups through write-through stores + arrival counters) against the layer-by-layer launches: pre-BN outputs,
    BatchNorm coefficients, running statistics and the head's output; repeated calls (monotonic epoch counters) and the
    error word stays clear."""
    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B + bneck)
    net_a = SampleNet(64, bneck, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    net_b = copy.deepcopy(net_a)
    xs = [(torch.rand(B, 256, 3, device="cuda") - 0.5).contiguous() for _ in range(4)]
    old = pointnet.FC_CHAIN
    try:
        for x in xs:
            pointnet.FC_CHAIN = True
            ya, sa = pointnet.forward_impl(net_a, x, True)
            pointnet.FC_CHAIN = False
            yb, sb = pointnet.forward_impl(net_b, x, True)
            assert "fc_chain" in sa and "fc_chain" not in sb
            # same GEMM arithmetic (layer 0's pre-BN output is bit-identical); the chain finishes the BatchNorm with fp32
            # 1 / sqrt (as torch does) and host-side reciprocals instead of double divisions: coefficients within 2 ulp,
            # which the following layers inherit
            assert torch.equal(sa["zf"][0], sb["zf"][0])
            for l in range(3):
                tol = 3e-7 if l == 0 else 1e-5  # (layers 1.. see inputs that already differ by an ulp or two)
                assert torch.allclose(sa["cf"][l], sb["cf"][l], rtol=tol, atol=tol), l
                assert float((sa["zf"][l] - sb["zf"][l]).abs().max()) <= 1e-5 * float(sb["zf"][l].abs().max()), l
            assert float((ya - yb).abs().max()) <= 1e-5 * float(yb.abs().max())
    finally:
        pointnet.FC_CHAIN = old
    torch.cuda.synchronize()
    assert int(net_a._fc_sync[15, 0]) == 0 and int(net_a._fc_sync[0, 0]) == len(xs)
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        assert torch.allclose(ba.float(), bb.float(), rtol=1e-5, atol=1e-6), n


@pytest.mark.parametrize("B,N", [(32, 1024), (32, 256), (5, 1024), (2, 64), (17, 704)])
def test_pool_stage_of_the_fc_chain_equals_the_separate_launch(B, N):
    """sn_fc_chain_forward_pool (last conv BatchNorm from the fixed-point sums + max-pool decoded from the per-cloud (value,
    row) keys that conv5's epilogue combined by atomicMax, as the first stage of the FC chain) against the block-partial path
    (sn_conv_stack_forward_bn's own finalisation launch + sn_fc_chain_forward): bit for bit -- pooled features, selected rows
    (ties: the first row), pre-BN values, bn5 coefficients, every FC layer, running statistics -- with negative BatchNorm
    scales on some channels (those pick the MINIMA) and a zero scale, repeatedly; the statistics accumulators are left zero."""
    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B * 7 + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn5.weight[::5] *= -1.0
        net_a.bn5.weight[3] = 0.0
        net_a.bn5.bias.normal_(0, 0.1)
    net_b = copy.deepcopy(net_a)
    old = pointnet.POOL_IN_CHAIN
    try:
        for rep in range(3):
            x = (torch.rand(B, N, 3, device="cuda") - 0.5).contiguous()
            pointnet.POOL_IN_CHAIN = True
            ya, sa = pointnet.forward_impl(net_a, x, True)
            pointnet.POOL_IN_CHAIN = False
            yb, sb = pointnet.forward_impl(net_b, x, True)
            assert "fc_chain" in sa and "fc_chain" in sb
            for k in ("pooled", "argsel", "zsel"):
                assert torch.equal(sa[k], sb[k]), k
            assert torch.equal(sa["cc"][-1], sb["cc"][-1])
            for l in range(3):
                assert torch.equal(sa["zf"][l], sb["zf"][l]) and torch.equal(sa["cf"][l], sb["cf"][l]), l
            assert torch.equal(ya, yb)
            assert _acc_sums_zero(net_a._fx_acc) and _acc_sums_zero(net_b._fx_acc)
    finally:
        pointnet.POOL_IN_CHAIN = old
    assert int(net_a._fc_sync[15, 0]) == 0 and int(net_a._fc_sync[0, 0]) == 3
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        # (bn5's running statistics: same expression compiled into two kernels -- the momentum blend contracts into a
        #  different fma; one ulp)
        assert torch.equal(ba, bb) or (n.startswith("bn5.running") and torch.allclose(ba, bb, rtol=2.5e-7, atol=1e-9)), n


@pytest.mark.parametrize("B,bneck,variant,training", [(32, 128, None, True), (4, 128, None, True), (17, 256, None, True),
                                                     (32, 128, "reconstruction", True), (32, 128, None, False)])
def test_fc_chain_backward_equals_per_layer_launches(B, bneck, variant, training):
    """sn_fc_chain_backward (the FC head's whole backward -- data gradients, BatchNorm backward, weight and bias gradients,
    pooling backward -- as ONE launch with in-kernel hand-offs) against the layer-by-layer launches on the same saved
    forward: every parameter gradient of the head and of the conv stack (the top layer's bit for bit), repeatedly; error
    word clear."""
    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(B + bneck + 3)
    kw = VARIANTS[variant] if variant else {}
    net = SampleNet(64, bneck, group_size=8, input_shape="bnc", output_shape="bnc", **kw).cuda().train(training)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.add_(0.2 * torch.randn_like(m.weight))
    old = pointnet.FC_CHAIN
    try:
        for rep in range(3):
            x = (torch.rand(B, 256, 3, device="cuda") - 0.5).contiguous()
            gy = torch.randn(B, 192, device="cuda")
            pointnet.FC_CHAIN = True
            _, saved = pointnet.forward_impl(net, x, training)
            ga = pointnet.backward_impl(net, saved, gy)
            assert "fc_chain_b" in saved
            pointnet.FC_CHAIN = False
            gb = pointnet.backward_impl(net, saved, gy)
            assert set(ga) == set(gb) and len(ga) == len(pointnet.param_order(net))
            # same arithmetic, but the compiler contracts the two epilogues' sums differently: last-bit differences in the
            # BatchNorm-backward coefficients, which everything below inherits (the biases in front of a BatchNorm hold pure
            # rounding noise on both sides: absolute floor relative to the largest gradient)
            gmax = max(float(v.abs().max()) for v in gb.values())
            # (B < 16: BatchNorm over a handful of rows amplifies those last bits further -- measured up to 4.6e-5 at B = 4)
            rel = 2e-5 if B >= 16 else 6e-5
            for n in ga:
                assert float((ga[n] - gb[n]).abs().max()) <= rel * float(gb[n].abs().max()) + 3e-6 * gmax, (rep, n)
            assert torch.equal(ga["fc4.weight" if "fc4.weight" in ga else "fc3.weight"], gb["fc4.weight" if "fc4.weight" in gb else "fc3.weight"])
    finally:
        pointnet.FC_CHAIN = old
    torch.cuda.synchronize()
    assert int(net._fc_sync_b[15, 0]) == 0 and int(net._fc_sync_b[0, 0]) == 3


def _provoke(sync, counter):
    """A hand-off of the NEXT chain launch that can never complete: its arrival counter lags a thousand arrivals behind what
    the launch will wait for (the effect of a workgroup that is not resident), with a short poll bound instead of seconds."""
    sync[13, 0] = 3000
    sync[counter, 0] -= 1000


@pytest.mark.parametrize("which", ["forward", "backward"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_fc_chain_timeout_is_never_silent(which, use_graph):
    """VERDICT r2 / ADVICE r2: a chain kernel whose inter-workgroup poll gives up used to set sync[15] and train on garbage with a
    finite loss.  Now: the workgroups that saw the timeout write NaN instead of their outputs (forward: the head's last
    activations -> NaN simplified cloud, NaN loss, NaN gradients; backward: NaN parameter gradients), the fused step's deferred
    tail turns the loss VALUE into NaN from the error words, and the host check raises and re-arms the launch state -- after
    which the step is healthy again and reproduces the loss it had before."""
    from samplenet_amd import SampleNet, pointnet
    from samplenet_amd._lib import SampleNetHipError
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    torch.manual_seed(5)
    net = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    red = FlatGradAllReducer(net)
    x = torch.rand(32, 1024, 3, device="cuda") - 0.5
    step = SamplerTrainStep(net, x, reducer=red, use_graph=use_graph)
    assert step._fast_path()
    good = float(step(x))
    step.check()
    assert good == good and pointnet.chain_error_words(net) == (0, 0)
    flat_good = red.flat.clone()
    if which == "forward":
        _provoke(net._fc_sync, 1)       # seam 0 of the forward chain
    else:
        _provoke(net._fc_sync_b, 2)     # arrivals of the backward chain's second stage
    loss = step(x)
    torch.cuda.synchronize()
    words = pointnet.chain_error_words(net)
    assert words[0 if which == "forward" else 1] != 0, words
    assert torch.isnan(loss).item(), float(loss)            # no finite loss on incomplete data
    assert torch.isnan(red.flat).any().item()                # ... and no clean-looking gradients
    with pytest.raises(SampleNetHipError, match="timed out"):
        step.check()
    assert pointnet.chain_error_words(net) == (0, 0)         # re-armed by the check
    for t in (net._fc_sync, net._fc_sync_b):
        t[13, 0] = 0                                         # (default poll bound again)
    again = step(x)
    torch.cuda.synchronize()
    step.check()
    assert float(again) == good and torch.equal(red.flat, flat_good)


def test_fc_chain_timeout_in_the_module_surface():
    """The same through the plain module surface (no engine, no deferred tail): a timed-out forward chain yields a NaN
    simplified cloud (hence NaN losses), pointnet.check_chain_errors raises."""
    from samplenet_amd import SampleNet, pointnet
    from samplenet_amd._lib import SampleNetHipError

    torch.manual_seed(6)
    net = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    x = torch.rand(16, 512, 3, device="cuda") - 0.5
    simp, proj = net(x)
    assert torch.isfinite(simp).all() and not pointnet.check_chain_errors(net)
    _provoke(net._fc_sync, 2)
    simp, proj = net(x)
    loss = net.get_simplification_loss(x, simp, 64, 1, 0) + proj.mean()
    assert torch.isnan(simp).any() and torch.isnan(loss)
    with pytest.raises(SampleNetHipError):
        pointnet.check_chain_errors(net)
    net._fc_sync[13, 0] = 0
    simp, _ = net(x)
    assert torch.isfinite(simp).all() and not pointnet.check_chain_errors(net)


def test_forward_plan_replays_are_identical_and_isolated():
    """pointnet._ForwardPlan: once a shape has been seen, the head's training forward re-issues the recorded C calls on
    recycled buffers.  Same bits as the allocate-per-step route; a second forward before the first one's backward runs on
    buffers of its own (two sampler passes under one loss, main.py:516-524); moving the module drops the plans."""
    from samplenet_amd import SampleNet, pointnet

    torch.manual_seed(31)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    net_b = copy.deepcopy(net_a)
    xs = [(torch.rand(32, 1024, 3, device="cuda") - 0.5) for _ in range(4)]
    gys = [torch.randn(32, 192, device="cuda") for _ in range(4)]
    old = pointnet.FORWARD_PLAN
    try:
        for i, (x, gy) in enumerate(zip(xs, gys)):
            pointnet.FORWARD_PLAN = True
            ya, sa = pointnet.forward_impl(net_a, x, True)
            ga = pointnet.backward_impl(net_a, sa, gy)
            assert ("_lease" in sa) and len(net_a._sn_plans) == 1
            pointnet.FORWARD_PLAN = False
            yb, sb = pointnet.forward_impl(net_b, x, True)
            gb = pointnet.backward_impl(net_b, sb, gy)
            assert "_lease" not in sb
            assert torch.equal(ya, yb), i
            for n in ga:
                assert torch.equal(ga[n], gb[n]), (i, n)
            del sa, sb
        for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
            assert torch.equal(ba, bb), n
        # two forwards alive at once: the second must not run on the first one's buffers
        pointnet.FORWARD_PLAN = True
        y1, s1 = pointnet.forward_impl(net_a, xs[0], True)
        z1 = [t.clone() for t in s1["zf"]]
        y2, s2 = pointnet.forward_impl(net_a, xs[1], True)
        assert len(net_a._sn_plans) == 2 and s1["zf"][0].data_ptr() != s2["zf"][0].data_ptr()
        assert all(torch.equal(a, b) for a, b in zip(z1, s1["zf"]))
        g1 = pointnet.backward_impl(net_a, s1, gys[0])
        pointnet.FORWARD_PLAN = False
        yr, sr = pointnet.forward_impl(net_b, xs[0], True)
        pointnet.forward_impl(net_b, xs[1], True)  # (running statistics in step)
        assert torch.equal(y1, yr)
        del s1, s2, sr
        pointnet.FORWARD_PLAN = True
        assert not any(q.busy for q in net_a._sn_plans)
        # skip_last (the fused step's form) has plans of its own; a moved / cast module starts over
        _, s3 = pointnet.forward_impl(net_a, xs[2], True, skip_last=True)
        assert len(net_a._sn_plans) == 3
        del s3
        net_a.float()
        assert "_sn_plans" not in net_a.__dict__
    finally:
        pointnet.FORWARD_PLAN = old


def test_fp32_mfma_twin_agrees_with_the_split_bf16_build(tmp_path):
    """The -DSN_BF16X3=0 build of pointnet_mlp.hip / pointnet_mlp_backward.hip (conv GEMMs and fused conv backward on the exact fp32 MFMA) against the
    product build (fp32 products as six bf16 products of split operands) through the same C entry points: one 64 -> 128 layer
    forward and its fused backward at R = 4096 -- outputs within 1e-6 of the largest value, i.e. the split products are
    fp32-accurate against the hardware's own fp32 matrix path."""
    import ctypes

    from samplenet_amd._lib import LIB_PATH, bind
    from samplenet_amd.build import build_variant

    # the twin units with the product's flags (no compiler-packed fp32 arithmetic: this test runs on a GPU that others share), every
    # other unit as the product build has it
    so = build_variant("fp32", {"pointnet_mlp.hip": ["-DSN_BF16X3=0"], "pointnet_mlp_backward.hip": ["-DSN_BF16X3=0"]}, out_dir=str(tmp_path))
    libs = [bind(ctypes.CDLL(path), ("sn_linear_forward", "sn_conv_backward_partials", "sn_linear_wgrad_splits", "sn_linear_stats_blocks"))
            for path in (LIB_PATH, so)]
    g = torch.Generator(device="cuda").manual_seed(2)
    R, Ci, Co = 4096, 64, 128
    a = torch.randn(R, Ci, device="cuda", generator=g)
    coefp = torch.stack([torch.rand(Ci, device="cuda", generator=g) + 0.5, torch.randn(Ci, device="cuda", generator=g) * 0.1,
                         torch.zeros(Ci, device="cuda"), torch.ones(Ci, device="cuda")]).contiguous()
    W = torch.randn(Co, Ci, device="cuda", generator=g) * 0.1
    b = torch.randn(Co, device="cuda", generator=g)
    dy = torch.randn(R, Co, device="cuda", generator=g)
    kc = torch.stack([torch.rand(Co, device="cuda", generator=g) + 0.5, torch.randn(Co, device="cuda", generator=g) * 0.01,
                      torch.randn(Co, device="cuda", generator=g) * 0.01]).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for L in libs:
        z = torch.empty(R, Co, device="cuda")
        assert L.sn_linear_forward(R, Ci, Co, a.data_ptr(), coefp.data_ptr(), W.data_ptr(), b.data_ptr(), z.data_ptr(), None, st) == 0
        G = L.sn_linear_wgrad_splits(R, Ci, Co, 0)
        dyprev = torch.empty(R, Ci, device="cuda")
        stats = torch.empty(L.sn_linear_stats_blocks(R), 2, Ci, device="cuda")
        part = torch.zeros(G, Co, Ci, device="cuda")
        assert L.sn_conv_backward_partials(R, Ci, Co, 1, dy.data_ptr(), z.data_ptr(), kc.data_ptr(), None, None, 1, W.data_ptr(),
                                           a.data_ptr(), coefp.data_ptr(), dyprev.data_ptr(), stats.data_ptr(), part.data_ptr(), st) == 0
        torch.cuda.synchronize()
        outs.append((z, dyprev, part.sum(0)))
    for (x, y, name) in zip(outs[0], outs[1], ("z", "dYprev", "dW")):
        assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max()) * (8 if name == "dW" else 1), name


@pytest.mark.parametrize("B,N", [(32, 1024), (3, 160), (1, 1), (5, 777)])
def test_qrot_cloud_equals_the_reference_composition(B, N):
    """sn_qrot_forward / sn_qrot_backward (one launch each) against the reference's composition (src/quaternion.py:35-53: two
    cross products, scale, adds -- task_features.qrot, the form the PCRNet golden pins) with the quaternion expanded over the
    points: values, gradient to the points, gradient to the quaternion (a sum over the cloud), in fp32 against the same
    composition in fp64; quaternions NOT normalised (the formula is used as it stands)."""
    from samplenet_amd.task_features import qrot, qrot_cloud

    g = torch.Generator(device="cuda").manual_seed(B * 1000 + N)
    q = torch.randn(B, 4, device="cuda", generator=g).requires_grad_(True)
    v = (torch.rand(B, N, 3, device="cuda", generator=g) - 0.5).requires_grad_(True)
    go = torch.randn(B, N, 3, device="cuda", generator=g)
    out = qrot_cloud(q, v)
    gq, gv = torch.autograd.grad(out, [q, v], go)
    q64, v64 = q.detach().double().requires_grad_(True), v.detach().double().requires_grad_(True)
    ref = qrot(q64.unsqueeze(1).expand(-1, N, -1), v64)
    rq, rv = torch.autograd.grad(ref, [q64, v64], go.double())
    assert float((out.double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))
    assert float((gv.double() - rv).abs().max()) <= 2e-6 * max(1.0, float(rv.abs().max()))
    assert float((gq.double() - rq).abs().max()) <= 2e-6 * max(1.0, float(rq.abs().max())) * max(1, N) ** 0.5
    # data-only cloud (the registration loop: the template is data): no gradient tensor for it
    out2 = qrot_cloud(q, v.detach())
    (gq2,) = torch.autograd.grad(out2, [q], go)
    assert torch.equal(gq2, gq)


@pytest.mark.parametrize("B,N,bneck,grad_x", [(32, 64, 1024, True), (32, 1024, 1024, False), (3, 64, 256, True), (2, 128, 128, True),
                                              (4, 40, 64, True)])
def test_task_features_fused_maxpool_equals_the_layer_by_layer_route(B, N, bneck, grad_x):
    """PointNetFeatures (the registration task network's extractor): last layer + max over the points as one GEMM launch
    (sn_linear_forward_maxpool: per-cloud (max, first row) keys combined by atomicMax in the epilogue; without a gradient the
    (B N, bottleneck) activations are never written) against sn_linear_forward + sn_pool_forward: pooled features bit-identical
    (same GEMM, same maxima), gradients to the cloud and to the weights equal (the backward is the same kernels on the same
    selected rows; a channel that is negative everywhere may name another row, its gradient is masked either way)."""
    from samplenet_amd import task_features as TF

    torch.manual_seed(B * 31 + N)
    feat = TF.PointNetFeatures(bottleneck_size=bneck, input_shape="bnc").cuda()
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).requires_grad_(grad_x)
    go = torch.randn(B, bneck, device="cuda")
    res = {}
    old = TF.FUSE_MAXPOOL
    try:
        for tag, flag in (("fused", True), ("plain", False)):
            TF.FUSE_MAXPOOL = flag
            for trainable in (False, True):
                for p in feat.parameters():
                    p.requires_grad_(trainable)
                    p.grad = None
                if x.grad is not None:
                    x.grad = None
                if not trainable and not grad_x:
                    with torch.no_grad():
                        res[(tag, trainable)] = (feat(x), None, None)
                    continue
                y = feat(x)
                y.backward(go)
                res[(tag, trainable)] = (y.detach(), x.grad.clone() if grad_x else None,
                                         [p.grad.clone() for p in feat.parameters()] if trainable else None)
    finally:
        TF.FUSE_MAXPOOL = old
    for trainable in (False, True):
        yf, gxf, gpf = res[("fused", trainable)]
        yp, gxp, gpp = res[("plain", trainable)]
        assert torch.equal(yf, yp), trainable
        if gxf is not None:
            assert float((gxf - gxp).norm()) <= 1e-6 * float(gxp.norm()) + 1e-9, trainable
        if gpf is not None:
            for a, b in zip(gpf, gpp):
                assert float((a - b).norm()) <= 1e-6 * float(b.norm()) + 1e-9


@pytest.mark.parametrize("B,N,bneck", [(32, 64, 1024), (5, 64, 512), (3, 40, 1024), (2, 17, 64), (8, 128, 1024), (4, 256, 1024), (3, 200, 512)])
def test_task_features_sparse_pool_dgrad(B, N, bneck):
    """Frozen PointNetFeatures with at most 256 points per cloud (the sampled cloud of the registration step, the progressive
    sampler's prefixes): the last layer's data
    gradient from its one non-zero per cloud and channel (sn_pool_dgrad_sparse, pooling backward folded in, no (B N, bottleneck)
    activation tensor at all) against the dense DZ_POOL GEMM route and against torch in fp64; run to run bit-identical (fixed
    summation order: sixteen channel groups, each ascending, summed in group order)."""
    import torch.nn.functional as F

    from samplenet_amd import task_features as TF

    torch.manual_seed(B * 7 + N)
    feat = TF.PointNetFeatures(bottleneck_size=bneck, input_shape="bnc").cuda()
    for p in feat.parameters():
        p.requires_grad_(False)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).requires_grad_(True)
    go = torch.randn(B, bneck, device="cuda")
    assert TF.lib.sn_pool_dgrad_sparse_supported(B, N, 128, bneck)
    got = {}
    old = TF.SPARSE_POOL_DGRAD
    try:
        for tag, flag in (("sparse", True), ("sparse2", True), ("dense", False)):
            TF.SPARSE_POOL_DGRAD = flag
            y = feat(x)
            (got[tag],) = torch.autograd.grad(y, [x], go)
            got["y_" + tag] = y.detach()
    finally:
        TF.SPARSE_POOL_DGRAD = old
    assert torch.equal(got["y_sparse"], got["y_dense"])
    assert torch.equal(got["sparse"], got["sparse2"])
    xr = x.detach().double().requires_grad_(True)
    h = xr.permute(0, 2, 1)
    for conv in (feat.conv1, feat.conv2, feat.conv3, feat.conv4, feat.conv5):
        h = F.relu(F.conv1d(h, conv.weight.double(), conv.bias.double()))
    (want,) = torch.autograd.grad(torch.max(h, 2)[0], [xr], go.double())
    scale = float(want.abs().max())
    e_sparse = float((got["sparse"].double() - want).abs().max())
    e_dense = float((got["dense"].double() - want).abs().max())
    assert e_sparse <= 2e-5 * scale and e_sparse <= 2 * e_dense + 1e-6 * scale, (e_sparse, e_dense, scale)
    assert float((got["sparse"] - got["dense"]).norm()) <= 2e-5 * float(got["dense"].norm())


@pytest.mark.parametrize("B,N,bneck,cin", [(32, 1024, 1024, 128), (16, 1024, 512, 128), (128, 128, 1024, 128), (256, 64, 512, 128),
                                            (512, 32, 512, 128)])
def test_task_features_wide_maxpool_is_bit_identical(B, N, bneck, cin):
    """The wide last layer (sn_linear_forward_maxpool_wide: A fragments of 128 rows resident in registers for all columns, weights
    split once into bf16 planes) against the 64 x 64 tile kernel (sn_linear_forward_maxpool): same six bf16 products per 16 k in the
    same order, so pooled features, selected rows and pre-activations are EQUAL; the weight planes are re-split when the
    weights change in place (version counter) and when a new parameter object takes an old one's place."""
    from samplenet_amd import task_features as TF

    assert TF.lib.sn_linear_forward_maxpool_wide_supported(B * N, cin, bneck, N)
    torch.manual_seed(B + N)
    feat = TF.PointNetFeatures(bottleneck_size=bneck, input_shape="bnc").cuda()
    x = torch.rand(B, N, 3, device="cuda") - 0.5
    old = TF.WIDE_MAXPOOL
    try:
        out = {}
        for tag, flag in (("wide", True), ("tile", False)):
            TF.WIDE_MAXPOOL = flag
            with torch.no_grad():
                out[tag] = feat(x)
            xg = x.clone().requires_grad_(True)
            y = feat(xg)  # trainable weights: the activations are kept and read by the dense backward
            y.sum().backward()
            out[tag + "_y"], out[tag + "_gx"] = y.detach(), xg.grad.clone()
            out[tag + "_gw"] = feat.conv5.weight.grad.clone()
            feat.zero_grad(set_to_none=True)
        assert torch.equal(out["wide"], out["tile"]) and torch.equal(out["wide_y"], out["tile_y"])
        assert torch.equal(out["wide_gx"], out["tile_gx"]) and torch.equal(out["wide_gw"], out["tile_gw"])
        # in-place weight update -> new planes
        TF.WIDE_MAXPOOL = True
        with torch.no_grad():
            feat.conv5.weight.mul_(-0.5)
            y1 = feat(x)
            TF.WIDE_MAXPOOL = False
            y2 = feat(x)
        assert torch.equal(y1, y2) and not torch.equal(y1, out["wide"])
    finally:
        TF.WIDE_MAXPOOL = old


@pytest.mark.parametrize("R", [32, 5])
def test_skinny_linear_trunk_matches_torch(R):
    """PCRNet's frozen FC trunk on sn_skinny_linear (2048 -> 1024 -> 1024 -> 512 -> 512 -> 256 -> 7 on <= 32 rows: K-sliced weight stream,
    slices summed in order by the last workgroup to arrive) against torch.nn.Linear in fp64: output and the gradient to the input
    features within fp32 GEMM rounding, and bit-identical run to run."""
    from samplenet_amd import task_features as TF

    torch.manual_seed(R)
    net = TF.PCRNet(bottleneck_size=1024, input_shape="bnc").cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    y0 = torch.randn(R, 2048, device="cuda").requires_grad_(True)
    fcs = [net.fc1, net.fc2, net.fc3, net.fc4, net.fc5, net.fc6]
    wb = []
    for fc in fcs:
        wb += [fc.weight, fc.bias]
    go = torch.randn(R, 7, device="cuda")
    outs = []
    for _ in range(2):
        fa, fb = y0[:, :1024], y0[:, 1024:]  # the two clouds' feature vectors, as two tensors
        o = TF._TrunkFunction.apply(fa, fb, *wb)
        (gy,) = torch.autograd.grad(o, [y0], go)
        outs.append((o.detach(), gy))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    yr = y0.detach().double().requires_grad_(True)
    hcur = yr
    for i, fc in enumerate(fcs):
        hcur = torch.nn.functional.linear(hcur, fc.weight.double(), fc.bias.double())
        if i < 5:
            hcur = torch.relu(hcur)
    (gr,) = torch.autograd.grad(hcur, [yr], go.double())
    # torch fp32 for the yardstick
    h32 = y0.detach().clone().requires_grad_(True)
    t = h32
    for i, fc in enumerate(fcs):
        t = fc(t)
        if i < 5:
            t = torch.relu(t)
    (g32,) = torch.autograd.grad(t, [h32], go)
    eo, eo32 = float((outs[0][0].double() - hcur).abs().max()), float((t.double() - hcur).abs().max())
    eg, eg32 = float((outs[0][1].double() - gr).abs().max()), float((g32.double() - gr).abs().max())
    so, sg = float(hcur.abs().max()), float(gr.abs().max())
    assert eo <= max(2 * eo32, 2e-6 * so), (eo, eo32, so)
    assert eg <= max(2 * eg32, 2e-6 * sg), (eg, eg32, sg)


def test_pcrnet_head_and_chamfer_mean_loss_match_the_op_chain():
    """The registration task's loss pieces as fused launches against the torch op chain of registration/main.py:557-577 and
    models/pcrnet.py:78-82: twist = [normalize(y[:, :4]) | y[:, 4:]], qnorm = mean((||y[:, :4]||^2 - 1)^2) with gradients to y from
    both outputs; chamfer_mean_loss = mean(d1) + mean(d2) with gradients to both clouds (equal to the unfused Chamfer path, whose
    kernels it shares, up to the rounding of the mean's scaling)."""
    from samplenet_amd import task_features as TF
    from samplenet_amd.chamfer_distance import ChamferDistance
    from samplenet_amd.ops import chamfer_mean_loss

    torch.manual_seed(3)
    B = 32
    y = torch.randn(B, 7, device="cuda").requires_grad_(True)
    wt, wq = torch.randn(B, 7, device="cuda"), 0.7
    w4 = torch.randn(B, 4, device="cuda")
    twist, quat, qn = TF._HeadFunction.apply(y)
    assert torch.equal(quat, twist[:, 0:4])
    (gy,) = torch.autograd.grad((twist * wt).sum() + wq * qn + (quat * w4).sum(), [y])
    yr = y.detach().double().requires_grad_(True)
    pre = yr[:, 0:4]
    tr = torch.cat([torch.nn.functional.normalize(pre, dim=1), yr[:, 4:]], dim=1)
    qr = torch.mean((torch.sum(pre ** 2, dim=1) - 1) ** 2)
    (gr,) = torch.autograd.grad((tr * wt.double()).sum() + wq * qr + (tr[:, 0:4] * w4.double()).sum(), [yr])
    assert float((twist.double() - tr).abs().max()) <= 2e-7
    assert abs(float(qn) - float(qr)) <= 2e-6 * max(1.0, abs(float(qr)))
    assert float((gy.double() - gr).abs().max()) <= 5e-6 * max(1.0, float(gr.abs().max()))

    a = (torch.rand(B, 64, 3, device="cuda") - 0.5).requires_grad_(True)
    b = (torch.rand(B, 1024, 3, device="cuda") - 0.5).requires_grad_(True)
    loss = chamfer_mean_loss(a, b)
    ga, gb = torch.autograd.grad(loss, [a, b])
    d1, d2 = ChamferDistance()(a, b)
    ref = torch.mean(d1) + torch.mean(d2)
    ra, rb = torch.autograd.grad(ref, [a, b])
    assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref))
    assert float((ga - ra).abs().max()) <= 1e-6 * float(ra.abs().max()) and float((gb - rb).abs().max()) <= 1e-6 * float(rb.abs().max())


@pytest.mark.parametrize("B,N,vgrad", [(32, 1024, False), (32, 1024, True), (5, 300, True), (1, 7, False), (128, 64, False)])
def test_head_with_rotation_is_bit_identical_to_the_two_launches(B, N, vgrad):
    """sn_pcrnet_head_rot_* (PCRNet's output head AND the rotation of the template by the estimated quaternion as one launch each
    way: registration/main.py:563-571) against _HeadFunction + qrot_cloud: twist, quaternion, regulariser, rotated cloud and the
    gradients to y (through all four outputs) and to the cloud are EQUAL, bit for bit -- incl. a rotated cloud nobody differentiates
    and an unused twist."""
    from samplenet_amd import task_features as TF

    torch.manual_seed(B + N)
    y0 = torch.randn(B, 7, device="cuda")
    v0 = torch.rand(B, N, 3, device="cuda") - 0.5
    wt, w4, wo = torch.randn(B, 7, device="cuda"), torch.randn(B, 4, device="cuda"), torch.randn(B, N, 3, device="cuda")

    def run(fused, use):
        y = y0.clone().requires_grad_(True)
        v = v0.clone().requires_grad_(vgrad)
        if fused:
            twist, quat, qn, rot = TF._HeadRotFunction.apply(y, v)
        else:
            twist, quat, qn = TF._HeadFunction.apply(y)
            rot = TF.qrot_cloud(quat, v)
        loss = 0.0
        if "t" in use:
            loss = loss + (twist * wt).sum()
        if "q" in use:
            loss = loss + (quat * w4).sum()
        if "n" in use:
            loss = loss + 0.7 * qn
        if "r" in use:
            loss = loss + (rot * wo).sum()
        gs = torch.autograd.grad(loss, [y, v] if vgrad and "r" in use else [y])
        return (twist, quat, qn, rot) + tuple(gs)

    for use in ("tqnr", "nr", "r", "tn", "rq"):
        a, b = run(True, use), run(False, use)
        assert len(a) == len(b)
        for i, (u, w) in enumerate(zip(a, b)):
            assert torch.equal(u, w), (use, i, float((u - w).abs().max()))


@pytest.mark.parametrize("B,N,grad", [(32, 1024, False), (32, 64, True), (3, 64, True), (5, 192, True), (3, 50, True), (2, 1024, True)])
def test_task_features_narrow_front_is_bit_identical(B, N, grad):
    """conv1..conv4 of PointNetFeatures as one launch (sn_pointnet_narrow_forward: a wave takes 32 rows through 3 -> 64 -> 64 -> 64 -> 128,
    activations stay in registers / LDS) against the four layer launches: same products in the same order, so the pooled features
    and -- through identical saved pre-activations -- every gradient are EQUAL (row counts that are not whole 64-row tiles keep the
    layer-by-layer route)."""
    from samplenet_amd import task_features as TF

    assert bool(TF.lib.sn_pointnet_narrow_forward_supported(B * N, 64, 64, 64, 128)) == ((B * N) % 64 == 0)
    torch.manual_seed(B * 13 + N)
    feat = TF.PointNetFeatures(bottleneck_size=1024, input_shape="bnc").cuda()
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).requires_grad_(grad)
    go = torch.randn(B, 1024, device="cuda")
    old = TF.FUSE_NARROW
    res = {}
    try:
        for flag in (True, False):
            TF.FUSE_NARROW = flag
            if not grad:
                for p in feat.parameters():
                    p.requires_grad_(False)
                with torch.no_grad():
                    res[flag] = (feat(x),)
                continue
            y = feat(x)
            gs = torch.autograd.grad(y, [x] + list(feat.parameters()), go)
            res[flag] = (y.detach(),) + tuple(gs)
    finally:
        TF.FUSE_NARROW = old
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_pcrnet_shared_template_features():
    """Several task evaluations against ONE template within a step (the progressive sampler's prefixes): the template's extractor
    pass computed once (PCRNet.template_features) and handed to pcrnet_chamfer_loss gives the same losses and the same gradients to
    the sampled clouds as recomputing it per evaluation."""
    from samplenet_amd.task_features import PCRNet, pcrnet_chamfer_loss

    torch.manual_seed(1)
    pcr = PCRNet(bottleneck_size=1024, input_shape="bnc").cuda().eval()
    for p in pcr.parameters():
        p.requires_grad_(False)
    template = torch.rand(8, 1024, 3, device="cuda") - 0.5
    qs = [(torch.rand(8, m, 3, device="cuda") - 0.5).requires_grad_(True) for m in (32, 64, 128)]
    plain = sum(pcrnet_chamfer_loss(pcr, template, q)[0] for q in qs)
    gp = torch.autograd.grad(plain, qs)
    f0 = pcr.template_features(template)
    shared = sum(pcrnet_chamfer_loss(pcr, template, q, template_features=f0)[0] for q in qs)
    gs = torch.autograd.grad(shared, qs)
    assert torch.equal(plain, shared)
    for a, b in zip(gp, gs):
        assert torch.equal(a, b)
    # ... and with the FC trunk run ONCE on all evaluations' rows (3 x 8 = 24 -> one row tile; the K-slice sums see the same operands
    # in the same order, so nothing changes), then on 3 x 32 = 96 rows (three row tiles per workgroup)
    from samplenet_amd.task_features import pcrnet_chamfer_loss_multi

    multi = sum(t for t, _, _ in pcrnet_chamfer_loss_multi(pcr, template, qs, template_features=f0))
    gm = torch.autograd.grad(multi, qs)
    assert torch.equal(plain, multi)
    for a, b in zip(gp, gm):
        assert torch.equal(a, b)
    t32 = torch.rand(32, 1024, 3, device="cuda") - 0.5
    q32 = [(torch.rand(32, m, 3, device="cuda") - 0.5).requires_grad_(True) for m in (32, 64, 128)]
    one = [pcrnet_chamfer_loss(pcr, t32, q) for q in q32]
    many = pcrnet_chamfer_loss_multi(pcr, t32, q32)
    for (la, qa, ta), (lb, qb, tb) in zip(one, many):
        assert torch.equal(la, lb) and torch.equal(qa, qb) and torch.equal(ta, tb)
    ga = torch.autograd.grad(sum(l for l, _, _ in one), q32)
    gb = torch.autograd.grad(sum(l for l, _, _ in many), q32)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


def test_cyclic_pad_cat_and_the_one_pass_extractor():
    """ops.cyclic_pad_cat (sn_cyclic_pad_cat / _backward) against torch indexing, and what it is for: PCRNet's extractor (per-point
    layers without BatchNorm + a maximum over the points, registration/models/pcrnet.py:23-46) on the progressive sampler's four
    prefixes as ONE batch of 128 clouds x 256 points gives every prefix's features and the gradient to every prefix EQUAL, bit for
    bit, to its own pass (BASELINE configs[4]'s shape: the padded batch runs the wide pooled layer, the single passes the tile kernel)."""
    from samplenet_amd import ops
    from samplenet_amd import task_features as TF

    g = torch.Generator(device="cuda").manual_seed(12)
    B, sizes = 5, [3, 7, 8, 20]
    cl = [torch.randn(B, s, 3, device="cuda", generator=g).requires_grad_(s != 7) for s in sizes]
    out = ops.cyclic_pad_cat(cl)
    P = max(sizes)
    ref = torch.cat([c[:, torch.arange(P, device="cuda") % c.shape[1], :] for c in cl], dim=0)
    assert out.shape == (len(sizes) * B, P, 3) and torch.equal(out, ref)
    w = torch.randn_like(out)
    need = [c for c in cl if c.requires_grad]
    ga = torch.autograd.grad((out * w).sum(), need)
    gb = torch.autograd.grad((ref * w).sum(), need)
    for a, b in zip(ga, gb):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6)

    torch.manual_seed(4)
    pcr = TF.PCRNet(bottleneck_size=1024, input_shape="bnc").cuda().eval()
    for p in pcr.parameters():
        p.requires_grad_(False)
    B, sizes = 32, [32, 64, 128, 256]
    cloud = torch.rand(B, 256, 3, device="cuda", generator=g) - 0.5
    qs = [cloud[:, :s, :].contiguous().requires_grad_(True) for s in sizes]
    f_multi = pcr._feat_multi(qs)
    f_single = torch.cat([pcr.feat(q) for q in qs], dim=0)
    assert torch.equal(f_multi, f_single)
    wf = torch.randn_like(f_multi)
    gm = torch.autograd.grad((f_multi * wf).sum(), qs)
    gs = torch.autograd.grad((f_single * wf).sum(), qs)
    for a, b in zip(gm, gs):
        assert torch.equal(a, b)
    # ... and the whole task term of the four evaluations as ONE batch (extractor, trunk, grouped head + rotation, grouped Chamfer term:
    # the copies left out of the loss) against evaluation by evaluation: losses, regularisers, twists and the gradient to every prefix
    template = torch.rand(B, 1024, 3, device="cuda", generator=g) - 0.5
    assert pcr._one_batch_ok(template, qs)
    many = TF.pcrnet_chamfer_loss_multi(pcr, template, qs)
    one = [TF.pcrnet_chamfer_loss(pcr, template, q) for q in qs]
    for (la, qa, ta), (lb, qb, tb) in zip(one, many):
        assert torch.equal(la, lb) and torch.equal(qa, qb) and torch.equal(ta, tb)
    wl = [0.3, 1.0, 0.7, 1.9]
    ga = torch.autograd.grad(sum(w * (l + 0.1 * q) for w, (l, q, _) in zip(wl, one)), qs)
    gb = torch.autograd.grad(sum(w * (l + 0.1 * q) for w, (l, q, _) in zip(wl, many)), qs)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N", [(32, 64), (4, 256), (3, 50), (2, 1024)])
def test_task_features_narrow_backward(B, N):
    """Frozen PointNetFeatures: the data gradient through conv4..conv1 as one launch (sn_pointnet_narrow_backward, split-bf16 MFMAs
    against transposed weight planes) against the four layer launches (fp32 MFMA) and against torch in fp64; bit-identical run to run."""
    import torch.nn.functional as F

    from samplenet_amd import task_features as TF

    torch.manual_seed(B * 3 + N)
    feat = TF.PointNetFeatures(bottleneck_size=1024, input_shape="bnc").cuda()
    for p in feat.parameters():
        p.requires_grad_(False)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).requires_grad_(True)
    go = torch.randn(B, 1024, device="cuda")
    old = TF.FUSE_NARROW
    got = {}
    try:
        for tag, flag in (("fused", True), ("fused2", True), ("layers", False)):
            TF.FUSE_NARROW = flag
            (got[tag],) = torch.autograd.grad(feat(x), [x], go)
    finally:
        TF.FUSE_NARROW = old
    assert torch.equal(got["fused"], got["fused2"])
    xr = x.detach().double().requires_grad_(True)
    hcur = xr.permute(0, 2, 1)
    for conv in (feat.conv1, feat.conv2, feat.conv3, feat.conv4, feat.conv5):
        hcur = F.relu(F.conv1d(hcur, conv.weight.double(), conv.bias.double()))
    (want,) = torch.autograd.grad(torch.max(hcur, 2)[0], [xr], go.double())
    scale = float(want.abs().max())
    ef = float((got["fused"].double() - want).abs().max())
    el = float((got["layers"].double() - want).abs().max())
    assert ef <= max(2 * el, 2e-6 * scale), (ef, el, scale)


@pytest.mark.parametrize("Ci,Co,R,mode", [(128, 256, 4096, "bn"), (128, 256, 2090, "bn"), (256, 128, 4096, "bn"), (256, 128, 2090, "bn"),
                                         (256, 128, 2560, "pool")])
def test_fused_conv_backward_two_passes_for_256_channels(Ci, Co, R, mode):
    """The reconstruction sampler's 128 -> 256 -> 128 layers (reconstruction/src/samplers.py:23): a 256-channel side runs as two passes
    of the fused 128 x 128 backward kernel (output-channel halves: raw partial data gradient + second pass that adds it; input-channel
    halves: independent) -- sn_linear_backward's dYprev, dW and the (sum dYprev, sum dYprev Zprev) partials against fp64, ragged row
    counts and the pooled form included."""
    from samplenet_amd._lib import check, lib, ptr

    torch.manual_seed(Ci + R)
    dev = "cuda"
    z = torch.randn(R, Co, device=dev)
    zprev = torch.randn(R, Ci, device=dev)
    W = torch.randn(Co, Ci, device=dev) * 0.1
    kcoef = torch.randn(3, Co, device=dev) * torch.tensor([[1.0], [0.05], [0.01]], device=dev)
    coef_prev = torch.zeros(4, Ci, device=dev)
    coef_prev[0] = torch.rand(Ci, device=dev) + 0.5
    coef_prev[1] = torch.randn(Ci, device=dev) * 0.3
    npts = 320
    if mode == "pool":
        B = R // npts
        gsel = torch.randn(B, Co, device=dev)
        argsel = torch.randint(0, npts, (B, Co), device=dev, dtype=torch.int32)
        dy = None
        d = torch.zeros(B, npts, Co, device=dev, dtype=torch.float64)
        d.scatter_(1, argsel.long().unsqueeze(1), gsel.double().unsqueeze(1))
        d = d.reshape(R, Co)
        zmode = 2
    else:
        dy = torch.randn(R, Co, device=dev)
        gsel = argsel = None
        d = dy.double()
        zmode = 1
    dyprev = torch.empty(R, Ci, device=dev)
    nblk = lib.sn_linear_stats_blocks(R)
    stats = torch.zeros(nblk, 2, Ci, device=dev)
    part = torch.empty(lib.sn_linear_wgrad_splits(R, Ci, Co, 0) * Co * Ci, device=dev)
    dW = torch.empty(Co, Ci, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    check(lib.sn_linear_backward(R, Ci, Co, zmode, ptr(dy), ptr(z), ptr(kcoef), ptr(gsel), ptr(argsel), npts, ptr(W), ptr(zprev),
                                 ptr(coef_prev), ptr(dyprev), ptr(stats), ptr(part), ptr(dW), st), "sn_linear_backward")
    k = kcoef.double()
    dz = k[0] * d + k[1] * z.double() + k[2]
    pre = coef_prev[0].double() * zprev.double() + coef_prev[1].double()
    want_dy = (dz @ W.double()) * (pre > 0)
    want_dw = dz.t() @ torch.relu(pre)
    s = float(want_dy.abs().max())
    assert float((dyprev.double() - want_dy).abs().max()) <= 2e-6 * s * (Co ** 0.5)
    assert float((dW.double() - want_dw).abs().max()) <= 2e-6 * float(want_dw.abs().max()) * (R ** 0.5) / 8
    got = stats.double().sum(0)
    want_s = torch.stack([want_dy.sum(0), (want_dy * zprev.double()).sum(0)])
    assert float((got - want_s).abs().max()) <= 1e-4 * float(want_s.abs().max())


@pytest.mark.parametrize("B,N,blocks", [(256, 1024, 8), (128, 1024, 2), (96, 320, 4), (40, 1024, 3)])
def test_xyz_layer_statistics_do_not_depend_on_the_block_grouping(B, N, blocks):
    """Large batches: a workgroup of the xyz layer's statistics pass walks several 64-row blocks and issues ONE pair of atomics per
    channel (1 M atomics on 2 K addresses paced the kernel at 512 x 1024 points).  Every block's float partial is converted to fixed
    point on its own, so the integer totals -- hence every coefficient, activation and running statistic of the stack -- are the same
    bit for bit whatever the grouping (also a grouping that leaves the last workgroup short)."""
    import copy

    from samplenet_amd import SampleNet, pointnet
    from samplenet_amd._lib import lib

    torch.manual_seed(B + N + blocks)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    net_b = copy.deepcopy(net_a)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).contiguous()
    old = lib.sn_conv_stack_set_in3_blocks(blocks)
    try:
        ya, sa = pointnet.forward_impl(net_a, x, True, use_plan=False)
        assert _acc_sums_zero(net_a._fx_acc)
        lib.sn_conv_stack_set_in3_blocks(1)
        yb, sb = pointnet.forward_impl(net_b, x, True, use_plan=False)
    finally:
        lib.sn_conv_stack_set_in3_blocks(old)
    for l in range(5):
        assert torch.equal(sa["cc"][l], sb["cc"][l]), l
    assert torch.equal(sa["pooled"], sb["pooled"]) and torch.equal(ya, yb)
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        assert torch.equal(ba, bb), n


@pytest.mark.parametrize("B,N", [(256, 1024), (160, 2048), (300, 512)])
def test_persistent_forward_is_bit_identical(B, N):
    """Large batches run the conv stack's GEMM layers as persistent, weight-stationary kernels (linear_fwd_persist_kernel: one
    workgroup per CU walks over its tiles, B fragments in registers, the next tile's activations in flight, one set of statistics
    atomics per workgroup).  Same products in the same order, integer statistics: every pre-activation, every BatchNorm
    coefficient, the pooled features with their selected rows, the head's output and the running statistics are BIT-identical
    to the one-workgroup-per-tile kernels; the accumulators are left zero."""
    import copy

    from samplenet_amd import SampleNet, pointnet
    from samplenet_amd._lib import lib

    torch.manual_seed(B + N)
    net_a = SampleNet(64, 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().train()
    with torch.no_grad():
        net_a.bn2.weight[::3] *= -1.0  # negative scales: the pool picks the minimum there
        net_a.bn5.weight[::5] *= -1.0
    net_b = copy.deepcopy(net_a)
    x = (torch.rand(B, N, 3, device="cuda") - 0.5).contiguous()
    old = lib.sn_conv_stack_set_persist_min_tiles(1)
    try:
        ya, sa = pointnet.forward_impl(net_a, x, True, use_plan=False)
        assert _acc_sums_zero(net_a._fx_acc)
        ya2, sa2 = pointnet.forward_impl(net_a, x, True, use_plan=False)  # (a second step: accumulators were left clean)
        lib.sn_conv_stack_set_persist_min_tiles(0)
        yb, sb = pointnet.forward_impl(net_b, x, True, use_plan=False)
        pointnet.forward_impl(net_b, x, True, use_plan=False)
    finally:
        lib.sn_conv_stack_set_persist_min_tiles(old)
    for l in range(5):
        assert torch.equal(sa["cc"][l], sb["cc"][l]), l
        if sa["zc"][l] is not None:
            assert torch.equal(sa["zc"][l], sb["zc"][l]), l
            assert torch.equal(sa2["zc"][l], sa["zc"][l]), l
    for k in ("pooled", "argsel", "zsel"):
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(ya, yb)
    for (n, ba), (_, bb) in zip(net_a.named_buffers(), net_b.named_buffers()):
        assert torch.equal(ba, bb), n


@pytest.mark.parametrize("bneck", [100, 36])
def test_pcrnet_trunk_with_a_bottleneck_that_is_not_a_multiple_of_eight(bneck):
    """until round 5 such widths fell back to torch.nn.Linear (rocBLAS).  Now the two clouds' feature vectors are
    re-cut at a multiple of 8 columns and the trunk stays on sn_skinny_linear: against the torch composition in fp64 -- twist,
    the gradient to the source cloud -- and the library's trunk function is what ran."""
    from samplenet_amd import task_features as tf

    torch.manual_seed(bneck)
    net = tf.PCRNet(bottleneck_size=bneck, input_shape="bnc").cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    p0 = torch.rand(6, 128, 3, device="cuda") - 0.5
    q = (torch.rand(6, 64, 3, device="cuda") - 0.5).requires_grad_(True)
    calls = []
    orig = tf._TrunkFunction.apply
    try:
        tf._TrunkFunction.apply = staticmethod(lambda *a: (calls.append(a[0].shape), orig(*a))[1])
        twist, pre = net(p0, q)
    finally:
        tf._TrunkFunction.apply = orig
    assert len(calls) == 1 and calls[0][1] % 8 == 0
    gw = torch.randn(6, 7, device="cuda")
    (gq,) = torch.autograd.grad((twist * gw).sum(), [q])
    ref = copy.deepcopy(net).double()
    q64 = q.detach().double().requires_grad_(True)
    f0, f1 = net.feat(p0).double(), None
    # fp64 trunk on the library's fp32 features of the template and an fp64 recomputation through the source cloud's features
    f1 = net.feat(q)
    y = torch.cat([f0, f1.double()], dim=1)
    for fc in (ref.fc1, ref.fc2, ref.fc3, ref.fc4, ref.fc5):
        y = torch.relu(fc(y))
    y = ref.fc6(y)
    tr = torch.cat([torch.nn.functional.normalize(y[:, 0:4], dim=1), y[:, 4:]], dim=1)
    (gr,) = torch.autograd.grad((tr * gw.double()).sum(), [q])
    assert float((twist.double() - tr).abs().max()) <= 1e-5
    assert float((gq.double() - gr.double()).norm()) <= 1e-4 * float(gr.double().norm())


@pytest.mark.parametrize("B", [32, 5, 100, 200, 300])
def test_trainable_pcrnet_trunk_stays_on_the_library(B):
    """registration/models/pcrnet.py:62-82 under main.py --train-pcrnet: with a TRAINABLE FC trunk the six layers still run on
    sn_skinny_linear (forward, data gradient) and their weight / bias gradients on sn_skinny_wgrad -- against the torch.nn.Linear
    composition (rocBLAS; spelled out HERE, the product has no such route) on the same weights: twist 1e-5, every gradient of the trunk and the gradient that reaches both clouds within
    1e-4 of its norm; deterministic from run to run.  Above 128 rows the trunk runs in row blocks of 128 (no
    torch.nn.Linear / rocBLAS on the GPU path at any batch)."""
    import copy

    from samplenet_amd import task_features as tf

    if B > 128:  # the route must be the library's, not a silent torch fallback
        calls = []
        orig = tf._TrunkFunction.apply
        try:
            tf._TrunkFunction.apply = staticmethod(lambda *a: (calls.append(a[0].shape[0]), orig(*a))[1])
            m = tf.PCRNet(bottleneck_size=1024, input_shape="bnc").cuda().eval()
            with torch.no_grad():
                m(torch.rand(B, 64, 3, device="cuda"), torch.rand(B, 64, 3, device="cuda"))
        finally:
            tf._TrunkFunction.apply = orig
        assert sum(calls) == B and max(calls) <= 128 and len(calls) == (B + 127) // 128, calls
    torch.manual_seed(B)
    net = tf.PCRNet(bottleneck_size=1024, input_shape="bnc").cuda().train()
    for p in net.feat.parameters():
        p.requires_grad_(False)
    ref = copy.deepcopy(net)
    p0 = torch.rand(B, 256, 3, device="cuda") - 0.5
    q = torch.rand(B, 64, 3, device="cuda") - 0.5
    gw = torch.randn(B, 7, device="cuda")
    def torch_route(model, p0, qq):
        # the reference composition (models/pcrnet.py:62-82) on torch.nn ops behind the library's feature extractor
        y = torch.cat([model.feat(p0), model.feat(qq)], dim=1)
        for fc in (model.fc1, model.fc2, model.fc3, model.fc4, model.fc5):
            y = torch.relu(fc(y))
        y = model.fc6(y)
        pre = y[:, 0:4]
        return torch.cat([torch.nn.functional.normalize(pre, dim=1), y[:, 4:]], dim=1), pre

    outs = []
    for model, fused in ((net, True), (ref, False), (net, True)):
        for p in model.parameters():
            p.grad = None
        qq = q.clone().requires_grad_(True)
        twist, pre = model(p0, qq) if fused else torch_route(model, p0, qq)
        ((twist * gw).sum() + (pre * pre).sum()).backward()
        outs.append((twist.detach().clone(), qq.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    (ta, ga, wa), (tb, gb, wb), (tc, gc, wc) = outs
    assert len(wa) == 12 and set(wa) == set(wb)
    assert float((ta - tb).abs().max()) <= 1e-5 * max(1.0, float(tb.abs().max()))
    assert float((ga - gb).norm()) <= 1e-4 * float(gb.norm())
    for n in wa:
        assert float((wa[n] - wb[n]).norm()) <= 1e-4 * float(wb[n].norm()) + 1e-9, n
        assert torch.equal(wa[n], wc[n]), n
    assert torch.equal(ta, tc) and torch.equal(ga, gc)

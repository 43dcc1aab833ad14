"""The conv stack's bulk stores leave through buffer stores with a compile-time cache policy (mlp_device.h: SN_ST_Z forward Z tiles,
SN_ST_DY backward dYprev tiles, SN_ST_PART the weight-gradient / statistics partials).  A policy may change when bytes travel, never
which bytes: the conv stack is driven through the C ABI at the smallest shapes at which a store family can go wrong -- one tile per
workgroup (every dYprev store is the tail store), several tiles per workgroup at both tile heights (store_prev at the top of an
iteration), the two-pass 256-channel kernels (a raw dYprev stored by one launch and read back in place by the next), a ragged row
count, and the partial-tile forward the policy must leave alone -- against the fp64 torch twin of tests/torch_mlp.py, at the
tolerances tests/test_gpu_mlp.py uses for the same entry points.  Every backward runs twice on the same inputs and must return the
same bits: a store still in flight when its reader starts shows up as run-to-run differences."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from torch_mlp import rel as _rel, torch_mlp_copy

pytestmark = pytest.mark.gpu

CHANNELS = (3, 64, 64, 64, 128, 128)


def _arr(ts):
    from samplenet_amd._lib import ptr

    return (ctypes.c_void_p * len(ts))(*[ptr(t) for t in ts])


def _twin_stack(ref64, x_bcn):
    """conv/bn/relu x 5 of the fp64 twin's own modules (TorchMLPSampleNet._features up to the pool): pre-BN outputs, last activation."""
    zs, y = [], x_bcn
    for i in range(1, 6):
        z = getattr(ref64, "conv%d" % i)(y)
        zs.append(z)
        y = F.relu(getattr(ref64, "bn%d" % i)(z))
    return zs, y


@pytest.mark.parametrize("B,N,z1", [(2, 128, "stored"), (3, 192, "stored"), (2, 1024, "rebuilt")])
def test_conv_stack_forward_backward_vs_fp64(B, N, z1):
    """sn_conv_stack_forward_bn + sn_conv_stack_backward, channels 3-64-64-64-128-128.
    R = 256 is the fused backward's floor: four workgroups, one 64-row tile each on the 64-channel layers (every dYprev store is the
    tail store, every workgroup writes a partial), two 32-row tiles each on the 128-channel layers.  R = 576: 9 tiles of 64 rows and 18
    of 32 over 9 workgroups -- on the 32-row layers every workgroup stores a tile at the top of its second iteration.
    z1: the xyz layer's activation stored by the xyz kernel (the only route below 2048 rows), or rebuilt from the cloud by conv2 -- the
    training step's route, whose forward and backward kernels above the xyz layer are other instantiations; R = 2048 is its floor
    (sn_conv_stack_z1_free_supported: the first launch's row blocks must carry the weight split): 32 workgroups, one 64-row tile each.
    Bars: every pre-BN activation and the pooled features within 2e-4 of the fp64 twin (Frobenius; the suite's bar for an fp32 run of
    this stack against fp64, torch_mlp.fp64_floor), every gradient within 2e-4 of its norm + 1e-6 of the largest gradient norm
    (test_conv_stack_one_call_backward's noise floor); the biases in front of a BatchNorm, whose true gradient is 0, within 1e-3 of
    their weight's gradient norm (test_mlp_forward_backward_vs_torch).  The backward's inputs at the top (pooled gradient at the
    selected points, the top BatchNorm's dZ coefficients) are computed in fp64 from the twin, at the points the forward selected."""
    from samplenet_amd import SampleNet
    from samplenet_amd._lib import check, lib, ptr

    torch.manual_seed(17 * B + N)
    dev = "cuda"
    net = SampleNet(16, 128, group_size=4, input_shape="bnc", output_shape="bnc").to(dev).train()
    with torch.no_grad():
        for n_, p in net.named_parameters():
            if n_.startswith("bn") and "fc" not in n_:
                p.add_(0.2 * torch.randn_like(p))
        net.bn3.weight[::4] *= -1.0
    ref64 = torch_mlp_copy(net).double().train()
    n = 5
    R = B * N
    chans = (ctypes.c_int * (n + 1))(*CHANNELS)
    assert lib.sn_conv_stack_forward_supported(B, N, n, chans)
    nscr = lib.sn_conv_stack_backward_scratch_floats(B, N, n, chans)
    assert nscr > 0
    convs = [getattr(net, "conv%d" % i) for i in range(1, 6)]
    bns = [getattr(net, "bn%d" % i) for i in range(1, 6)]
    x = torch.rand(B, N, 3, device=dev) - 0.5
    st = torch.cuda.current_stream().cuda_stream

    # ---- forward
    zs = [torch.empty(R, c, device=dev) for c in CHANNELS[1:]]
    if z1 == "rebuilt":
        assert lib.sn_conv_stack_z1_free_supported(B, N, n, chans)
        zs[0] = None
    cs = [torch.empty(4, c, device=dev) for c in CHANNELS[1:]]
    acc_f = torch.zeros(lib.sn_conv_stack_acc_elems(n), device=dev, dtype=torch.int64)
    nblk = lib.sn_linear_stats_blocks(R)
    Cn = CHANNELS[-1]
    pool_val = torch.empty(nblk, 2, Cn, device=dev)
    pool_idx = torch.empty(nblk, 2, Cn, device=dev, dtype=torch.int32)
    pooled, argsel, zsel = torch.empty(B, Cn, device=dev), torch.empty(B, Cn, device=dev, dtype=torch.int32), torch.empty(B, Cn, device=dev)
    rm = [b.running_mean.clone() for b in bns]
    rv = [b.running_var.clone() for b in bns]
    nbt = [b.num_batches_tracked.clone() for b in bns]
    eps = (ctypes.c_float * n)(*[float(b.eps) for b in bns])
    mom = (ctypes.c_float * n)(*[float(b.momentum) for b in bns])
    check(lib.sn_conv_stack_forward_bn(B, N, n, chans, ptr(x), _arr([c.weight for c in convs]), _arr([c.bias for c in convs]),
                                       _arr([b.weight for b in bns]), _arr([b.bias for b in bns]), _arr(rm), _arr(rv), _arr(nbt), eps, mom,
                                       _arr(zs), _arr(cs), ptr(acc_f), ptr(pool_val), ptr(pool_idx), ptr(pooled), ptr(argsel), ptr(zsel), st),
          "sn_conv_stack_forward_bn")
    torch.cuda.synchronize()

    x64 = x.double().permute(0, 2, 1)
    zt, yt = _twin_stack(ref64, x64)  # (B, C, N)
    for l in range(n):
        if zs[l] is None:
            continue
        want = zt[l].permute(0, 2, 1).reshape(R, -1)
        e = _rel(zs[l], want)
        print("forward z%d rel %.3g" % (l + 1, e))
        assert e <= 2e-4, (l, e)
    idx = argsel.long().unsqueeze(2)
    assert int(argsel.min()) >= 0 and int(argsel.max()) < N
    picked = yt.gather(2, idx).squeeze(2)  # the twin's activation at the points the forward selected
    e = _rel(pooled, yt.max(dim=2).values)
    print("pooled rel %.3g" % e)
    assert e <= 2e-4, e
    assert float((picked - yt.max(dim=2).values).detach().abs().max()) <= 1e-5 * float(yt.detach().abs().max())

    # ---- the backward's inputs at the top, from the twin in fp64
    g = torch.randn(B, Cn, device=dev)
    (picked * g.double()).sum().backward()
    gsel64 = g.double() * (picked.detach() > 0)
    z5 = zt[-1].detach()
    mean, var = z5.mean(dim=(0, 2)), z5.var(dim=(0, 2), unbiased=False)
    invstd = (var + bns[-1].eps).rsqrt()
    scale = ref64.bn5.weight.detach() * invstd
    s = gsel64.sum(0)
    dgam = invstd * (gsel64 * (z5.gather(2, idx).squeeze(2) - mean)).sum(0)
    kcoef_top = torch.stack([scale, -scale * invstd * dgam / R, scale * (invstd * mean * dgam / R - s / R)]).float().contiguous()
    gsel = gsel64.float().contiguous()

    # ---- backward, twice
    def backward():
        acc_b = torch.zeros(lib.sn_conv_stack_acc_elems(n), device=dev, dtype=torch.int64)
        scratch = torch.empty(nscr, device=dev)
        dW = [torch.full_like(c.weight, float("nan")) for c in convs]
        dg = [torch.full_like(b.weight, float("nan")) for b in bns[:-1]]
        db = [torch.full_like(b.bias, float("nan")) for b in bns[:-1]]
        dbias = [torch.full_like(c.bias, float("nan")) for c in convs[:-1]]
        check(lib.sn_conv_stack_backward(B, N, n, chans, ptr(x), _arr([c.weight for c in convs]), ptr(convs[0].bias), _arr(zs), _arr(cs),
                                         ptr(gsel), ptr(argsel), ptr(kcoef_top), ptr(acc_b), ptr(scratch), _arr(dW), _arr(dg + [None]),
                                         _arr(db + [None]), _arr(dbias + [None]), None, st), "sn_conv_stack_backward")
        torch.cuda.synchronize()
        return dW, dg, db, dbias

    first, second = backward(), backward()
    for a, b in zip(sum(first, []), sum(second, [])):
        assert torch.equal(a, b)  # (NaN would fail too: every output is written)
    dW, dg, db, dbias = first
    want = {}
    for i in range(n):
        want["conv%d.weight" % (i + 1)] = (dW[i], getattr(ref64, "conv%d" % (i + 1)).weight.grad)
    for i in range(n - 1):
        want["bn%d.weight" % (i + 1)] = (dg[i], getattr(ref64, "bn%d" % (i + 1)).weight.grad)
        want["bn%d.bias" % (i + 1)] = (db[i], getattr(ref64, "bn%d" % (i + 1)).bias.grad)
    gmax = max(float(w.norm()) for _, w in want.values())
    for name, (got, w) in want.items():
        err, nrm = float((got.double() - w).norm()), float(w.norm())
        print("%s err %.3g of %.3g" % (name, err, nrm))
        assert err <= 2e-4 * nrm + 1e-6 * gmax, (name, err, nrm)
    for i in range(n - 1):
        wn = float(getattr(ref64, "conv%d" % (i + 1)).weight.grad.norm())
        assert float(dbias[i].double().norm()) <= 1e-3 * wn + 1e-6, i


@pytest.mark.parametrize("R", [288, 300])
def test_256_channel_layer_pair_backward(R):
    """128 -> 256 -> 128 through sn_linear_backward, top layer first, the lower layer fed with the dYprev the upper one stored.
    A 256-channel side runs as two launches of the 128 x 128 kernel on 32-row tiles: 256 inputs -- independent column halves of
    dYprev; 256 outputs -- the first launch stores a raw dYprev (DM = 1), the second reads it back in place, adds its half and stores
    the result (DM = 2).  R = 288: 9 full tiles over 5 workgroups (one or two tiles each); R = 300: a ragged last tile, so the
    masked instantiation (FULLR = false) runs and the rows past R are dropped by the buffer's bound.
    Bars as in test_fused_conv_backward_two_passes_for_256_channels: dYprev within 2e-6 sqrt(Co) of its largest entry, dW within
    2e-6 sqrt(R) / 8 of its largest entry, the statistics partials' sums within 1e-4."""
    from samplenet_amd._lib import check, lib, ptr

    torch.manual_seed(R)
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream

    def layer(Ci, Co, dy):
        z = torch.randn(R, Co, device=dev)
        zprev = torch.randn(R, Ci, device=dev)
        W = torch.randn(Co, Ci, device=dev) * 0.1
        kcoef = torch.randn(3, Co, device=dev) * torch.tensor([[1.0], [0.05], [0.01]], device=dev)
        coef_prev = torch.zeros(4, Ci, device=dev)
        coef_prev[0] = torch.rand(Ci, device=dev) + 0.5
        coef_prev[1] = torch.randn(Ci, device=dev) * 0.3
        nblk = lib.sn_linear_stats_blocks(R)
        nsplit = lib.sn_linear_wgrad_splits(R, Ci, Co, 0)
        runs = []
        for _ in range(2):
            dyprev = torch.full((R, Ci), float("nan"), device=dev)
            stats = torch.zeros(nblk, 2, Ci, device=dev)
            part = torch.empty(nsplit * Co * Ci, device=dev)
            dW = torch.full((Co, Ci), float("nan"), device=dev)
            check(lib.sn_linear_backward(R, Ci, Co, 1, ptr(dy), ptr(z), ptr(kcoef), None, None, 0, ptr(W), ptr(zprev), ptr(coef_prev),
                                         ptr(dyprev), ptr(stats), ptr(part), ptr(dW), st), "sn_linear_backward")
            torch.cuda.synchronize()
            runs.append((dyprev, dW, stats))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        dyprev, dW, stats = runs[0]
        k = kcoef.double()
        dz = k[0] * dy.double() + k[1] * z.double() + k[2]
        pre = coef_prev[0].double() * zprev.double() + coef_prev[1].double()
        want_dy = (dz @ W.double()) * (pre > 0)
        want_dw = dz.t() @ torch.relu(pre)
        e_dy, s_dy = float((dyprev.double() - want_dy).abs().max()), float(want_dy.abs().max())
        e_dw, s_dw = float((dW.double() - want_dw).abs().max()), float(want_dw.abs().max())
        print("%d -> %d: dYprev err %.3g of %.3g, dW err %.3g of %.3g" % (Ci, Co, e_dy, s_dy, e_dw, s_dw))
        assert e_dy <= 2e-6 * s_dy * (Co ** 0.5)
        assert e_dw <= 2e-6 * s_dw * (R ** 0.5) / 8
        got = stats.double().sum(0)
        want_s = torch.stack([want_dy.sum(0), (want_dy * zprev.double()).sum(0)])
        assert float((got - want_s).abs().max()) <= 1e-4 * float(want_s.abs().max())
        return dyprev

    dy_mid = layer(256, 128, torch.randn(R, 128, device=dev))  # the upper layer: 256 inputs
    layer(128, 256, dy_mid)                                    # the lower layer: 256 outputs, two passes over its dYprev


def test_partial_tile_forward_is_left_alone():
    """One per-layer forward at R = 100 (64 -> 128): no whole 64-row tile grid, so Z leaves through the partial-tile path -- guarded
    dword stores, no buffer resource, no policy.  Bar of test_split_bf16_products_are_fp32_accurate: every element within 4e-7 of
    sum |a b| of the fp64 product (or twice torch's own fp32 error), and nothing written past row R."""
    from samplenet_amd._lib import check, lib, ptr

    g = torch.Generator(device="cuda").manual_seed(100)
    R, Ci, Co = 100, 64, 128
    A = (torch.rand(R, Ci, device="cuda", generator=g) * 6.0 - 2.5).clamp_min(0.0)
    W = (torch.rand(Co, Ci, device="cuda", generator=g) * 2.0 - 1.0) * 0.2
    bias = torch.rand(Co, device="cuda", generator=g) - 0.5
    Z = torch.full((R + 28, Co), -7.0, device="cuda")
    check(lib.sn_linear_forward(R, Ci, Co, ptr(A), None, ptr(W), ptr(bias), ptr(Z), None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ref = A.double() @ W.double().t() + bias.double()
    mag = A.double().abs() @ W.double().abs().t() + bias.double().abs()
    ours = float(((Z[:R].double() - ref).abs() / mag).max())
    theirs = float((((A @ W.t() + bias).double() - ref).abs() / mag).max())
    print("partial-tile forward: ours %.3g torch %.3g" % (ours, theirs))
    assert ours <= max(4e-7, 2.0 * theirs), (ours, theirs)
    assert bool((Z[R:] == -7.0).all())

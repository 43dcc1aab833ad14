"""PointnetFPModule of the pointnet2 stand-in with fused=True on the GPU, B = 2, train and eval.

Against float64: a hand-written float64 run of the composition a user would write (inverse-distance weights, interpolation, cat,
1 x 1 convolutions, BatchNorm, ReLU) on the kernel's own idx.  Forward values, running statistics and every gradient stay within
max(floor, 2 x torch-fp32-error) of float64 (tests/test_gpu_set_abstraction.py's rule and way of measuring: forward values and
running statistics by their largest element, a gradient by the norm of its difference from float64 relative to the float64
gradient's norm), the torch fp32 error taken from the same run of the module with fused=False on the GPU.  No case is left out: the
test asserts that no float64 pre-activation lies within the forward bound of zero (a ReLU decided differently would be a
difference of its own kind), which holds for the seeds used here.
Two runs of forward + backward give identical bits: no float atomics on the fused route.

FLOORS: the worst torch-fp32-against-float64 error over 16 seeds per level and mode, measured by tools/fp_floors.py (torch only
behind ops.three_nn's indices; the fused route takes no part) into profiles/fp_rows/floors.txt, one per quantity kind.  A kind that
file does not list for a level and mode has floor 0: the 2 x term alone."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
LEVELS = {
    "fp-64-16": dict(n=64, m=16, c2=16, c1=8, mlp=[24, 32, 16]),
    "fp-no-skip": dict(n=96, m=12, c2=8, c1=0, mlp=[8, 16, 16]),
    "fp-m2": dict(n=40, m=2, c2=5, c1=3, mlp=[8, 16, 8]),
}
# the seed of each level's test case: among 0..7 the one whose float64 pre-activations stay farthest from zero in both modes
# (checked on the CPU with tests/interp_ref.py's indices: 5e-5, 1.9e-4 and 5e-4 at the least, against forward bounds of a few 1e-6)
SEEDS = {"fp-64-16": 4, "fp-no-skip": 4, "fp-m2": 2}
# the lines of profiles/fp_rows/floors.txt (tools/fp_floors.py on an MI355X): level, mode, then quantity kind and worst torch-fp32 error
_FLOOR_LINES = """
    fp-64-16    train  out 1.25e-06  known_feats.grad 2.34e-07  skip_feats.grad 1.90e-07  conv.weight.grad 2.57e-07  bn.weight.grad 3.35e-07  bn.bias.grad 2.81e-07  running_mean 3.05e-08  running_var 9.43e-08
    fp-64-16    eval   out 2.83e-07  known_feats.grad 1.73e-07  skip_feats.grad 1.40e-07  running_mean 0.00e+00  running_var 0.00e+00
    fp-no-skip  train  out 1.95e-06  known_feats.grad 3.94e-07  conv.weight.grad 3.99e-07  bn.weight.grad 3.95e-07  bn.bias.grad 2.71e-07  running_mean 3.73e-08  running_var 9.29e-08
    fp-no-skip  eval   out 2.31e-07  known_feats.grad 1.93e-07  running_mean 0.00e+00  running_var 0.00e+00
    fp-m2       train  out 2.32e-06  known_feats.grad 9.95e-07  skip_feats.grad 3.26e-07  conv.weight.grad 6.64e-07  bn.weight.grad 7.66e-07  bn.bias.grad 3.84e-07  running_mean 2.60e-08  running_var 9.41e-08
    fp-m2       eval   out 2.69e-07  known_feats.grad 2.73e-07  skip_feats.grad 1.32e-07  running_mean 0.00e+00  running_var 0.00e+00
"""
FLOORS = {(r[0], r[1], r[i]): float(r[i + 1]) for r in (line.split() for line in _FLOOR_LINES.strip().splitlines())
          for i in range(2, len(r), 2)}   # (level, mode, quantity kind) -> floor


def quantity_kind(name):
    """the quantities of one kind share a floor: the layers' weight gradients, BatchNorm gradients, running statistics"""
    for k in ("conv.weight.grad", "bn.weight.grad", "bn.bias.grad", "running_mean", "running_var"):
        if name.endswith(k):
            return k
    return name


def make_module(level, seed=0, **kw):
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    torch.manual_seed(seed)
    m = PM.PointnetFPModule(list(LEVELS[level]["mlp"]), **kw)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):   # real-valued BatchNorm state, scales of both signs
            C = mod.num_features
            sign = torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
            mod.weight.data = (torch.rand(C, generator=g) + 0.5) * sign
            mod.bias.data = torch.randn(C, generator=g) * 0.3
            mod.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return m.cuda()


def make_inputs(level, seed=0):
    """-> unknown (B,n,3), known (B,m,3), skip features (B,c1,n) or None, known features (B,c2,m), the loss weights (B,Co,n); drawn
    on the CPU so that a CPU check of the seeds sees the same numbers"""
    cfg = LEVELS[level]
    g = torch.Generator().manual_seed(100 + seed)
    unknown, known = torch.rand(B, cfg["n"], 3, generator=g), torch.rand(B, cfg["m"], 3, generator=g)
    sf = torch.randn(B, cfg["c1"], cfg["n"], generator=g) if cfg["c1"] else None
    kf = torch.randn(B, cfg["c2"], cfg["m"], generator=g)
    w = torch.randn(B, cfg["mlp"][-1], cfg["n"], generator=g)
    return tuple(None if t is None else t.cuda() for t in (unknown, known, sf, kf, w))


def run(m, level, fused, seed=0):
    """forward + backward of the module -> dict of everything that is compared"""
    unknown, known, sf, kf, w = make_inputs(level, seed)
    kf.requires_grad_(True)
    if sf is not None:
        sf.requires_grad_(True)
    out = m(unknown, known, sf, kf, fused=fused)
    (out * w).sum().backward()
    got = {"out": out.detach(), "known_feats.grad": kf.grad}
    if sf is not None:
        got["skip_feats.grad"] = sf.grad
    for n, p in m.named_parameters():
        if p.grad is not None:
            got[n + ".grad"] = p.grad
    for n, b_ in m.named_buffers():
        got[n] = b_.detach().clone()
    return got


def mlp64(m0, P, bufs, a, training):
    """the shared MLP in float64 on rows a (R, Ci) -> activated rows, the smallest |pre-activation|; bufs: updated in training mode"""
    closest = float("inf")
    for j, layer in enumerate(m0.mlp):
        pre = "mlp.%d." % j
        z = a @ P[pre + "conv.weight"].view(layer.conv.out_channels, -1).t()
        bn = layer.bn
        if training:
            mean, var = z.mean(0), z.var(0, unbiased=False)
            n = z.shape[0]
            bufs[pre + "bn.running_mean"] = (1 - bn.momentum) * bufs[pre + "bn.running_mean"].double() + bn.momentum * mean.detach()
            bufs[pre + "bn.running_var"] = (1 - bn.momentum) * bufs[pre + "bn.running_var"].double() + bn.momentum * var.detach() * n / (n - 1)
            bufs[pre + "bn.num_batches_tracked"] = bufs[pre + "bn.num_batches_tracked"] + 1
        else:
            mean, var = bn.running_mean.double(), bn.running_var.double()
        y = (z - mean) / torch.sqrt(var + bn.eps) * P[pre + "bn.weight"] + P[pre + "bn.bias"]
        closest = min(closest, float(y.detach().abs().min()))
        a = torch.relu(y)
    return a, closest


def float64_reference(m0, level, idx, filled, seed=0):
    """m0: the module in its state BEFORE the step; idx (B,n,3): the indices to interpolate on, filled (B,n,3) bool: False where a
    slot has no neighbour (m < 3: an infinite distance, weight 0).  -> the compared quantities and the smallest |pre-activation|"""
    cfg = LEVELS[level]
    training = m0.training
    unknown, known, sf, kf, w = make_inputs(level, seed)
    kf64 = kf.double().requires_grad_(True)
    sf64 = None if sf is None else sf.double().requires_grad_(True)
    P = {n: p.detach().double().requires_grad_(True) for n, p in m0.named_parameters()}
    bufs = {n: b_.detach().clone() for n, b_ in m0.named_buffers()}
    li = idx.long().view(B, cfg["n"] * 3)
    nb = torch.gather(known.double(), 1, li[:, :, None].expand(-1, -1, 3)).view(B, cfg["n"], 3, 3)
    dist = (unknown.double()[:, :, None, :] - nb).pow(2).sum(-1).sqrt()
    recip = torch.where(filled, 1.0 / (dist + 1e-8), torch.zeros_like(dist))
    weight = recip / recip.sum(2, keepdim=True)
    f = torch.gather(kf64.transpose(1, 2), 1, li[:, :, None].expand(-1, -1, cfg["c2"])).view(B, cfg["n"], 3, cfg["c2"])
    rows = (f * weight[..., None]).sum(2)
    if sf64 is not None:
        rows = torch.cat([rows, sf64.transpose(1, 2)], dim=2)
    a, closest = mlp64(m0, P, bufs, rows.reshape(B * cfg["n"], -1), training)
    out = a.view(B, cfg["n"], -1).transpose(1, 2)
    (out * w.double()).sum().backward()
    ref = {"out": out.detach(), "known_feats.grad": kf64.grad}
    if sf is not None:
        ref["skip_feats.grad"] = sf64.grad
    for n, p in P.items():
        if training:   # (an eval-mode module is frozen: its parameters' gradients are not compared)
            ref[n + ".grad"] = p.grad
    ref.update(bufs)
    return ref, closest


def kernel_idx(level, seed=0):
    from samplenet_amd import ops

    unknown, known = make_inputs(level, seed)[:2]
    dist, idx = ops.three_nn(unknown, known)
    return idx, torch.isfinite(dist)


def fresh_module(level, mode, seed=0, **kw):
    m = make_module(level, seed, **kw)
    m.train(mode == "train")
    if mode == "eval":
        m.requires_grad_(False)   # an eval-mode module is differentiated towards its inputs only
    return m


def _err(a, b, name="out"):
    """the error of `a` against the float64 `b`: a gradient's by the norm, relative to the reference's; anything else by the largest element"""
    d = a.double() - b.double()
    if name.endswith(".grad"):
        return float(d.norm()) / max(float(b.double().norm()), 1e-300)
    return float(d.abs().max())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("mode", ("train", "eval"))
@pytest.mark.parametrize("level", list(LEVELS))
def test_module(level, mode):
    seed = SEEDS[level]

    def fresh():
        return fresh_module(level, mode, seed)

    t32 = run(fresh(), level, fused=False, seed=seed)
    idx, filled = kernel_idx(level, seed)
    assert bool(filled.all()) == (LEVELS[level]["m"] >= 3)
    ref, closest = float64_reference(fresh(), level, idx, filled, seed=seed)
    fwd_bound = max(FLOORS.get((level, mode, "out"), 0.0), 2 * _err(t32["out"], ref["out"]))
    print("fp %s %s: smallest |float64 pre-activation| %.3g, forward bound %.3g" % (level, mode, closest, fwd_bound))
    assert closest > fwd_bound, "a float64 pre-activation lies within the forward bound of zero: pick another seed"
    got = run(fresh(), level, fused=True, seed=seed)
    again = run(fresh(), level, fused=True, seed=seed)
    assert got["out"].shape == (B, LEVELS[level]["mlp"][-1], LEVELS[level]["n"])
    assert set(got) == set(ref) == set(t32) == set(again), sorted(set(got) ^ set(ref))
    for name in got:
        assert _same_bits(got[name], again[name]), (name, "two runs differ")
        if name.endswith("num_batches_tracked"):
            assert int(got[name]) == int(ref[name]) == int(t32[name]) == (1 if mode == "train" else 0)
            continue
        e_hip, e_ref = _err(got[name], ref[name], name), _err(t32[name], ref[name], name)
        bound = max(FLOORS.get((level, mode, quantity_kind(name)), 0.0), 2 * e_ref)
        print("fp %s %s %s: error %.3g  torch fp32 %.3g  bound %.3g" % (level, mode, name, e_hip, e_ref, bound))
        assert e_hip <= bound, (name, e_hip, e_ref)


def test_unsupported_specs_and_no_known_cloud_take_the_default_route():
    from samplenet_amd import feature_propagation as FP
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    torch.manual_seed(0)
    unknown, known = torch.rand(B, 40, 3, device="cuda"), torch.rand(B, 6, 3, device="cuda")
    sf, kf = torch.randn(B, 3, 40, device="cuda"), torch.randn(B, 4, 6, device="cuda")
    for m in (PM.PointnetFPModule([7, 16], fused=True).cuda(),                  # one layer
              PM.PointnetFPModule([7, 16, 16], bn=False, fused=True).cuda(),     # no BatchNorm
              PM.PointnetFPModule([7, 16, 6], fused=True).cuda()):               # top width % 4
        outs = []
        for fused in (None, False):
            mm = copy.deepcopy(m)
            k = kf.clone().requires_grad_(True)
            out = mm(unknown, known, sf, k, fused=fused)
            out.sum().backward()
            outs.append([out.detach(), k.grad] + [p.grad for p in mm.parameters()])
        # (the same torch launches twice: the forward repeats bit for bit; torch's own weight-gradient sums need not)
        assert _same_bits(outs[0][0], outs[1][0])
        assert all(a.shape == b.shape and torch.allclose(a, b, rtol=1e-4, atol=1e-5) for a, b in zip(outs[0][1:], outs[1][1:]))
    # known=None: the features of one point, expanded -- always the default route
    m = PM.PointnetFPModule([7, 16, 16], fused=True).cuda()
    one = torch.randn(B, 4, 1, device="cuda")
    a, b_ = copy.deepcopy(m)(unknown, None, sf, one), copy.deepcopy(m)(unknown, None, sf, one, fused=False)
    assert a.shape == (B, 16, 40) and _same_bits(a, b_)
    # the constructor's default is today's route; the keyword overrides it either way
    d = PM.PointnetFPModule([7, 16, 16]).cuda()
    f = copy.deepcopy(d)
    assert _same_bits(copy.deepcopy(d)(unknown, known, sf, kf), copy.deepcopy(d)(unknown, known, sf, kf, fused=False))
    out = f(unknown, known, sf, kf, fused=True)
    assert out.shape == (B, 16, 40) and out.transpose(1, 2).is_contiguous()      # a view of the walk's rows
    # eval mode with trainable parameters: weight gradients are refused, as in set abstraction
    e = PM.PointnetFPModule([7, 16, 16], fused=True).cuda().eval()
    with pytest.raises(RuntimeError) as err:
        e(unknown, known, sf, kf).sum().backward()
    assert str(err.value) == ("samplenet_amd.feature_propagation: weight gradients need training mode (.train()); an eval-mode module is "
                              "differentiated w.r.t. its input only -- freeze it with requires_grad_(False)")
    with pytest.raises(ValueError):
        FP.propagate_mlp(PM.PointnetFPModule([7, 16]).cuda().mlp, torch.rand(B, 9, 7, device="cuda"))
    with pytest.raises(ValueError):
        FP.propagate_mlp(e.mlp, torch.rand(B, 9, 5, device="cuda"))


def test_rows_pool_has_the_none_pool_forward():
    """POOL_ROWS against POOL_NONE on one stack: the forward and the running statistics bit for bit (the same launches); the
    gradients differ by the order of the top BatchNorm's two sums and are held to float64 by test_module"""
    from samplenet_amd import set_abstraction, stack_node
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    torch.manual_seed(1)
    mlp = PM.PointnetFPModule([8, 16, 12]).cuda().mlp
    x = torch.randn(3, 100, 8, device="cuda")
    w = torch.randn(3, 100, 12, device="cuda")
    res = []
    for pool in (stack_node.POOL_NONE, stack_node.POOL_ROWS):
        mm = copy.deepcopy(mlp)
        xi = x.clone().requires_grad_(True)
        spec = stack_node.StackSpec(set_abstraction.layer_records(mm), True, pool, None, stack_node.WGRADS_TRAINING, "no")
        out, none = stack_node.conv_stack(spec, xi)
        assert none is None
        (out * w).sum().backward()
        res.append([out.detach(), xi.grad] + [p.grad for p in mm.parameters()] + [b_.clone() for b_ in mm.buffers()])
    assert len(res[0]) == 2 + 6 + 6
    assert _same_bits(res[0][0], res[1][0]) and all(_same_bits(a, b_) for a, b_ in zip(res[0][-6:], res[1][-6:]))
    assert all(a.shape == b_.shape and bool(torch.isfinite(b_).all()) for a, b_ in zip(res[0][1:-6], res[1][1:-6]))


def test_encoder_decoder_trains_one_step():
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    torch.manual_seed(0)
    sa1 = PM.PointnetSAModule([4, 16, 32], npoint=32, radius=0.4, nsample=8).cuda()
    sa2 = PM.PointnetSAModule([32, 32, 64], npoint=8, radius=0.8, nsample=8).cuda()
    fp2 = PM.PointnetFPModule([64 + 32, 64, 32], fused=True).cuda()
    fp1 = PM.PointnetFPModule([32 + 4, 32, 16], fused=True).cuda()
    params = [p for mod in (sa1, sa2, fp2, fp1) for p in mod.parameters()]
    opt = torch.optim.SGD(params, lr=0.01)
    xyz, f0 = torch.rand(B, 128, 3, device="cuda"), torch.randn(B, 4, 128, device="cuda")
    before = [p.detach().clone() for p in params]
    xyz1, f1 = sa1(xyz, f0)
    xyz2, f2 = sa2(xyz1, f1)
    u1 = fp2(xyz1, xyz2, f1, f2)
    u0 = fp1(xyz, xyz1, f0, u1)
    assert u0.shape == (B, 16, 128)
    u0.square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in params)
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params))

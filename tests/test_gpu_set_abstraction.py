"""The set-abstraction modules of the pointnet2 stand-in (PointnetSAModule, PointnetSAModuleMSG) on the GPU, B = 2, train and eval.

Bit for bit: the fused forward against the composition of this library's existing launches -- ops.ball_group, a permute, the
conv-stack node (stack_node.py) with the points pool and zero bias tensors, as the classifier runs a pooled stack (the same GEMM
launches on the same data; the pool is a pure selection) --, the running
statistics and num_batches_tracked after a training step against that composition's, and the weight / BatchNorm gradients wherever
the existing pool pair is the chosen route (at these sizes set_abstraction.group_pool_route always chooses it; every case runs a
second time with the group-pool pair forced, where the forward must still agree bit for bit and the gradients are held to float64).
Two runs of forward + backward give identical bits for every gradient: no float atomics on the fused route.
Both sides of that comparison are the one node now (once classifier._StackFunction against a node of set abstraction's own), so it no
longer anchors the MLP half; what it still separates: the grouping route (ops.ball_group + permute against the row-layout launch), the
bias route (a zero bias tensor against NULL + sink) and the pool pair.  The MLP half's anchor is the float64 comparison below.

Against float64: a hand-written float64 run of the composition a user would write (grouping, 1 x 1 convolutions, BatchNorm, ReLU, max)
on the kernel's own idx, its pool teacher-forced with the GPU's argsel -- after every GPU pick was verified to reach the float64
maximum of its group and channel within the forward bound, so no case is left out.  Forward values, running statistics and every
gradient stay within max(floor, 2 x torch-fp32-error) of float64 (tests/test_gpu_classifier.py's rule), the torch fp32 error taken
from the same run of the module with fused=False on the GPU.  The errors are measured as in that file: forward values and running
statistics by their largest element, a gradient by the norm of its difference from float64 relative to the float64 gradient's norm.
(Measured by the largest element instead, a gradient's figure is one element's luck: at sa-64-8-16 in training mode the first
layer's weight gradient stood at 7.29e-05 where torch's own run stood at 3.48e-05, and torch's figure itself moved between 1.8e-06
and 2.1e-06 from one machine to the next for a BatchNorm gradient.  By the norm the worst ratio to torch over all cases is 1.9.)

FLOORS: the worst torch-fp32-against-float64 error over 16 seeds per level, measured by tools/sa_floors.py (torch only; the code
under test takes no part) into profiles/sa/floors.txt, one per quantity kind (the layers' weight gradients share one, and so on).  A
kind that file does not list for a level and mode (a frozen module's unchanged running statistics) has floor 0: the 2 x term alone."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
LEVELS = {
    "sa-96-12-8": dict(N=96, npoint=12, radii=(0.4,), nsamples=(8,), C=0, mlps=([0, 16, 32],)),
    "sa-64-8-16": dict(N=64, npoint=8, radii=(0.6,), nsamples=(16,), C=5, mlps=([5, 32, 64],)),
    "group-all": dict(N=64, npoint=None, radii=(None,), nsamples=(None,), C=5, mlps=([5, 32, 64],)),
    "msg": dict(N=64, npoint=8, radii=(0.3, 0.6), nsamples=(4, 16), C=5, mlps=([5, 16, 32], [5, 32, 64])),
}
# the lines of profiles/sa/floors.txt (tools/sa_floors.py on an MI355X): level, mode, then quantity kind and worst torch-fp32 error
# (a gradient: norm of the difference / norm of the float64 gradient; anything else: the largest element)
_FLOOR_LINES = """
    sa-96-12-8  train  out 2.14e-06  xyz.grad 2.99e-07  conv.weight.grad 1.26e-06  bn.weight.grad 7.55e-07  bn.bias.grad 5.40e-07  running_mean 3.85e-08  running_var 9.34e-08
    sa-96-12-8  eval   out 1.46e-07  xyz.grad 9.90e-08  running_mean 0.00e+00  running_var 0.00e+00
    sa-64-8-16  train  out 1.74e-06  xyz.grad 2.32e-07  features.grad 2.64e-07  conv.weight.grad 4.12e-07  bn.weight.grad 4.74e-07  bn.bias.grad 4.89e-07  running_mean 3.14e-08  running_var 9.40e-08
    sa-64-8-16  eval   out 3.65e-07  xyz.grad 1.06e-07  features.grad 1.30e-07  running_mean 0.00e+00  running_var 0.00e+00
    group-all   train  out 1.55e-06  xyz.grad 2.53e-07  features.grad 2.49e-07  conv.weight.grad 4.03e-07  bn.weight.grad 4.67e-07  bn.bias.grad 4.36e-07  running_mean 4.32e-08  running_var 9.64e-08
    group-all   eval   out 2.51e-07  xyz.grad 1.34e-07  features.grad 1.28e-07  running_mean 0.00e+00  running_var 0.00e+00
    msg         train  out 2.76e-06  xyz.grad 2.67e-07  features.grad 2.44e-07  conv.weight.grad 4.67e-07  bn.weight.grad 3.77e-07  bn.bias.grad 4.27e-07  running_mean 4.02e-08  running_var 9.28e-08
    msg         eval   out 3.97e-07  xyz.grad 1.17e-07  features.grad 1.36e-07  running_mean 0.00e+00  running_var 0.00e+00
"""
FLOORS = {(r[0], r[1], r[i]): float(r[i + 1]) for r in (line.split() for line in _FLOOR_LINES.strip().splitlines())
          for i in range(2, len(r), 2)}   # (level, mode, quantity kind) -> floor


def quantity_kind(name):
    """the quantities of one kind share a floor: the layers' weight gradients, BatchNorm gradients, running statistics"""
    for k in ("conv.weight.grad", "bn.weight.grad", "bn.bias.grad", "running_mean", "running_var"):
        if name.endswith(k):
            return k
    return name


def make_module(level, seed=0):
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    cfg = LEVELS[level]
    torch.manual_seed(seed)
    m = PM.PointnetSAModuleMSG(cfg["npoint"], cfg["radii"], cfg["nsamples"], [list(s) for s in cfg["mlps"]])
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):   # real-valued BatchNorm state, scales of both signs (the pool's min route)
            C = mod.num_features
            sign = torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
            mod.weight.data = (torch.rand(C, generator=g) + 0.5) * sign
            mod.bias.data = torch.randn(C, generator=g) * 0.3
            mod.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return m.cuda()


def make_inputs(level, seed=0):
    cfg = LEVELS[level]
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    xyz = torch.rand(B, cfg["N"], 3, device="cuda", generator=g)
    f = torch.randn(B, cfg["C"], cfg["N"], device="cuda", generator=g) if cfg["C"] else None
    cout = sum(s[-1] for s in cfg["mlps"])
    npoint = cfg["npoint"] or 1
    w = torch.randn(B, cout, npoint, device="cuda", generator=g)
    w2 = torch.randn(B, npoint, 3, device="cuda", generator=g)
    return xyz, f, w, w2


def run(m, level, fused, seed=0):
    """forward + backward of the module -> dict of everything that is compared"""
    xyz, f, w, w2 = make_inputs(level, seed)
    xyz.requires_grad_(True)
    if f is not None:
        f.requires_grad_(True)
    new_xyz, out = m(xyz, f, fused=fused)
    loss = (out * w).sum()
    if new_xyz is not None:
        loss = loss + (new_xyz * w2).sum()
    loss.backward()
    got = {"out": out.detach(), "xyz.grad": xyz.grad}
    if f is not None:
        got["features.grad"] = f.grad
    for n, p in m.named_parameters():
        if p.grad is not None:
            got[n + ".grad"] = p.grad
    for n, b_ in m.named_buffers():
        got[n] = b_.detach().clone()
    return got


class _ZeroBiasLayer:
    """pointnet._Layer record of a bias-free conv on the bias route: a zero bias tensor (z + 0 has z's bits), whose gradient the
    backward allocates like the bias instead of sending it to the sink."""

    def __init__(self, name, conv, bn_name, bn):
        self.name, self.bn_name, self.W, self.bn = name, bn_name, conv.weight, bn
        self.b = torch.zeros(conv.out_channels, device=conv.weight.device)
        self.Co, self.Ci = conv.weight.shape[0], conv.weight.shape[1]


def composition(m, level, seed=0):
    """the module's computation out of the library's existing launches"""
    from samplenet_amd import classifier, ops

    cfg = LEVELS[level]
    xyz, f, w, w2 = make_inputs(level, seed)
    training = m.training
    new_xyz = None
    if cfg["npoint"] is not None:
        fps = ops.furthest_point_sample(xyz, cfg["npoint"])
        new_xyz = ops.gather_operation(xyz.transpose(1, 2).contiguous(), fps).transpose(1, 2).contiguous()
    outs = []
    for i, mlp in enumerate(m.mlps):
        if cfg["npoint"] is None:
            x = torch.cat([xyz] + ([] if f is None else [f.transpose(1, 2)]), dim=2).contiguous()
        else:
            g = ops.ball_group(cfg["radii"][i], cfg["nsamples"][i], xyz, new_xyz, f, use_xyz=True, rule="squared")
            x = g.permute(0, 2, 3, 1).contiguous().view(B * cfg["npoint"], cfg["nsamples"][i], g.shape[1])
        layers = [_ZeroBiasLayer("%d.conv" % j, l.conv, "%d.bn" % j, l.bn) for j, l in enumerate(mlp)]
        pooled, _ = classifier._stack(layers, True, training, x)   # the node with the points pool; x is float32 contiguous already
        outs.append(pooled.view(B, -1, pooled.shape[1]))
    out = torch.cat(outs, dim=2).transpose(1, 2).contiguous()
    got = {"out": out.detach()}
    if training:
        (out * w).sum().backward()
        for n, p in m.named_parameters():
            got[n + ".grad"] = p.grad
    for n, b_ in m.named_buffers():
        got[n] = b_.detach().clone()
    return got


def float64_reference(m0, level, fwd_bound, seed=0, picks="hip"):
    """m0: the module in its state BEFORE the step.  The composition in float64 on the kernel's idx, the pool teacher-forced with the
    GPU's argsel once every pick is verified against the float64 maximum.  picks="torch" (tools/sa_floors.py: the fused route takes
    no part): idx from ops.ball_query, the pool teacher-forced with the picks of the torch fp32 layers, unverified."""
    from samplenet_amd import ops, set_abstraction

    cfg = LEVELS[level]
    training = m0.training
    xyz, f, w, w2 = make_inputs(level, seed)
    x64 = xyz.double().requires_grad_(True)
    f64 = None if f is None else f.double().requires_grad_(True)
    P = {n: p.detach().double().requires_grad_(True) for n, p in m0.named_parameters()}
    bufs = {n: b_.detach().clone() for n, b_ in m0.named_buffers()}
    new64 = None
    if cfg["npoint"] is not None:
        fps = ops.furthest_point_sample(xyz, cfg["npoint"]).long()
        new64 = torch.gather(x64, 1, fps[:, :, None].expand(B, cfg["npoint"], 3))
        new32 = torch.gather(xyz, 1, fps[:, :, None].expand(B, cfg["npoint"], 3)).contiguous()
    outs = []
    for i, mlp in enumerate(m0.mlps):
        rows_f = None if f is None else f.transpose(1, 2).contiguous()
        if cfg["npoint"] is None:
            rows32 = torch.cat([xyz] + ([] if f is None else [rows_f]), dim=2).contiguous()
            rows64 = torch.cat([x64] + ([] if f is None else [f64.transpose(1, 2)]), dim=2)
            G, S = B, cfg["N"]
        else:
            ns = cfg["nsamples"][i]
            if picks == "hip":
                rows32, idx, _ = ops.ball_group_rows(cfg["radii"][i], ns, xyz, new32, rows_f, return_idx=True)
            else:
                rows32, idx = None, ops.ball_query(cfg["radii"][i], ns, xyz, new32, rule="squared")[0]
            G, S = B * cfg["npoint"], ns
            li = idx.long().view(B, G // B * S)
            gx = torch.gather(x64, 1, li[:, :, None].expand(-1, -1, 3)).view(B, -1, S, 3) - new64[:, :, None, :]
            parts = [gx]
            if f is not None:
                parts.append(torch.gather(f64.transpose(1, 2), 1, li[:, :, None].expand(-1, -1, cfg["C"])).view(B, -1, S, cfg["C"]))
            rows64 = torch.cat(parts, dim=3)
            assert rows32 is None or torch.equal(rows32, rows64.detach().float())   # a float32 difference, rounded from the exact one
        if picks == "hip":
            _, argsel = set_abstraction.grouped_mlp_max(copy.deepcopy(mlp), rows32.view(G, S, -1), return_argsel=True)
        else:
            with torch.no_grad():   # (B, Ci, G / B, S) through the torch layers
                y32 = copy.deepcopy(mlp)(rows64.detach().float().view(B, G // B, S, -1).permute(0, 3, 1, 2).contiguous())
            argsel = y32.argmax(3).permute(0, 2, 1).reshape(G, -1)
        a = rows64.reshape(G * S, -1)
        for j, layer in enumerate(mlp):
            pre = "mlps.%d.%d." % (i, j)
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
            a = torch.relu((z - mean) / torch.sqrt(var + bn.eps) * P[pre + "bn.weight"] + P[pre + "bn.bias"])
        y = a.view(G, S, -1)
        picked = torch.gather(y, 1, argsel.long()[:, None, :])[:, 0]
        gap = float((y.amax(1) - picked).detach().max())
        assert gap <= fwd_bound, ("a GPU pick misses the float64 maximum of its group by more than the forward bound", i, gap, fwd_bound)
        outs.append(picked.view(B, -1, picked.shape[1]))
    out = torch.cat(outs, dim=2).transpose(1, 2)
    loss = (out * w.double()).sum()
    if new64 is not None:
        loss = loss + (new64 * w2.double()).sum()
    loss.backward()
    ref = {"out": out.detach(), "xyz.grad": x64.grad}
    if f is not None:
        ref["features.grad"] = f64.grad
    for n, p in P.items():
        if training:   # (an eval-mode module is frozen: its parameters' gradients are not compared)
            ref[n + ".grad"] = p.grad
    ref.update(bufs)
    return ref


def fresh_module(level, mode, seed=0):
    m = make_module(level, seed)
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


@pytest.mark.parametrize("group_pool", (None, True), ids=("pool-rule", "group-pool"))
@pytest.mark.parametrize("mode", ("train", "eval"))
@pytest.mark.parametrize("level", list(LEVELS))
def test_module(level, mode, group_pool, monkeypatch):
    from samplenet_amd import set_abstraction

    def fresh():
        return fresh_module(level, mode)

    # the torch composition in fp32 and the error it makes: the yardstick of the bound
    t32 = run(fresh(), level, fused=False)
    # (the forward bound needs the reference's forward, which needs the bound for its pick check: the reference first runs with
    #  the pick check open, to give the torch error of the forward values; the checked run follows)
    ref = float64_reference(fresh(), level, float("inf"))
    fwd_bound = max(FLOORS.get((level, mode, "out"), 0.0), 2 * _err(t32["out"], ref["out"]))
    monkeypatch.setattr(set_abstraction, "FORCE_GROUP_POOL", group_pool)
    ref = float64_reference(fresh(), level, fwd_bound)
    got = run(fresh(), level, fused=True)
    again = run(fresh(), level, fused=True)
    assert set(got) == set(ref) == set(t32) == set(again), sorted(set(got) ^ set(ref))
    for name in got:
        assert _same_bits(got[name], again[name]), (name, "two runs differ")
        if name.endswith("num_batches_tracked"):
            assert int(got[name]) == int(ref[name]) == int(t32[name]) == (1 if mode == "train" else 0)
            continue
        e_hip, e_ref = _err(got[name], ref[name], name), _err(t32[name], ref[name], name)
        bound = max(FLOORS.get((level, mode, quantity_kind(name)), 0.0), 2 * e_ref)
        print("sa %s %s %s %s: error %.3g  torch fp32 %.3g" % (level, mode, "group-pool" if group_pool else "pool-rule", name, e_hip, e_ref))
        assert e_hip <= bound, (name, e_hip, e_ref)
    # the library's own composition, bit for bit
    comp = composition(fresh(), level)
    routes = [set_abstraction.group_pool_route(B * (LEVELS[level]["npoint"] or 1), ns or LEVELS[level]["N"]) for ns in LEVELS[level]["nsamples"]]
    assert routes == [bool(group_pool)] * len(routes)
    for name, t in comp.items():
        if name.endswith(".grad") and group_pool:
            continue   # (the group-pool pair sums the top BatchNorm's backward in another order)
        assert _same_bits(got[name], t), (name, "differs from the composition of ops.ball_group + classifier._StackFunction")


def test_fused_false_and_unsupported_specs_take_the_torch_route():
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    torch.manual_seed(0)
    xyz, f = torch.rand(B, 40, 3, device="cuda"), torch.randn(B, 4, 40, device="cuda")
    for m in (PM.PointnetSAModule([4, 16], npoint=6, radius=0.5, nsample=4).cuda(),             # one layer
              PM.PointnetSAModule([4, 16, 16], npoint=6, radius=0.5, nsample=4, bn=False).cuda()):  # no BatchNorm
        new_xyz, out = m(xyz, f)
        new2, out2 = m(xyz, f, fused=False)
        assert out.shape == (B, 16, 6) and torch.equal(out, out2) and torch.equal(new_xyz, new2)
    m = PM.PointnetSAModule([4, 16, 16], npoint=6, radius=0.5, nsample=4, use_xyz=False).cuda()
    assert m(xyz, f)[1].shape == (B, 16, 6)
    with pytest.raises(ValueError):
        m(xyz, None)
    # a transposed view of a contiguous (B,N,C) tensor is read where it lies
    rows = torch.randn(B, 40, 4, device="cuda")
    assert PM._rows_of(rows.transpose(1, 2)).data_ptr() == rows.data_ptr() and PM._rows_of(f).is_contiguous()
    # eval mode with trainable parameters: weight gradients are refused, as in the classifier
    m = PM.PointnetSAModule([4, 16, 16], npoint=6, radius=0.5, nsample=4).cuda().eval()
    with pytest.raises(RuntimeError):
        m(xyz, f)[1].sum().backward()


def test_grouped_mlp_max_refuses_weight_gradients_in_eval_mode():
    from samplenet_amd import set_abstraction
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    torch.manual_seed(0)
    mlp = PM.PointnetSAModule([5, 16, 16], npoint=2, radius=0.5, nsample=4, use_xyz=False).cuda().eval().mlps[0]
    assert mlp[0].conv.in_channels == 5 and all(p.requires_grad for p in mlp.parameters())
    rows = torch.randn(2, 4, 5, device="cuda", requires_grad=True)
    out = set_abstraction.grouped_mlp_max(mlp, rows)
    assert out.shape == (2, 16)
    with pytest.raises(RuntimeError) as e:
        out.sum().backward()
    assert str(e.value) == ("samplenet_amd.set_abstraction: weight gradients need training mode (.train()); an eval-mode module is "
                            "differentiated w.r.t. its input only -- freeze it with requires_grad_(False)")

"""sn_weighted_gather_backward_inverted on the device behind sn_gather_invert, both called by raw pointer into poisoned and guarded
buffers, over every shape row, index recipe and value recipe of tests/gather_inv_ref.py: grad_X bit for bit the sequential
float32 sum of the restatement, bit for bit sn_weighted_gather_backward_ordered on the same inputs (the contract), within
(L + 1) * 2^-24 * sum|term| of float64, exact on the integer values; every element written, guards untouched; every case twice, bit
for bit.  The Python surface: ops.three_interpolate's backward is the ordered entry's grad_X and the existing entry's
grad_weights bit for bit, with and without inverse=; past the bound it is the ordered route; PointnetFPModule's gradient towards
known_feats is the bits it had on WeightedGatherFunction.  The two entries captured as one chain on one stream and replayed twice.
(No backward() runs inside a capture anywhere in this file.)"""
import numpy as np
import pytest
import torch

import gather_inv_ref as G
from cabi_ref import POISON, Guarded, bits as _bits, stream as _stream

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _ok(lib, rc):
    assert rc == 0, lib.sn_last_error_string()


class Inputs:
    def __init__(self, shape, ref):
        self.shape = shape
        self.idx, self.w, self.g = dev(ref["idx"]), dev(ref["weights"]), dev(ref["grad_out"])


def _inverted(lib, x, start=None, order=None, grad=None):
    """sn_gather_invert + sn_weighted_gather_backward_inverted into fresh guarded buffers (or the given ones)"""
    b, c, n, m, k = x.shape
    start = start or Guarded((b, n + 1), torch.int32)
    order = order or Guarded((b, m * k), torch.int32)
    grad = grad or Guarded((b, c, n))
    _ok(lib, lib.sn_gather_invert(b, n, m * k, x.idx.data_ptr(), start.ptr(), order.ptr(), _stream()))
    _ok(lib, lib.sn_weighted_gather_backward_inverted(b, c, n, m, k, x.w.data_ptr(), x.g.data_ptr(), start.ptr(), order.ptr(),
                                                      grad.ptr(), _stream()))
    return start, order, grad


def _ordered(lib, shape, idx, w, g, want_gw=False):
    """sn_weighted_gather_backward_ordered on the same inputs.  X is a guarded buffer of zeros: the ordered kernel reads X at
    every index for the weights' gradient, an index of -1 or n included, and those reads stay inside the guards."""
    b, c, n, m, k = shape
    X = Guarded((b, c, n), fill=np.zeros((b, c, n), np.float32))
    grad, scratch = Guarded((b, c, n)), torch.empty(max(b * c * m * k, 1), device="cuda")
    gw = torch.empty(b, m, k, device="cuda") if want_gw else None
    _ok(lib, lib.sn_weighted_gather_backward_ordered(b, c, n, m, k, X.ptr(), idx.data_ptr(), w.data_ptr(), g.data_ptr(),
                                                     gw.data_ptr() if want_gw else None, grad.ptr(), scratch.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return grad, gw


@pytest.mark.parametrize("values", G.VALUE_RECIPES)
@pytest.mark.parametrize("recipe", G.INDEX_RECIPES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
def test_backward_bit_for_bit(shape, recipe, values):
    from samplenet_amd._lib import lib

    ref = G.case(shape, recipe, values)
    x = Inputs(shape, ref)
    start, order, grad = _inverted(lib, x)
    torch.cuda.synchronize()
    assert np.array_equal(start.check("start").cpu().numpy(), ref["start"]) and np.array_equal(order.check("order").cpu().numpy(), ref["order"])
    got = grad.check("grad_X").cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref["grad32"])), "grad_X differs from the sequential float32 sum"
    old, _ = _ordered(lib, shape, x.idx, x.w, x.g)
    assert np.array_equal(_bits(got), _bits(old.check("ordered grad_X").cpu().numpy())), "grad_X differs from the ordered entry"
    err = np.abs(got.astype(np.float64) - ref["grad64"])
    pos = ref["bound"] > 0
    print("worst error / bound %.3g" % (float((err[pos] / ref["bound"][pos]).max()) if pos.any() else 0.0))
    assert (err <= ref["bound"]).all()
    if values == "int":
        assert np.array_equal(got.astype(np.float64), ref["grad64"])
    again = _inverted(lib, x)
    torch.cuda.synchronize()
    assert all(torch.equal(a.raw, f.raw) for a, f in zip(again, (start, order, grad)))


def _surface_case():
    shape = (2, 16, 65, 257, 3)
    ref = G.case(shape, "nn", "mixed")
    feats = np.random.default_rng(11).standard_normal((shape[0], shape[1], shape[2])).astype(np.float32)
    return shape, ref, feats


def test_three_interpolate_backward_is_the_ordered_entry():
    from samplenet_amd import ops
    from samplenet_amd._lib import lib
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    shape, ref, feats = _surface_case()
    b, c, n, m, k = shape
    idx, g = dev(ref["idx"]), dev(ref["grad_out"])
    # what the parent computed: the ordered entry's grad_X, and grad_weights of either existing entry
    X = dev(feats)
    want_gx, scratch = torch.empty_like(X), torch.empty(b * c * m * k, device="cuda")
    want_gw, gw2 = torch.empty(b, m, k, device="cuda"), torch.empty(b, m, k, device="cuda")
    w0 = dev(ref["weights"])
    _ok(lib, lib.sn_weighted_gather_backward_ordered(b, c, n, m, k, X.data_ptr(), idx.data_ptr(), w0.data_ptr(), g.data_ptr(),
                                                     want_gw.data_ptr(), want_gx.data_ptr(), scratch.data_ptr(), _stream()))
    _ok(lib, lib.sn_weighted_gather_backward(b, c, n, m, k, X.data_ptr(), idx.data_ptr(), w0.data_ptr(), g.data_ptr(), gw2.data_ptr(),
                                             None, _stream()))
    assert torch.equal(want_gw.view(torch.int32), gw2.view(torch.int32))
    inverse = ops.gather_invert(idx, n)
    outs = []
    for fn, kwargs in ((ops.three_interpolate, {}), (ops.three_interpolate, {"inverse": inverse}), (PU.three_interpolate, {}),
                       (lambda f, i, w: ops.WeightedGatherFunction.apply(f, i, w), {})):
        f, w = dev(feats).requires_grad_(True), dev(ref["weights"]).requires_grad_(True)
        out = fn(f, idx, w, **kwargs)
        out.backward(g)
        assert torch.equal(f.grad.view(torch.int32), want_gx.view(torch.int32)) and torch.equal(w.grad.view(torch.int32), want_gw.view(torch.int32))
        outs.append(out.detach())
        # the features alone (as inside PointnetFPModule: the weights carry no gradient), and the weights alone
        f2 = dev(feats).requires_grad_(True)
        fn(f2, idx, dev(ref["weights"]), **kwargs).backward(g)
        assert torch.equal(f2.grad.view(torch.int32), want_gx.view(torch.int32))
        w2 = dev(ref["weights"]).requires_grad_(True)
        fn(dev(feats), idx, w2, **kwargs).backward(g)
        assert torch.equal(w2.grad.view(torch.int32), want_gw.view(torch.int32))
    assert all(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)) for o in outs)
    f, w = dev(feats).requires_grad_(True), dev(ref["weights"])
    for bad in (ops.GatherInverse(inverse.start[:, :-1], inverse.order), ops.GatherInverse(inverse.start, inverse.order[:1]),
                ops.GatherInverse(inverse.start.long(), inverse.order), ops.GatherInverse(inverse.start, inverse.order.cpu())):
        with pytest.raises(ValueError):
            ops.three_interpolate(f, idx, w, inverse=bad)


def test_past_the_bound_three_interpolate_takes_the_ordered_route():
    from samplenet_amd import ops
    from samplenet_amd._lib import lib

    b, c, n, m, k = shape = (1, 1, 1 << 20, 1366, 3)        # 16384 groups of 64 rows * 4098 entries: past 2^26
    assert not ops.gather_invert_supported(n, m * k)
    rng = np.random.default_rng(5)
    idx = dev(rng.integers(0, 50, (b, m, k)).astype(np.int32) * 20000)     # 50 rows, lists of about 80
    w, g = dev(rng.integers(-3, 4, (b, m, k)).astype(np.float32)), dev(rng.integers(-3, 4, (b, c, m)).astype(np.float32))
    f = torch.zeros(b, c, n, device="cuda", requires_grad=True)
    ops.three_interpolate(f, idx, w).backward(g)
    want, _ = _ordered(lib, shape, idx, w, g)     # (integers: exact in the unordered order the ordered entry takes at this size)
    assert torch.equal(f.grad.view(torch.int32), want.view().view(torch.int32))
    ref = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, idx.view(-1).long(), (g[0, 0, :, None].double() * w[0].double()).view(-1))
    assert torch.equal(f.grad[0, 0].double(), ref) and int((f.grad != 0).sum()) > 10
    made_up = ops.GatherInverse(torch.zeros(b, n + 1, dtype=torch.int32, device="cuda"), torch.zeros(b, m * k, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):       # no inverse exists past the bound: a hand-built one is refused, not walked
        ops.three_interpolate(f, idx, w, inverse=made_up)


@pytest.mark.parametrize("mlp", [[], [8, 4]])
def test_fp_module_gradient_keeps_its_bits(mlp, monkeypatch):
    from samplenet_amd import ops
    from samplenet_amd._lib import lib
    from samplenet_amd.compat.pointnet2.utils.pointnet2_modules import PointnetFPModule
    import interp_ref as R

    ishape = (2, 257, 65, 16, 1)          # interp_ref's order: (b, n unknown, m known, c2, c1)
    b, n, m, c2, c1 = ishape
    u, kn = R.make_case(ishape, "lattice")
    kf, uf, _ = R.make_feats(ishape)
    torch.manual_seed(5)
    fp = PointnetFPModule([c2 + c1] + mlp).cuda()
    wt = torch.randn(b, (mlp or [c2 + c1])[-1], n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    seen = {}

    def run():
        dkf, duf = dev(kf).requires_grad_(True), dev(uf).requires_grad_(True)
        fp.zero_grad()
        hook = fp.mlp.register_forward_pre_hook(lambda _m, args: args[0].register_hook(lambda gr: seen.__setitem__("grad", gr.detach().clone())) and None)
        out = fp(dev(u), dev(kn), duf, dkf)
        hook.remove()
        (out * wt).sum().backward()
        return out.detach(), dkf.grad, seen.get("grad")

    out_new, g_new, arrived = run()
    if arrived is None:                   # no layer: the module's output is the assembled tensor itself
        arrived = wt.unsqueeze(-1)
    # the ordered entry on exactly the gradient that arrived at the interpolation
    dist, idx = ops.three_nn(dev(u), dev(kn))
    recip = 1.0 / (dist + 1e-8)
    weight = (recip / torch.sum(recip, dim=2, keepdim=True)).contiguous()
    want, _ = _ordered(lib, (b, c2, m, n, 3), idx, weight, arrived[:, :c2, :, 0].contiguous())
    assert torch.equal(g_new.view(torch.int32), want.view().view(torch.int32))
    if not mlp:                           # nothing but the assembly runs: the whole module with the new route switched off
        monkeypatch.setattr(ops, "three_interpolate", lambda f, i, w: ops.WeightedGatherFunction.apply(f, i, w))
        out_old, g_old, _ = run()
        assert torch.equal(out_old.view(torch.int32), out_new.view(torch.int32)) and torch.equal(g_old.view(torch.int32), g_new.view(torch.int32))


def test_the_two_entries_captured_as_one_chain():
    from samplenet_amd._lib import lib

    shape = (2, 16, 65, 257, 3)
    b, c, n, m, k = shape
    ref = G.case(shape, "oob", "mixed")
    x = Inputs(shape, ref)
    eager = _inverted(lib, x)
    torch.cuda.synchronize()
    bufs = (Guarded((b, n + 1), torch.int32), Guarded((b, m * k), torch.int32), Guarded((b, c, n)))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _inverted(lib, x, *bufs)          # warm-up outside the capture (first-use runtime work)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):         # the two launches, in order, on the capture's stream; no autograd inside
        _inverted(lib, x, *bufs)
    for replay in range(2):
        for buf in bufs:
            buf.raw.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for buf, e, name in zip(bufs, eager, ("start", "order", "grad_X")):
            buf.check("%s, replay %d" % (name, replay))
            assert torch.equal(buf.raw, e.raw), "%s: replay %d differs from the eager call" % (name, replay)
    assert np.array_equal(_bits(bufs[2].numpy()), _bits(ref["grad32"]))

"""sn_interp_rows_forward / sn_interp_rows_backward on the device, called directly into poisoned and guarded buffers, every case
twice with equal bits, then the autograd surface over them (ops.interp_rows) and one capture of the direct chain.

Forward: weights and rows bit for bit the numpy restatement (tests/fp_rows_ref.py on tests/interp_ref.py), the interpolated columns
bit for bit sn_weighted_gather_forward at k = 3 given the kernel's weights, the weights within interp_ref.WEIGHT_BOUND of float64.
Backward: grad_known bit for bit the sequential float32 sum in list order and bit for bit sn_weighted_gather_backward_inverted on
transposed operands, within (L + 1) * 2^-24 * sum|term| of float64, exact on integer values."""
import numpy as np
import pytest
import torch

import fp_rows_ref as FR
import interp_ref as R
from cabi_ref import Guarded, bits as _bits, invert as _invert, stream as _stream

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _forward(lib, shape, rule, kr, sr, idx, d2):
    b, n, m, c2, c1 = shape
    w, rows = Guarded((b, n, 3)), Guarded((b, n, c2 + c1))
    rc = lib.sn_interp_rows_forward(b, n, m, c2, c1, rule, kr.data_ptr(), sr.data_ptr() if c1 else None, idx.data_ptr(), d2.data_ptr(),
                                    w.ptr(), rows.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return w, rows


@pytest.mark.parametrize("recipe", FR.RECIPES)
@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.SHAPE_IDS)
def test_forward(shape, recipe):
    from samplenet_amd._lib import lib

    b, n, m, c2, c1 = shape
    d = FR.forward_case(shape, recipe)
    kr, sr, idx, d2 = dev(d["known_rows"]), dev(d["skip_rows"]), dev(d["idx"]), dev(d["d2"])
    # the inputs are what sn_three_nn writes for this case
    gi, gd = torch.empty(b, n, 3, device="cuda", dtype=torch.int32), torch.empty(b, n, 3, device="cuda")
    assert lib.sn_three_nn(b, n, m, dev(d["unknown"]).data_ptr(), dev(d["known"]).data_ptr(), gd.data_ptr(), None, gi.data_ptr(), _stream()) == 0
    assert torch.equal(gi, idx) and torch.equal(gd.view(torch.int32), d2.view(torch.int32))
    kf = kr.transpose(1, 2).contiguous()                       # (b,c2,m) for sn_weighted_gather_forward
    for rule in R.RULES:
        w, rows = _forward(lib, shape, rule, kr, sr, idx, d2)
        got_w, got = w.check("weights").cpu().numpy(), rows.check("rows").cpu().numpy()
        assert np.array_equal(_bits(got_w), _bits(d["w%d" % rule])), "weights"
        assert np.array_equal(_bits(got), _bits(d["rows%d" % rule])), "rows"
        w64 = R.weights64(d["d2"], rule)
        err = np.abs(got_w - w64)
        print("interp rows %s %s rule %d: worst weight error / bound %.3g" % (
            "x".join(map(str, shape)), recipe, rule, (err / np.maximum(R.WEIGHT_BOUND[rule] * np.abs(w64), 1e-300)).max()))
        assert (err <= R.WEIGHT_BOUND[rule] * np.abs(w64)).all()
        out = torch.empty(b, c2, n, device="cuda")
        assert lib.sn_weighted_gather_forward(b, c2, m, n, 3, kf.data_ptr(), idx.data_ptr(), w.ptr(), out.data_ptr(), _stream()) == 0
        assert torch.equal(out.transpose(1, 2).contiguous().view(torch.int32), rows.view()[:, :, :c2].contiguous().view(torch.int32))
        w2, rows2 = _forward(lib, shape, rule, kr, sr, idx, d2)
        assert torch.equal(w2.raw, w.raw) and torch.equal(rows2.raw, rows.raw)


def test_forward_clamps_a_foreign_index():
    from samplenet_amd._lib import lib

    shape = (1, 4, 3, 2, 1)
    kr = torch.arange(1, 7, device="cuda", dtype=torch.float32).view(1, 3, 2)
    sr = torch.full((1, 4, 1), 9.0, device="cuda")
    idx = torch.tensor([[[0, 1, 2], [-7, 1, 2], [0, 1, 3], [99, -1, 2 ** 31 - 1]]], device="cuda", dtype=torch.int32)
    d2 = torch.ones(1, 4, 3, device="cuda")
    good = torch.tensor([[[0, 1, 2], [0, 1, 2], [0, 1, 2], [2, 0, 2]]], device="cuda", dtype=torch.int32)
    w, rows = _forward(lib, shape, 0, kr, sr, idx, d2)
    w2, rows2 = _forward(lib, shape, 0, kr, sr, good, d2)
    assert torch.equal(w.check("w"), w2.check("w")) and torch.equal(rows.check("rows"), rows2.check("rows"))


def _backward(lib, shape, w, g, start, order):
    b, n, m, c2, c1 = shape
    gk = Guarded((b, m, c2))
    rc = lib.sn_interp_rows_backward(b, n, m, c2, c1, w.data_ptr(), g.data_ptr(), start.data_ptr(), order.data_ptr(), gk.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return gk


@pytest.mark.parametrize("recipe", FR.INDEX_RECIPES)
@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.SHAPE_IDS)
def test_backward(shape, recipe):
    from samplenet_amd._lib import lib

    b, n, m, c2, c1 = shape
    for integer in (False, True):
        d = FR.backward_case(shape, recipe, integer)
        idx, w, g = dev(d["idx"]), dev(d["weights"]), dev(d["grad_rows"])
        start, order = _invert(lib, b, m, 3 * n, idx)
        assert np.array_equal(start.cpu().numpy(), d["start"]) and np.array_equal(order.cpu().numpy(), d["order"])
        gk = _backward(lib, shape, w, g, start, order)
        got = gk.check("grad_known").cpu().numpy()
        assert np.array_equal(_bits(got), _bits(d["grad32"])), "the sequential float32 sum"
        if integer:
            assert np.array_equal(got, d["grad64"])
        else:
            err = np.abs(got - d["grad64"])
            print("interp rows backward %s %s: worst error / bound %.3g" % ("x".join(map(str, shape)), recipe,
                                                                             (err / np.maximum(d["bound"], 1e-300)).max()))
            assert (err <= d["bound"]).all()
        # the channel-major inverted walk on transposed operands
        g_cm = g[:, :, :c2].transpose(1, 2).contiguous()
        gx = torch.empty(b, c2, m, device="cuda")
        assert lib.sn_weighted_gather_backward_inverted(b, c2, m, n, 3, w.data_ptr(), g_cm.data_ptr(), start.data_ptr(), order.data_ptr(),
                                                        gx.data_ptr(), _stream()) == 0
        assert torch.equal(gx.transpose(1, 2).contiguous().view(torch.int32), gk.view().view(torch.int32))
        assert torch.equal(_backward(lib, shape, w, g, start, order).raw, gk.raw)


def test_foreign_lists_are_clamped_and_skipped():
    from samplenet_amd._lib import lib

    shape = (1, 2, 4, 2, 1)                                    # ne = 6
    g = torch.arange(1, 7, device="cuda", dtype=torch.float32).view(1, 2, 3)
    w = torch.tensor([[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]], device="cuda")
    start = torch.tensor([[-5, 2, 2, 4, 99]], device="cuda", dtype=torch.int32)
    order = torch.tensor([[0, 7, 5, -1, 3, 2]], device="cuda", dtype=torch.int32)
    gk = _backward(lib, shape, w, g, start, order).check("grad_known").cpu().numpy()[0]
    gh, wh = g.cpu().numpy()[0, :, :2], w.cpu().numpy().reshape(6)
    want = np.stack([gh[0] * wh[0], np.zeros(2, np.float32), gh[1] * wh[5], gh[1] * wh[3] + gh[0] * wh[2]])   # entries 7 and -1 name nothing
    assert np.array_equal(gk, want)


def test_autograd_surface():
    from samplenet_amd import ops

    shape = (2, 257, 65, 16, 1)
    b, n, m, c2, c1 = shape
    d = FR.forward_case(shape, "rand")
    unknown, known = dev(d["unknown"]), dev(d["known"])
    dist2, idx = ops.three_nn(unknown, known, return_dist2=True)
    dist, idx1 = ops.three_nn(unknown, known)
    assert torch.equal(idx, idx1) and torch.equal(dist2, dev(d["d2"])) and torch.equal(dist, dev(np.sqrt(d["d2"])))
    kr, sr = dev(d["known_rows"]).requires_grad_(True), dev(d["skip_rows"]).requires_grad_(True)
    rng = np.random.default_rng(3)
    g = dev(rng.standard_normal((b, n, c2 + c1)).astype(np.float32))
    for rule_name, rule in (("sqrt_eps", R.SQRT_EPS), ("squared_clamp", R.SQUARED_CLAMP)):
        kr.grad = sr.grad = None
        rows = ops.interp_rows(kr, sr, idx, dist2, rule=rule_name)
        assert np.array_equal(_bits(rows.detach().cpu().numpy()), _bits(d["rows%d" % rule]))
        rows.backward(g)
        start, order = FR.G.invert(d["idx"], m)
        want = FR.backward32(m, c2, d["w%d" % rule], g.cpu().numpy(), start, order)
        assert np.array_equal(_bits(kr.grad.cpu().numpy()), _bits(want))
        assert torch.equal(sr.grad, g[:, :, c2:])
        # the weights are three_interpolate's: the default route's pieces give the same interpolated columns and gradient
        kf = kr.detach().transpose(1, 2).contiguous().requires_grad_(True)
        out = ops.three_interpolate(kf, idx, dev(d["w%d" % rule]))
        assert torch.equal(out.transpose(1, 2), rows.detach()[:, :, :c2])
        out.backward(g[:, :, :c2].transpose(1, 2).contiguous())
        assert torch.equal(kf.grad.transpose(1, 2), kr.grad)
        # a prebuilt inverse; only the requested gradients
        k2 = kr.detach().clone().requires_grad_(True)
        ops.interp_rows(k2, sr.detach(), idx, dist2, rule=rule_name, inverse=ops.gather_invert(idx, m)).backward(g)
        assert torch.equal(k2.grad, kr.grad)
    assert ops.interp_rows(kr.detach(), None, idx, dist2).shape == (b, n, c2)
    with pytest.raises(ValueError):
        ops.interp_rows(kr, sr, idx, dist2, rule="nearest")
    with pytest.raises(ValueError):
        ops.interp_rows(kr, sr[:, :5], idx, dist2)
    with pytest.raises(ValueError):
        ops.interp_rows(kr, sr, idx, dist2, inverse=(torch.zeros(b, m, device="cuda", dtype=torch.int32), torch.zeros(b, 3 * n, device="cuda", dtype=torch.int32)))


def test_beyond_the_inversion_bound_the_ordered_route_serves():
    from samplenet_amd import ops

    # ceil(16385 / 64) * 3 * 87400 > 2^26: no inverse exists; integer terms are exact in any order
    b, n, m, c2 = 1, 87400, 16385, 2
    assert not ops.gather_invert_supported(m, 3 * n) and ops.gather_invert_supported(m, 261123)
    rng = np.random.default_rng(9)
    idx = torch.from_numpy(rng.integers(0, m, (b, n, 3)).astype(np.int32)).cuda()
    d2 = torch.from_numpy(rng.integers(1, 4, (b, n, 3)).astype(np.float32)).cuda() ** 2
    kr = torch.from_numpy(rng.integers(-3, 4, (b, m, c2)).astype(np.float32)).cuda().requires_grad_(True)
    rows = ops.interp_rows(kr, None, idx, d2)
    g = torch.from_numpy(rng.integers(-3, 4, (b, n, c2)).astype(np.float32)).cuda()
    rows.backward(g)
    w = torch.from_numpy(R.weights(d2.cpu().numpy(), R.SQRT_EPS)).cuda().double()
    want = torch.zeros(b, m, c2, device="cuda", dtype=torch.float64)
    terms = (g.double()[:, :, None, :] * w[..., None]).view(b, 3 * n, c2)
    want.scatter_add_(1, idx.long().view(b, 3 * n, 1).expand(-1, -1, c2), terms)
    mag = torch.zeros_like(want).scatter_add_(1, idx.long().view(b, 3 * n, 1).expand(-1, -1, c2), terms.abs())
    cnt = torch.zeros(b, m, device="cuda", dtype=torch.float64).scatter_add_(1, idx.long().view(b, 3 * n), torch.ones(b, 3 * n, device="cuda", dtype=torch.float64))
    assert bool(((kr.grad.double() - want).abs() <= (cnt[..., None] + 1) * FR.U * mag).all())
    with pytest.raises(ValueError):
        ops.interp_rows(kr, None, idx, d2, inverse=(torch.zeros(b, m + 1, device="cuda", dtype=torch.int32), idx.view(b, -1)))


def test_the_direct_chain_captured_once_and_replayed():
    from samplenet_amd._lib import lib

    shape = (2, 257, 65, 16, 1)
    b, n, m, c2, c1 = shape
    d = FR.forward_case(shape, "rand")
    unknown, known, kr, sr = dev(d["unknown"]), dev(d["known"]), dev(d["known_rows"]), dev(d["skip_rows"])
    g = dev(np.random.default_rng(17).standard_normal((b, n, c2 + c1)).astype(np.float32))

    def buffers():
        f32, i32 = torch.float32, torch.int32
        spec = [((b, n, 3), i32), ((b, n, 3), f32), ((b, n, 3), f32), ((b, n, c2 + c1), f32), ((b, m + 1), i32), ((b, 3 * n), i32),
                ((b, m, c2), f32)]
        return [torch.full(s, -7, device="cuda", dtype=t) for s, t in spec]

    def chain(t):
        idx, d2, w, rows, start, order, gk = (x.data_ptr() for x in t)
        st = _stream()
        rcs = [lib.sn_three_nn(b, n, m, unknown.data_ptr(), known.data_ptr(), d2, None, idx, st),
               lib.sn_interp_rows_forward(b, n, m, c2, c1, 0, kr.data_ptr(), sr.data_ptr(), idx, d2, w, rows, st),
               lib.sn_gather_invert(b, m, 3 * n, idx, start, order, st),
               lib.sn_interp_rows_backward(b, n, m, c2, c1, w, g.data_ptr(), start, order, gk, st)]
        assert rcs == [0] * 4, lib.sn_last_error_string()

    eager = buffers()
    chain(eager)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(eager[3].cpu().numpy()), _bits(d["rows0"]))
    cap = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(cap)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in cap)            # capturing ran nothing
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(cap, eager):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, e.view(torch.int32) if e.dtype == torch.float32 else e)
        for t in cap:
            t.fill_(-7)

"""sn_ball_group_forward / sn_ball_group_backward on the device, called directly into poisoned and guarded buffers, then the autograd
surface over them (ops.ball_group, the pointnet2_utils stand-in's QueryAndGroup and GroupAll).

Forward: bit for bit the numpy restatement of tests/ball_ref.py, and bit for bit the composition sn_ball_query + sn_grouping_operation
+ one subtraction.  Backward: exact for integer-valued gradients (every partial sum is a small integer); for real gradients every
element within k * 2^-24 * sum|terms| of float64, k the number of terms added into that element counted from the reference's index
lists (a sum of k float32 terms in any order is off by at most (k - 1) 2^-24 sum|terms| to first order; nsample stands in for k
for the centre's gradient).  grad_new_xyz has one summation order: the same bits twice."""
import numpy as np
import pytest
import torch

import ball_ref as R
from cabi_ref import Guarded, bits as _bits, stream as _stream

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (500, 3, 17, 2): two queries per wave; n = 16384 / 16385: the last cloud size of the backward's LDS scatter and the first beyond it
SHAPES = [(1, 1, 1, 1), (2, 65, 7, 3), (2, 200, 33, 70), (3, 257, 9, 16), (500, 3, 17, 2), (1, 16384, 2, 2), (1, 16385, 2, 2)]
RECIPES = [r for r in R.RECIPES if r[0] in ("uniform-0.3", "grid-2", "clusters", "fill-lastn")]  # fill-lastn: the last point is a hit
CHANNELS = [(0, 1), (1, 0), (1, 1), (5, 0), (5, 1), (64, 0), (64, 1)]  # (c, use_xyz); (0, 0) has no output channel: refused
_REF = {}


def case(shape, recipe):
    key = (shape, recipe[0])
    if key not in _REF:
        P, Q, radius = R.make_case(shape, recipe)
        rng = np.random.default_rng(R._seed(shape, 11))
        feat = rng.standard_normal((shape[0], 64, shape[1])).astype(np.float32)
        refs = {rule: R.ball_query(P, Q, radius, shape[3], rule) for rule in R.RULES}
        for a in (P, Q, feat) + refs[0] + refs[1]:
            a.setflags(write=False)
        _REF[key] = (P, Q, radius, feat, refs)
    return _REF[key]


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _forward(lib, shape, c, u, radius, rule, dP, dQ, dF, with_cnt=True):
    b, n, m, ns = shape
    out, idx, cnt = Guarded((b, 3 * u + c, m, ns)), Guarded((b, m, ns), torch.int32), Guarded((b, m), torch.int32)
    rc = lib.sn_ball_group_forward(b, n, m, c, float(radius), ns, rule, u, dP.data_ptr(), dQ.data_ptr(), dF.data_ptr() if c else None,
                                   idx.ptr(), cnt.ptr() if with_cnt else None, out.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return out, idx, cnt


@pytest.mark.parametrize("c,u", CHANNELS)
@pytest.mark.parametrize("recipe", RECIPES, ids=[r[0] for r in RECIPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_forward_is_the_restatement_and_the_composition(shape, recipe, c, u):
    from samplenet_amd._lib import lib

    b, n, m, ns = shape
    P, Q, radius, feat, refs = case(shape, recipe)
    dP, dQ = dev(P), dev(Q)
    dF = dev(np.ascontiguousarray(feat[:, :c]))
    for rule in R.RULES:
        want_idx, want_cnt = refs[rule]
        out, idx, cnt = _forward(lib, shape, c, u, radius, rule, dP, dQ, dF)
        got = out.check("out").cpu().numpy()
        assert np.array_equal(idx.check("idx").cpu().numpy(), want_idx) and np.array_equal(cnt.check("cnt").cpu().numpy(), want_cnt)
        assert np.array_equal(_bits(got), _bits(R.group(P, Q, feat[:, :c], want_idx, u)))
        # the library's own composition: query, gather (the cloud as three channels, then the features), one subtraction
        qi = torch.empty(b, m, ns, device="cuda", dtype=torch.int32)
        assert lib.sn_ball_query(b, n, m, float(radius), ns, rule, dP.data_ptr(), 0, dQ.data_ptr(), 0, qi.data_ptr(), None, _stream()) == 0
        parts = []
        if u:
            cloud = dP.transpose(1, 2).contiguous()
            g = torch.empty(b, 3, m, ns, device="cuda")
            assert lib.sn_grouping_operation(b, 3, n, m, ns, cloud.data_ptr(), qi.data_ptr(), g.data_ptr(), _stream()) == 0
            parts.append(g - dQ.transpose(1, 2).unsqueeze(-1))
        if c:
            g = torch.empty(b, c, m, ns, device="cuda")
            assert lib.sn_grouping_operation(b, c, n, m, ns, dF.data_ptr(), qi.data_ptr(), g.data_ptr(), _stream()) == 0
            parts.append(g)
        assert torch.equal(torch.cat(parts, 1).view(torch.int32), out.view().view(torch.int32)) and torch.equal(qi, idx.view())
        out2, idx2, cnt2 = _forward(lib, shape, c, u, radius, rule, dP, dQ, dF)
        assert torch.equal(out2.raw, out.raw) and torch.equal(idx2.raw, idx.raw) and torch.equal(cnt2.raw, cnt.raw)


def test_forward_pts_cnt_may_be_null_and_no_channel_is_refused():
    from samplenet_amd._lib import lib

    shape = (2, 65, 7, 3)
    P, Q, radius, feat, refs = case(shape, RECIPES[0])
    dP, dQ, dF = dev(P), dev(Q), torch.from_numpy(np.ascontiguousarray(feat[:, :5])).cuda()
    out, idx, cnt = _forward(lib, shape, 5, 1, radius, R.SQUARED, dP, dQ, dF, with_cnt=False)
    assert cnt.untouched() and np.array_equal(_bits(out.check("out").cpu().numpy()), _bits(R.group(P, Q, feat[:, :5], refs[R.SQUARED][0], 1)))
    o = Guarded((2, 1, 7, 3))
    rc = lib.sn_ball_group_forward(2, 65, 7, 0, float(radius), 3, 1, 0, dP.data_ptr(), dQ.data_ptr(), None, idx.ptr(), None, o.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 10001 and o.untouched()


def _backward(lib, shape, c, u, idx, g, want=(True, True, True)):
    b, n, m, ns = shape
    gf, gx, gn = Guarded((b, max(c, 1), n)), Guarded((b, n, 3)), Guarded((b, m, 3))  # (c == 0: a buffer that must stay untouched)
    rc = lib.sn_ball_group_backward(b, n, m, c, ns, u, idx.data_ptr(), g.data_ptr(), gf.ptr() if want[0] and c else None,
                                    gx.ptr() if want[1] else None, gn.ptr() if want[2] else None, _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return gf, gx, gn


def _within(got, ref, k, sab, what):
    err = np.abs(got.astype(np.float64) - ref)
    bound = k * U * sab
    assert (err <= bound).all(), "%s: worst error / bound %.3g" % (what, (err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("c,u", CHANNELS)
@pytest.mark.parametrize("recipe", RECIPES, ids=[r[0] for r in RECIPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_backward(shape, recipe, c, u):
    from samplenet_amd._lib import lib

    b, n, m, ns = shape
    _, _, _, _, refs = case(shape, recipe)
    idx_np = refs[R.SQUARED][0]
    idx = dev(idx_np)
    rng = np.random.default_rng(R._seed(shape, 13 + c + u))
    ch = 3 * u + c
    # integer-valued gradients: exact, whatever the order of the atomics
    gi = rng.integers(-3, 4, (b, ch, m, ns)).astype(np.float32)
    ref = R.group_backward(n, c, u, idx_np, gi)
    gf, gx, gn = _backward(lib, shape, c, u, idx, torch.from_numpy(gi).cuda())
    assert np.array_equal(gx.check("grad_xyz").cpu().numpy(), ref["grad_xyz"])
    assert np.array_equal(gn.check("grad_new_xyz").cpu().numpy(), ref["grad_new_xyz"])
    if c:
        assert np.array_equal(gf.check("grad_features").cpu().numpy(), ref["grad_features"])
    else:
        assert gf.untouched()
    # each output alone: the same numbers, and nothing else is written (an output that is not requested is a NULL pointer)
    for which in range(3):
        if which == 0 and not c:
            continue
        one = _backward(lib, shape, c, u, idx, torch.from_numpy(gi).cuda(), want=tuple(w == which for w in range(3)))
        for w, (buf, full) in enumerate(zip(one, (gf, gx, gn))):
            assert torch.equal(buf.raw, full.raw) if w == which else buf.untouched(), (which, w)
    # real gradients: element by element against float64
    gr = rng.standard_normal((b, ch, m, ns)).astype(np.float32)
    ref = R.group_backward(n, c, u, idx_np, gr)
    dg = torch.from_numpy(gr).cuda()
    gf, gx, gn = _backward(lib, shape, c, u, idx, dg)
    mult = ref["mult"]
    _within(gx.check("grad_xyz").cpu().numpy(), ref["grad_xyz"], mult[:, :, None], ref["abs_xyz"], "grad_xyz")
    _within(gn.check("grad_new_xyz").cpu().numpy(), ref["grad_new_xyz"], ns, ref["abs_new_xyz"], "grad_new_xyz")
    if c:
        _within(gf.check("grad_features").cpu().numpy(), ref["grad_features"], mult[:, None, :], ref["abs_features"], "grad_features")
    _, _, gn2 = _backward(lib, shape, c, u, idx, dg)
    assert torch.equal(gn2.raw, gn.raw)  # one summation order: bit-identical


def test_query_and_group_through_autograd():
    from samplenet_amd import ops
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    shape, c = (2, 200, 33, 70), 5
    b, n, m, ns = shape
    P, Q, radius, feat, refs = case(shape, RECIPES[0])
    idx_np = refs[R.SQUARED][0]
    rng = np.random.default_rng(3)
    w_np = rng.standard_normal((b, 3 + c, m, ns)).astype(np.float32)
    xyz, new, f = (dev(np.ascontiguousarray(a)).requires_grad_(True) for a in (P, Q, feat[:, :c]))
    w = torch.from_numpy(w_np).cuda()
    out = PU.QueryAndGroup(float(radius), ns)(xyz, new, f)
    assert out.shape == (b, 3 + c, m, ns)
    (out * w).sum().backward()
    # the torch.gather composition on the reference's indices, in float64
    li = dev(idx_np).long().view(b, 1, m * ns)
    x64, q64, f64 = (t.detach().double().requires_grad_(True) for t in (xyz, new, f))
    gxyz = torch.gather(x64.transpose(1, 2), 2, li.expand(b, 3, m * ns)).view(b, 3, m, ns) - q64.transpose(1, 2).unsqueeze(-1)
    gfeat = torch.gather(f64, 2, li.expand(b, c, m * ns)).view(b, c, m, ns)
    ref_out = torch.cat([gxyz, gfeat], 1)
    assert torch.equal(out.detach(), ref_out.detach().float())  # a float32 difference of float32 values, rounded from the exact one
    (ref_out * w.double()).sum().backward()
    ref = R.group_backward(n, c, 1, idx_np, w_np)
    mult = ref["mult"]
    for got, r64, k, sab in ((xyz.grad, x64.grad, mult[:, :, None], ref["abs_xyz"]), (new.grad, q64.grad, ns, ref["abs_new_xyz"]),
                             (f.grad, f64.grad, mult[:, None, :], ref["abs_features"])):
        _within(got.cpu().numpy(), r64.cpu().numpy(), k, sab, "autograd")
    # ops.ball_group: the indices come back on request and carry no gradient; features alone get a gradient when only they ask
    f2 = f.detach().clone().requires_grad_(True)
    out2, idx, cnt = ops.ball_group(float(radius), ns, xyz.detach(), new.detach(), f2, use_xyz=False, rule="squared", return_idx=True)
    assert out2.shape == (b, c, m, ns) and torch.equal(out2, out[:, 3:].detach()) and not idx.requires_grad
    assert np.array_equal(idx.cpu().numpy(), idx_np) and np.array_equal(cnt.cpu().numpy(), refs[R.SQUARED][1])
    out2.backward(w[:, 3:])
    _within(f2.grad.cpu().numpy(), f64.grad.cpu().numpy(), mult[:, None, :], ref["abs_features"], "features only")
    # no features: the three coordinate channels
    assert torch.equal(PU.QueryAndGroup(float(radius), ns)(xyz.detach(), new.detach()), out[:, :3].detach())
    # the reference's rule through ops
    o3, i3, _ = ops.ball_group(float(radius), ns, xyz.detach(), new.detach(), rule="sqrt", return_idx=True)
    assert np.array_equal(i3.cpu().numpy(), refs[R.SQRT][0])


def test_group_all():
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    xyz = torch.rand(2, 9, 3, device="cuda", requires_grad=True)
    f = torch.rand(2, 4, 9, device="cuda", requires_grad=True)
    out = PU.GroupAll()(xyz, None, f)
    assert out.shape == (2, 7, 1, 9) and torch.equal(out[:, :3, 0], xyz.transpose(1, 2)) and torch.equal(out[:, 3:, 0], f)
    out.sum().backward()
    assert bool((xyz.grad == 1).all()) and bool((f.grad == 1).all())
    assert torch.equal(PU.GroupAll(use_xyz=False)(xyz, None, f), f.unsqueeze(2)) and PU.GroupAll()(xyz, None).shape == (2, 3, 1, 9)

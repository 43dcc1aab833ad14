"""sn_ball_group_rows_forward / sn_group_rows_backward on the device, called directly into poisoned and guarded buffers, then the
autograd surface over them (ops.ball_group_rows) and one capture of the direct chain.

Forward: rows / idx / pts_cnt bit for bit the numpy restatement (tests/group_rows_ref.py on tests/ball_ref.py's index rows) and bit
for bit sn_ball_group_forward's output permuted.  Backward: grad_features / grad_xyz bit for bit the sequential float32 sum over
ascending entries, and every element within k * 2^-24 * sum|terms| of float64, k the length of that element's list (a sum of k
float32 terms is off by at most (k - 1) 2^-24 sum|terms| to first order); grad_new_xyz bit for bit sn_ball_group_backward's on the
permuted gradient and the lane-strided + xor-tree restatement; every case twice with equal bits; every combination of NULL outputs
leaves the others as they were and every guard intact."""
import itertools

import numpy as np
import pytest
import torch

import ball_ref as R
import group_rows_ref as GR
from cabi_ref import Guarded, bits as _bits, invert as _invert, stream as _stream

pytestmark = pytest.mark.gpu

CMAX = 131
BAD_ARGUMENT = 10001
_REF, _GRAD = {}, {}
_IDS = ["x".join(map(str, s)) for s in GR.SHAPES]


def case(shape, recipe):
    key = (shape, recipe[0])
    if key not in _REF:
        P, Q, radius = R.make_case(shape, recipe)
        feat = np.random.default_rng(R._seed(shape, 11)).standard_normal((shape[0], shape[1], CMAX)).astype(np.float32)  # (b,n,c) rows
        refs = {rule: R.ball_query(P, Q, radius, shape[3], rule) for rule in R.RULES}
        for a in (P, Q, feat) + refs[0] + refs[1]:
            a.setflags(write=False)
        _REF[key] = (P, Q, radius, feat, refs)
    return _REF[key]


def grad_case(shape, recipe):
    """the gradient at all 3 + CMAX columns with its sequential sums and float64 references, shared by the channel cases (the
    columns are summed independently of one another, so a case with fewer columns is a slice)"""
    key = (shape, recipe[0])
    if key not in _GRAD:
        b, n, m, ns = shape
        idx = case(shape, recipe)[4][R.SQUARED][0].reshape(b, m * ns).astype(np.int64)
        g = np.random.default_rng(R._seed(shape, 13)).standard_normal((b, m * ns, 3 + CMAX)).astype(np.float32)
        seq = GR.sequential_sum(n, idx, g)
        s64, sab, mult = GR.scatter_f64(n, idx, g)
        centre = GR.centre_sum(g[:, :, :3].reshape(b, m, ns, 3))
        for a in (idx, g, seq, s64, sab, mult, centre):
            a.setflags(write=False)
        _GRAD[key] = (idx, g, seq, s64, sab, mult, centre)
    return _GRAD[key]


def cols(c, u):
    return ([0, 1, 2] if u else []) + list(range(3, 3 + c))


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _forward(lib, shape, c, u, radius, rule, dP, dQ, dF, with_cnt=True):
    b, n, m, ns = shape
    rows, idx, cnt = Guarded((b, m, ns, 3 * u + c)), Guarded((b, m, ns), torch.int32), Guarded((b, m), torch.int32)
    rc = lib.sn_ball_group_rows_forward(b, n, m, c, float(radius), ns, rule, u, dP.data_ptr(), dQ.data_ptr(), dF.data_ptr() if c else None,
                                        idx.ptr(), cnt.ptr() if with_cnt else None, rows.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return rows, idx, cnt


@pytest.mark.parametrize("c,u", GR.CHANNELS)
@pytest.mark.parametrize("recipe", GR.RECIPES, ids=[r[0] for r in GR.RECIPES])
@pytest.mark.parametrize("shape", GR.SHAPES, ids=_IDS)
def test_forward_is_the_restatement_and_ball_group_permuted(shape, recipe, c, u):
    from samplenet_amd._lib import lib

    b, n, m, ns = shape
    P, Q, radius, feat, refs = case(shape, recipe)
    dP, dQ = dev(P), dev(Q)
    dF = dev(np.ascontiguousarray(feat[:, :, :c]))
    dFt = dF.transpose(1, 2).contiguous()                      # (b,c,n) for sn_ball_group_forward
    for rule in R.RULES:
        want_idx, want_cnt = refs[rule]
        rows, idx, cnt = _forward(lib, shape, c, u, radius, rule, dP, dQ, dF)
        got = rows.check("rows").cpu().numpy()
        assert np.array_equal(idx.check("idx").cpu().numpy(), want_idx) and np.array_equal(cnt.check("cnt").cpu().numpy(), want_cnt)
        assert np.array_equal(_bits(got), _bits(GR.group_rows(P, Q, feat[:, :, :c], want_idx, u)))
        out = torch.empty(b, 3 * u + c, m, ns, device="cuda")
        i2 = torch.empty(b, m, ns, device="cuda", dtype=torch.int32)
        assert lib.sn_ball_group_forward(b, n, m, c, float(radius), ns, rule, u, dP.data_ptr(), dQ.data_ptr(), dFt.data_ptr() if c else None,
                                         i2.data_ptr(), None, out.data_ptr(), _stream()) == 0
        assert torch.equal(out.permute(0, 2, 3, 1).contiguous().view(torch.int32), rows.view().view(torch.int32)) and torch.equal(i2, idx.view())
        rows2, idx2, cnt2 = _forward(lib, shape, c, u, radius, rule, dP, dQ, dF)
        assert torch.equal(rows2.raw, rows.raw) and torch.equal(idx2.raw, idx.raw) and torch.equal(cnt2.raw, cnt.raw)


def test_forward_pts_cnt_may_be_null_and_the_argument_errors():
    from samplenet_amd._lib import lib

    shape = (2, 70, 5, 3)
    b, n, m, ns = shape
    P, Q, radius, feat, refs = case(shape, GR.RECIPES[0])
    dP, dQ, dF = dev(P), dev(Q), dev(np.ascontiguousarray(feat[:, :, :5]))
    rows, idx, cnt = _forward(lib, shape, 5, 1, radius, R.SQUARED, dP, dQ, dF, with_cnt=False)
    assert cnt.untouched() and np.array_equal(_bits(rows.check("rows").cpu().numpy()), _bits(GR.group_rows(P, Q, feat[:, :, :5], refs[R.SQUARED][0], 1)))
    o, gi = Guarded((b, m, ns, 8)), Guarded((b, m, ns), torch.int32)
    p, q, f, st = dP.data_ptr(), dQ.data_ptr(), dF.data_ptr(), _stream()
    fwd = lib.sn_ball_group_rows_forward
    bad = [fwd(b, n, m, 0, 0.3, ns, 1, 0, p, q, None, gi.ptr(), None, o.ptr(), st),      # no output column
           fwd(b, n, m, 5, 0.3, 0, 1, 1, p, q, f, gi.ptr(), None, o.ptr(), st),          # nsample < 1
           fwd(b, n, m, 5, 0.3, ns, 2, 1, p, q, f, gi.ptr(), None, o.ptr(), st),         # unknown rule
           fwd(b, n, m, 5, 0.3, ns, 1, 2, p, q, f, gi.ptr(), None, o.ptr(), st),         # unknown use_xyz
           fwd(b, n, m, 5, 0.3, ns, 1, 1, p, q, None, gi.ptr(), None, o.ptr(), st),      # features NULL with c > 0
           fwd(b, n, m, 5, 0.3, ns, 1, 1, p, q, f, gi.ptr(), None, None, st),            # rows NULL
           fwd(b, 0, m, 5, 0.3, ns, 1, 1, p, q, f, gi.ptr(), None, o.ptr(), st),         # an empty dataset with queries
           fwd(-1, n, m, 5, 0.3, ns, 1, 1, p, q, f, gi.ptr(), None, o.ptr(), st)]
    assert bad == [BAD_ARGUMENT] * len(bad)
    assert fwd(0, n, m, 5, 0.3, ns, 1, 1, None, None, None, None, None, None, st) == 0   # no-ops
    assert fwd(b, n, 0, 5, 0.3, ns, 1, 1, None, None, None, None, None, None, st) == 0
    bwd = lib.sn_group_rows_backward
    s_, o_, g_ = Guarded((b, n + 1), torch.int32), Guarded((b, m * ns), torch.int32), torch.zeros(b, m * ns, 8, device="cuda")
    gf, gx, gn = Guarded((b, n, 5)), Guarded((b, n, 3)), Guarded((b, m, 3))
    bad = [bwd(b, n, m, 0, ns, 0, None, s_.ptr(), o_.ptr(), g_.data_ptr(), gf.ptr(), gx.ptr(), gn.ptr(), st),
           bwd(b, n, m, 5, 0, 1, None, s_.ptr(), o_.ptr(), g_.data_ptr(), gf.ptr(), gx.ptr(), gn.ptr(), st),
           bwd(b, n, m, 5, ns, 3, None, s_.ptr(), o_.ptr(), g_.data_ptr(), gf.ptr(), gx.ptr(), gn.ptr(), st),
           bwd(b, n, m, 5, ns, 1, None, s_.ptr(), o_.ptr(), None, gf.ptr(), gx.ptr(), gn.ptr(), st),
           bwd(b, n, m, 5, ns, 1, None, None, o_.ptr(), g_.data_ptr(), gf.ptr(), None, None, st),
           bwd(b, n, m, 5, ns, 1, None, s_.ptr(), None, g_.data_ptr(), None, gx.ptr(), None, st),
           bwd(b, n, 1 << 20, 5, 1 << 12, 1, None, s_.ptr(), o_.ptr(), g_.data_ptr(), gf.ptr(), gx.ptr(), gn.ptr(), st)]
    torch.cuda.synchronize()
    assert bad == [BAD_ARGUMENT] * len(bad)
    assert bwd(0, n, m, 5, ns, 1, None, None, None, None, None, None, None, st) == 0
    assert all(t.untouched() for t in (o, gi, gf, gx, gn, s_, o_))


def _backward(lib, shape, c, u, idx, inv, g, want=(True, True, True)):
    b, n, m, ns = shape
    gf, gx, gn = Guarded((b, n, max(c, 1))), Guarded((b, n, 3)), Guarded((b, m, 3))  # (c == 0: a buffer that must stay untouched)
    rc = lib.sn_group_rows_backward(b, n, m, c, ns, u, idx.data_ptr(), inv[0].data_ptr(), inv[1].data_ptr(), g.data_ptr(),
                                    gf.ptr() if want[0] and c else None, gx.ptr() if want[1] else None, gn.ptr() if want[2] else None, _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return gf, gx, gn


def _within(got, ref, k, sab, what):
    err = np.abs(got.astype(np.float64) - ref)
    bound = k * GR.U * sab
    print("%s: worst error / bound %.3g" % (what, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("c,u", GR.CHANNELS)
@pytest.mark.parametrize("recipe", GR.RECIPES, ids=[r[0] for r in GR.RECIPES])
@pytest.mark.parametrize("shape", GR.SHAPES, ids=_IDS)
def test_backward(shape, recipe, c, u):
    from samplenet_amd._lib import lib

    b, n, m, ns = shape
    idx_np, g_all, seq, s64, sab, mult, centre = grad_case(shape, recipe)
    cc = cols(c, u)
    g_np = np.ascontiguousarray(g_all[:, :, cc])
    idx, g = dev(idx_np.astype(np.int32)), dev(g_np)
    inv = _invert(lib, b, n, m * ns, idx)
    gf, gx, gn = _backward(lib, shape, c, u, idx, inv, g)
    got_x, got_n = gx.check("grad_xyz").cpu().numpy(), gn.check("grad_new_xyz").cpu().numpy()
    if u:
        assert np.array_equal(_bits(got_x), _bits(seq[:, :, :3]))
        _within(got_x, s64[:, :, :3], mult[:, :, None], sab[:, :, :3], "grad_xyz")
        assert np.array_equal(_bits(got_n), _bits(centre))
    else:
        assert not _bits(got_x).any() and not _bits(got_n).any()   # zeros, +0
    if c:
        got_f = gf.check("grad_features").cpu().numpy()
        assert np.array_equal(_bits(got_f), _bits(seq[:, :, 3:3 + c]))
        _within(got_f, s64[:, :, 3:3 + c], mult[:, :, None], sab[:, :, 3:3 + c], "grad_features")
    else:
        assert gf.untouched()
    # the centre's gradient of sn_ball_group_backward on the permuted gradient
    gn_old = torch.empty(b, m, 3, device="cuda")
    g_cm = g.view(b, m, ns, 3 * u + c).permute(0, 3, 1, 2).contiguous()
    assert lib.sn_ball_group_backward(b, n, m, c, ns, u, idx.data_ptr(), g_cm.data_ptr(), None, None, gn_old.data_ptr(), _stream()) == 0
    assert torch.equal(gn_old.view(torch.int32), gn.view().view(torch.int32))
    # twice: the same bits; every combination of NULL outputs: the others as they were, nothing else written
    for want in itertools.product((True, False), repeat=3):
        one = _backward(lib, shape, c, u, idx, inv, g, want=want)
        for w, (buf, full) in enumerate(zip(one, (gf, gx, gn))):
            assert torch.equal(buf.raw, full.raw) if want[w] and (w or c) else buf.untouched(), (want, w)


def test_foreign_lists_are_clamped_and_skipped():
    from samplenet_amd._lib import lib

    b, n, m, ns, c = 1, 4, 2, 3, 2
    g = torch.arange(1, 1 + m * ns * (3 + c), device="cuda", dtype=torch.float32).view(b, m * ns, 3 + c)
    start = torch.tensor([[-5, 2, 2, 4, 99]], device="cuda", dtype=torch.int32)
    order = torch.tensor([[0, 7, 5, -1, 3, 2]], device="cuda", dtype=torch.int32)
    idx = torch.zeros(b, m, ns, device="cuda", dtype=torch.int32)
    gf, gx, _ = _backward(lib, (b, n, m, ns), c, 1, idx, (start, order), g, want=(True, True, False))
    gh = g.cpu().numpy()[0]
    want = np.stack([gh[0], np.zeros(5, np.float32), gh[5], gh[3] + gh[2]])   # entries 7 and -1 name nothing
    assert np.array_equal(gx.check("gx").cpu().numpy()[0], want[:, :3]) and np.array_equal(gf.check("gf").cpu().numpy()[0], want[:, 3:])


def test_autograd_surface_both_routes():
    from samplenet_amd import ops

    # the inverted route: the entries' bits through autograd, only the requested gradients
    shape, c = (2, 200, 33, 69), 5
    b, n, m, ns = shape
    P, Q, radius, feat, refs = case(shape, GR.RECIPES[0])
    idx_np, g_all, seq, s64, sab, mult, centre = grad_case(shape, GR.RECIPES[0])
    xyz, new, f = (dev(np.ascontiguousarray(a)).requires_grad_(True) for a in (P, Q, feat[:, :, :c]))
    rows, idx, cnt = ops.ball_group_rows(float(radius), ns, xyz, new, f, return_idx=True)
    assert rows.shape == (b, m, ns, 3 + c) and not idx.requires_grad and np.array_equal(idx.cpu().numpy(), refs[R.SQUARED][0])
    assert torch.equal(rows.detach(), ops.ball_group(float(radius), ns, xyz, new, f.transpose(1, 2).contiguous()).permute(0, 2, 3, 1).detach())
    w = dev(np.ascontiguousarray(g_all[:, :, cols(c, 1)])).view(b, m, ns, 3 + c)
    rows.backward(w)
    assert np.array_equal(_bits(xyz.grad.cpu().numpy()), _bits(seq[:, :, :3])) and np.array_equal(_bits(f.grad.cpu().numpy()), _bits(seq[:, :, 3:3 + c]))
    assert np.array_equal(_bits(new.grad.cpu().numpy()), _bits(centre))
    f2 = f.detach().clone().requires_grad_(True)
    r2 = ops.ball_group_rows(float(radius), ns, xyz.detach(), new.detach(), f2, use_xyz=False)
    r2.backward(w[..., 3:].contiguous())
    assert torch.equal(f2.grad, f.grad)
    with pytest.raises(ValueError):
        ops.ball_group_rows(0.3, 4, xyz, new, None, use_xyz=False)
    # beyond sn_gather_invert_supported (ceil(16385 / 64) * 262144 > 2^26): the atomic route on the permuted gradient; integer
    # terms are exact in any order
    n, m, ns = 16385, 4096, 64
    assert not ops.gather_invert_supported(n, m * ns) and ops.gather_invert_supported(n, 261123)
    rng = np.random.default_rng(5)
    xyz = torch.from_numpy(rng.random((1, n, 3), dtype=np.float32)).cuda().requires_grad_(True)
    new = xyz.detach()[:, :m].clone().requires_grad_(True)
    f = torch.from_numpy(rng.standard_normal((1, n, 1)).astype(np.float32)).cuda().requires_grad_(True)
    rows, idx, _ = ops.ball_group_rows(0.05, ns, xyz, new, f, return_idx=True)
    gi = torch.from_numpy(rng.integers(-3, 4, (1, m, ns, 4)).astype(np.float32)).cuda()
    rows.backward(gi)
    s64 = GR.scatter_f64(n, idx.cpu().numpy().reshape(1, m * ns).astype(np.int64), gi.cpu().numpy().reshape(1, m * ns, 4))[0]
    assert np.array_equal(xyz.grad.cpu().numpy(), s64[:, :, :3]) and np.array_equal(f.grad.cpu().numpy(), s64[:, :, 3:])
    assert np.array_equal(new.grad.cpu().numpy(), -gi.cpu().numpy().astype(np.float64).sum(2)[:, :, :3])


def test_the_direct_chain_captured_once_and_replayed():
    from samplenet_amd._lib import lib

    shape, c = (3, 257, 9, 16), 5
    b, n, m, ns = shape
    Ci, G = 3 + c, b * m
    P, Q, radius, feat, _ = case(shape, GR.RECIPES[0])
    dP, dQ, dF = dev(P), dev(Q), dev(np.ascontiguousarray(feat[:, :, :c]))
    rng = np.random.default_rng(17)
    g_rows = dev(rng.standard_normal((b, m * ns, Ci)).astype(np.float32))
    g_pool = dev(rng.standard_normal((G, Ci)).astype(np.float32))
    coef = dev(np.stack([np.where(np.arange(Ci) % 2, -1.5, 0.75), np.full(Ci, 0.1), np.zeros(Ci), np.ones(Ci)]).astype(np.float32))
    nblk = lib.sn_group_pool_stats_blocks(G)

    def buffers():
        f32, i32 = torch.float32, torch.int32
        spec = [((b, m, ns, Ci), f32), ((b, m, ns), i32), ((b, m), i32), ((b, n + 1), i32), ((b, m * ns), i32), ((b, n, c), f32),
                ((b, n, 3), f32), ((b, m, 3), f32), ((G, Ci), f32), ((G, Ci), i32), ((G, Ci), f32), ((G, Ci), f32), ((nblk, 2, Ci), f32)]
        return [torch.full(s, -7, device="cuda", dtype=d) for s, d in spec]

    def chain(t):
        rows, idx, cnt, start, order, gf, gx, gn, pooled, argsel, zsel, gsel, stats = (x.data_ptr() for x in t)
        st = _stream()
        rcs = [lib.sn_ball_group_rows_forward(b, n, m, c, float(radius), ns, R.SQUARED, 1, dP.data_ptr(), dQ.data_ptr(), dF.data_ptr(),
                                              idx, cnt, rows, st),
               lib.sn_gather_invert(b, n, m * ns, idx, start, order, st),
               lib.sn_group_rows_backward(b, n, m, c, ns, 1, idx, start, order, g_rows.data_ptr(), gf, gx, gn, st),
               lib.sn_group_pool_forward(G, ns, Ci, rows, coef.data_ptr(), pooled, argsel, zsel, st),
               lib.sn_group_pool_backward(G, Ci, g_pool.data_ptr(), pooled, zsel, gsel, stats, st)]
        assert rcs == [0] * 5, lib.sn_last_error_string()

    eager = buffers()
    chain(eager)
    torch.cuda.synchronize()
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

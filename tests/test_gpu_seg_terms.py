"""sn_segmentation_terms_forward / _backward called directly, against the fp64 restatement and the counted bounds of
tests/seg_terms_ref.py.  Every tensor sits in a guarded buffer (tests/cabi_ref.py: poisoned words on both sides, checked after every
call; inputs compared bit for bit afterwards).  pred and cloud_counts involve no arithmetic: they are compared bit for bit with
numpy's argmax and counts on the same float32 logits.  Every test prints its largest observed error beside the bound (`pytest -s`;
recorded in profiles/seg/errors.txt)."""
import itertools

import numpy as np
import pytest
import torch

import cabi_ref as G
import seg_terms_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def _report(what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if err.size:
        i = np.argmax(err / np.maximum(bound, 1e-300))
        print("SEG_ERR %-52s observed %.3e  bound %.3e  ratio %.3f" % (what, err.flat[i], bound.flat[i], err.flat[i] / max(bound.flat[i], 1e-300)))


def _within(what, got, ref, bound):
    """finite reference entries under the bound; the others non-finite of the same kind"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert R.same_kind(got, ref), "%s: non-finite results differ from the restatement's" % what
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    bound = np.broadcast_to(bound, ref.shape)[fin]
    _report(what, err, bound)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d outside the bound, worst %.3e against %.3e" % (what, bad.sum(), err[bad].max(), bound[bad].min())


def _same_bits(buf, arr):
    return np.array_equal(buf.numpy().view(np.int32), np.ascontiguousarray(arr).view(np.int32))


def _workspace(lib, R_, C):
    n = lib.sn_segmentation_terms_workspace_bytes(R_, C)
    assert n == 16 * R.blocks(R_, C)
    return G.Guarded((max(n // 4, 1),), torch.int32)


def forward(x, lab, N, w=None, want=(True, True, True, True)):
    """One guarded call -> [ce, pred, cloud_counts, means] as numpy (None where not asked for)."""
    lib, check = _lib()
    R_, C = x.shape
    gx, gl = G.Guarded((R_, C), fill=x), G.Guarded((R_,), torch.int32, fill=lab)
    gw = None if w is None else G.Guarded((C,), fill=w)
    kinds = (((R_,), torch.float32), ((R_,), torch.int32), ((R_ // N, C, 3), torch.int32), ((3,), torch.float32))
    outs = [G.Guarded(shape, dt) if wanted else None for (shape, dt), wanted in zip(kinds, want)]
    ws = _workspace(lib, R_, C)
    check(lib.sn_segmentation_terms_forward(R_, N, C, gx.ptr(), gl.ptr(), G.arg(gw), *[G.arg(o) for o in outs], ws.ptr(), None),
          "sn_segmentation_terms_forward")
    torch.cuda.synchronize()
    assert gx.guards_intact() and gl.guards_intact() and ws.guards_intact() and _same_bits(gx, x) and _same_bits(gl, lab)
    assert gw is None or (gw.guards_intact() and _same_bits(gw, w))
    return [None if o is None else o.check("forward output").cpu().numpy().copy() for o in outs]


def backward(x, lab, w, means, gm, gce):
    lib, check = _lib()
    R_, C = x.shape
    gx, gl = G.Guarded((R_, C), fill=x), G.Guarded((R_,), torch.int32, fill=lab)
    arrays = (w, means, gm, gce)
    ins = [None if a is None else G.Guarded(a.shape, fill=a) for a in arrays]
    out = G.Guarded((R_, C))
    check(lib.sn_segmentation_terms_backward(R_, C, gx.ptr(), gl.ptr(), *[G.arg(i) for i in ins], out.ptr(), None),
          "sn_segmentation_terms_backward")
    torch.cuda.synchronize()
    assert all(i is None or i.guards_intact() for i in ins) and gx.guards_intact() and gl.guards_intact()
    assert _same_bits(gx, x) and _same_bits(gl, lab) and all(i is None or _same_bits(i, a) for i, a in zip(ins, arrays))
    return out.check("g_logits").cpu().numpy().copy()


def _check_forward(tag, x, lab, N, w, got):
    ce, pred, counts, means = got
    T = R.terms(x, lab, N, w)
    C = x.shape[1]
    valid = (lab >= 0) & (lab < C)
    if pred is not None:
        assert pred.dtype == np.int32 and np.array_equal(pred, np.argmax(x, axis=1).astype(np.int32)), tag
    if counts is not None:
        assert counts.dtype == np.int32 and np.array_equal(counts, T["cloud_counts"].astype(np.int32)), tag
    if ce is not None:
        _within(tag + " ce", ce, T["ce"], R.bound_ce(T))
        assert np.array_equal(G.bits(ce[~valid]), np.zeros(int((~valid).sum()), dtype=np.int32)), tag + ": an ignored row's ce is not +0"
    if means is not None:
        b = R.bound_means(T)
        if np.isfinite(T["ce"]).all() and np.isfinite(T["means"][0]):
            _within(tag + " means[0]", means[:1], T["means"][:1], b[0])
        else:
            assert R.same_kind(means[:1], T["means"][:1]), tag
        assert abs(float(means[1]) - T["means"][1]) <= b[1], tag
        if w is None:
            assert float(means[2]) == T["means"][2] == valid.sum(), tag  # the count, exact
        else:
            _within(tag + " means[2]", means[2:], T["means"][2:], b[2])
    return T


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("C", R.CLASSES)
@pytest.mark.parametrize("B,N", R.CLOUDS)
def test_forward_and_backward_against_fp64(recipe, B, N, C):
    x, lab = R.make_case(recipe, B, N, C)
    gm, gce = R.upstream_case(B * N)
    for kind in R.WEIGHTS:
        w = R.make_weights(kind, C)
        tag = "%s w=%s (%dx%d,%d)" % (recipe, kind, B, N, C)
        got = forward(x, lab, N, w)
        T = _check_forward(tag, x, lab, N, w, got)
        if C == 1 and recipe == "random":
            assert np.array_equal(got[0], np.zeros(B * N, dtype=np.float32))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, forward(x, lab, N, w))), "two runs differ"
        parts = (("both", gm, gce), ("means", gm, None), ("ce", None, gce)) if kind == "given" else (("both", gm, gce),)
        for name, g_means, g_ce in parts:
            g = backward(x, lab, w, got[3], g_means, g_ce)
            valid = (lab >= 0) & (lab < C)
            assert not G.bits(g[~valid]).any(), tag + ": an ignored row's gradient is not +0"
            if np.isfinite(T["means"][2]) and (T["means"][2] > 0 or g_means is None):
                _within("%s g_logits[%s]" % (tag, name), g, R.backward(T, g_means, g_ce), R.bound_backward(T, g_means, g_ce))
            if name == "both":
                assert np.array_equal(g, backward(x, lab, w, got[3], g_means, g_ce), equal_nan=True), "two runs differ"


@pytest.mark.parametrize("B,N,C", [(3, 7, 13), (2, 100, 65), (2, 1027, 13), (5, 257, 130)])
def test_every_null_output_combination(B, N, C):
    x, lab = R.make_case("mixed_ignored", B, N, C)
    w = R.make_weights("given", C)
    full = forward(x, lab, N, w)
    for want in itertools.product((False, True), repeat=4):
        got = forward(x, lab, N, w, want)
        _check_forward("null %s (%dx%d,%d)" % ("".join("x" if v else "-" for v in want), B, N, C), x, lab, N, w, got)
        for v, a, b in zip(want, got, full):
            assert not v or np.array_equal(a, b, equal_nan=True)  # what is asked for does not depend on what else is


def test_means_without_a_workspace_and_the_refused_range():
    lib, check = _lib()
    outs = [G.Guarded((4,)), G.Guarded((4,), torch.int32), G.Guarded((1, 5, 3), torch.int32), G.Guarded((3,))]
    ws, g = G.Guarded((16,), torch.int32), G.Guarded((4, 5))
    check(lib.sn_segmentation_terms_forward(0, 4, 5, None, None, None, *[o.ptr() for o in outs], ws.ptr(), None), "forward R = 0")
    check(lib.sn_segmentation_terms_backward(0, 5, None, None, None, None, None, None, g.ptr(), None), "backward R = 0")
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and g.untouched() and ws.untouched()
    x, lab = G.Guarded((4, 5), fill=np.zeros((4, 5), np.float32)), G.Guarded((4,), torch.int32, fill=np.zeros(4, np.int32))
    fwd = lambda R_, rpc, C, lg=x.ptr(), lb=lab.ptr(), mw=None: lib.sn_segmentation_terms_forward(  # noqa: E731
        R_, rpc, C, lg, lb, None, outs[0].ptr(), None, None, outs[3].ptr(), mw, None)
    assert fwd(4, 4, 0) == G.BAD_ARGUMENT and fwd(-1, 1, 5) == G.BAD_ARGUMENT and fwd(4, 0, 5) == G.BAD_ARGUMENT
    assert fwd(4, 3, 5, mw=ws.ptr()) == G.BAD_ARGUMENT          # rows_per_cloud does not divide R
    assert fwd(1 << 20, 1 << 20, 1 << 11, mw=ws.ptr()) == G.BAD_ARGUMENT  # R * C = 2^31
    assert fwd(4, 4, 5, lg=None, mw=ws.ptr()) == G.BAD_ARGUMENT and fwd(4, 4, 5, lb=None, mw=ws.ptr()) == G.BAD_ARGUMENT
    assert fwd(4, 4, 5) == G.BAD_ARGUMENT                       # means without the workspace
    assert b"sn_segmentation_terms_forward" in lib.sn_last_error_string()
    bwd = lambda R_, C, means, gmeans, out=g.ptr(): lib.sn_segmentation_terms_backward(  # noqa: E731
        R_, C, x.ptr(), lab.ptr(), None, means, gmeans, None, out, None)
    assert bwd(4, 0, None, None) == G.BAD_ARGUMENT and bwd(4, 5, None, None, out=None) == G.BAD_ARGUMENT
    assert bwd(4, 5, None, outs[3].ptr()) == G.BAD_ARGUMENT     # g_means without the forward's means
    assert bwd(1 << 20, 1 << 11, None, None) == G.BAD_ARGUMENT
    assert b"sn_segmentation_terms_backward" in lib.sn_last_error_string()
    assert lib.sn_segmentation_terms_workspace_bytes(1 << 20, 1 << 11) == -1 and lib.sn_segmentation_terms_workspace_bytes(0, 5) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and g.untouched() and ws.untouched()


def test_graph_capture_replays_the_eager_bits():
    """the forward pair and the backward launch, captured without autograd inside and replayed"""
    lib, check = _lib()
    B, N, C = 2, 1027, 13
    R_ = B * N
    x, lab = R.make_case("mixed_ignored", B, N, C)
    w = R.make_weights("given", C)
    gm, gce = R.upstream_case(R_)
    eager = forward(x, lab, N, w)
    eager.append(backward(x, lab, w, eager[3], gm, gce))
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dx, dl, dw, dgm, dgce = dev(x), dev(lab), dev(w), dev(gm), dev(gce)
    ce, pred = torch.zeros(R_, device="cuda"), torch.zeros(R_, device="cuda", dtype=torch.int32)
    counts, means, g = torch.zeros(B, C, 3, device="cuda", dtype=torch.int32), torch.zeros(3, device="cuda"), torch.zeros(R_, C, device="cuda")
    ws = torch.zeros(lib.sn_segmentation_terms_workspace_bytes(R_, C), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        check(lib.sn_segmentation_terms_forward(R_, N, C, dx.data_ptr(), dl.data_ptr(), dw.data_ptr(), ce.data_ptr(), pred.data_ptr(),
                                                counts.data_ptr(), means.data_ptr(), ws.data_ptr(), st), "captured forward")
        check(lib.sn_segmentation_terms_backward(R_, C, dx.data_ptr(), dl.data_ptr(), dw.data_ptr(), means.data_ptr(), dgm.data_ptr(),
                                                 dgce.data_ptr(), g.data_ptr(), st), "captured backward")
    for t in (ce, pred, means, g):
        t.zero_()
    counts.fill_(7)  # the captured forward clears the counts itself
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (ce, pred, counts, means, g)):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)

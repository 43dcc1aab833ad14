"""sn_classification_terms_forward / _backward called directly, against the fp64 restatement and the counted bounds of
tests/cls_terms_ref.py.  Every tensor sits in a guarded buffer (tests/cabi_ref.py: poisoned words on both sides, checked after every
call; inputs compared bit for bit afterwards).  Every test prints its largest observed error beside the bound (`pytest -s`; recorded
in profiles/eval/errors.txt)."""
import itertools

import numpy as np
import pytest
import torch

import cabi_ref as G
import cls_terms_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def _report(what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if err.size:
        i = np.argmax(err / np.maximum(bound, 1e-300))
        print("CLS_ERR %-44s observed %.3e  bound %.3e  ratio %.3f" % (what, err.flat[i], bound.flat[i], err.flat[i] / max(bound.flat[i], 1e-300)))


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


def forward(x, lab, want=(True, True, True, True)):
    """One guarded call -> [ce, pred, correct, means] as numpy (None where not asked for)."""
    lib, check = _lib()
    B, C = x.shape
    gx, gl = G.Guarded((B, C), fill=x), G.Guarded((B,), torch.int32, fill=lab)
    kinds = ((B, torch.float32), (B, torch.int32), (B, torch.int32), (2, torch.float32))
    outs = [G.Guarded((n,), dt) if w else None for (n, dt), w in zip(kinds, want)]
    check(lib.sn_classification_terms_forward(B, C, gx.ptr(), gl.ptr(), *[G.arg(o) for o in outs], None), "sn_classification_terms_forward")
    torch.cuda.synchronize()
    assert gx.guards_intact() and gl.guards_intact() and _same_bits(gx, x) and _same_bits(gl, lab)
    return [None if o is None else o.check("forward output").cpu().numpy().copy() for o in outs]


def backward(x, lab, gm, gce):
    lib, check = _lib()
    B, C = x.shape
    gx, gl = G.Guarded((B, C), fill=x), G.Guarded((B,), torch.int32, fill=lab)
    ins = [None if a is None else G.Guarded(a.shape, fill=a) for a in (gm, gce)]
    out = G.Guarded((B, C))
    check(lib.sn_classification_terms_backward(B, C, gx.ptr(), gl.ptr(), *[G.arg(i) for i in ins], out.ptr(), None),
          "sn_classification_terms_backward")
    torch.cuda.synchronize()
    assert all(i is None or i.guards_intact() for i in ins) and gx.guards_intact() and gl.guards_intact()
    assert _same_bits(gx, x) and _same_bits(gl, lab) and all(i is None or _same_bits(i, a) for i, a in zip(ins, (gm, gce)))
    return out.check("g_logits").cpu().numpy().copy()


def _check_forward(tag, x, lab, got):
    ce, pred, correct, means = got
    T = R.terms(x, lab)
    B, C = x.shape
    inside = (lab >= 0) & (lab < C)
    if pred is not None:
        assert np.array_equal(pred, np.argmax(x, axis=1).astype(np.int32)), tag
    if correct is not None:
        assert np.array_equal(correct, (inside & (np.argmax(x, axis=1) == lab)).astype(np.int32)), tag
    if ce is not None:
        _within(tag + " ce", ce, T["ce"], R.bound_ce(T))
    if means is not None:
        if np.isfinite(T["ce"]).all():
            _within(tag + " mean ce", means[:1], T["means"][:1], R.bound_mean_ce(T))
        else:
            assert R.same_kind(means[:1], T["means"][:1]), tag
        # the count is exact, one conversion and one division
        assert abs(float(means[1]) - T["means"][1]) <= 1.01 * 2 * R.U * T["means"][1], tag
    return T


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("B,C", R.SHAPES)
def test_forward_and_backward_against_fp64(recipe, B, C):
    x, lab = R.make_case(recipe, B, C)
    tag = "%s (%d,%d)" % (recipe, B, C)
    got = forward(x, lab)
    T = _check_forward(tag, x, lab, got)
    if C == 1 and recipe == "normal":
        assert np.array_equal(got[0], np.zeros(B, dtype=np.float32))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, forward(x, lab))), "two runs differ"
    gm, gce = R.upstream_case(B)
    for name, g_means, g_ce in (("both", gm, gce), ("means", gm, None), ("ce", None, gce)):
        g = backward(x, lab, g_means, g_ce)
        ref = R.backward(x, lab, g_means, g_ce)
        # rows whose softmax is not finite (NaN logit, all -inf) are NaN in both; a row with s finite is compared entry by entry
        _within("%s g_logits[%s]" % (tag, name), g, ref, R.bound_backward(T, g_means, g_ce))
        if name == "both":
            assert np.array_equal(g, backward(x, lab, g_means, g_ce), equal_nan=True), "two runs differ"


@pytest.mark.parametrize("B,C", [(3, 65), (33, 40)])
def test_every_null_output_combination(B, C):
    x, lab = R.make_case("normal", B, C)
    full = forward(x, lab)
    for want in itertools.product((False, True), repeat=4):
        got = forward(x, lab, want)
        _check_forward("null %s (%d,%d)" % ("".join("x" if w else "-" for w in want), B, C), x, lab, got)
        for w, a, b in zip(want[:3], got[:3], full[:3]):
            # (with the means the rows run in one workgroup, without them in several: the per-row values are the same bits)
            assert not w or np.array_equal(a, b)


def test_empty_batch_and_bad_sizes():
    lib, check = _lib()
    outs = [G.Guarded((4,)), G.Guarded((4,), torch.int32), G.Guarded((4,), torch.int32), G.Guarded((2,))]
    check(lib.sn_classification_terms_forward(0, 5, None, None, *[o.ptr() for o in outs], None), "forward B = 0")
    g = G.Guarded((4, 5))
    check(lib.sn_classification_terms_backward(0, 5, None, None, None, None, g.ptr(), None), "backward B = 0")
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and g.untouched()
    assert lib.sn_classification_terms_forward(2, 0, g.ptr(), outs[1].ptr(), outs[0].ptr(), None, None, None, None) == G.BAD_ARGUMENT
    assert lib.sn_classification_terms_forward(2, 5, None, outs[1].ptr(), outs[0].ptr(), None, None, None, None) == G.BAD_ARGUMENT
    assert lib.sn_classification_terms_backward(2, 5, g.ptr(), outs[1].ptr(), None, None, None, None) == G.BAD_ARGUMENT
    assert b"sn_classification_terms_backward" in lib.sn_last_error_string()


@pytest.mark.parametrize("model", ["basic", "full"])
def test_fused_classification_loss(model):
    """classification_loss(fused=True) and its gradient w.r.t. the logits against the restatement, under the same bounds; the
    regulariser is the same node either way."""
    from samplenet_amd import classification_loss, ops

    B, C = 33, 40
    x, lab = R.make_case("normal", B, C)
    T = R.terms(x, lab)
    logits = torch.from_numpy(x).cuda().requires_grad_(True)
    labels = torch.from_numpy(lab).cuda().long()
    end_points = {}
    if model == "full":
        torch.manual_seed(3)
        end_points["transform"] = (torch.eye(64, device="cuda") + 0.01 * torch.randn(B, 64, 64, device="cuda")).requires_grad_(True)
    loss = classification_loss(logits, labels, end_points, fused=True)
    base = classification_loss(logits.detach(), labels, {k: v.detach() for k, v in end_points.items()}, fused=False)
    reg = 0.0
    if model == "full":
        from samplenet_amd.classifier import orthogonality_loss

        reg = 0.001 * float(orthogonality_loss(end_points["transform"].detach()))
    loss.backward()
    # (the sum with the regulariser: one more rounding of the total)
    _within("fused loss " + model, [float(loss)], [T["means"][0] + reg], R.bound_mean_ce(T) + 2 * R.U * abs(T["means"][0] + reg) + 3 * R.U * reg)
    gm = np.array([1.0, 0.0], dtype=np.float32)
    _within("fused loss gradient " + model, logits.grad.cpu().numpy(), R.backward(x, lab, gm, None), R.bound_backward(T, gm, None))
    print("CLS_ERR fused %-5s loss %.9g, F.cross_entropy route %.9g" % (model, float(loss), float(base)))
    # gradients through ce as well as means[0]; pred / correct / means[1] carry none
    lg = torch.from_numpy(x).cuda().requires_grad_(True)
    ce, pred, correct, means = ops.classification_terms(lg, labels)
    assert not pred.requires_grad and not correct.requires_grad and pred.dtype == torch.int32
    gce = R.upstream_case(B)[1]
    ((ce * torch.from_numpy(gce).cuda()).sum() + 0.5 * means[0] + 7.0 * means[1]).backward()
    gm = np.array([0.5, np.nan], dtype=np.float32)
    _within("terms gradient " + model, lg.grad.cpu().numpy(), R.backward(x, lab, gm, gce), R.bound_backward(T, gm, gce))


def test_graph_capture_replays_the_eager_bits():
    lib, check = _lib()
    B, C = 33, 40
    x, lab = R.make_case("normal", B, C)
    gm, gce = R.upstream_case(B)
    eager = forward(x, lab) + [backward(x, lab, gm, gce)]
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    dgm, dgce = torch.from_numpy(gm).cuda(), torch.from_numpy(gce).cuda()
    ce, pred, cor = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda", dtype=torch.int32), torch.zeros(B, device="cuda", dtype=torch.int32)
    means, g = torch.zeros(2, device="cuda"), torch.zeros(B, C, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        check(lib.sn_classification_terms_forward(B, C, dx.data_ptr(), dl.data_ptr(), ce.data_ptr(), pred.data_ptr(), cor.data_ptr(),
                                                  means.data_ptr(), st), "captured forward")
        check(lib.sn_classification_terms_backward(B, C, dx.data_ptr(), dl.data_ptr(), dgm.data_ptr(), dgce.data_ptr(), g.data_ptr(), st),
              "captured backward")
    for t in (ce, pred, cor, means, g):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (ce, pred, cor, means, g)):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)

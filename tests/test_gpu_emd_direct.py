"""The EMD entry points called directly (include/samplenet_hip.h: sn_approxmatch, sn_matchcost, sn_matchcost_grad, sn_emd_loss;
samplenet_hip_internal.h: sn_emd_loss_fast) with raw device pointers, against the plain float64 restatement of tests/emd_ref.py.
Every output and every workspace is a poison-and-guard buffer (tests/cabi_ref.py) of exactly the documented / reported size: after each
call the guards are intact -- nothing wrote past an output, and no workspace word beyond sn_workspace_bytes' figure was touched --
and every output is written completely.  Shapes, recipes, bars and the rule that admits a (shape, recipe, seed) case: tests/emd_ref.py
(one table row per branch of emd.hip; tests/test_emd_host.py keeps the table honest).  Against the fp32 oracle the bars are those of
tests/test_gpu_emd.py: 5e-4 per match entry, mean 1e-7.

Rounding bounds of the sweeps on a GIVEN plan are counted from the kernels' operations, next to where they are used."""
import functools

import numpy as np
import pytest
import torch

import emd_ref as E
from cabi_ref import BAD_ARGUMENT, POISON, Guarded, arg

pytestmark = pytest.mark.gpu

U = E.U
ALL = E.cases()
ENTRIES5 = ("sn_approxmatch", "sn_matchcost", "sn_matchcost_grad", "sn_emd_loss", "sn_emd_loss_fast")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def L():
    from samplenet_amd._lib import lib

    return lib


def call(name, *args, expect=0):
    rc = getattr(L(), name)(*[arg(a) for a in args])
    assert rc == expect, "%s returned %d: %s" % (name, rc, (L().sn_last_error_string() or b"").decode())
    return rc


def bits(x):
    x = x.view() if isinstance(x, Guarded) else x
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and torch.equal(bits(a), bits(b))


def workspace(op, b, n, m):
    """A guarded, poisoned workspace of exactly the reported size (the payload of a Guarded buffer is 256-byte aligned)."""
    wb = int(L().sn_workspace_bytes(op.encode(), b, n, m, 0))
    assert wb > 0 and wb % 4 == 0
    g = Guarded((wb // 4,))
    assert g.ptr() % 16 == 0
    return g


class hooks:
    """sn_emd_set_segments / sn_emd_set_sweep2d for a block, restored afterwards."""

    def __init__(self, segments=None, sweep2d=None):
        self.want = (segments, sweep2d)

    def __enter__(self):
        self.prev = [None, None]
        try:
            for i, (fn, v) in enumerate(zip(("sn_emd_set_segments", "sn_emd_set_sweep2d"), self.want)):
                if v is not None:
                    self.prev[i] = getattr(L(), fn)(v)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for fn, p in zip(("sn_emd_set_segments", "sn_emd_set_sweep2d"), self.prev):
            if p is not None:
                getattr(L(), fn)(p)
        return False


def finite(*gs):
    for g in gs:
        if g is not None:
            assert bool(torch.isfinite(g.view() if isinstance(g, Guarded) else g).all()), "NaN / Inf in an output"


# ------------------------------------------------------------------------------------------------ raw calls
class Case:
    """Device inputs + the float64 reference of one admitted case (the reference is shared and read-only)."""

    def __init__(self, case):
        self.ref = E.reference(*case)
        self.b, self.n, self.m = self.ref.shape
        self.x1, self.x2 = dev(self.ref.x1), dev(self.ref.x2)
        self.tag = E.case_id(case)

    def approxmatch(self, with_match=True):
        b, n, m = self.ref.shape
        match = Guarded((b, m, n)) if with_match else None
        temp = workspace("approxmatch", b, n, m)
        call("sn_approxmatch", b, n, m, self.x1, self.x2, match, temp, stream())
        torch.cuda.synchronize()
        if with_match:
            match.check(self.tag + " match")
        assert temp.guards_intact(), self.tag + ": sn_approxmatch wrote beyond the reported workspace"
        return match, temp

    def level_words(self, temp):
        b, n, m = self.ref.shape
        return temp.words()[: b * 11 * (n + m)]

    def matchcost(self, match):
        b, n, m = self.ref.shape
        cost, ws = Guarded((b,)), workspace("matchcost", b, n, m)
        call("sn_matchcost", b, n, m, self.x1, self.x2, match, cost, ws, stream())
        torch.cuda.synchronize()
        cost.check(self.tag + " cost")
        assert ws.guards_intact() and ws.fully_written(), self.tag + ": sn_matchcost's partials are not the reported workspace"
        return cost

    def matchcost_grad(self, match, want1=True, want2=True):
        b, n, m = self.ref.shape
        g1, g2 = Guarded((b, n, 3)), Guarded((b, m, 3))
        call("sn_matchcost_grad", b, n, m, self.x1, self.x2, match, g1 if want1 else None, g2 if want2 else None, stream())
        torch.cuda.synchronize()
        for g, want, nm in ((g1, want1, "grad1"), (g2, want2, "grad2")):
            if want:
                g.check("%s %s" % (self.tag, nm))
            else:
                assert g.untouched(), "%s: %s was written although NULL was passed" % (self.tag, nm)
        return (g1 if want1 else None), (g2 if want2 else None)

    def emd_loss(self, entry, want1=True, want2=True):
        b, n, m = self.ref.shape
        cost, g1, g2 = Guarded((b,)), Guarded((b, n, 3)), Guarded((b, m, 3))
        temp = workspace("emd_loss", b, n, m)
        call(entry, b, n, m, self.x1, self.x2, cost, g1 if want1 else None, g2 if want2 else None, temp, stream())
        torch.cuda.synchronize()
        cost.check("%s %s cost" % (self.tag, entry))
        for g, want, nm in ((g1, want1, "grad1"), (g2, want2, "grad2")):
            if want:
                g.check("%s %s %s" % (self.tag, entry, nm))
            else:
                assert g.untouched(), "%s %s: %s was written although NULL was passed" % (self.tag, entry, nm)
        assert temp.guards_intact(), "%s: %s wrote beyond the reported workspace" % (self.tag, entry)
        finite(cost, g1 if want1 else None, g2 if want2 else None)
        return cost, (g1 if want1 else None), (g2 if want2 else None)


@functools.lru_cache(maxsize=None)
def oracle_match(O, case):
    ref = E.reference(*case)
    return O.approxmatch(ref.x1, ref.x2)


def hold(tag, fig):
    print(E.show(tag, fig))
    assert not E.misses(fig), (tag, E.misses(fig))


# ------------------------------------------------------------------------------------------------ sn_approxmatch
@pytest.mark.parametrize("case", ALL, ids=E.case_id)
def test_approxmatch_against_fp64_and_the_oracle(oracle, case):
    """match and the ten ratio-vector pairs left in `temp` against float64 (ratioR element by element at every level, ratioL element by
    element where float64 calls it well-posed, all of them through the match they define: tests/emd_ref.py); match against the oracle
    under the bars of tests/test_gpu_emd.py; match = NULL leaves the same level vectors bit for bit; two runs agree bit for bit with the segmented level
    passes and again with the one-range form."""
    c = Case(case)
    b, n, m = c.ref.shape
    match, temp = c.approxmatch()
    finite(match)
    mh = match.numpy()
    lv = c.level_words(temp).view(torch.float32).view(b, 11 * (n + m))
    assert bool(torch.isfinite(lv).all())
    hold(c.tag + " sn_approxmatch", E.figures(c.ref, match=mh, ratios=lv[:, n + m:].cpu().numpy()))
    om = oracle_match(oracle, case)
    d = np.abs(mh - om)
    print("%s vs oracle: max %.1e mean %.1e" % (c.tag, d.max(), d.mean()))
    assert d.max() <= 5e-4 and d.mean() < 1e-7, (d.max(), d.mean())
    assert mh.min() >= 0.0
    _, temp0 = c.approxmatch(with_match=False)
    assert torch.equal(c.level_words(temp0), c.level_words(temp)), "match = NULL changed the level vectors"
    again, _ = c.approxmatch()
    assert same_bits(again, match), "two runs with segments differ"
    with hooks(segments=0):
        one, _ = c.approxmatch()
        two, _ = c.approxmatch()
    assert same_bits(one, two), "two runs of the one-range form differ"


@pytest.mark.parametrize("case", E.cases(shapes=E.SEGMENTED), ids=E.case_id)
def test_segmented_level_passes_match_the_one_range_form(case):
    """The bars of test_emd_segmented_level_passes_match_the_one_range_form (match 5e-4 per entry, mean 1e-7, cost 1e-6) at plans
    that segment ONE pass only (the two passes share the partials and the counter array with different grid widths) and at three and
    four ranges."""
    c = Case(case)
    with hooks(segments=1):
        a, _ = c.approxmatch()
        ca = c.matchcost(a)
    with hooks(segments=0):
        o, _ = c.approxmatch()
        co = c.matchcost(o)
    d = (a.view() - o.view()).abs()
    rel = float(((ca.view() - co.view()) / co.view()).abs().max())
    print("%s segments on/off: match max %.1e mean %.1e cost %.1e" % (c.tag, float(d.max()), float(d.mean()), rel))
    assert float(d.max()) <= 5e-4 and float(d.mean()) <= 1e-7 and rel <= 1e-6


# ------------------------------------------------------------------------------------------------ the sweeps on a given plan
@pytest.mark.parametrize("case", ALL, ids=E.case_id)
def test_matchcost_and_gradients_on_a_given_plan(case):
    """sn_matchcost / sn_matchcost_grad fed the float64 plan rounded to float32 -- the sweeps apart from the auction -- against float64
    on that same rounded plan.  Bound per output element: (additions on the longest chain + roundings per term) 2^-24 sum |terms|.
      roundings per term: the differences of two float32 coordinates (1 each), d2 = (dx dx + dy dy) + dz dz (3 products + 2 sums on
      top, all terms positive: 5 on d2), then
        cost:      sqrtf (halves d2's 5, adds 1), times match (1)                                        -> 5 (counted: 6)
        gradient:  rsqrtf (halves d2's 5, 1 ulp = 2 units), times match (1), times the difference (1 + 1) -> 8
      chains: cost     m sequential terms per thread, 8 tree levels over 256 threads, ceil(n / 256) partials in order
              grad1    m sequential terms
              grad2    ceil(n / 64) terms per lane, 6 butterfly levels
    (1e-30 absolute on top: a term below the smallest normal float32 may be flushed.)  grad1 = NULL and grad2 = NULL each: the other
    output keeps its bits and the NULL one's stand-in stays untouched."""
    c = Case(case)
    b, n, m = c.ref.shape
    plan = c.ref.match.astype(np.float32)
    mt = dev(plan)
    cost = c.matchcost(mt)
    g1, g2 = c.matchcost_grad(mt)
    finite(cost, g1, g2)
    x1, x2 = c.ref.x1, c.ref.x2
    want_c, abs_c = E.match_cost_fp64(x1, x2, plan), E.match_cost_fp64(x1, x2, plan, absolute=True)
    (want_1, want_2), (abs_1, abs_2) = E.match_cost_grad_fp64(x1, x2, plan), E.match_cost_grad_fp64(x1, x2, plan, absolute=True)
    bound_c = (m + 8 + (n + 255) // 256 + 6) * U * abs_c + 1e-30
    bound_1 = (m + 8) * U * abs_1 + 1e-30
    bound_2 = ((n + 63) // 64 + 6 + 8) * U * abs_2 + 1e-30
    for name, got, want, bound in (("cost", cost, want_c, bound_c), ("grad1", g1, want_1, bound_1), ("grad2", g2, want_2, bound_2)):
        err = np.abs(got.numpy().astype(np.float64) - want)
        print("%s %s on a given plan: worst error / bound %.2f" % (c.tag, name, float((err / bound).max())))
        assert (err <= bound).all(), (name, float((err / bound).max()))
    only1, _ = c.matchcost_grad(mt, want2=False)
    _, only2 = c.matchcost_grad(mt, want1=False)
    assert same_bits(only1, g1) and same_bits(only2, g2)
    c.matchcost_grad(mt, want1=False, want2=False)  # nothing to do: nothing written


# ------------------------------------------------------------------------------------------------ sn_emd_loss / sn_emd_loss_fast
@pytest.mark.parametrize("case", ALL, ids=E.case_id)
def test_emd_loss_entries_against_fp64_and_the_three_calls(case):
    """Both one-call forms under both sweep hooks and both segment hooks: every NULL combination of grad1 / grad2 leaves the outputs
    given bit-identical; cost and gradients against float64 under the bars at every setting; sn_emd_loss's cost and grad1 are bit for
    bit those of sn_approxmatch -> sn_matchcost -> sn_matchcost_grad in guarded buffers, its grad2 within 1e-5 of its scale (the
    gradient's largest component; multiL multiR for `same`), and the sweep hook does not reach it."""
    c = Case(case)
    for seg in (1, 0):
        exact_by_sweep = []
        for s2d in (1, 0):
            with hooks(segments=seg, sweep2d=s2d):
                for entry in ("sn_emd_loss", "sn_emd_loss_fast"):
                    cost, g1, g2 = c.emd_loss(entry)
                    tag = "%s %s seg=%d 2d=%d" % (c.tag, entry, seg, s2d)
                    hold(tag, E.figures(c.ref, cost=cost.numpy(), grad1=g1.numpy(), grad2=g2.numpy()))
                    for w1, w2 in ((True, False), (False, True), (False, False)):
                        cc, h1, h2 = c.emd_loss(entry, w1, w2)
                        assert same_bits(cc, cost), tag
                        assert (h1 is None or same_bits(h1, g1)) and (h2 is None or same_bits(h2, g2)), tag
                    if entry == "sn_emd_loss":
                        exact_by_sweep.append((cost, g1, g2))
        for u, w in zip(*exact_by_sweep):
            assert same_bits(u, w), "sn_emd_set_sweep2d changed sn_emd_loss"
        with hooks(segments=seg):
            match, _ = c.approxmatch()
            cost3 = c.matchcost(match)
            g31, g32 = c.matchcost_grad(match)
        cost, g1, g2 = exact_by_sweep[0]
        assert same_bits(cost, cost3) and same_bits(g1, g31), "%s seg=%d: sn_emd_loss is not the three-call composition" % (c.tag, seg)
        scale = c.ref.mlmr if c.ref.recipe == "same" else float(g32.view().abs().max())
        d2 = float((g2.view() - g32.view()).abs().max())
        print("%s seg=%d grad2 vs three calls: %.1e of its scale" % (c.tag, seg, d2 / scale))
        assert d2 <= 1e-5 * scale
        hold("%s three calls seg=%d" % (c.tag, seg), E.figures(c.ref, match=match.numpy(), cost=cost3.numpy(), grad1=g31.numpy(), grad2=g32.numpy()))


# ------------------------------------------------------------------------------------------------ coincident points
def test_identical_clouds_put_the_plan_on_the_diagonal():
    """`same` with n = m: every point sits on its partner (d2 = 0: the gradient's rsqrtf(max(d2, 1e-20)) times an exact zero), and
    the diagonal carries >= 0.99 of each column's mass -- in float64 and on the device."""
    case = E.cases(shapes=((2, 64, 64),), recipes=("same",))[0]
    c = Case(case)
    match, _ = c.approxmatch()
    for mt in (c.ref.match, match.numpy().astype(np.float64)):
        col, diag = mt.sum(1), np.einsum("bkk->bk", mt)
        assert (diag >= 0.99 * col).all() and (col > 0.5).all()


@pytest.mark.parametrize("case", E.cases(recipes=("cluster",)), ids=E.case_id)
def test_coincident_points_receive_identical_plans(case):
    """`cluster`: the repeated xyz1 points have identical match columns, the repeated xyz2 points identical match rows -- the same
    arithmetic in the same order, so bit for bit on the device (and exactly in float64)."""
    c = Case(case)
    b, n, m = c.ref.shape
    cn, cm = E.cluster_len(n), E.cluster_len(m)
    assert cn >= 2 and cm >= 2
    assert np.array_equal(c.ref.match[:, :, :cn], np.repeat(c.ref.match[:, :, :1], cn, 2))
    assert np.array_equal(c.ref.match[:, :cm], np.repeat(c.ref.match[:, :1], cm, 1))
    for seg in (1, 0):
        with hooks(segments=seg):
            match, _ = c.approxmatch()
        mt = match.view()
        finite(match)
        assert torch.equal(mt[:, :, :cn], mt[:, :, :1].expand(b, m, cn)) and torch.equal(mt[:, :cm], mt[:, :1].expand(b, cm, n))


# ------------------------------------------------------------------------------------------------ empty and bad arguments
def _empty_buffers(b, n, m):
    """Small real buffers for calls that must return before any device work (temp would hold the (2, 5, 4) workspace all the same)."""
    return dict(x1=torch.zeros(max(1, b * n * 3), device="cuda"), x2=torch.zeros(max(1, b * m * 3), device="cuda"),
                match=Guarded((b, m, n)), cost=Guarded((b,)), g1=Guarded((b, n, 3)), g2=Guarded((b, m, 3)), temp=Guarded((1024,)))


@pytest.mark.parametrize("shape", [(0, 5, 4), (3, 0, 4), (3, 5, 0), (2, 0, 0)], ids=str)
def test_empty_sizes_are_no_ops_that_zero_what_they_own(shape):
    """b = 0, n = 0, m = 0: every entry returns 0; cost is zeroed for b > 0; every gradient buffer given is written with zeros (the
    gradient of a constant zero cost); match has no element; nothing else is touched."""
    b, n, m = shape

    def zeros(g, what):
        if g.shape and int(np.prod(g.shape)) > 0:
            g.check(what)
            assert not bool(g.words().any()), what + " is not zero"
        else:
            assert g.untouched(), what

    q = _empty_buffers(b, n, m)
    call("sn_approxmatch", b, n, m, q["x1"], q["x2"], q["match"], q["temp"], stream())
    torch.cuda.synchronize()
    assert q["temp"].untouched() and q["match"].guards_intact()
    q = _empty_buffers(b, n, m)
    call("sn_matchcost", b, n, m, q["x1"], q["x2"], q["match"], q["cost"], q["temp"], stream())
    torch.cuda.synchronize()
    zeros(q["cost"], "sn_matchcost cost") if b else None
    assert q["temp"].untouched()
    for w1, w2 in ((True, True), (True, False), (False, True)):
        q = _empty_buffers(b, n, m)
        call("sn_matchcost_grad", b, n, m, q["x1"], q["x2"], q["match"], q["g1"] if w1 else None, q["g2"] if w2 else None, stream())
        torch.cuda.synchronize()
        zeros(q["g1"], "sn_matchcost_grad grad1") if w1 else None
        zeros(q["g2"], "sn_matchcost_grad grad2") if w2 else None
        assert (w1 or q["g1"].untouched()) and (w2 or q["g2"].untouched())
        for entry in ("sn_emd_loss", "sn_emd_loss_fast"):
            q = _empty_buffers(b, n, m)
            call(entry, b, n, m, q["x1"], q["x2"], q["cost"], q["g1"] if w1 else None, q["g2"] if w2 else None, q["temp"], stream())
            torch.cuda.synchronize()
            zeros(q["cost"], entry + " cost") if b else None
            zeros(q["g1"], entry + " grad1") if w1 else None
            zeros(q["g2"], entry + " grad2") if w2 else None
            assert (w1 or q["g1"].untouched()) and (w2 or q["g2"].untouched()) and q["temp"].untouched()


def test_empty_second_cloud_gives_a_zero_gradient_through_ops():
    from samplenet_amd import ops

    torch.empty(1 << 20, device="cuda").fill_(float("nan"))  # (what the allocator hands back next is not zero)
    for fn in (lambda a, c: ops.emd_loss(a, c), lambda a, c: ops.emd_loss(a, c, exact=True),
               lambda a, c: ops.match_cost(a, c, ops.approx_match(a, c))):
        x1 = torch.rand(3, 50, 3, device="cuda").requires_grad_(True)
        x2 = torch.rand(3, 0, 3, device="cuda").requires_grad_(True)
        cost = fn(x1, x2)
        assert cost.shape == (3,) and not bool(cost.any())
        g1, g2 = torch.autograd.grad(cost.sum(), [x1, x2])
        assert g1.shape == x1.shape and not bool(g1.view(torch.int32).any()) and g2.shape == x2.shape


BASES = {  # entry -> (argument names in order, the required pointers)
    "sn_approxmatch": (("x1", "x2", "match", "temp"), ("x1", "x2", "temp")),
    "sn_matchcost": (("x1", "x2", "match", "cost", "temp"), ("x1", "x2", "match", "cost", "temp")),
    "sn_matchcost_grad": (("x1", "x2", "match", "g1", "g2"), ("x1", "x2", "match")),
    "sn_emd_loss": (("x1", "x2", "cost", "g1", "g2", "temp"), ("x1", "x2", "cost", "temp")),
    "sn_emd_loss_fast": (("x1", "x2", "cost", "g1", "g2", "temp"), ("x1", "x2", "cost", "temp")),
}


def test_emd_loss_refuses_a_misaligned_workspace():
    """"temp: ... 16-byte aligned": a workspace 4, 8 or 12 bytes off is SN_ERR_BAD_ARGUMENT under the entry's name before any device
    work (P1 is written and read as float4 at a 16-byte offset from it); sn_approxmatch, which has no float4 access, takes it."""
    b, n, m = 3, 7, 5
    x1, x2 = E.make("cube", b, n, m, 0)
    x1, x2 = dev(x1), dev(x2)
    for entry in ("sn_emd_loss", "sn_emd_loss_fast"):
        for off in (4, 8, 12):
            cost, g1, g2, temp = Guarded((b,)), Guarded((b, n, 3)), Guarded((b, m, 3)), workspace("emd_loss", b, n, m)
            call(entry, b, n, m, x1, x2, cost, g1, g2, temp.ptr() + off, stream(), expect=BAD_ARGUMENT)
            msg = (L().sn_last_error_string() or b"").decode()
            assert msg.startswith(entry + ":") and "16-byte aligned" in msg, msg
            torch.cuda.synchronize()
            assert all(g.untouched() for g in (cost, g1, g2, temp))
    wb = int(L().sn_workspace_bytes(b"approxmatch", b, n, m, 0))
    match, temp = Guarded((b, m, n)), Guarded((wb // 4 + 1,))
    call("sn_approxmatch", b, n, m, x1, x2, match, temp.ptr() + 4, stream())
    torch.cuda.synchronize()
    assert temp.guards_intact() and int(temp.words()[0]) == POISON
    want, _ = Case(((b, n, m), "cube", 0)).approxmatch()
    assert same_bits(match.check("match"), want)


@pytest.mark.parametrize("entry", ENTRIES5)
def test_bad_arguments_name_their_entry(entry):
    """Negative sizes and each required NULL pointer: SN_ERR_BAD_ARGUMENT, sn_last_error_string() starts with the entry's own name,
    and no buffer is touched."""
    names, required = BASES[entry]
    b, n, m = 2, 5, 4
    cases = [((-1, n, m), None), ((b, -1, m), None), ((b, n, -1), None)] + [((b, n, m), r) for r in required]
    for sizes, null in cases:
        q = _empty_buffers(b, n, m)
        args = [None if k == null else q[k] for k in names]
        call(entry, *sizes, *args, stream(), expect=BAD_ARGUMENT)
        msg = (L().sn_last_error_string() or b"").decode()
        assert msg.startswith(entry + ":"), (entry, sizes, null, msg)
        assert ("negative" in msg) == (null is None) and ("null" in msg) == (null is not None), msg
        torch.cuda.synchronize()
        assert all(g.untouched() for g in q.values() if isinstance(g, Guarded))


# ------------------------------------------------------------------------------------------------ streams and capture
def _five(c, plan):
    """All five entries once, on the current stream -> the outputs, in a fixed order."""
    match, temp = c.approxmatch()
    cost = c.matchcost(plan)
    g1, g2 = c.matchcost_grad(plan)
    return [match, c.level_words(temp), cost, g1, g2] + list(c.emd_loss("sn_emd_loss")) + list(c.emd_loss("sn_emd_loss_fast"))


@pytest.mark.parametrize("case", E.cases(shapes=((3, 7, 5), (1, 520, 600)), recipes=("sphere",)), ids=E.case_id)
def test_entries_on_a_side_stream(case):
    """Each of the five entries on a non-default stream while the default stream has work in flight: the default-stream bits."""
    c = Case(case)
    plan = dev(c.ref.match.astype(np.float32))
    want = _five(c, plan)
    side = torch.cuda.Stream()
    busy = torch.randn(1024, 1024, device="cuda")
    torch.cuda.synchronize()
    for _ in range(4):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        got = _five(c, plan)
    torch.cuda.synchronize()
    for u, w in zip(got, want):
        assert same_bits(u, w)


@pytest.mark.parametrize("entry", ["sn_emd_loss_fast", "sn_approxmatch"])
def test_capture_and_replay_rearm_the_arrival_counters(entry):
    """(1, 520, 600) -- both level passes segmented -- captured with torch.cuda.graph (the path reconstruction_loss takes) and replayed
    twice into re-poisoned guarded buffers: each replay equals the eager call bit for bit, the workspace guards stay intact.  A counter
    left non-zero by one replay would make the next one's last-arrival test fire early or never."""
    c = Case(E.cases(shapes=((1, 520, 600),), recipes=("cube",))[0])
    b, n, m = c.ref.shape
    if entry == "sn_approxmatch":
        eager = [c.approxmatch()[0]]
        outs = [Guarded((b, m, n))]
        temp = workspace("approxmatch", b, n, m)
        args = (b, n, m, c.x1, c.x2, outs[0], temp)
    else:
        eager = list(c.emd_loss(entry))
        outs = [Guarded((b,)), Guarded((b, n, 3)), Guarded((b, m, 3))]
        temp = workspace("emd_loss", b, n, m)
        args = (b, n, m, c.x1, c.x2, outs[0], outs[1], outs[2], temp)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call(entry, *args, stream())  # warm-up outside the capture (first-use runtime work)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(entry, *args, stream())
    for replay in range(2):
        for g in outs + [temp]:
            g.raw.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for g, e in zip(outs, eager):
            g.check("%s replay %d" % (entry, replay))
            assert same_bits(g, e), "%s: replay %d differs from the eager call" % (entry, replay)
        assert temp.guards_intact()

"""samplenet_amd.optim.Adam (csrc/optimizer.hip: sn_adam_update) against torch.optim.Adam(foreach=False) on float64 CPU copies.

The parameter set has tensors of 1, 3, 5, 64, 1023, 1025 and 4097 elements: the smallest sizes that exercise the scalar tail, unaligned
gradient offsets, a one-element tensor and more than one chunk per tensor.  Gradients sit in ONE unpadded flat buffer behind a
one-element slot, as parallel.FlatGradAllReducer lays them out; two parameters start off a 16-byte boundary as well.  Every buffer the
kernel writes or reads (parameters, gradient bucket, both moment buffers) is a view into a sentinel-filled buffer (tests/skinny_ref.py's
bit pattern): a write outside a view is a failed assertion.

THE COMPARISON IS ALWAYS ONE STEP FROM IDENTICAL STATE: before every step the fp64 twin is loaded from the device's fp32 p, m, v, t, so
the bound is a single step's rounding.  For tf_epsilon=True the reference is the TensorFlow formula restated in fp64 below
(tf.train.AdamOptimizer's documented update; TensorFlow itself cannot run here).

The bound (constants 4, 6, 13 and its derivation from the kernel's pinned operation order) is in tests/adam_ref.py.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402
import skinny_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 5, 64, 1023, 1025, 4097)
LEAD = (0, 0, 1, 0, 3, 0, 0)   # words by which a parameter starts off a 16-byte boundary
LR, BETAS, EPS = R.LR, R.BETAS, R.EPS
U, CP, SLACK = R.U, R.CP, R.SLACK
reference_step, check_step = R.reference_step, R.check_step


class Guard:
    """n fp32 words, `lead` words off a 16-byte boundary, with sentinel words on both sides."""

    def __init__(self, n, lead=0):
        self.lo, self.n = S.GUARD + lead, n
        self.buf = torch.full((2 * S.GUARD + lead + n,), S.SENTINEL, dtype=torch.int32, device="cuda")
        self.view = self.buf[self.lo:self.lo + n].view(torch.float32)
        self.view.zero_()

    def intact(self):
        return bool((self.buf[:self.lo] == S.SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == S.SENTINEL).all())


def _guarded_adam():
    from samplenet_amd.optim import Adam

    class GuardedAdam(Adam):
        guards = []

        def _alloc(self, n, device):
            g = Guard(n)
            type(self).guards.append(g)
            return g.view

    GuardedAdam.guards = []
    return GuardedAdam


class World:
    """Parameters, the gradient bucket and an optimizer over them."""

    def __init__(self, seed=0, **kw):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.pg = [Guard(n, lead) for n, lead in zip(SIZES, LEAD)]
        self.params = []
        for g in self.pg:
            g.view.copy_(torch.randn(g.n, device="cuda", generator=gen))
            self.params.append(torch.nn.Parameter(g.view))
        self.bucket = Guard(1 + sum(SIZES))
        self.gviews, off = [], 1
        for n in SIZES:
            self.gviews.append(self.bucket.view[off:off + n])
            off += n
        assert any(v.data_ptr() % 16 for v in self.gviews) and any(p.data_ptr() % 16 for p in self.params)
        self.gen = gen
        self.bind()
        self.cls = _guarded_adam()
        self.opt = self.cls(self.params, **dict(dict(lr=LR, betas=BETAS, eps=EPS), **kw))
        self.dev = self.opt._dev[0]

    def bind(self, none=()):
        for i, (p, v) in enumerate(zip(self.params, self.gviews)):
            p.grad = None if i in none else v

    def randn_grads(self, scale=1.0):
        self.bucket.view.copy_(torch.randn(self.bucket.n, device="cuda", generator=self.gen) * scale)

    def seed_moments(self):
        """Moments as after some training: m of either sign, v positive (the padding between segments stays zero)."""
        for i in range(len(SIZES)):
            m, v = self.dev.views(i)
            m.copy_(torch.randn(m.shape, device="cuda", generator=self.gen) * 0.1)
            v.copy_(torch.rand(v.shape, device="cuda", generator=self.gen) * 0.01)

    def set_step(self, t):
        self.dev.write_block(self.opt.param_groups[0], t)

    def snapshot(self):
        """fp32 state of the device: (p, m, v) lists and the step count."""
        torch.cuda.synchronize()
        return ([p.detach().clone() for p in self.params], [self.dev.views(i)[0].clone() for i in range(len(SIZES))],
                [self.dev.views(i)[1].clone() for i in range(len(SIZES))], self.dev.step_count())

    def flat_state(self):
        torch.cuda.synchronize()
        return (torch.cat([p.detach().view(-1) for p in self.params]).clone(), self.dev.exp_avg.clone(), self.dev.exp_avg_sq.clone(),
                self.dev.block.clone())

    def intact(self):
        torch.cuda.synchronize()
        pad = torch.ones(self.dev.total, dtype=torch.bool, device="cuda")
        for o, n in zip(self.dev.offsets, SIZES):
            pad[o:o + n] = False
        return (all(g.intact() for g in self.pg) and self.bucket.intact() and all(g.intact() for g in self.cls.guards)
                and not bool(self.dev.exp_avg[pad].any()) and not bool(self.dev.exp_avg_sq[pad].any())
                and int(self.dev.block.view(torch.int32)[8]) == 0)  # the arrival counter is back at zero


def _one_step(w, none=(), **kw):
    before = w.snapshot()
    grads = [None if i in none else v.clone() for i, v in enumerate(w.gviews)]
    versions = [p._version for p in w.params]
    w.opt.step()
    after = w.snapshot()
    assert w.intact()
    for i, p in enumerate(w.params):  # the kernel wrote through raw pointers: autograd must hear of it
        assert (p._version == versions[i]) if i in none else (p._version > versions[i]), i
    return before, after, grads


@pytest.mark.parametrize("tf", [False, True], ids=["torch", "tf"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_single_steps_within_the_rounding_bound(wd, tf):
    """t = 1, 2, 3 (consecutive steps from a fresh optimizer, randn gradients), then t = 1000, and t = 100001 / 400001 after a
    load_state_dict with step 100000 / 400000 (beta1^t has underflowed: bc1 = 1; bc2 = 1 - beta2^t is still formed exactly)."""
    w = World(seed=1, weight_decay=wd, tf_epsilon=tf)
    kw = dict(wd=wd, tf=tf)
    for t in (1, 2, 3):
        w.randn_grads()
        before, after, grads = _one_step(w)
        assert after[3] == t
        check_step(before, after, grads, "t=%d wd=%g tf=%d" % (t, wd, tf), **kw)
    w.seed_moments()
    w.set_step(999)
    w.randn_grads(1e-2)
    before, after, grads = _one_step(w)
    assert after[3] == 1000
    check_step(before, after, grads, "t=1000 wd=%g tf=%d" % (wd, tf), **kw)
    for t in (100000, 400000):
        sd = w.opt.state_dict()
        for st in sd["state"].values():
            st["step"] = torch.tensor(float(t))
        w.opt.load_state_dict(sd)
        w.randn_grads(1e-3)
        before, after, grads = _one_step(w)
        assert before[3] == t and after[3] == t + 1
        check_step(before, after, grads, "t=%d wd=%g tf=%d" % (t + 1, wd, tf), **kw)
        assert w.opt.state_dict()["state"][0]["step"].item() == t + 1


def test_grad_scale_folds_into_the_update():
    w = World(seed=2, weight_decay=1e-2, grad_scale=1.0 / 3.0)
    w.seed_moments()
    w.set_step(7)
    w.randn_grads()
    before, after, grads = _one_step(w)
    check_step(before, after, grads, "grad_scale=1/3", wd=1e-2, gs=1.0 / 3.0)


def test_exact_zeros_leave_the_parameters_bit_identical():
    w = World(seed=3)
    before, after, grads = _one_step(w)  # zero gradients (the bucket is zero-filled), zero moments
    assert all(not bool(g.any()) for g in grads)
    for i in range(len(SIZES)):
        assert torch.equal(after[0][i].view(torch.int32), before[0][i].view(torch.int32)), i
        assert not bool(after[1][i].any()) and not bool(after[2][i].any())
    assert after[3] == 1


@pytest.mark.parametrize("none", [0, 4, 5])
def test_a_none_gradient_is_skipped(none):
    """Its parameter and its moment slices stay bit for bit; every other tensor is updated within the bound; nothing outside any view
    is written (the one-element tensor, the tensor with a scalar tail, a two-chunk tensor)."""
    w = World(seed=4 + none, weight_decay=1e-2)
    w.seed_moments()
    w.set_step(5)
    w.randn_grads()
    w.bind(none=(none,))
    before, after, grads = _one_step(w, none=(none,))
    check_step(before, after, grads, "none=%d" % none, wd=1e-2)
    # ... and comes back when the gradient does
    w.bind()
    before, after, grads = _one_step(w)
    check_step(before, after, grads, "none=%d rebound" % none, wd=1e-2)


def test_step_count_and_determinism():
    """`step` in state_dict() equals the number of launches; two runs of five steps from the same state are bit-identical."""
    runs = []
    for _ in range(2):
        w = World(seed=9, weight_decay=1e-2)
        for k in range(5):
            w.randn_grads()
            w.opt.step()
        sd = w.opt.state_dict()
        assert all(float(st["step"]) == 5 for st in sd["state"].values()) and len(sd["state"]) == len(SIZES)
        for i, p in enumerate(w.params):
            assert sd["state"][i]["exp_avg"].data_ptr() == w.dev.views(i)[0].data_ptr()  # views of the flat buffers
            assert sd["state"][i]["exp_avg"].shape == p.shape
        runs.append(w.flat_state())
        assert w.intact()
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))


def test_state_dicts_travel_both_ways():
    """torch.optim.Adam on the GPU, three steps -> its state dict loads here and the next step is within the bound of the fp64
    continuation; and the converse: three steps here -> torch.optim.Adam loads the dict and continues from the same state."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    w = World(seed=10, weight_decay=1e-2)
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in w.params]
    topt = torch.optim.Adam(tparams, lr=3e-4, betas=BETAS, eps=EPS, weight_decay=1e-2)
    for _ in range(3):
        for p in tparams:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen)
        topt.step()
    w.opt.load_state_dict(topt.state_dict())
    assert w.opt.param_groups[0]["lr"] == 3e-4 and w.opt.param_groups[0]["tf_epsilon"] is False
    for p, q in zip(w.params, tparams):
        p.data.copy_(q.detach())
    before = w.snapshot()
    assert before[3] == 3
    for i, q in enumerate(tparams):
        assert torch.equal(before[1][i], topt.state[q]["exp_avg"]) and torch.equal(before[2][i], topt.state[q]["exp_avg_sq"])
    w.randn_grads()
    before, after, grads = _one_step(w)
    check_step(before, after, grads, "continuing torch's run", lr=3e-4, wd=1e-2)
    # the converse: three steps here; the dict loads into torch.optim.Adam -- on fp64 CPU copies, whose next step is the reference our
    # own fourth step is held to, and on the GPU in fp32, where it arrives bit for bit
    w2 = World(seed=12, weight_decay=1e-2)
    for _ in range(3):
        w2.randn_grads()
        w2.opt.step()
    sd = w2.opt.state_dict()
    assert sd["param_groups"][0]["tf_epsilon"] is False  # (an extra key torch ignores)
    p0, m0, v0, t0 = w2.snapshot()
    t32 = [torch.nn.Parameter(x.clone()) for x in p0]
    topt32 = torch.optim.Adam(t32, lr=1.0)
    topt32.load_state_dict(sd)
    assert topt32.param_groups[0]["lr"] == LR and topt32.param_groups[0]["weight_decay"] == 1e-2
    for i, q in enumerate(t32):
        st = topt32.state[q]
        assert float(st["step"]) == 3 == t0 and torch.equal(st["exp_avg"], m0[i]) and torch.equal(st["exp_avg_sq"], v0[i])
    t64 = [torch.nn.Parameter(x.double().cpu()) for x in p0]
    topt64 = torch.optim.Adam(t64, lr=1.0, foreach=False)
    topt64.load_state_dict(sd)  # (moments cast to the parameters' fp64)
    w2.randn_grads()
    for q, g in zip(t64, w2.gviews):
        q.grad = g.double().cpu()
    topt64.step()
    before, after, grads = _one_step(w2)
    pr, mr, vr = check_step(before, after, grads, "our fourth step", wd=1e-2)
    for i, q in enumerate(t64):  # the injected-state reference and torch's own continuation of the loaded dict are the same numbers
        assert torch.equal(q.detach(), pr[i]) and torch.equal(topt64.state[q]["exp_avg"], mr[i]), i
        assert torch.equal(topt64.state[q]["exp_avg_sq"], vr[i]) and float(topt64.state[q]["step"]) == 4, i


def test_captured_updates_replay_bit_identically():
    """Three updates captured in one graph, replayed four times with lr changed between the replays: parameters, moments and step
    count equal the same twelve updates issued eagerly, bit for bit (everything that changes lives on the device)."""
    lrs = (1e-3, 5e-4, 2e-3, 1e-4)
    a, b = World(seed=20, weight_decay=1e-2), World(seed=20, weight_decay=1e-2)
    for w in (a, b):
        w.randn_grads()
    assert torch.equal(a.bucket.view, b.bucket.view)
    for lr in lrs:  # eager
        a.opt.param_groups[0]["lr"] = lr
        for _ in range(3):
            a.opt.step()
    b.opt.prepare()  # the host side, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            b.opt.step()
    torch.cuda.synchronize()
    assert b.dev.step_count() == 0  # capturing ran nothing
    for lr in lrs:
        b.opt.param_groups[0]["lr"] = lr
        b.opt.prepare()
        graph.replay()
    assert a.dev.step_count() == 12 == b.dev.step_count()
    for x, y in zip(a.flat_state(), b.flat_state()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a.intact() and b.intact()


def test_zero_grad_keeps_torch_semantics_and_param_groups_work():
    w = World(seed=30)
    w.randn_grads()
    w.opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not bool(p.grad.any()) for p in w.params) and not bool(w.bucket.view[1:].any())  # (word 0 is the slot in front: no parameter's)
    w.opt.zero_grad()
    assert all(p.grad is None for p in w.params)
    w.opt.step()  # nothing has a gradient: not a step
    assert w.dev.step_count() == 0
    # two groups with their own options, gradients that autograd allocated (no bucket)
    from samplenet_amd.optim import Adam

    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, device="cuda")) for n in (7, 1030)]
    opt = Adam([{"params": ps[:1], "lr": 1e-2}, {"params": ps[1:], "weight_decay": 1e-2}], lr=1e-3)
    loss = sum((p * p).sum() for p in ps)
    loss.backward()
    p0 = [p.detach().clone() for p in ps]
    g0 = [p.grad.clone() for p in ps]
    z = [torch.zeros_like(p) for p in ps]
    opt.step()
    torch.cuda.synchronize()
    for i, (lr, wd) in enumerate(((1e-2, 0.0), (1e-3, 1e-2))):
        pr, _, _, A, scale = reference_step(p0[i:i + 1], g0[i:i + 1], z[i:i + 1], z[i:i + 1], 0, lr=lr, wd=wd)
        err = (ps[i].detach().double().cpu() - pr[0]).abs()
        assert bool((err <= (U * pr[0].abs() + CP * U * A[0] * scale[0]) * SLACK).all()), i
    assert [d.step_count() for d in opt._dev] == [1, 1]

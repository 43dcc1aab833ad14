"""samplenet_amd.optim.SGD and RMSprop (csrc/optimizer.hip: sn_sgd_update, sn_rmsprop_update) against torch.optim.SGD(foreach=False)
and torch.optim.RMSprop(foreach=False) on float64 CPU copies.

The world is tests/test_gpu_adam.py's, for the same reasons: tensors of 1, 3, 5, 64, 1023, 1025 and 4097 elements (scalar tail,
unaligned gradient offsets, a one-element tensor, more than one chunk per tensor); the gradients in ONE unpadded flat buffer behind a
one-element slot, as parallel.FlatGradAllReducer lays them out; two parameters start off a 16-byte boundary.  Every buffer the kernels
read or write (parameters, gradient bucket, every state buffer) is a view into a sentinel-filled buffer (tests/skinny_ref.py's bit
pattern): a write outside a view is a failed assertion.  After every step the guards and the padding between state segments are
intact, the arrival counter is zero, and the autograd version of every updated parameter -- and only theirs -- has moved.

THE COMPARISON IS ALWAYS ONE STEP FROM IDENTICAL STATE; the bounds and their derivation from the kernels' pinned operation order are in
tests/optim_ref.py.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R  # noqa: E402
import skinny_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 5, 64, 1023, 1025, 4097)
LEAD = (0, 0, 1, 0, 3, 0, 0)   # words by which a parameter starts off a 16-byte boundary
NP = len(SIZES)


class Guard:
    """n fp32 words, `lead` words off a 16-byte boundary, with sentinel words on both sides."""

    def __init__(self, n, lead=0):
        self.lo, self.n = S.GUARD + lead, n
        self.buf = torch.full((2 * S.GUARD + lead + n,), S.SENTINEL, dtype=torch.int32, device="cuda")
        self.view = self.buf[self.lo:self.lo + n].view(torch.float32)
        self.view.zero_()

    def intact(self):
        return bool((self.buf[:self.lo] == S.SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == S.SENTINEL).all())


def _guarded(kind):
    from samplenet_amd import optim

    class Guarded(getattr(optim, kind)):
        guards = []

        def _alloc(self, n, device):
            g = Guard(n)
            type(self).guards.append(g)
            return g.view

    return Guarded


class World:
    """Parameters, the gradient bucket and an optimizer of class `kind` ('SGD' / 'RMSprop') over them."""

    def __init__(self, kind, seed=0, **kw):
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
        self.gen, self.kind = gen, kind
        self.bind()
        self.cls = _guarded(kind)
        self.opt = self.cls(self.params, **kw)
        self.dev = self.opt._dev[0]
        self.dev.block[1:3].fill_(-7.5)  # words 1 and 2 of the block are not these kernels': _one_step finds them as they were

    def bind(self, none=()):
        for i, (p, v) in enumerate(zip(self.params, self.gviews)):
            p.grad = None if i in none else v

    def randn_grads(self, scale=1.0):
        self.bucket.view.copy_(torch.randn(self.bucket.n, device="cuda", generator=self.gen) * scale)

    def seed_state(self):
        """State as after some training: momentum of either sign, square_avg positive (the padding between segments stays zero)."""
        for i in range(NP):
            for name, v in zip(self.dev.names, self.dev.views(i)):
                if name == "square_avg":
                    v.copy_(torch.rand(v.shape, device="cuda", generator=self.gen) * 0.01)
                else:
                    v.copy_(torch.randn(v.shape, device="cuda", generator=self.gen) * 0.1)

    def set_step(self, t):
        self.dev.write_block(self.opt.param_groups[0], t)

    def buffers(self, name):
        if name not in self.dev.names:
            return None
        k = self.dev.names.index(name)
        return [self.dev.views(i)[k].clone() for i in range(NP)]

    def snapshot(self):
        """fp32 state of the device: SGD (p, b, t), RMSprop (p, s, b, t); b None without momentum."""
        torch.cuda.synchronize()
        p = [q.detach().clone() for q in self.params]
        if self.kind == "SGD":
            return p, self.buffers("momentum_buffer"), self.dev.step_count()
        return p, self.buffers("square_avg"), self.buffers("momentum_buffer"), self.dev.step_count()

    def flat_state(self):
        torch.cuda.synchronize()
        return [torch.cat([p.detach().view(-1) for p in self.params]).clone()] + \
               [getattr(self.dev, n).clone() for n in self.dev.names] + [self.dev.block.clone()]

    def intact(self):
        torch.cuda.synchronize()
        pad = torch.ones(self.dev.total, dtype=torch.bool, device="cuda")
        for o, n in zip(self.dev.offsets, SIZES):
            pad[o:o + n] = False
        return (all(g.intact() for g in self.pg) and self.bucket.intact() and all(g.intact() for g in self.cls.guards)
                and len(self.cls.guards) == len(self.dev.names)
                and all(not bool(getattr(self.dev, n)[pad].any()) for n in self.dev.names)
                and int(self.dev.block.view(torch.int32)[8]) == 0)  # the arrival counter is back at zero


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64)


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def _one_step(w, none=()):
    before = w.snapshot()
    grads = [None if i in none else v.clone() for i, v in enumerate(w.gviews)]
    versions = [p._version for p in w.params]
    block = w.dev.block.clone()
    w.opt.step()
    after = w.snapshot()
    assert w.intact()
    assert torch.equal(w.dev.block[1:3].view(torch.int64), block[1:3].view(torch.int64))  # words 1 and 2: left as found
    for i, p in enumerate(w.params):  # the kernel wrote through raw pointers: autograd must hear of it
        assert (p._version == versions[i]) if i in none else (p._version > versions[i]), i
    return before, after, grads


def _check(w, before, after, grads, what, **kw):
    return (R.check_sgd_step if w.kind == "SGD" else R.check_rmsprop_step)(before, after, grads, what, **kw)


# ---- single steps within the bound --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_single_steps_within_the_rounding_bound(momentum, wd):
    """The first step (t = 0: the buffer becomes the gradient), the second, and a later one from seeded buffers."""
    w = World("SGD", seed=1, lr=1e-3, momentum=momentum, weight_decay=wd)
    kw = dict(lr=1e-3, momentum=momentum, wd=wd)
    for t in (0, 1):
        w.randn_grads()
        before, after, grads = _one_step(w)
        assert before[-1] == t
        _check(w, before, after, grads, "t=%d mu=%g wd=%g" % (t, momentum, wd), **kw)
    w.seed_state()
    w.set_step(1000)
    w.randn_grads(1e-2)
    before, after, grads = _one_step(w)
    assert after[-1] == 1001
    _check(w, before, after, grads, "t=1000 mu=%g wd=%g" % (momentum, wd), **kw)


def test_sgd_dampening_applies_from_the_second_step():
    """dampening 0.1: the first step must ignore it -- and whatever the buffer holds (torch: the buffer does not exist yet and becomes
    a copy of the gradient); the second applies it."""
    w = World("SGD", seed=2, lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=1e-2)
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.1, wd=1e-2)
    w.seed_state()  # t is still 0: stale content the first step must not read
    for t in (0, 1):
        w.randn_grads()
        before, after, grads = _one_step(w)
        assert before[-1] == t
        pr, br = _check(w, before, after, grads, "dampening t=%d" % t, **kw)
    # (the two rules give different numbers: had the first step applied dampening, its buffer would be 0.9 g1 + ..., far outside u)
    g1 = grads[3].double().cpu() + 1e-2 * before[0][3].double().cpu()
    assert not torch.allclose(br[3], g1)


def test_sgd_nesterov():
    w = World("SGD", seed=3, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-2)
    kw = dict(lr=1e-2, momentum=0.9, nesterov=True, wd=1e-2)
    for t in (0, 1):
        w.randn_grads()
        before, after, grads = _one_step(w)
        _check(w, before, after, grads, "nesterov t=%d" % t, **kw)
    w.seed_state()
    w.randn_grads(1e-2)
    before, after, grads = _one_step(w)
    _check(w, before, after, grads, "nesterov seeded", **kw)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_single_steps_within_the_rounding_bound(momentum, wd):
    """From zero state (two consecutive steps), then from seeded positive square_avg (and momentum of either sign)."""
    w = World("RMSprop", seed=4, lr=1e-2, momentum=momentum, weight_decay=wd)
    kw = dict(lr=1e-2, momentum=momentum, wd=wd)
    for t in (0, 1):
        w.randn_grads()
        before, after, grads = _one_step(w)
        assert before[-1] == t
        _check(w, before, after, grads, "t=%d mu=%g wd=%g" % (t, momentum, wd), **kw)
    w.seed_state()
    w.set_step(1000)
    w.randn_grads(1e-2)
    before, after, grads = _one_step(w)
    assert after[-1] == 1001
    _check(w, before, after, grads, "t=1000 mu=%g wd=%g" % (momentum, wd), **kw)


# ---- exact properties ---------------------------------------------------------------------------------------------------------------
KINDS = [("SGD", dict(lr=1e-3, momentum=0.9, weight_decay=1e-2)), ("SGD", dict(lr=1e-3, momentum=0.9, nesterov=True)),
         ("SGD", dict(lr=1e-3, weight_decay=1e-2)), ("RMSprop", dict(lr=1e-2, weight_decay=1e-2)),
         ("RMSprop", dict(lr=1e-2, momentum=0.9, weight_decay=1e-2))]
KIND_IDS = ["sgd-momentum", "sgd-nesterov", "sgd-plain", "rmsprop", "rmsprop-momentum"]


@pytest.mark.parametrize("kind,kw", KINDS, ids=KIND_IDS)
def test_grad_scale_folds_into_the_update(kind, kw):
    """Gradients g with grad_scale 1/8 against gradients g / 8 with grad_scale 1: scaling by a power of two is exact, so every array
    agrees bit for bit -- on the first step and on one from seeded state."""
    a, b = World(kind, seed=5, grad_scale=0.125, **kw), World(kind, seed=5, **kw)
    for k in range(2):
        for w in (a, b):
            w.randn_grads()
        b.bucket.view.mul_(0.125)
        assert torch.equal(a.bucket.view * 0.125, b.bucket.view)
        _one_step(a)
        _one_step(b)
        _same_bits(a.flat_state(), b.flat_state())
        for w in (a, b):
            w.seed_state()
    assert a.dev.step_count() == 2


@pytest.mark.parametrize("kind,kw", KINDS, ids=KIND_IDS)
def test_exact_zeros(kind, kw):
    """lr = 0: the parameters stay bit for bit while the state advances.  Zero gradients, wd = 0, zero state: everything stays bit for
    bit and finite (RMSprop divides 0 by 0 + eps)."""
    w = World(kind, seed=6, **dict(kw, lr=0.0))
    w.randn_grads()
    before, after, grads = _one_step(w)
    _same_bits(before[0], after[0])
    assert after[-1] == before[-1] + 1
    for b0, b1 in zip(before[1:-1], after[1:-1]):
        assert (b0 is None) == (b1 is None)
        if b0 is not None:
            assert all(bool((x != y).any()) for x, y in zip(b0, b1))  # every tensor's state moved
    _check(w, before, after, grads, "lr=0", **{{"weight_decay": "wd"}.get(k, k): v for k, v in dict(kw, lr=0.0).items()})
    w = World(kind, seed=7, **dict(kw, weight_decay=0.0))
    before, after, grads = _one_step(w)  # (the bucket is zero-filled)
    assert all(not bool(g.any()) for g in grads)
    _same_bits(before[0], after[0])
    for b1 in after[1:-1]:
        assert b1 is None or all(not bool(x.any()) and bool(torch.isfinite(x).all()) for x in b1)
    assert after[-1] == 1


@pytest.mark.parametrize("none", [0, 4, 5])
@pytest.mark.parametrize("kind,kw", [KINDS[0], KINDS[4]], ids=[KIND_IDS[0], KIND_IDS[4]])
def test_a_none_gradient_is_skipped(kind, kw, none):
    """Its parameter and its state segments stay bit for bit; every other tensor is updated within the bound; nothing outside any view
    is written (the one-element tensor, the tensor with a scalar tail, a two-chunk tensor)."""
    w = World(kind, seed=8 + none, **kw)
    rkw = {{"weight_decay": "wd"}.get(k, k): v for k, v in kw.items()}
    w.seed_state()
    w.set_step(5)
    w.randn_grads()
    w.bind(none=(none,))
    before, after, grads = _one_step(w, none=(none,))
    _check(w, before, after, grads, "none=%d" % none, **rkw)
    # ... and comes back when the gradient does
    w.bind()
    before, after, grads = _one_step(w)
    _check(w, before, after, grads, "none=%d rebound" % none, **rkw)


@pytest.mark.parametrize("kind,kw", [KINDS[0], KINDS[4]], ids=[KIND_IDS[0], KIND_IDS[4]])
def test_step_count_and_determinism(kind, kw):
    """The step count equals the number of launches; two runs of five steps from the same state are bit-identical."""
    runs = []
    for _ in range(2):
        w = World(kind, seed=9, **kw)
        for k in range(5):
            w.randn_grads()
            w.opt.step()
            assert w.dev.step_count() == k + 1
        sd = w.opt.state_dict()
        assert len(sd["state"]) == NP
        if kind == "RMSprop":
            assert all(float(st["step"]) == 5 for st in sd["state"].values())
        for i, p in enumerate(w.params):
            b = sd["state"][i]["momentum_buffer"]
            assert b.data_ptr() == w.dev.views(i)[-1].data_ptr() and b.shape == p.shape  # views of the flat buffer
        runs.append(w.flat_state())
        assert w.intact()
    _same_bits(*runs)


def test_sgd_without_momentum_allocates_no_buffer():
    w = World("SGD", seed=10, lr=1e-2)
    assert w.dev.names == () and not w.cls.guards and not hasattr(w.dev, "momentum_buffer")
    w.randn_grads()
    before, after, grads = _one_step(w)
    _check(w, before, after, grads, "plain", lr=1e-2)
    assert not w.cls.guards
    sd = w.opt.state_dict()
    assert all(st == {"momentum_buffer": None} for st in sd["state"].values()) and len(sd["state"]) == NP
    # loading a dict with momentum allocates the buffer, one without drops it again
    m = World("SGD", seed=10, lr=1e-2, momentum=0.9)
    m.randn_grads()
    m.opt.step()
    w.opt.load_state_dict(m.opt.state_dict())
    assert w.dev.names == ("momentum_buffer",) and w.dev.step_count() == 1
    _same_bits([w.dev.momentum_buffer], [m.dev.momentum_buffer])
    w.opt.load_state_dict(sd)
    assert w.dev.names == () and not hasattr(w.dev, "momentum_buffer") and w.dev.step_count() == 0


# ---- state dicts --------------------------------------------------------------------------------------------------------------------
def _torch_twin(kind, params, device, dtype, **kw):
    ps = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in params]
    return ps, getattr(torch.optim, kind)(ps, **kw)


@pytest.mark.parametrize("kind,kw", [KINDS[0], KINDS[1], KINDS[3], KINDS[4]], ids=[KIND_IDS[0], KIND_IDS[1], KIND_IDS[3], KIND_IDS[4]])
def test_state_dicts_travel_both_ways(kind, kw):
    """Three steps here -> the dict loads into the torch class (fp32 on the GPU: bit for bit; fp64 on the CPU: its next step from the
    same gradients is the reference our own fourth step is held to).  And the converse: three steps of the torch class on the GPU ->
    its dict loads here and the next step is within the bound of the fp64 continuation."""
    rkw = {{"weight_decay": "wd"}.get(k, k): v for k, v in kw.items()}
    names = ("momentum_buffer",) if kind == "SGD" else ("square_avg", "momentum_buffer")
    w = World(kind, seed=11, **kw)
    for _ in range(3):
        w.randn_grads()
        w.opt.step()
    sd = w.opt.state_dict()
    assert sd["param_groups"][0]["grad_scale"] == 1.0  # (an extra key torch ignores)
    snap = w.snapshot()
    assert snap[-1] == 3
    t32, topt32 = _torch_twin(kind, snap[0], "cuda", torch.float32, lr=1.0)
    topt32.load_state_dict(sd)
    assert topt32.param_groups[0]["lr"] == kw["lr"] and topt32.param_groups[0]["weight_decay"] == kw.get("weight_decay", 0)
    for i, q in enumerate(t32):
        st = topt32.state[q]
        for name in names:
            if name in w.dev.names:
                assert torch.equal(st[name], w.buffers(name)[i]), (name, i)
        assert kind == "SGD" or float(st["step"]) == 3
    t64, topt64 = _torch_twin(kind, snap[0], "cpu", torch.float64, lr=1.0, foreach=False)
    topt64.load_state_dict(sd)  # (state cast to the parameters' fp64)
    w.randn_grads()
    for q, g in zip(t64, w.gviews):
        q.grad = g.double().cpu()
    topt64.step()
    before, after, grads = _one_step(w)
    ref = _check(w, before, after, grads, "our fourth step", **rkw)
    for i, q in enumerate(t64):  # the injected-state reference and torch's own continuation of the loaded dict are the same numbers
        assert torch.equal(q.detach(), ref[0][i]), i
        assert torch.equal(topt64.state[q]["momentum_buffer"], ref[-1][i]) if "momentum_buffer" in w.dev.names else True, i
    # the converse
    gen = torch.Generator(device="cuda").manual_seed(12)
    w2 = World(kind, seed=13, **dict(kw, lr=0.5))
    tp, topt = _torch_twin(kind, w2.params, "cuda", torch.float32, **kw)
    for _ in range(3):
        for p in tp:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen)
        topt.step()
    w2.opt.load_state_dict(topt.state_dict())
    assert w2.opt.param_groups[0]["lr"] == kw["lr"] and w2.opt.param_groups[0]["grad_scale"] == 1.0
    for p, q in zip(w2.params, tp):
        p.data.copy_(q.detach())
    before = w2.snapshot()
    assert before[-1] == (1 if kind == "SGD" else 3)
    for name in w2.dev.names:
        for i, q in enumerate(tp):
            assert torch.equal(w2.buffers(name)[i], topt.state[q][name]), (name, i)
    assert w2.intact()
    w2.randn_grads()
    before, after, grads = _one_step(w2)
    _check(w2, before, after, grads, "continuing torch's run", **rkw)


def test_sgd_none_buffer_forms_travel():
    """Before the first step, and always with momentum == 0, torch.optim.SGD holds no buffer (momentum_buffer None, or no state): both
    forms load here as step 0, and what this class writes then loads into torch.optim.SGD, whose first step clones the gradient."""
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.1)
    w = World("SGD", seed=14, **kw)
    sd = w.opt.state_dict()
    assert all(st == {"momentum_buffer": None} for st in sd["state"].values()) and len(sd["state"]) == NP
    tp, topt = _torch_twin("SGD", w.params, "cpu", torch.float64, lr=1.0, foreach=False)
    topt.load_state_dict(sd)
    w.randn_grads()
    for q, g in zip(tp, w.gviews):
        q.grad = g.double().cpu()
    topt.step()
    before, after, grads = _one_step(w)
    pr, br = _check(w, before, after, grads, "first step after the None form", wd=0.0, **kw)
    for i, q in enumerate(tp):
        assert torch.equal(q.detach(), pr[i]) and torch.equal(topt.state[q]["momentum_buffer"], br[i]), i
    # torch's own forms: no state at all (fresh), and mixed (parameter 0 had no gradient in the first step)
    w.seed_state()
    w.opt.load_state_dict(torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in w.params], **kw).state_dict())
    assert w.dev.step_count() == 0 and not bool(w.dev.momentum_buffer.any())
    tp, topt = _torch_twin("SGD", w.params, "cuda", torch.float32, **kw)
    for i, p in enumerate(tp):
        p.grad = None if i == 0 else torch.ones_like(p)
    topt.step()
    with pytest.raises(ValueError, match="dampening"):
        w.opt.load_state_dict(topt.state_dict())
    # ... which loads with dampening == 0: the missing buffer is zeroed, and the next step gives what torch's clone gives
    kw0 = dict(lr=1e-2, momentum=0.9)
    w0 = World("SGD", seed=15, **kw0)
    tp, topt = _torch_twin("SGD", w0.params, "cuda", torch.float32, **kw0)
    for i, p in enumerate(tp):
        p.grad = None if i == 0 else torch.randn_like(p)
    topt.step()
    w0.seed_state()
    w0.opt.load_state_dict(topt.state_dict())
    for p, q in zip(w0.params, tp):
        p.data.copy_(q.detach())
    before = w0.snapshot()
    assert before[-1] == 1 and not bool(before[1][0].any()) and torch.equal(before[1][5], topt.state[tp[5]]["momentum_buffer"])
    w0.randn_grads()
    _, after, grads = _one_step(w0)
    mixed = (before[0], [None] + before[1][1:], 1)
    _check(w0, mixed, after, grads, "mixed buffers, dampening 0", wd=0.0, **kw0)
    assert torch.equal(after[1][0], grads[0])  # fmaf(mu, 0, 1 * g1) == g1: the bits of a clone


# ---- captured updates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [KINDS[0], KINDS[4]], ids=[KIND_IDS[0], KIND_IDS[4]])
def test_captured_updates_replay_bit_identically(kind, kw):
    """step() captured once after prepare(): five replays equal five eager steps bit for bit (the first of them the t = 0 step), and a
    changed lr takes effect after prepare() / _sync_lr() without a new capture."""
    a, b = World(kind, seed=20, **kw), World(kind, seed=20, **kw)
    for w in (a, b):
        w.randn_grads()
    assert torch.equal(a.bucket.view, b.bucket.view)
    b.opt.prepare()  # the host side, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.opt.step()
    torch.cuda.synchronize()
    assert b.dev.step_count() == 0  # capturing ran nothing
    for _ in range(5):
        a.opt.step()
        graph.replay()
    assert a.dev.step_count() == 5 == b.dev.step_count()
    _same_bits(a.flat_state(), b.flat_state())
    for k, lr in enumerate((5e-4, 2e-3)):
        before = b.flat_state()[0]
        a.opt.param_groups[0]["lr"] = b.opt.param_groups[0]["lr"] = lr
        a.opt.step()
        b.opt.prepare() if k == 0 else b.opt._sync_lr()
        graph.replay()
        fa, fb = a.flat_state(), b.flat_state()
        _same_bits(fa, fb)
        assert float(fb[-1][0]) == lr and not torch.equal(fb[0], before)
    assert a.intact() and b.intact()

"""engine.SamplerTrainStep(optimizer=samplenet_amd.optim.SGD(...) / RMSprop(...)): the update as the last node of the captured step.

Shape B = 4, N = 1024, M = 64, K = 8 (tests/test_gpu_adam_engine.py's), three different batches.  Twin nets from one state_dict:
(a) the captured step carries the optimizer, (b) the same step issued eagerly without it, followed by opt.step() from Python.  It is the
same kernel on the same inputs and the step is deterministic: parameters, every state buffer and the step count are bit-identical
after every step."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, M, K = 4, 1024, 64, 8


def _nets(n):
    from samplenet_amd import SampleNet

    torch.manual_seed(0)
    mk = lambda: SampleNet(M, 128, group_size=K, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()  # noqa: E731
    first = mk()
    sd = copy.deepcopy(first.state_dict())
    nets = [first]
    for _ in range(n - 1):
        net = mk()
        net.load_state_dict(sd)
        nets.append(net)
    return nets


def _batches():
    g = torch.Generator(device="cuda").manual_seed(5)
    return [torch.rand(B, N, 3, device="cuda", generator=g) - 0.5 for _ in range(3)]


def _make(kind, net):
    from samplenet_amd import optim

    if kind == "SGD":
        return optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-2)
    return optim.RMSprop(net.parameters(), lr=1e-3)


def _state(net, opt):
    torch.cuda.synchronize()
    dev = opt._dev[0]
    return [p.detach().clone() for p in net.parameters()], [getattr(dev, n).clone() for n in dev.names], dev.step_count()


def _same(sa, sb, what):
    (pa, ba, ta), (pb, bb, tb) = sa, sb
    assert ta == tb and len(ba) == len(bb) > 0, what
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, "parameter", i)
    for x, y in zip(ba, bb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what


@pytest.mark.parametrize("kind", ["SGD", "RMSprop"])
def test_captured_step_with_the_update_equals_eager_step_then_update(kind):
    from samplenet_amd import SampleNet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    na, nb = _nets(2)
    xs = _batches()
    simp0, _ = na(xs[2])
    ra, rb = FlatGradAllReducer(na), FlatGradAllReducer(nb)
    oa, ob = _make(kind, na), _make(kind, nb)
    sa = SamplerTrainStep(na, xs[0], reducer=ra, optimizer=oa)
    sb = SamplerTrainStep(nb, xs[0], reducer=rb, use_graph=False)
    assert sa._update_in_graph() and len(sa._ring_graphs[0]) == 1  # one graph: the update is a node of it, not a launch behind it
    _same(_state(na, oa), _state(nb, ob), "construction trains nothing")
    assert oa._dev[0].step_count() == 0
    for i, x in enumerate(xs):
        la = sa(x)
        lb = sb(x)
        ob.step()
        torch.cuda.synchronize()
        assert float(la) == float(lb), i
        assert torch.equal(ra.flat, rb.flat), i
        st = _state(na, oa)
        _same(st, _state(nb, ob), "step %d" % i)
        assert st[2] == i + 1
    assert float(ra.flat.abs().sum()) > 0
    # the module computes something different afterwards -- and what a fresh module loaded with the new weights computes
    fresh = SampleNet(M, 128, group_size=K, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()
    fresh.load_state_dict(copy.deepcopy(na.state_dict()))
    simp_a, _ = na(xs[2])
    simp_f, _ = fresh(xs[2])
    torch.cuda.synchronize()
    assert torch.equal(simp_a, simp_f) and not torch.equal(simp_a, simp0)


def test_other_optimizers_are_still_refused():
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    net = _nets(1)[0]
    x = _batches()[0]
    for other in (torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9), torch.optim.RMSprop(net.parameters())):
        with pytest.raises(TypeError, match="Adam, SGD or RMSprop"):
            SamplerTrainStep(net, x, reducer=FlatGradAllReducer(net), optimizer=other)
    for p in net.parameters():
        p.grad = None
    from samplenet_amd.optim import SGD

    with pytest.raises(ValueError, match="gradient sink"):
        SamplerTrainStep(net, x, optimizer=SGD(net.parameters(), momentum=0.9))

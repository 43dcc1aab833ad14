"""engine.SamplerTrainStep(optimizer=samplenet_amd.optim.Adam(...)): the update as one more node of the captured step.

Shape B = 4, N = 1024, M = 64, K = 8 (the plumbing shape of smoke()), three different batches.  Twin nets from one state_dict:
(a) the step carries the optimizer, (b) the same step without it, followed by opt.step() from Python.  It is the same kernel on the
same inputs and the step is deterministic: parameters, both moment buffers and the step count are bit-identical after every step."""
import copy
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, N, M, K = 4, 1024, 64, 8


@pytest.fixture(scope="module")
def rccl():
    """torch.distributed backend "nccl" (= RCCL) at world size 1, as tests/test_gpu_rccl.py sets it up."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    torch.cuda.synchronize()
    dist.destroy_process_group()


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


def _adam(net, **kw):
    from samplenet_amd.optim import Adam

    return Adam(net.parameters(), lr=1e-3, weight_decay=1e-2, **kw)


def _state(net, opt):
    torch.cuda.synchronize()
    dev = opt._dev[0]
    return [p.detach().clone() for p in net.parameters()], dev.exp_avg.clone(), dev.exp_avg_sq.clone(), dev.step_count()


def _same(sa, sb, what):
    (pa, ma, va, ta), (pb, mb, vb, tb) = sa, sb
    assert ta == tb, what
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, "parameter", i)
    assert torch.equal(ma.view(torch.int32), mb.view(torch.int32)) and torch.equal(va.view(torch.int32), vb.view(torch.int32)), what


def _twin_run(make_reducer, **step_kw):
    """(a) with optimizer=, (b) without + opt.step(); compared after each of three steps on three batches."""
    from samplenet_amd.engine import SamplerTrainStep

    na, nb = _nets(2)
    xs = _batches()
    ra, rb = make_reducer(na), make_reducer(nb)
    oa, ob = _adam(na), _adam(nb)
    sa = SamplerTrainStep(na, xs[0], reducer=ra, optimizer=oa, **step_kw)
    sb = SamplerTrainStep(nb, xs[0], reducer=rb, **step_kw)
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
        assert st[3] == i + 1
    assert float(ra.flat.abs().sum()) > 0
    return sa, sb


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_update_inside_the_step_equals_update_behind_it(use_graph):
    from samplenet_amd.parallel import FlatGradAllReducer

    sa, sb = _twin_run(FlatGradAllReducer, use_graph=use_graph)
    assert bool(sa._ring_graphs) == use_graph and sa._update_in_graph() == use_graph
    assert len(sa._ring_graphs[0]) == 1 if use_graph else True  # one graph: the update is a node of it, not a launch behind it


@pytest.mark.parametrize("mode", ["graph", "after"])
def test_update_with_the_collective_forced(rccl, mode):
    """world size 1, all_reduce(AVG) really issued: inside the graph the update follows it as the next node; with 'after' it is a
    launch of its own behind the Python-side collective."""
    from samplenet_amd.parallel import FlatGradAllReducer

    sa, sb = _twin_run(lambda net: FlatGradAllReducer(net, force_collective=True), allreduce=mode)
    assert sa.allreduce == mode and sa.in_graph == (mode == "graph") and sa._update_in_graph() == (mode == "graph")


def test_auto_placement_probe_does_not_train(rccl):
    """allreduce='auto' captures and times three placements (tens of replays) while the step is constructed: none of them may carry
    the update."""
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    net = _nets(1)[0]
    ring = _batches()[:2]
    red = FlatGradAllReducer(net, force_collective=True)
    opt = _adam(net)
    before = _state(net, opt)
    step = SamplerTrainStep(net, ring[0], reducer=red, input_ring=ring, allreduce="auto", optimizer=opt)
    assert step.allreduce_probe is not None and step.optimizer is opt
    _same(before, _state(net, opt), "construction with allreduce='auto'")
    assert before[3] == 0
    step.replay(1)
    after = _state(net, opt)
    assert after[3] == 1 and not torch.equal(after[0][0], before[0][0])


def test_first_step_within_the_single_step_bound():
    """After (a)'s first step the parameters are within the single-step bound (tests/adam_ref.py) of torch.optim.Adam in fp64 applied
    to the gradients read back from the bucket; a parameter the reducer does not cover keeps its value."""
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    net = _nets(1)[0]
    x = _batches()[0]
    red = FlatGradAllReducer(net)
    opt = _adam(net)
    step = SamplerTrainStep(net, x, reducer=red, optimizer=opt)
    params = list(net.parameters())
    p0, m0, v0, t0 = [p.detach().clone() for p in params], None, None, 0
    zeros = [torch.zeros_like(p) for p in params]
    step(x)
    torch.cuda.synchronize()
    grads = [p.grad.detach().clone() for p in params]
    assert all(red.flat.data_ptr() <= p.grad.data_ptr() < red.flat.data_ptr() + 4 * red.flat.numel() for p in params)
    dev = opt._dev[0]
    after = ([p.detach().clone() for p in params], [dev.views(i)[0].clone() for i in range(len(params))],
             [dev.views(i)[1].clone() for i in range(len(params))], dev.step_count())
    R.check_step((p0, zeros, zeros, t0), after, grads, "engine step 1", lr=1e-3, wd=1e-2)


def test_versions_move_and_the_surface_sees_the_new_weights():
    """The kernel writes the parameters through raw pointers inside a graph replay: every updated parameter's version counter must move
    (surface.projection_loss, task_features and graphed._ModuleGuard key caches on it), and an op-by-op net(x) afterwards must compute
    with the new weights -- the same output as a fresh module loaded with them."""
    from samplenet_amd import SampleNet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    net = _nets(1)[0]
    xs = _batches()
    simp0, proj0 = net(xs[2])  # the surface has seen the module (and holds a live record of this forward) before any update
    sigma0 = float(net.get_projection_loss())
    red = FlatGradAllReducer(net)
    opt = _adam(net)
    step = SamplerTrainStep(net, xs[0], reducer=red, optimizer=opt)
    versions = [p._version for p in net.parameters()]
    tv = net.project._temperature._version
    for x in xs[:2]:
        step(x)
    torch.cuda.synchronize()
    assert net.project._temperature._version > tv
    assert all(p._version >= v + 2 for p, v in zip(net.parameters(), versions))  # at least one per step
    fresh = SampleNet(M, 128, group_size=K, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()
    fresh.load_state_dict(copy.deepcopy(net.state_dict()))
    simp_a, proj_a = net(xs[2])
    sigma_a = float(net.get_projection_loss())
    simp_f, proj_f = fresh(xs[2])
    sigma_f = float(fresh.get_projection_loss())
    torch.cuda.synchronize()
    assert torch.equal(simp_a, simp_f) and torch.equal(proj_a, proj_f) and sigma_a == sigma_f
    assert not torch.equal(simp_a, simp0) and sigma_a != sigma0  # (the update did change what the module computes)


def test_optimizer_argument_checks():
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    net = _nets(1)[0]
    x = _batches()[0]
    with pytest.raises(TypeError):
        SamplerTrainStep(net, x, reducer=FlatGradAllReducer(net), optimizer=torch.optim.Adam(net.parameters()))
    for p in net.parameters():
        p.grad = None
    with pytest.raises(ValueError):
        SamplerTrainStep(net, x, optimizer=_adam(net))

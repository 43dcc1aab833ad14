"""Host side of samplenet_amd.optim.SGD / RMSprop / make_optimizer (no GPU): the argument errors of sn_sgd_update and
sn_rmsprop_update, the parsing of torch.optim.SGD's and torch.optim.RMSprop's state-dict formats on dicts torch's own CPU optimizers
wrote, and the constructors' checks."""
import ctypes

import pytest
import torch

P = ctypes.c_void_p
BAD = 10001  # SN_ERR_BAD_ARGUMENT


def _sgd(lib, nchunks, table, buf, state, momentum=0.9, dampening=0.0, wd=0.0, gs=1.0, nesterov=0):
    return lib.sn_sgd_update(nchunks, table, buf, state, momentum, dampening, wd, gs, nesterov, None)


def _rms(lib, nchunks, table, sq, buf, state, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0, gs=1.0):
    return lib.sn_rmsprop_update(nchunks, table, sq, buf, state, alpha, eps, wd, momentum, gs, None)


def test_sgd_argument_errors_are_reported_without_a_gpu():
    from samplenet_amd._lib import lib

    ok = (P(64), P(128), P(512))  # (never dereferenced: every call below fails its checks, or has nothing to do)
    err = lib.sn_last_error_string
    assert _sgd(lib, -1, *ok) == BAD and b"negative chunk count" in err()
    assert _sgd(lib, 3, None, P(128), P(512)) == BAD and b"null chunk table" in err()
    assert _sgd(lib, 3, P(64), P(128), None) == BAD and b"null" in err()
    assert _sgd(lib, 3, P(64), None, P(512)) == BAD and b"momentum_buf" in err()                  # momentum 0.9 without a buffer
    assert _sgd(lib, 3, P(64), P(128), P(512), momentum=0.0) == BAD and b"momentum_buf" in err()  # a buffer without momentum
    assert _sgd(lib, 3, P(68), P(128), P(512)) == BAD and b"misaligned" in err()    # the table: 8 bytes
    assert _sgd(lib, 3, P(64), P(128), P(516)) == BAD and b"misaligned" in err()    # the block: 8 bytes
    assert _sgd(lib, 3, P(64), P(136), P(512)) == BAD and b"misaligned" in err()    # the buffer: 16 bytes
    assert _sgd(lib, 3, *ok, momentum=-0.1) == BAD and b"negative" in err()
    assert _sgd(lib, 3, *ok, dampening=-0.1) == BAD
    assert _sgd(lib, 3, *ok, wd=-1.0) == BAD
    assert _sgd(lib, 3, P(64), None, P(512), momentum=0.0, nesterov=1) == BAD and b"nesterov" in err()
    assert _sgd(lib, 3, *ok, dampening=0.1, nesterov=1) == BAD and b"nesterov" in err()
    assert _sgd(lib, 0, None, None, None) == 0  # no parameters: a no-op that touches nothing
    assert _sgd(lib, 0, None, None, None, momentum=-1.0) == BAD  # (the hyperparameters are checked first)


def test_rmsprop_argument_errors_are_reported_without_a_gpu():
    from samplenet_amd._lib import lib

    ok = (P(64), P(128), None, P(512))
    okm = (P(64), P(128), P(256), P(512))
    err = lib.sn_last_error_string
    assert _rms(lib, -1, *ok) == BAD and b"negative chunk count" in err()
    assert _rms(lib, 3, None, P(128), None, P(512)) == BAD and b"null chunk table" in err()
    assert _rms(lib, 3, P(64), None, None, P(512)) == BAD and b"null" in err()
    assert _rms(lib, 3, P(64), P(128), None, None) == BAD and b"null" in err()
    assert _rms(lib, 3, *ok, momentum=0.9) == BAD and b"momentum_buf" in err()   # momentum without a buffer
    assert _rms(lib, 3, *okm) == BAD and b"momentum_buf" in err()                # a buffer without momentum
    assert _rms(lib, 3, P(64), P(128), P(128), P(512), momentum=0.9) == BAD and b"distinct" in err()
    assert _rms(lib, 3, P(68), P(128), None, P(512)) == BAD and b"misaligned" in err()
    assert _rms(lib, 3, P(64), P(132), None, P(512)) == BAD and b"misaligned" in err()
    assert _rms(lib, 3, P(64), P(128), None, P(516)) == BAD and b"misaligned" in err()
    assert _rms(lib, 3, P(64), P(128), P(264), P(512), momentum=0.9) == BAD and b"misaligned" in err()
    assert _rms(lib, 3, *ok, alpha=1.0) == BAD and b"alpha" in err()
    assert _rms(lib, 3, *ok, alpha=-0.1) == BAD and b"alpha" in err()
    assert _rms(lib, 3, *ok, eps=-1e-8) == BAD and b"negative" in err()
    assert _rms(lib, 3, *ok, wd=-1.0) == BAD
    assert _rms(lib, 3, *okm, momentum=-0.9) == BAD
    assert _rms(lib, 0, None, None, None, None) == 0


def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(n)) for n in (1, 5, 64)]


def _run(opt, params, steps=1, none=()):
    for _ in range(steps):
        for i, p in enumerate(params):
            p.grad = None if i in none else torch.randn_like(p)
        opt.step()
    return opt.state_dict()


def test_sgd_parser_accepts_what_torch_sgd_writes():
    from samplenet_amd.optim import parse_sgd_state_dict

    params = _params()
    opt = torch.optim.SGD([{"params": params[:2]}, {"params": params[2:], "lr": 3e-4}], lr=1e-3, momentum=0.9, weight_decay=1e-2)
    fresh = parse_sgd_state_dict(opt.state_dict())  # before the first step torch has no state at all
    assert [g["step"] for g in fresh] == [0, 0] and not fresh[0]["buffers"]
    groups = parse_sgd_state_dict(_run(opt, params))
    assert [g["ids"] for g in groups] == [[0, 1], [2]] and [g["step"] for g in groups] == [1, 1]
    assert groups[1]["options"]["lr"] == 3e-4 and groups[0]["options"]["momentum"] == 0.9
    assert torch.equal(groups[0]["buffers"][1], opt.state[params[1]]["momentum_buffer"])
    # momentum == 0: torch keeps no buffers (an empty state, or momentum_buffer None in the form older releases and this package write)
    params = _params()
    opt = torch.optim.SGD(params, lr=1e-3)
    sd = _run(opt, params)
    assert all(not st or st.get("momentum_buffer") is None for st in sd["state"].values())
    assert parse_sgd_state_dict(sd)[0]["step"] == 0 and not parse_sgd_state_dict(sd)[0]["buffers"]
    sd["state"] = {i: {"momentum_buffer": None} for i in range(3)}
    assert parse_sgd_state_dict(sd)[0]["step"] == 0 and not parse_sgd_state_dict(sd)[0]["buffers"]


def test_sgd_parser_mixed_buffers_need_zero_dampening():
    """A parameter whose gradient was None in the first step has no buffer: with dampening == 0 the group loads (a zeroed buffer
    gives the bits a missing one gives), with dampening != 0 it cannot (one first-step flag per group)."""
    from samplenet_amd.optim import parse_sgd_state_dict

    for dampening in (0.0, 0.1):
        params = _params()
        opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, dampening=dampening)
        sd = _run(opt, params, none=(0,))
        assert 0 not in sd["state"] or sd["state"][0].get("momentum_buffer") is None
        if dampening == 0:
            g = parse_sgd_state_dict(sd)[0]
            assert g["step"] == 1 and sorted(g["buffers"]) == [1, 2]
        else:
            with pytest.raises(ValueError, match="dampening"):
                parse_sgd_state_dict(sd)
        # all buffers present: dampening of either value loads
        assert parse_sgd_state_dict(_run(opt, params))[0]["step"] == 1


def test_sgd_parser_refuses_what_the_optimizer_cannot_represent():
    from samplenet_amd.optim import parse_sgd_state_dict

    params = _params()
    sd = _run(torch.optim.SGD(params, lr=1e-3, momentum=0.9, maximize=True), params)
    with pytest.raises(ValueError, match="maximize"):
        parse_sgd_state_dict(sd)
    params = _params()
    sd = _run(torch.optim.SGD(params, lr=1e-3, momentum=0.9), params)
    sd["state"][0]["exp_avg"] = torch.zeros(1)
    with pytest.raises(ValueError, match="keys"):
        parse_sgd_state_dict(sd)
    del sd["state"][0]["exp_avg"]
    sd["param_groups"][0]["momentum"] = 0
    with pytest.raises(ValueError, match="momentum == 0"):
        parse_sgd_state_dict(sd)
    sd["param_groups"][0]["momentum"] = 0.9
    sd["state"][7] = {"momentum_buffer": None}
    with pytest.raises(ValueError, match="no group names"):
        parse_sgd_state_dict(sd)
    with pytest.raises(ValueError):
        parse_sgd_state_dict({"state": {}})


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_parser_accepts_what_torch_rmsprop_writes(momentum):
    from samplenet_amd.optim import parse_rmsprop_state_dict

    params = _params()
    opt = torch.optim.RMSprop([{"params": params[:2]}, {"params": params[2:], "lr": 3e-4}], lr=1e-3, momentum=momentum)
    fresh = parse_rmsprop_state_dict(opt.state_dict())
    assert fresh[0]["step"] == 0 and not fresh[0]["state"]
    sd = _run(opt, params, steps=2)
    keys = {"step", "square_avg"} | ({"momentum_buffer"} if momentum else set())
    assert all(set(st) == keys for st in sd["state"].values())  # the key set the loader expects
    groups = parse_rmsprop_state_dict(sd)
    assert [g["ids"] for g in groups] == [[0, 1], [2]] and [g["step"] for g in groups] == [2, 2]
    assert groups[1]["options"]["lr"] == 3e-4 and groups[0]["options"]["alpha"] == 0.99
    sq, buf = groups[0]["state"][1]
    assert torch.equal(sq, opt.state[params[1]]["square_avg"])
    assert (buf is None) if momentum == 0 else torch.equal(buf, opt.state[params[1]]["momentum_buffer"])


def test_rmsprop_parser_refuses_what_the_optimizer_cannot_represent():
    from samplenet_amd.optim import parse_rmsprop_state_dict

    params = _params()
    sd = _run(torch.optim.RMSprop(params, centered=True), params)
    assert "grad_avg" in sd["state"][0]
    with pytest.raises(ValueError, match="centered"):
        parse_rmsprop_state_dict(sd)
    sd["param_groups"][0]["centered"] = False  # (the flag cleared, the centered state still there)
    with pytest.raises(ValueError, match="keys"):
        parse_rmsprop_state_dict(sd)
    # a momentum buffer without momentum, and momentum without its buffer
    params = _params()
    sd = _run(torch.optim.RMSprop(params, momentum=0.9), params)
    sd["param_groups"][0]["momentum"] = 0
    with pytest.raises(ValueError, match="keys"):
        parse_rmsprop_state_dict(sd)
    # a parameter that missed a step: torch counts per parameter, this optimizer per group
    params = _params()
    opt = torch.optim.RMSprop(params)
    _run(opt, params)
    with pytest.raises(ValueError, match="one step count"):
        parse_rmsprop_state_dict(_run(opt, params, none=(0,)))
    with pytest.raises(ValueError):
        parse_rmsprop_state_dict({"param_groups": []})


def test_constructors_are_torchs_and_gpu_only():
    import samplenet_amd
    from samplenet_amd.optim import SGD, Adam, RMSprop, _OneLaunchOptimizer

    p = torch.nn.Parameter(torch.zeros(4))
    for cls in (SGD, RMSprop):
        with pytest.raises(RuntimeError, match="GPU only"):
            cls([p])
        with pytest.raises(ValueError):
            cls([p], lr=torch.tensor(1e-3))
        assert issubclass(cls, _OneLaunchOptimizer) and issubclass(cls, torch.optim.Optimizer)
        assert getattr(samplenet_amd.optim, cls.__name__) is cls
    assert issubclass(Adam, _OneLaunchOptimizer)
    for kw in ({"maximize": True}, {"foreach": True}, {"differentiable": True}, {"fused": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            SGD([p], **kw)
    for kw in ({"lr": -1.0}, {"momentum": -0.1}, {"dampening": -0.1}, {"weight_decay": -1.0}, {"nesterov": True},
               {"nesterov": True, "momentum": 0.9, "dampening": 0.1}):
        with pytest.raises(ValueError):
            SGD([p], **kw)
    for kw in ({"centered": True}, {"capturable": True}, {"foreach": True}, {"maximize": True}, {"differentiable": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            RMSprop([p], **kw)
    for kw in ({"lr": -1.0}, {"alpha": 1.0}, {"alpha": -0.1}, {"eps": -1e-8}, {"weight_decay": -1.0}, {"momentum": -0.9}):
        with pytest.raises(ValueError):
            RMSprop([p], **kw)


def test_make_optimizer_names_the_three():
    """registration/main.py:166-171: Adam(lr=1e-3), RMSprop(lr=0.001), SGD(lr=0.001, momentum=0.9).  (No GPU here: the classes are
    reached, then refuse the CPU parameter; an empty parameter list shows the hyperparameters.)"""
    from samplenet_amd import optim

    p = torch.nn.Parameter(torch.zeros(4))
    for name in ("Adam", "RMSProp", "SGD"):
        with pytest.raises(RuntimeError, match="GPU only"):
            optim.make_optimizer(name, [p])
    for name in ("adam", "RMSprop", "Momentum", None):
        with pytest.raises(ValueError, match="one of"):
            optim.make_optimizer(name, [p])
    empty = [torch.nn.Parameter(torch.zeros(0))]  # (a group of empty tensors owns no device memory)
    a, r, s = (optim.make_optimizer(n, empty) for n in ("Adam", "RMSProp", "SGD"))
    assert type(a) is optim.Adam and a.defaults["lr"] == 1e-3 and a.defaults["betas"] == (0.9, 0.999)
    assert type(r) is optim.RMSprop and r.defaults["lr"] == 1e-3 and r.defaults["alpha"] == 0.99 and r.defaults["momentum"] == 0
    assert type(s) is optim.SGD and s.defaults["lr"] == 1e-3 and s.defaults["momentum"] == 0.9 and s.defaults["dampening"] == 0
    assert not s.defaults["nesterov"]

"""Host side of samplenet_amd.optim.Adam (no GPU): sn_adam_update's argument errors, the chunk table as a pure host function, and the
parsing of torch.optim.Adam's state-dict format."""
import ctypes

import pytest
import torch

SIZES = (1, 3, 5, 64, 1023, 1025, 4097)


def _update(lib, nchunks, table, m, v, state, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gs=1.0, tf=0):
    return lib.sn_adam_update(nchunks, table, m, v, state, b1, b2, eps, wd, gs, tf, None)


def test_argument_errors_are_reported_without_a_gpu():
    from samplenet_amd._lib import lib

    P = ctypes.c_void_p
    ok = (P(64), P(128), P(256), P(512))  # (never dereferenced: every call below fails its checks, or has nothing to do)
    assert _update(lib, -1, *ok) == 10001 and b"negative" in lib.sn_last_error_string()
    assert _update(lib, 3, None, P(128), P(256), P(512)) == 10001 and b"null chunk table" in lib.sn_last_error_string()
    assert _update(lib, 3, P(64), None, P(256), P(512)) == 10001 and b"null" in lib.sn_last_error_string()
    assert _update(lib, 3, P(64), P(128), None, P(512)) == 10001
    assert _update(lib, 3, P(64), P(128), P(256), None) == 10001
    assert _update(lib, 3, P(64), P(128), P(128), P(512)) == 10001 and b"distinct" in lib.sn_last_error_string()
    assert _update(lib, 3, P(64), P(132), P(256), P(512)) == 10001 and b"misaligned" in lib.sn_last_error_string()
    assert _update(lib, 3, *ok, b1=1.0) == 10001 and b"betas" in lib.sn_last_error_string()
    assert _update(lib, 3, *ok, b2=-0.1) == 10001
    assert _update(lib, 3, *ok, eps=-1.0) == 10001
    assert _update(lib, 3, *ok, wd=-1.0) == 10001
    assert _update(lib, 0, None, None, None, None) == 0  # no parameters: a no-op
    assert lib.sn_adam_chunk_elems() == 1024 and lib.sn_adam_state_bytes() == 64


def test_chunk_table_construction():
    from samplenet_amd.optim import CHUNK, build_chunk_table, pack_chunk_table, plan_segments

    assert CHUNK == 1024
    offsets, total = plan_segments(SIZES)
    assert all(o % 4 == 0 for o in offsets) and total % 4 == 0  # every moment segment starts on a 16-byte boundary
    assert offsets == [0, 4, 8, 16, 80, 1104, 2132] and total == 2132 + 4100
    for (o, n), o2 in zip(zip(offsets, SIZES), offsets[1:] + [total]):
        assert o + n <= o2  # segments do not overlap
    # parameters at arbitrary 4-byte aligned addresses; gradients packed in one unpadded buffer (odd offsets), one of them None
    pp = [0x10000 * (i + 1) + 4 * i for i in range(len(SIZES))]
    gp, off = [], 0
    for n in SIZES:
        gp.append(0x900000 + 4 * off)
        off += n
    gp[4] = None
    table = build_chunk_table(pp, gp, SIZES)
    per_tensor = [sum(1 for e in table if pp[i] <= e[0] < pp[i] + 4 * SIZES[i]) for i in range(len(SIZES))]
    assert per_tensor == [1, 1, 1, 1, 1, 2, 5] and len(table) == 12
    for i, n in enumerate(SIZES):
        mine = [e for e in table if pp[i] <= e[0] < pp[i] + 4 * n]
        assert sum(e[3] for e in mine) == n and all(1 <= e[3] <= CHUNK for e in mine)  # no chunk crosses a tensor
        covered = 0
        for p, g, moff, cnt in mine:  # in order, contiguous, the three addresses advance together
            assert p == pp[i] + 4 * covered and moff == offsets[i] + covered and moff % 4 == 0
            assert g == (0 if gp[i] is None else gp[i] + 4 * covered)
            covered += cnt
    assert [e[1] for e in table if pp[4] <= e[0] < pp[4] + 4 * SIZES[4]] == [0]  # the None gradient: a skipped chunk
    assert sum(1 for e in table if e[1] == 0) == 1
    blob = pack_chunk_table(table)
    assert len(blob) == 32 * len(table)
    import struct

    assert struct.unpack_from("<QQqii", blob, 32 * 5) == table[5] + (0,)
    assert build_chunk_table([], [], []) == []
    assert len(build_chunk_table([64], [128], [4097], chunk=64)) == 65
    with pytest.raises(ValueError):
        build_chunk_table([66], [128], [4])  # a misaligned parameter address
    with pytest.raises(ValueError):
        build_chunk_table([64], [128], [4], chunk=6)


def _torch_adam_state_dict(amsgrad=False, steps=2):
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n)) for n in (1, 5, 64)]
    opt = torch.optim.Adam([{"params": params[:2]}, {"params": params[2:], "lr": 3e-4}], lr=1e-3, weight_decay=1e-2, amsgrad=amsgrad)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
    return opt, params


def test_parser_accepts_what_torch_adam_writes():
    from samplenet_amd.optim import parse_state_dict

    opt, params = _torch_adam_state_dict()
    sd = opt.state_dict()
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())  # the key set the loader expects
    groups = parse_state_dict(sd)
    assert [g["ids"] for g in groups] == [[0, 1], [2]] and [g["step"] for g in groups] == [2, 2]
    assert groups[1]["options"]["lr"] == 3e-4 and groups[0]["options"]["weight_decay"] == 1e-2
    assert torch.equal(groups[0]["moments"][1][0], opt.state[params[1]]["exp_avg"])
    assert torch.equal(groups[1]["moments"][2][1], opt.state[params[2]]["exp_avg_sq"])
    # before the first step torch has no state at all: step 0, no moments
    fresh = parse_state_dict(torch.optim.Adam(params).state_dict())
    assert fresh[0]["step"] == 0 and not fresh[0]["moments"]


def test_parser_refuses_what_the_optimizer_cannot_represent():
    from samplenet_amd.optim import parse_state_dict

    opt, params = _torch_adam_state_dict(amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        parse_state_dict(opt.state_dict())
    opt, params = _torch_adam_state_dict()
    sd = opt.state_dict()
    sd["state"][0]["max_exp_avg_sq"] = torch.zeros(1)
    with pytest.raises(ValueError, match="keys"):
        parse_state_dict(sd)
    del sd["state"][0]["max_exp_avg_sq"]  # (the dict shares the optimizer's own state)
    # a parameter that missed a step (its gradient was None once): torch counts per parameter, this optimizer per group
    params[0].grad = None
    params[1].grad = torch.randn_like(params[1])
    opt.step()
    with pytest.raises(ValueError, match="one step count"):
        parse_state_dict(opt.state_dict())
    with pytest.raises(ValueError):
        parse_state_dict({"state": {}})


def test_constructor_is_torch_adams_and_gpu_only():
    from samplenet_amd.optim import Adam

    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        Adam([p])
    for kw in ({"amsgrad": True}, {"maximize": True}, {"foreach": True}, {"fused": True}, {"capturable": True},
               {"differentiable": True}, {"decoupled_weight_decay": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Adam([p], **kw)
    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}, {"eps": -1e-8}, {"weight_decay": -1.0}):
        with pytest.raises(ValueError):
            Adam([p], **kw)
    import samplenet_amd

    assert samplenet_amd.optim.Adam is Adam and issubclass(Adam, torch.optim.Optimizer)

"""sn_ball_query on the device, called directly into poisoned and guarded buffers: every shape row x recipe x rule of
tests/ball_ref.py (and every layout pair a row lists) must give idx and pts_cnt bit for bit, with the guards intact, every element
written -- empty balls included -- and the same bits from a second call.  Then the Python surface over it: ops.ball_query,
ops.query_ball_point and the pointnet2_utils stand-in's ball_query."""
import numpy as np
import pytest
import torch

import ball_ref as R
from cabi_ref import Guarded

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["x".join(map(str, s[0])) for s in R.SHAPES]
_REF = {}  # (shape, recipe id, rule) -> (idx, cnt): computed once, shared, never changed


def case(shape, recipe):
    key = (shape, recipe[0])
    if key not in _REF:
        P, Q, radius = R.make_case(shape, recipe)
        refs = {}
        for rule in R.RULES:
            refs[rule] = R.ball_query(P, Q, radius, shape[3], rule)
            for a in refs[rule]:
                a.setflags(write=False)
        _REF[key] = (P, Q, radius, refs)
    return _REF[key]


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _call(lib, shape, radius, rule, P, l1, Q, l2, with_cnt=True):
    b, n, m, ns = shape
    dP, dQ = dev(R.lay(P, l1)), dev(R.lay(Q, l2))
    idx, cnt = Guarded((b, m, ns), torch.int32), Guarded((b, m), torch.int32)
    rc = lib.sn_ball_query(b, n, m, float(radius), ns, rule, dP.data_ptr(), l1, dQ.data_ptr(), l2, idx.ptr(), cnt.ptr() if with_cnt else None,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return idx, cnt


@pytest.mark.parametrize("recipe", R.RECIPES, ids=R.RECIPE_IDS)
@pytest.mark.parametrize("row", R.SHAPES, ids=SHAPE_IDS)
def test_ball_query_bit_for_bit(row, recipe):
    from samplenet_amd._lib import lib

    shape, _, layouts = row
    P, Q, radius, refs = case(shape, recipe)
    for rule in R.RULES:
        want_idx, want_cnt = refs[rule]
        for l1, l2 in layouts:
            what = "rule %d layouts %d,%d" % (rule, l1, l2)
            idx, cnt = _call(lib, shape, radius, rule, P, l1, Q, l2)
            got_idx, got_cnt = idx.check(what + " idx").cpu().numpy(), cnt.check(what + " pts_cnt").cpu().numpy()
            assert np.array_equal(got_cnt, want_cnt), what
            assert np.array_equal(got_idx, want_idx), what
            idx2, cnt2 = _call(lib, shape, radius, rule, P, l1, Q, l2)
            assert torch.equal(idx2.raw, idx.raw) and torch.equal(cnt2.raw, cnt.raw), what + ": second call"
    if recipe[0] == "boundary":  # the rules must be told apart: here their results differ
        assert not (np.array_equal(refs[R.SQRT][0], refs[R.SQUARED][0]) and np.array_equal(refs[R.SQRT][1], refs[R.SQUARED][1]))


def test_pts_cnt_may_be_null():
    from samplenet_amd._lib import lib

    shape = (2, 65, 7, 3)
    P, Q, radius, refs = case(shape, R.RECIPES[1])
    idx, cnt = _call(lib, shape, radius, R.SQRT, P, R.BNC, Q, R.BNC, with_cnt=False)
    assert np.array_equal(idx.check("idx").cpu().numpy(), refs[R.SQRT][0]) and cnt.untouched()


@pytest.mark.parametrize("radius", [float("nan"), -1.0, 0.0, -float("inf")])
def test_radius_without_a_ball_gives_empty_rows(radius):
    """NaN or a radius <= 0: every row zeros with count 0 under both rules, queries on top of dataset points included"""
    from samplenet_amd._lib import lib

    shape = (2, 65, 7, 3)
    P, Q, _ = R.copies(shape, 1e-3)
    for rule in R.RULES:
        idx, cnt = _call(lib, shape, radius, rule, P, R.BNC, Q, R.BNC)
        assert not idx.check("idx").any() and not cnt.check("cnt").any()
        assert not R.ball_query(P, Q, radius, 3, rule)[1].any()


def test_infinite_radius_takes_the_first_points():
    from samplenet_amd._lib import lib

    shape = (2, 200, 33, 70)
    P, Q, _ = R.uniform(shape, 0.3)
    for rule in R.RULES:
        idx, cnt = _call(lib, shape, float("inf"), rule, P, R.BNC, Q, R.BNC)
        assert bool((idx.check("idx") == torch.arange(70, device="cuda", dtype=torch.int32)).all()) and bool((cnt.check("cnt") == 70).all())


def test_python_surface():
    from samplenet_amd import ops
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    shape = (3, 257, 9, 16)
    P, Q, radius, refs = case(shape, [r for r in R.RECIPES if r[0] == "boundary"][0])
    dP, dQ = dev(P), dev(Q)
    for name, rule in (("sqrt", R.SQRT), ("squared", R.SQUARED)):
        idx, cnt = ops.ball_query(float(radius), 16, dP, dQ, rule=name)
        assert idx.dtype == torch.int32 and cnt.dtype == torch.int32 and idx.shape == (3, 9, 16) and cnt.shape == (3, 9)
        assert np.array_equal(idx.cpu().numpy(), refs[rule][0]) and np.array_equal(cnt.cpu().numpy(), refs[rule][1])
        # channel-major operands, each on its own selector; non-contiguous views are made contiguous
        idx2, cnt2 = ops.ball_query(float(radius), 16, dP.transpose(1, 2).contiguous(), dQ.transpose(1, 2), rule=name, layout=ops.BCN)
        assert torch.equal(idx2, idx) and torch.equal(cnt2, cnt)
        idx3, _ = ops.ball_query(float(radius), 16, dP.transpose(1, 2).contiguous(), dQ, rule=name, layout=ops.BNC, xyz_layout=ops.BCN)
        assert torch.equal(idx3, idx)
    idx, cnt = ops.query_ball_point(float(radius), 16, dP, dQ)  # the TF op: the reference's rule
    assert np.array_equal(idx.cpu().numpy(), refs[R.SQRT][0]) and np.array_equal(cnt.cpu().numpy(), refs[R.SQRT][1])
    idx = PU.ball_query(float(radius), 16, dP, dQ)              # the pointnet2 stand-in: the squared rule, indices only
    assert isinstance(idx, torch.Tensor) and np.array_equal(idx.cpu().numpy(), refs[R.SQUARED][0])
    assert not np.array_equal(refs[R.SQRT][1], refs[R.SQUARED][1])
    with pytest.raises(ValueError):
        ops.ball_query(0.1, 4, dP[:, :, :2], dQ)
    assert ops.ball_query(0.1, 4, dP[:0], dQ[:0])[0].shape == (0, 9, 4)

"""sn_three_nn on the device, called by raw pointer into poisoned and guarded buffers, over every shape row and input recipe of
tests/interp_ref.py: idx, dist2 and dist bit for bit the numpy float32 restatement (dist is the correctly rounded sqrtf of dist2,
which numpy's float32 sqrt is too); where the known cloud has three points or more, idx and dist2 bit for bit ops.knn(3, ..), an
independent kernel of this library (a wave per query) -- on the rows whose three slots are filled: sn_knn has no rule for a NaN
distance, and the only such rows are those of the nan recipe at m = 3, which the test asserts --; every case twice, bit for bit;
guards untouched; each of dist / dist2 optional."""
import numpy as np
import pytest
import torch

import interp_ref as R
from cabi_ref import Guarded, bits as _bits, stream as _stream

pytestmark = pytest.mark.gpu
_REF = {}


def case(shape, recipe):
    key = (shape, recipe)
    if key not in _REF:
        u, k = R.make_case(shape, recipe)
        idx, d2 = R.three_nn(u, k)
        for a in (u, k, idx, d2):
            a.setflags(write=False)
        _REF[key] = (u, k, idx, d2)
    return _REF[key]


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _run(lib, shape, du, dk, with_d2=True, with_d=True):
    b, n, m = shape[:3]
    d2, d, idx = Guarded((b, n, 3)), Guarded((b, n, 3)), Guarded((b, n, 3), torch.int32)
    rc = lib.sn_three_nn(b, n, m, du.data_ptr(), dk.data_ptr(), d2.ptr() if with_d2 else None, d.ptr() if with_d else None, idx.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return d2, d, idx


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_three_nn_bit_for_bit(shape, recipe):
    from samplenet_amd import ops
    from samplenet_amd._lib import lib

    b, n, m = shape[:3]
    u, k, want_idx, want_d2 = case(shape, recipe)
    du, dk = dev(u), dev(k)
    d2, d, idx = _run(lib, shape, du, dk)
    got_idx = idx.check("idx").cpu().numpy()
    assert ((got_idx >= 0) & (got_idx < m)).all()
    assert np.array_equal(got_idx, want_idx)
    assert np.array_equal(_bits(d2.check("dist2").cpu().numpy()), _bits(want_d2))
    assert np.array_equal(_bits(d.check("dist").cpu().numpy()), _bits(np.sqrt(want_d2)))
    if m >= 3:
        ki, kd = ops.knn(3, dk, du, ref_layout=ops.BNC, query_layout=ops.BNC)
        filled = np.isfinite(want_d2).all(-1)                     # (b,n)
        assert filled.all() or (recipe == "nan" and m == 3)
        assert np.array_equal(ki.cpu().numpy()[filled], want_idx[filled])
        assert np.array_equal(_bits(kd.cpu().numpy())[filled], _bits(want_d2)[filled])
    again = _run(lib, shape, du, dk)
    assert torch.equal(again[0].raw, d2.raw) and torch.equal(again[1].raw, d.raw) and torch.equal(again[2].raw, idx.raw)


@pytest.mark.parametrize("with_d2,with_d", [(True, False), (False, True), (False, False)])
def test_each_distance_output_is_optional(with_d2, with_d):
    from samplenet_amd._lib import lib

    shape = (2, 257, 65, 16, 1)
    u, k, want_idx, want_d2 = case(shape, "lattice")
    d2, d, idx = _run(lib, shape, dev(u), dev(k), with_d2, with_d)
    assert np.array_equal(idx.check("idx").cpu().numpy(), want_idx)
    assert np.array_equal(_bits(d2.check("dist2").cpu().numpy()), _bits(want_d2)) if with_d2 else d2.untouched()
    assert np.array_equal(_bits(d.check("dist").cpu().numpy()), _bits(np.sqrt(want_d2))) if with_d else d.untouched()


def test_python_surface():
    from samplenet_amd import ops
    from samplenet_amd.compat.pointnet2.utils import pointnet2_utils as PU

    shape = (3, 65, 4, 5, 0)
    u, k, want_idx, want_d2 = case(shape, "lattice")
    du, dk = dev(u).requires_grad_(True), dev(k)
    for fn in (ops.three_nn, PU.three_nn):
        dist, idx = fn(du, dk)
        assert not dist.requires_grad and idx.dtype == torch.int32 and dist.shape == idx.shape == (3, 65, 3)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(_bits(dist.cpu().numpy()), _bits(np.sqrt(want_d2)))
    with pytest.raises(ValueError):
        ops.three_nn(du[:, :, :2], dk)
    with pytest.raises(ValueError):
        ops.three_nn(du, dk[:2])
    with pytest.raises(ValueError):
        ops.three_nn(du, dk[:, :0])

"""sn_gather_invert on the device, called by raw pointer into poisoned and guarded buffers, over every shape row and index recipe of
tests/gather_inv_ref.py: start and order equal the numpy restatement element for element, the -1 tail included; every element of
both outputs written, guards untouched; every case twice, bit for bit.  Past the declared bound the entry returns
SN_ERR_UNSUPPORTED and writes nothing.  ops.gather_invert returns the same pair."""
import numpy as np
import pytest
import torch

import gather_inv_ref as G
from cabi_ref import UNSUPPORTED, Guarded, stream as _stream

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.tensor(a, device="cuda")  # (a copy: the shared references are read-only)


def _run(lib, b, n, ne, didx):
    start, order = Guarded((b, n + 1), torch.int32), Guarded((b, ne), torch.int32)
    rc = lib.sn_gather_invert(b, n, ne, didx.data_ptr(), start.ptr(), order.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return start, order


@pytest.mark.parametrize("recipe", G.INDEX_RECIPES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
def test_invert_equals_the_restatement(shape, recipe):
    from samplenet_amd._lib import lib

    b, c, n, m, k = shape
    ref = G.case(shape, recipe)
    didx = dev(ref["idx"])
    start, order = _run(lib, b, n, m * k, didx)
    got_start, got_order = start.check("start").cpu().numpy(), order.check("order").cpu().numpy()
    assert np.array_equal(got_start, ref["start"])
    assert np.array_equal(got_order, ref["order"])
    again = _run(lib, b, n, m * k, didx)
    assert torch.equal(again[0].raw, start.raw) and torch.equal(again[1].raw, order.raw)


def test_past_the_bound_nothing_is_written():
    from samplenet_amd._lib import lib

    n, ne = 1 << 20, 4097      # 16384 groups of 64 rows * 4097 entries: 16384 past 2^26
    assert not G.supported(n, ne) and G.supported(n, ne - 1) and lib.sn_gather_invert_supported(n, ne) == 0
    didx = torch.zeros(1, ne, dtype=torch.int32, device="cuda")
    start, order = Guarded((1, n + 1), torch.int32), Guarded((1, ne), torch.int32)
    rc = lib.sn_gather_invert(1, n, ne, didx.data_ptr(), start.ptr(), order.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and b"sn_gather_invert_supported" in lib.sn_last_error_string()
    assert start.untouched() and order.untouched()


def test_python_surface():
    from samplenet_amd import ops

    shape = (2, 16, 65, 257, 3)
    b, c, n, m, k = shape
    ref = G.case(shape, "oob")
    for idx in (dev(ref["idx"]), dev(ref["idx"]).long(), dev(ref["idx"]).view(b, m * k)):
        inv = ops.gather_invert(idx, n)
        assert isinstance(inv, ops.GatherInverse) and inv.start.dtype == inv.order.dtype == torch.int32
        assert np.array_equal(inv.start.cpu().numpy(), ref["start"]) and np.array_equal(inv.order.cpu().numpy(), ref["order"])
    empty = ops.gather_invert(dev(ref["idx"]), 0)        # no destination row: every entry is invalid, nothing is launched
    assert empty.start.shape == (b, 1) and not empty.start.any()
    with pytest.raises(ValueError):
        ops.gather_invert(dev(ref["idx"]).float(), n)
    with pytest.raises(ValueError):
        ops.gather_invert(dev(ref["idx"])[0, 0], n)
    with pytest.raises(ValueError):
        ops.gather_invert(torch.zeros(1, 4097, dtype=torch.int32, device="cuda"), 1 << 20)

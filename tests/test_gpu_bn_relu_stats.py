"""sn_bn_relu_backward_stats on the device, called directly into poisoned and guarded buffers: dy bit for bit its sibling
sn_bn_relu_backward(with_scale = 0), the partial-sum blocks bit for bit the restated block / slice order (tests/fp_rows_ref.py), the
coefficients sn_bn_backward_coef forms from them against float64 within bounds counted from that order, twice with equal bits.

The counted bound: an element of a block's sum carries 1 + ceil(256 / S) + S roundings (the product, a slice's adds, the slices'
adds: fp_rows_ref.block_sum_roundings), so the sums over all rows are off by at most that many 2^-24 of sum|term|;
sn_bn_backward_coef adds the blocks and forms dgamma = invstd (sz - mean s) and the dZ coefficients in double and rounds each
result to float32 once: 2^-24 of its magnitude, 2^-23 allowed (tests/test_gpu_group_pool.py's allowance)."""
import numpy as np
import pytest
import torch

import fp_rows_ref as FR
from cabi_ref import Guarded, stream as _stream

pytestmark = pytest.mark.gpu


def _run(lib, rows, C, z, coef, g):
    nblk = lib.sn_bn_relu_stats_blocks(rows)
    dy, stats = Guarded((rows, C)), Guarded((nblk, 2, C))
    rc = lib.sn_bn_relu_backward_stats(rows, C, z.data_ptr(), coef.data_ptr(), g.data_ptr(), dy.ptr(), stats.ptr(), _stream())
    assert rc == 0, lib.sn_last_error_string()
    torch.cuda.synchronize()
    return dy, stats, nblk


@pytest.mark.parametrize("C", FR.STATS_C)
@pytest.mark.parametrize("rows", FR.STATS_R)
def test_dy_blocks_and_coefficients(rows, C):
    from samplenet_amd._lib import lib

    z_np, coef_np, g_np = FR.stats_case(rows, C)
    z, coef, g = (torch.tensor(a, device="cuda") for a in (z_np, coef_np, g_np))
    dy, stats, nblk = _run(lib, rows, C, z, coef, g)
    assert nblk == FR.stats_blocks(rows)
    sib = torch.full((rows, C), 7.0, device="cuda")
    assert lib.sn_bn_relu_backward(rows, C, z.data_ptr(), coef.data_ptr(), g.data_ptr(), 0, sib.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dy.check("dy").view(torch.int32), sib.view(torch.int32)), "dy differs from sn_bn_relu_backward"
    dy_np = dy.numpy()
    assert np.array_equal(dy_np.view(np.int32), FR.mask_dy(z_np, coef_np, g_np).view(np.int32))
    assert np.array_equal(stats.check("stats").cpu().numpy().view(np.int32), FR.block_sums(dy_np, z_np).view(np.int32)), "block order"
    dy2, stats2, _ = _run(lib, rows, C, z, coef, g)
    assert torch.equal(dy2.raw, dy.raw) and torch.equal(stats2.raw, stats.raw)

    # the coefficients out of sn_bn_backward_coef against float64 of the terms
    outs = [torch.empty(C, device="cuda") for _ in range(3)] + [torch.empty(3, C, device="cuda")]
    assert lib.sn_bn_backward_coef(nblk, C, rows, stats.ptr(), coef.data_ptr(), *(t.data_ptr() for t in outs), _stream()) == 0
    torch.cuda.synchronize()
    dgam, dbet, _, kc = (t.cpu().numpy().astype(np.float64) for t in outs)
    d64 = dy_np.astype(np.float64)
    t1 = d64 * z_np.astype(np.float64)
    s, sz = d64.sum(0), t1.sum(0)
    k = FR.block_sum_roundings(C)
    ds, dsz = k * FR.U * np.abs(d64).sum(0), k * FR.U * np.abs(t1).sum(0)
    scale, mean, invstd = (coef_np[i].astype(np.float64) for i in (0, 2, 3))
    dg = invstd * (sz - mean * s)
    ddg = invstd * (dsz + np.abs(mean) * ds)
    RND = 2.0 ** -23 + 2.0 ** -40
    k2 = -scale * invstd * dg / rows
    k3 = scale * (invstd * mean * dg / rows - s / rows)
    worst = 0.0
    for what, got, ref, bound in (("dgamma", dgam, dg, ddg), ("dbeta", dbet, s, ds), ("k2", kc[1], k2, np.abs(scale) * invstd * ddg / rows),
                                  ("k3", kc[2], k3, np.abs(scale) * (invstd * np.abs(mean) * ddg + ds) / rows)):
        # (k3 is a difference of two rounded terms: its rounding allowance is taken on the terms' magnitudes)
        mag = np.abs(ref) if what != "k3" else np.abs(scale) * (invstd * np.abs(mean * dg) + np.abs(s)) / rows
        tol = bound + RND * np.maximum(mag, np.abs(got))
        err = np.abs(got - ref)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), what
    assert np.array_equal(kc[0], scale)
    print("bn relu stats R %d C %d: worst coefficient error / bound %.3g" % (rows, C, worst))


def test_stats_blocks():
    from samplenet_amd._lib import lib

    assert [lib.sn_bn_relu_stats_blocks(r) for r in (0, 1, 256, 257, 515)] == [0, 1, 1, 2, 3]

"""The recipes and shape tables of tests/fc_chain_ref.py, kept honest on the CPU (no GPU): the `_supported` answers restated in Python
(LDS formula included, constants read from the sources) against the library over a grid and on every table row; every `integer`
backward case proven exact -- each intermediate and output of the fp64 reference representable in fp32 and, for every fp32 sum, the sum
of |terms| below 2^24 units of the terms' common power of two, so that ANY summation order gives the same bits and "bit for bit" on the
GPU tests the kernel and not the recipe; and the integer recipes shown to hold what tells the mask `> 0` from `>= 0`."""
import ctypes
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fc_chain_ref as F  # noqa: E402

K = F.source_constants()
CPU = torch.device("cpu")


def test_constants_are_read_from_the_sources():
    assert K == {"kRsPitch": 20, "kRsFloats": 5120, "kFcChainMaxLayers": 4, "kFcBwdMaxStages": 5, "kFcSyncStride": F.SYNC_STRIDE}, K


def test_forward_supported_over_a_grid_and_on_the_table():
    from samplenet_amd._lib import lib

    for R, C0, Hh, nl in itertools.product((-1, 0, 1, 5, 32, 33), (0, 32, 64, 96, 128, 192, 256, 512), (128, 256, 512), range(0, 7)):
        assert lib.sn_fc_chain_forward_supported(R, C0, Hh, nl) == F.fwd_supported(R, C0, Hh, nl, K), (R, C0, Hh, nl)
    for (C0, nl), (branch, ok) in F.FWD_TABLE.items():
        for R in F.ROWS_FULL:
            assert lib.sn_fc_chain_forward_supported(R, C0, F.H, nl) == int(ok) == F.fwd_supported(R, C0, F.H, nl, K), (C0, nl, branch)
    # the figures the table quotes
    assert F.fwd_lds_bytes(256, 256, 3, K) == 162816 and F.fwd_lds_bytes(64, 256, 4, K) == 171520
    assert F.fwd_lds_bytes(128, 256, 4, K) == 179712 and F.fwd_lds_bytes(256, 256, 4, K) == 196096
    # every instantiation and every refusal has a row
    assert {(128, 3), (256, 3)} <= set(F.FWD_TABLE) and sum(ok for _, ok in F.FWD_TABLE.values()) == 6
    assert {nl for (_, nl), (_, ok) in F.FWD_TABLE.items() if ok} == {2, 3} and set(F.FWD_FULL_ROWS) <= set(F.FWD_TABLE)


def test_pool_supported_over_a_grid():
    from samplenet_amd._lib import lib

    for B, N, C0, Hh, nl in itertools.product((0, 1, 32, 33), (0, 32, 64, 96, 1024, 2048), (64, 128, 256), (128, 256), (2, 3, 4)):
        assert lib.sn_fc_chain_forward_pool_supported(B, N, C0, Hh, nl) == F.pool_supported(B, N, C0, Hh, nl), (B, N, C0, Hh, nl)
        for Co in (0, 16, 32, 48, 96, 256, 288):
            assert lib.sn_fc_chain_forward_pool_out_supported(B, N, C0, Hh, nl, Co) == F.pool_out_supported(B, N, C0, Hh, nl, Co)


def _bwd_lib(R, Co, Ci):
    from samplenet_amd._lib import lib

    n = len(Co)
    return lib.sn_fc_chain_backward_supported(R, n, ctypes.cast((ctypes.c_int * max(n, 1))(*Co), ctypes.c_void_p),
                                              ctypes.cast((ctypes.c_int * max(n, 1))(*Ci), ctypes.c_void_p))


def test_backward_supported_over_a_grid_and_on_the_table():
    from samplenet_amd._lib import lib

    widths_o, widths_i = (0, 32, 64, 128, 192, 256, 320), (0, 16, 32, 96, 160, 256, 288)
    for R in (0, 1, 32, 33):
        for co0, ci0, ci1 in itertools.product(widths_o, widths_i, widths_i):
            Co, Ci = (co0, ci0), (ci0, ci1)
            assert _bwd_lib(R, Co, Ci) == F.bwd_supported(R, 2, Co, Ci, K), (R, Co, Ci)
        for ns in range(1, 8):
            Co, Ci = (256,) * ns, (256,) * ns
            assert _bwd_lib(R, Co, Ci) == F.bwd_supported(R, ns, Co, Ci, K), (R, ns)
    assert _bwd_lib(4, (256, 128), (256, 128)) == 0 == F.bwd_supported(4, 2, (256, 128), (256, 128), K)  # Co[1] != Ci[0]
    assert _bwd_lib(4, (256, 128, 128), (128, 128, 64)) == 0                                               # an inner Ci != 256
    assert lib.sn_fc_chain_backward_supported(4, 2, None, None) == 0
    for Co, Ci, branch in F.BWD_TABLE:
        for R in F.ROWS_FULL:
            assert _bwd_lib(R, Co, Ci) == 1 == F.bwd_supported(R, len(Co), Co, Ci, K), branch
    # the branches the table must keep: the depths 2..5, Co[0] = 64, a last Ci of 32, 96 and one that is no power of two times 32
    assert {len(Co) for Co, _, _ in F.BWD_TABLE} == {2, 3, 4, 5}
    assert any(Co[0] == 64 for Co, _, _ in F.BWD_TABLE) and {32, 96, 128, 160, 224} <= {Ci[-1] for _, Ci, _ in F.BWD_TABLE}
    assert set(F.INT_BWD_ROWS) == set(range(len(F.BWD_TABLE))) and all(32 in F.INT_BWD_ROWS[i] for i in (0, 1)) and set(F.INT_OBN_ROWS) == set(F.INT_BWD_ROWS)


INT_CASES = ([(i, R, None) for i in sorted(F.INT_BWD_ROWS) for R in F.INT_BWD_ROWS[i]] +
             [(i, R, obn) for i in sorted(F.INT_OBN_ROWS) for R in F.INT_OBN_ROWS[i] for obn in (0, 1)])


@pytest.mark.parametrize("idx,R,obn", INT_CASES, ids=["shape%d-R%d-obn%s" % c for c in INT_CASES])
def test_integer_backward_cases_are_exact_in_any_order(idx, R, obn):
    c = F.bwd_case("integer", idx, R, CPU, obn=obn)
    trace = []
    ref = F.bwd_ref(c, trace=trace)
    for name, (val, bound) in ref.items():
        assert F.fp32_exact(val), ("output", name)
    nsums = 0
    for entry in trace:
        if entry[0] == "value":
            assert F.fp32_exact(entry[2]), ("intermediate", entry[1], float(entry[2].abs().max()), F.unit_of(entry[2]))
        else:
            _, name, mag, factors = entry
            unit = 1.0
            for f in factors:
                unit *= F.unit_of(f)
            assert float(mag.max()) < 2.0 ** 24 * unit, ("sum", name, float(mag.max()), unit)
            nsums += 1
    assert nsums == 4 * c.ns + 1
    # the inputs are what the recipe promises
    for s in range(c.ns):
        sc, inv = c.coef[s][0], c.coef[s][3]
        assert bool(((sc.abs() == 1) | (sc.abs() == 2)).all()) and bool((inv == F.int_invstd(R)).all()) and F.int_invstd(R) ** 2 in (R, 2 * R)
        assert all(bool((t == t.round()).all()) for t in (c.zprev[s], c.coef[s][1], c.coef[s][2], c.W[s], c.gy))
        assert c.bn_rows[s] == R and 1.0 / R == 2.0 ** -(R.bit_length() - 1)


@pytest.mark.parametrize("idx", sorted(F.INT_BWD_ROWS))
def test_integer_backward_cases_hold_exact_zeros_and_negatives(idx):
    """Every stage has an exactly zero pre-activation on a live row and a negative one; the wrong mask `>= 0` changes the outputs."""
    for R in F.INT_BWD_ROWS[idx]:
        c = F.bwd_case("integer", idx, R, CPU)
        for s in range(c.ns):
            pre = c.zprev[s].double() * c.coef[s][0].double() + c.coef[s][1].double()
            assert pre.shape[0] == R and bool((pre == 0).any()) and bool((pre < 0).any()) and bool((pre > 0).any()), (idx, R, s)
        right, wrong = F.bwd_ref(c), F.bwd_ref(c, mask_ge=True)
        differ = [n for n in right if not torch.equal(right[n][0], wrong[n][0])]
        assert "gout" in differ and "dgamma0" in differ and "dW1" in differ, (idx, R, differ)


def test_integer_forward_case_is_exact_in_any_order():
    for shape, (_, ok) in F.FWD_TABLE.items():
        if not ok:
            continue
        for R in F.fwd_rows(shape):
            c = F.fwd_case("integer", shape, R, CPU)
            z, bound = F.fwd_layer_z_ref(c.a0, None, None, c.W[0], c.bias[0])
            mag = c.a0.double().abs() @ c.W[0].double().abs().t() + c.bias[0].double().abs()
            assert float(mag.max()) < 2.0 ** 13 and F.fp32_exact(z) and bool((z == z.round()).all())


def test_real_backward_reference_against_autograd():
    """The fp64 backward reference itself, against torch.autograd in fp64 on the plain three-stage head (training-mode BatchNorm whose
    statistics are those of zprev): dW, the BatchNorm gradients and the bias gradients."""
    R, dev = 5, CPU
    c = F.bwd_case("real", 0, R, dev)
    # rebuild the forward that these saved tensors belong to: layer below stage s has pre-BN output zprev[s] and BatchNorm (gamma, beta)
    # with coef = (gamma invstd, beta - mean scale, mean, invstd); stage s computes y_s = relu(bn(zprev[s])) W[s]^T (+ b)
    ns = c.ns
    zs = [c.zprev[s].double().clone().requires_grad_(True) for s in range(ns)]
    gam = [(c.coef[s][0].double() / c.coef[s][3].double()).requires_grad_(True) for s in range(ns)]
    bet = [(c.coef[s][1].double() + c.coef[s][2].double() * c.coef[s][0].double()).requires_grad_(True) for s in range(ns)]
    Ws = [c.W[s].double().clone().requires_grad_(True) for s in range(ns)]
    ref = F.bwd_ref(c)
    # stage by stage (the chain's stages are linked through dZ only; zprev of different stages are independent inputs here)
    dZ = c.gy.double()
    for s in range(ns):
        z = zs[s]
        mean, var = z.mean(0), ((z - z.mean(0)) ** 2).mean(0)
        # the reference takes mean / invstd from coef (fp32 roundings of these statistics): use the same numbers, keep the graph
        inv = c.coef[s][3].double() + 0 * var
        a = torch.relu((z - (c.coef[s][2].double() + 0 * mean)) * inv * gam[s] + bet[s])
        y = a @ Ws[s].t()
        gW, gg, gb = torch.autograd.grad(y, (Ws[s], gam[s], bet[s]), dZ, retain_graph=True)
        assert torch.allclose(gW, ref["dW%d" % s][0], rtol=1e-4, atol=1e-5), s
        assert torch.allclose(gb, ref["dbeta%d" % s][0], rtol=1e-4, atol=1e-5), s
        # d/dgamma of ((z - mean) invstd gamma + beta) = (z - mean) invstd: the reference's dgamma up to the fp32 rounding of the
        # coefficients it was given (scale / invstd is gamma to 1e-7)
        assert torch.allclose(gg, ref["dgamma%d" % s][0], rtol=1e-4, atol=1e-5), s
        # dZ of the layer below through the full training-mode BatchNorm (statistics depend on z): autograd on the true expression
        z2 = c.zprev[s].double().clone().requires_grad_(True)
        m2 = z2.mean(0)
        v2 = ((z2 - m2) ** 2).mean(0)
        a2 = torch.relu((z2 - m2) * (v2 + F.EPS) ** -0.5 * gam[s].detach() + bet[s].detach())
        (gz,) = torch.autograd.grad(a2 @ Ws[s].detach().t(), z2, dZ)
        sc = c.coef[s][0].double()
        k2, k3 = ref["kout"][0][1:] if s == ns - 1 else (None, None)
        if s == ns - 1:
            gv = ref["gout"][0]
            mine = sc * gv + k2 * c.zprev[s].double() + k3
            assert torch.allclose(gz, mine, rtol=1e-4, atol=1e-4), float((gz - mine).abs().max())
        dZ = gz

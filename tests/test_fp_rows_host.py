"""The yardsticks of the row-layout feature propagation held to what they restate (no GPU): the forward to tests/interp_ref.py's
propagate transposed and to float64 torch, the backward's sequential sum to float64 torch autograd within its counted bound, the
partial sums' block order to a plain loop over the rows and to float64; then the host half of the three entries' contract (the
prototypes, the exports, argument errors and no-op cases in a child process that sees no GPU), fused_supported, and the module's
state-dict keys."""
import ctypes

import numpy as np
import pytest
import torch

import fp_rows_ref as FR
import interp_ref as R
from cabi_runner import check_case, run_cases

BAD, UNSUPPORTED = 10001, 10002


@pytest.mark.parametrize("recipe", FR.RECIPES)
@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.SHAPE_IDS)
def test_forward_yardstick_is_propagate_transposed_and_close_to_float64(shape, recipe):
    b, n, m, c2, c1 = shape
    d = FR.forward_case(shape, recipe)
    kf = np.ascontiguousarray(d["known_rows"].transpose(0, 2, 1))
    sf = np.ascontiguousarray(d["skip_rows"].transpose(0, 2, 1))
    for rule in R.RULES:
        idx, w, out = R.propagate(d["unknown"], d["known"], sf, kf, rule)
        assert np.array_equal(idx, d["idx"]) and np.array_equal(w.view(np.int32), d["w%d" % rule].view(np.int32))
        rows = d["rows%d" % rule]
        assert rows.shape == (b, n, c2 + c1)
        assert np.array_equal(rows.view(np.int32), np.ascontiguousarray(out.transpose(0, 2, 1)).view(np.int32))
        assert np.array_equal(rows[:, :, c2:].view(np.int32), d["skip_rows"].view(np.int32))
        w64 = R.weights64(d["d2"], rule)
        assert (np.abs(w - w64) <= R.WEIGHT_BOUND[rule] * np.abs(w64)).all()
        # float64 torch on the same indices: three products, two adds and the weights' own error on every term
        f = torch.tensor(d["known_rows"]).double()
        li = torch.tensor(d["idx"].astype(np.int64)).view(b, n * 3, 1).expand(-1, -1, c2)
        terms = torch.gather(f, 1, li).view(b, n, 3, c2) * torch.tensor(w64)[..., None]
        ref, mag = terms.sum(2).numpy(), terms.abs().sum(2).numpy()
        assert np.allclose(ref, FR.forward64(d["known_rows"], d["idx"], d["d2"], rule), rtol=1e-14, atol=0)
        assert (np.abs(rows[:, :, :c2] - ref) <= (R.WEIGHT_BOUND[rule] + 3 * FR.U) * mag).all()


@pytest.mark.parametrize("recipe", FR.INDEX_RECIPES)
@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.SHAPE_IDS)
def test_backward_yardstick_against_float64_autograd(shape, recipe):
    b, n, m, c2, c1 = shape
    d = FR.backward_case(shape, recipe)
    assert (np.abs(d["grad32"] - d["grad64"]) <= d["bound"]).all()
    idx = torch.tensor(d["idx"].astype(np.int64))
    valid = (idx >= 0) & (idx < m)
    f = torch.zeros(b, m, c2, dtype=torch.float64, requires_grad=True)
    li = idx.clamp(0, m - 1).view(b, n * 3, 1).expand(-1, -1, c2)
    w = torch.tensor(d["weights"]).double() * valid
    out = (torch.gather(f, 1, li).view(b, n, 3, c2) * w[..., None]).sum(2)
    out.backward(torch.tensor(d["grad_rows"][:, :, :c2]).double())
    assert np.allclose(f.grad.numpy(), d["grad64"], rtol=1e-12, atol=1e-12)
    di = FR.backward_case(shape, recipe, integer=True)
    assert np.array_equal(di["grad32"], di["grad64"])
    if recipe == "empty" and m >= 2:
        assert not d["grad32"][:, 1::2].any()


@pytest.mark.parametrize("C", FR.STATS_C)
@pytest.mark.parametrize("rows", FR.STATS_R)
def test_block_order_against_a_row_loop_and_float64(rows, C):
    z, coef, g = FR.stats_case(rows, C)
    dy = FR.mask_dy(z, coef, g)
    y = torch.from_numpy(z).double() * torch.from_numpy(coef[0]).double() + torch.from_numpy(coef[1]).double()
    assert np.array_equal(dy, torch.where(y > 0, torch.from_numpy(g), torch.zeros(())).numpy())
    assert 0.2 < (dy != 0).mean() < 0.8 or rows * C < 64
    got = FR.block_sums(dy, z)
    assert got.shape == (FR.stats_blocks(rows), 2, C) and FR.stats_blocks(rows) == -(-rows // 256)
    assert np.array_equal(got.view(np.int32), FR.block_sums_by_row_loop(dy, z).view(np.int32))
    terms = np.stack([dy.astype(np.float64), dy.astype(np.float64) * z.astype(np.float64)])
    for k in range(got.shape[0]):
        blk = terms[:, 256 * k:256 * (k + 1)]
        assert (np.abs(got[k] - blk.sum(1)) <= FR.block_sum_roundings(C) * FR.U * np.abs(blk).sum(1)).all()
    assert [FR.stats_slices(c) for c in (4, 8, 68, 256, 260, 1024)] == [256, 128, 8, 4, 4, 4]


def test_the_slice_order_shows_in_the_bits():
    z = np.ones((4, 4), np.float32)
    dy = np.array([[1.0], [2.0 ** -24], [-1.0], [2.0 ** -24]], np.float32) * np.ones((1, 4), np.float32)
    # C = 4: 256 slices, so rows 0..3 are four slices added in order: ((1 + u) + -1) + u = u, where a pairing (1 - 1) + (u + u) gives 2u
    assert FR.block_sums(dy, z)[0, 0, 0] == np.float32(2.0 ** -24)


# ------------------------------------------------------------------------------------------------ the entries' host half
P_ = "PTR"
FWD, BWD, STATS = "sn_interp_rows_forward", "sn_interp_rows_backward", "sn_bn_relu_backward_stats"
F_BASE = [2, 5, 3, 4, 2, 0, P_, P_, P_, P_, P_, P_, None]    # b n m c2 c1 rule known skip idx dist2 weights rows stream
B_BASE = [2, 5, 3, 4, 2, P_, P_, P_, P_, P_, None]           # b n m c2 c1 weights grad_rows start order grad_known stream
S_BASE = [300, 8, P_, P_, P_, P_, P_, None]                  # R C z coef g dy stats stream


def _with(base, changes):
    out = list(base)
    for k, v in changes.items():
        out[k] = v
    return out


def _cases():
    out = []
    for pos in range(5):
        out.append(("fwd-negative-%d" % pos, FWD, _with(F_BASE, {pos: -1}), BAD, "negative size"))
        out.append(("bwd-negative-%d" % pos, BWD, _with(B_BASE, {pos: -1}), BAD, "negative size"))
    for rule in (-1, 2):
        out.append(("fwd-rule-%d" % rule, FWD, _with(F_BASE, {5: rule}), BAD, "bad rule"))
    out.append(("fwd-no-column", FWD, _with(F_BASE, {3: 0, 4: 0}), BAD, "no output column"))
    out.append(("fwd-no-column-before-noop", FWD, _with(F_BASE, {0: 0, 3: 0, 4: 0}), BAD, "no output column"))
    out.append(("fwd-m0", FWD, _with(F_BASE, {2: 0}), BAD, "empty known cloud"))
    for pos in (6, 7, 8, 9, 10, 11):
        out.append(("fwd-null-%d" % pos, FWD, _with(F_BASE, {pos: None}), BAD, "null pointer"))
    out.append(("fwd-too-many-workgroups", FWD, _with(F_BASE, {0: 1 << 20, 1: 1 << 20, 3: 64}), UNSUPPORTED, "workgroups"))
    nf = F_BASE[:6] + [None] * 7
    for tag, ch in (("b0", {0: 0}), ("n0", {1: 0}), ("b0-m0", {0: 0, 2: 0})):
        out.append(("fwd-noop-" + tag, FWD, _with(nf, ch), 0, None))
    out.append(("bwd-3n-overflow", BWD, _with(B_BASE, {1: 1 << 30}), BAD, "31 bits"))
    for pos in (5, 6, 7, 8, 9):
        out.append(("bwd-null-%d" % pos, BWD, _with(B_BASE, {pos: None}), BAD, "null pointer"))
    out.append(("bwd-too-many-workgroups", BWD, _with(B_BASE, {0: 1 << 20, 2: 1 << 20, 3: 64}), UNSUPPORTED, "workgroups"))
    nb = B_BASE[:5] + [None] * 6
    for tag, ch in (("b0", {0: 0}), ("m0", {2: 0}), ("c2-0", {3: 0})):
        out.append(("bwd-noop-" + tag, BWD, _with(nb, ch), 0, None))
    for pos in (0, 1):
        out.append(("stats-negative-%d" % pos, STATS, _with(S_BASE, {pos: -4}), BAD, "negative size"))
    out.append(("stats-c-not-4", STATS, _with(S_BASE, {1: 6}), BAD, "multiple of 4"))
    for pos in (2, 3, 4, 5, 6):
        out.append(("stats-null-%d" % pos, STATS, _with(S_BASE, {pos: None}), BAD, "null pointer"))
    out.append(("stats-too-many-blocks", STATS, _with(S_BASE, {0: 1 << 40}), UNSUPPORTED, "workgroups"))
    ns = S_BASE[:2] + [None] * 6
    for tag, ch in (("r0", {0: 0}), ("c0", {1: 0})):
        out.append(("stats-noop-" + tag, STATS, _with(ns, ch), 0, None))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def results():
    return run_cases(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_table(results, case):
    check_case(results, case)


def test_the_header_declares_and_the_library_exports_the_entries():
    from samplenet_amd import _lib

    header = open(_lib.HEADERS[1]).read()
    for name, base in ((FWD, F_BASE), (BWD, B_BASE), (STATS, S_BASE)):
        assert ("int %s(" % name) in header and hasattr(_lib.lib, name), name
        proto = _lib.PROTOTYPES[name]
        assert len(proto) == len(base) and _lib.RESTYPES[name] is ctypes.c_int, name
        for ty, a in zip(proto, base):
            assert (ty is ctypes.c_void_p) == (a is None or a == P_), name
    assert _lib.PROTOTYPES[STATS][0] is ctypes.c_longlong
    assert _lib.PROTOTYPES["sn_bn_relu_stats_blocks"] == [ctypes.c_longlong]
    blocks = _lib.lib.sn_bn_relu_stats_blocks
    assert [blocks(r) for r in (-1, 0, 1, 256, 257, 131072)] == [0, 0, 1, 1, 2, 512] and blocks(1 << 40) == 0
    assert all(blocks(r) == FR.stats_blocks(r) for r in FR.STATS_R)
    assert len({c[0] for c in CASES}) == len(CASES)


def test_fused_supported_and_the_state_dict_keys():
    from samplenet_amd import feature_propagation as FP, set_abstraction, stack_node
    from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM

    m = PM.PointnetFPModule([7, 16, 4])
    assert list(m.state_dict()) == ["mlp.%d.%s" % (i, k) for i in (0, 1) for k in (
        "conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked")]
    assert list(PM.PointnetFPModule([7, 16, 4], fused=True).state_dict()) == list(m.state_dict())
    assert m.fused is False and PM.PointnetFPModule([7, 16, 4], fused=True).fused is True
    assert FP.fused_supported(m.mlp)
    assert not FP.fused_supported(PM.PointnetFPModule([7, 4]).mlp)                    # one layer
    assert not FP.fused_supported(PM.PointnetFPModule([7, 16, 4], bn=False).mlp)      # no BatchNorm
    assert not FP.fused_supported(PM.PointnetFPModule([7, 16, 6]).mlp)                # top width % 4
    assert FP.fused_supported(PM.PointnetFPModule([7, 6, 6, 8]).mlp)
    assert FP.layer_records is set_abstraction.layer_records and stack_node.POOL_ROWS != stack_node.POOL_NONE
    # the default route is today's composition and runs on CPU tensors; the fused route has no CPU fallback
    torch.manual_seed(0)
    u, k, sf, kf = torch.rand(2, 9, 3), torch.rand(2, 4, 3), torch.rand(2, 3, 9), torch.rand(2, 4, 4)
    with pytest.raises(RuntimeError):
        m(u, k, sf, kf)                                    # three_nn: GPU only
    assert m(u, None, sf, torch.rand(2, 4, 1)).shape == (2, 4, 9)
    with pytest.raises(RuntimeError):
        FP.propagate_mlp(m.mlp, torch.rand(2, 9, 7))


def test_the_python_surface_refuses_what_it_cannot_serve():
    from samplenet_amd import ops

    kr, idx, d2 = torch.zeros(1, 5, 4), torch.zeros(1, 8, 3, dtype=torch.int32), torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError):
        ops.interp_rows(kr, None, idx, d2)                  # CPU tensors: no CPU route exists
    assert ops.INTERP_RULES == {"sqrt_eps": R.SQRT_EPS, "squared_clamp": R.SQUARED_CLAMP}

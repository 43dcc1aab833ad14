"""The five FC-chain entries (csrc/fc_chain.hip: sn_fc_chain_forward, _forward_pool, _forward_pool_out, sn_fc_chain_backward, _backward_obn)
called directly, shape by shape, against fp64.

The module tests reach the two resident-workgroup kernels only with what SampleNet happens to pass (three hidden layers, ns = 3 or 4,
Co[0] = 192, last Ci a power of two, four row counts, every optional pointer set, torch tensors without guards).  Here every branch has
a row of its own (tests/fc_chain_ref.py: FWD_TABLE, BWD_TABLE), every output, the exchange slabs and the `sync` state are views into
sentinel-filled buffers of exactly the documented size (check() asserts that nothing outside a view changed and that the 31 words
between two sync words keep the sentinel), and every element is compared: integer data bit for bit (tests/test_fc_chain_host.py proves
those recipes exact in any summation order), real data element by element against first-order bounds counted from the kernels'
operations.  The forward is teacher-forced per layer -- BatchNorm over a few rows amplifies rounding, so layer l's reference starts
from the kernel's own z[l-1] and coef[l-1] -- and compared bit for bit with the per-layer launch it replaces; the backward's reference
is the whole chain in fp64 from the inputs, the bounds propagated stage to stage.

sn_fc_chain_forward_pool / _pool_out run behind their real producer (sn_conv_stack_forward_bn stopped after its last GEMM) and are judged
from the producer's last z.  Run with -s for the figures of profiles/fc_chain/errors.txt."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fc_chain_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
K = F.source_constants()

# What include/samplenet_hip_internal.h states for the chain against the per-layer launches: z bit-identical; the coefficients and
# running statistics within this many ulps -- of the larger value for scale, mean and invstd; of the sum of the magnitudes of its two
# terms for shift = beta - mean scale and for the running statistics (1 - m) old + m new, which cancel.  Twice the worst distance
# observed over this file's cases (profiles/fc_chain/errors.txt: the observed values); mean is bit-identical.
COEF_ULPS = {"scale": 4, "shift": 4, "mean": 0, "invstd": 4, "running_mean": 2, "running_var": 8}  # observed 2, 2, 0, 2, 1, 4
# sn_fc_chain_backward_obn against sn_bn_output_backward + sn_fc_chain_backward: every output bit-identical (observed: 0 ulps)
OBN_ULPS = 0

FWD_OK = [s for s, (_, ok) in F.FWD_TABLE.items() if ok]
_fid = lambda s: "C0_%d-nl%d" % s


def ulps(a, b, mag=None):
    """worst |a - b| in units of the fp32 spacing at max(|a|, |b|) (or at `mag`)"""
    a, b = a.double(), b.double()
    m = (torch.maximum(a.abs(), b.abs()) if mag is None else mag.double()).clamp_min(2.0 ** -100)
    return float(((a - b).abs() / torch.exp2(torch.floor(torch.log2(m)) - 23)).max())


def under(got, ref, bound, what):
    """element by element |got - ref| <= bound; -> worst err / bound (0 where both are 0)"""
    err = (got.double() - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), (what, "worst err / bound", float((err / bound.clamp_min(1e-300))[~ok].max()), "at", int((~ok).nonzero()[0].flatten()[0]))
    return float((err / bound.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0


def test_tables_against_the_library():
    """Every supported row of the two tables is reached by a launch below (the parametrisations ARE the tables); here: the `_supported`
    answers on every row, and every unsupported row refused by the entry itself with SN_ERR_UNSUPPORTED."""
    import ctypes

    from samplenet_amd._lib import SampleNetHipError, lib

    for (C0, nl), (branch, ok) in F.FWD_TABLE.items():
        for R in F.ROWS_FULL:
            assert lib.sn_fc_chain_forward_supported(R, C0, F.H, nl) == int(ok) == F.fwd_supported(R, C0, F.H, nl, K), (C0, nl, branch)
        if not ok:
            c = F.fwd_case("real", (C0, nl), 5, DEV)
            with pytest.raises(SampleNetHipError, match="code 10002.*sn_fc_chain_forward: shape not supported"):
                F.launch_forward(c, F.sync_block())
    for Co, Ci, branch in F.BWD_TABLE:
        n = len(Co)
        for R in F.ROWS_FULL:
            assert lib.sn_fc_chain_backward_supported(R, n, ctypes.cast((ctypes.c_int * n)(*Co), ctypes.c_void_p),
                                                      ctypes.cast((ctypes.c_int * n)(*Ci), ctypes.c_void_p)) == 1, branch
    assert sorted(FWD_OK) == sorted(s for s in F.FWD_TABLE if F.fwd_supported(5, s[0], F.H, s[1], K))


def _check_forward(c, call, worst):
    R = c.R
    for l in range(c.nl):
        assert call.filled(call.z[l]) and call.filled(call.coef[l]) and tuple(call.z[l].shape) == (R, F.H), (call.what, l)
        z_ref, bound = F.fwd_layer_z_ref(c.a0, call.z[l - 1] if l else None, call.coef[l - 1] if l else None, c.W[l], c.bias[l])
        if c.recipe == "integer" and l == 0:
            assert torch.equal(call.z[0].double(), z_ref), (call.what, "z[0] bit for bit")
        worst["z"] = max(worst.get("z", 0.0), under(call.z[l], z_ref, bound, (call.what, "z", l)))
        bn = F.bn_ref(call.z[l], c.gamma[l], c.beta[l], F.EPS, F.MOMENTUM, c.rm[l], c.rv[l], R)
        got = {"scale": call.coef[l][0], "shift": call.coef[l][1], "mean": call.coef[l][2], "invstd": call.coef[l][3],
               "running_mean": call.rm[l], "running_var": call.rv[l]}
        for name, (ref, bnd) in bn.items():
            worst[name] = max(worst.get(name, 0.0), under(got[name], ref, bnd, (call.what, name, l)))
        assert int(call.nbt[l][0]) == 7 + l + 1 and int(call.nbt[l][1]) == 0, (call.what, "num_batches_tracked", l)
        if R == 1:  # the variance of one row is 0: invstd = rsqrt(eps) exactly
            assert torch.equal(call.coef[l][3], torch.full((F.H,), float(torch.tensor(F.EPS, dtype=torch.float32).double() ** -0.5), device=DEV)), call.what


def _against_per_layer(c, call, dist):
    """The same inputs through sn_layer_forward_bn layer by layer, fed with the chain's own z[l-1] / coef[l-1]: z bit-identical (the GEMM
    arithmetic is the same), the coefficients' distance collected in ulps."""
    for l in range(c.nl):
        one = F.launch_layer_forward(c, l, c.a0 if l == 0 else call.z[l - 1], None if l == 0 else call.coef[l - 1]).check()
        assert torch.equal(one.z, call.z[l]), (call.what, "z against the per-layer launch", l)
        mean, var_term = call.coef[l][2], (call.rv[l] - (1 - F.MOMENTUM) * c.rv[l]).abs()
        mags = {"shift": c.beta[l].abs() + (mean * call.coef[l][0]).abs(),
                "running_mean": (1 - F.MOMENTUM) * c.rm[l].abs() + F.MOMENTUM * mean.abs(),
                "running_var": (1 - F.MOMENTUM) * c.rv[l].abs() + var_term}
        for i, name in enumerate(("scale", "shift", "mean", "invstd")):
            dist[name] = max(dist.get(name, 0.0), ulps(one.coef[i], call.coef[l][i], mags.get(name)))
        dist["running_mean"] = max(dist.get("running_mean", 0.0), ulps(one.rm, call.rm[l], mags["running_mean"]))
        dist["running_var"] = max(dist.get("running_var", 0.0), ulps(one.rv, call.rv[l], mags["running_var"]))


@pytest.mark.parametrize("recipe", ("integer", "real", "few"))
@pytest.mark.parametrize("shape", FWD_OK, ids=_fid)
def test_forward(shape, recipe):
    """sn_fc_chain_forward over the table x recipes: z[0] bit for bit on integers; every layer, coefficient, running statistic under the
    teacher-forced bounds; num_batches_tracked incremented once; nothing written past row R - 1 (z is exactly (R, H) between guard
    words) or outside xbuf (2 * 32 * H floats) and sync; z bit-identical to the per-layer launches and the coefficients within
    COEF_ULPS of them; the running-statistics arrays as a whole-array NULL leave z and coef bit-identical."""
    worst, dist = {}, {}
    for R in ((1, 2) if recipe == "few" else F.fwd_rows(shape)):
        c = F.fwd_case(recipe, shape, R, DEV)
        call = F.launch_forward(c, F.sync_block()).check()
        _check_forward(c, call, worst)
        assert F.sync_words(call.sync) == F.fwd_sync_closed_form(1, c.nl), call.what
        _against_per_layer(c, call, dist)
        bare = F.launch_forward(c, F.sync_block(), stats="none").check()
        for l in range(c.nl):
            assert torch.equal(bare.z[l], call.z[l]) and torch.equal(bare.coef[l], call.coef[l]), (bare.what, l)
            assert torch.equal(bare.rm[l], c.rm[l]) and torch.equal(bare.rv[l], c.rv[l]) and int(bare.nbt[l][0]) == 7 + l, (bare.what, l)
    print("\nfc_chain forward %s %s (%s): worst err / bound  %s" % (_fid(shape), recipe, F.FWD_TABLE[shape][0].split(":")[0],
                                                                   "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    print("fc_chain forward %s %s: chain against sn_layer_forward_bn, z bit-identical, ulps  %s" % (
        _fid(shape), recipe, "  ".join("%s %.2f" % kv for kv in sorted(dist.items()))))
    for name, d in dist.items():
        assert d <= COEF_ULPS[name], (shape, recipe, name, d)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", FWD_OK, ids=_fid)
def test_forward_launch_order_and_sync_state(shape):
    """A(x1), A(x2), A(x1) on ONE sync block (x2 with more rows than x1), the last two back to back: the third launch equals the first
    bit for bit (a stale slab or counter of the middle launch cannot pass), sync[15] stays 0, and the state is its closed form --
    sync[0] = E, sync[1 + l] = 8 E for the seams the shape has, nothing else -- after one launch and after three."""
    nl = shape[1]
    sync = F.sync_block()
    x1, x2 = F.fwd_case("real", shape, 17, DEV, seed=1), F.fwd_case("real", shape, 32, DEV, seed=2)
    a = F.launch_forward(x1, sync).check()
    assert F.sync_words(sync) == F.fwd_sync_closed_form(1, nl)
    b, c = F.launch_forward(x2, sync), F.launch_forward(x1, sync)
    b.check(), c.check()
    assert F.sync_words(sync) == F.fwd_sync_closed_form(3, nl)
    assert _same(a.z + a.coef, c.z + c.coef), shape
    alone = F.launch_forward(x2, F.sync_block()).check()
    assert _same(alone.z + alone.coef, b.z + b.coef), shape


# ---- backward --------------------------------------------------------------------------------------------------------------------
_bid = lambda i: "shape%d" % i
BWD_ALL = list(range(len(F.BWD_TABLE)))


def _bwd_exact(c, call):
    ref = F.bwd_ref(c)
    assert set(ref) == set(call.out), (call.what, sorted(set(ref) ^ set(call.out)))
    for name, (val, _) in ref.items():
        assert torch.equal(call.out[name].double(), val), (call.what, name, float((call.out[name].double() - val).abs().max()))


def _bwd_under(c, call, worst):
    ref = F.bwd_ref(c)
    assert set(ref) == set(call.out), (call.what, sorted(set(ref) ^ set(call.out)))
    for name, (val, bound) in ref.items():
        key = name.rstrip("0123456789")
        worst[key] = max(worst.get(key, 0.0), under(call.out[name], val, bound, (call.what, name)))


@pytest.mark.parametrize("idx", BWD_ALL, ids=_bid)
def test_backward_integers_bit_exact(idx):
    """sn_fc_chain_backward and _obn (fixed 0 and 1) on the integer recipe: EVERY output of every stage bit for bit (the recipe places
    exact zeros in zprev scale + shift on live rows: `> 0` is told from `>= 0`)."""
    for R in F.INT_BWD_ROWS[idx]:
        c = F.bwd_case("integer", idx, R, DEV)
        call = F.launch_backward(c, F.sync_block()).check()
        _bwd_exact(c, call)
        assert F.sync_words(call.sync) == F.bwd_sync_closed_form(1, c.ns), call.what
    for R in F.INT_OBN_ROWS[idx]:
        for fixed in (0, 1):
            c = F.bwd_case("integer", idx, R, DEV, obn=fixed)
            _bwd_exact(c, F.launch_backward(c, F.sync_block()).check())


@pytest.mark.parametrize("recipe", ("real", "few"))
@pytest.mark.parametrize("idx", BWD_ALL, ids=_bid)
def test_backward_real_data_under_the_propagated_bounds(idx, recipe):
    """Real data, element by element under the bounds of tests/fc_chain_ref.py: bn_rows in its three forms (R; < 0: fixed statistics,
    k2 = k3 = 0; R * 1024 with a raw operand on the last stage: the pooled-feature stage) and the output BatchNorm in front with
    `fixed` 0 and 1."""
    for form, obn in (("R", None), ("fixed", None), ("pool", None), ("R", 0), ("R", 1)):
        worst = {}
        for R in ((1, 2) if recipe == "few" else F.bwd_rows(idx)):
            c = F.bwd_case(recipe, idx, R, DEV, form=form, obn=obn)
            call = F.launch_backward(c, F.sync_block()).check()
            for name, t in call.out.items():
                assert call.filled(t), (call.what, name)
            _bwd_under(c, call, worst)
            if form == "fixed":
                assert not bool(call.out["kout"][1:].any()), call.what
        print("\nfc_chain backward %s %s bn_rows %s obn %s: worst err / bound  %s" % (_bid(idx), recipe, form, obn,
                                                                                      "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("idx", (0, 1, 3), ids=_bid)
def test_backward_optional_pointers(idx):
    """db_top, every dbias[s], gout and kout given and then NULL, one at a time and all at once: the remaining outputs bit-identical."""
    for R in (5, 32):
        for obn in (None, 0):
            c = F.bwd_case("real", idx, R, DEV, obn=obn)
            full = F.launch_backward(c, F.sync_block()).check()
            for without in [(n,) for n in F.BWD_OPTIONAL] + [F.BWD_OPTIONAL]:
                part = F.launch_backward(c, F.sync_block(), without=without).check()
                assert set(part.out) < set(full.out) and not [n for n in part.out if n.rstrip("0123456789") in without], part.what
                for name, t in part.out.items():
                    assert torch.equal(t, full.out[name]), (part.what, name)


@pytest.mark.parametrize("idx", BWD_ALL, ids=_bid)
def test_backward_obn_equals_the_separate_output_batchnorm(idx):
    """sn_fc_chain_backward_obn (fixed 0 and 1) against sn_bn_output_backward followed by the plain entry on its dz: every output
    within OBN_ULPS ulps (0: bit for bit), dgamma_o / dbeta_o included."""
    worst = 0.0
    for recipe, R in (("real", 5), ("real", 32), ("few", 1), ("few", 2), ("real", 17)):
        for fixed in (0, 1):
            c = F.bwd_case(recipe, idx, R, DEV, obn=fixed)
            fused = F.launch_backward(c, F.sync_block()).check()
            sep = F.launch_bn_output_backward(c).check()
            plain = copy.copy(c)
            plain.obn, plain.gy = None, sep.dz
            two = F.launch_backward(plain, F.sync_block()).check()
            pairs = [(fused.out[n], two.out[n]) for n in two.out] + [(fused.out["odgamma"], sep.dgamma), (fused.out["odbeta"], sep.dbeta)]
            worst = max([worst] + [ulps(a, b) for a, b in pairs])
    print("\nfc_chain backward_obn %s: against sn_bn_output_backward + sn_fc_chain_backward, worst distance %.2f ulps" % (_bid(idx), worst))
    assert worst <= OBN_ULPS, (idx, worst)


@pytest.mark.parametrize("idx", BWD_ALL, ids=_bid)
def test_backward_launch_order_and_sync_state(idx):
    """A(x1), A(x2), A(x1) on ONE sync block: as the forward's; closed form sync[0] = E, sync[1 + s] = 8 E for s < ns - 1,
    sync[14] = 16 E, sync[15] = 0."""
    ns = len(F.BWD_TABLE[idx][0])
    sync = F.sync_block()
    x1, x2 = F.bwd_case("real", idx, 17, DEV, seed=1), F.bwd_case("real", idx, 32, DEV, seed=2)
    a = F.launch_backward(x1, sync).check()
    assert F.sync_words(sync) == F.bwd_sync_closed_form(1, ns)
    b, c = F.launch_backward(x2, sync), F.launch_backward(x1, sync)
    b.check(), c.check()
    assert F.sync_words(sync) == F.bwd_sync_closed_form(3, ns)
    for name in a.out:
        assert torch.equal(a.out[name], c.out[name]), (idx, name)
    alone = F.launch_backward(x2, F.sync_block()).check()
    for name in b.out:
        assert torch.equal(alone.out[name], b.out[name]), (idx, name)


# ---- the counters' wrap ------------------------------------------------------------------------------------------------------------
POLLS = 1 << 16  # sync[13]: a wrong comparison reports through sync[15] within milliseconds and never spins for seconds
WRAPS = [("forward", (1 << 29) - 2, "an 8-arrival counter"), ("forward", (1 << 32) - 2, "the epoch word"),
         ("backward", (1 << 29) - 2, "an 8-arrival counter"), ("backward", (1 << 28) - 2, "the 16-arrival word"),
         ("backward", (1 << 32) - 2, "the epoch word")]


@pytest.mark.parametrize("direction,E0,what", WRAPS, ids=["%s-E%d" % w[:2] for w in WRAPS])
def test_counters_cross_their_wrap(direction, E0, what):
    """The state a long run reaches by itself -- the closed form (verified above) at E' launches, modulo 2^32 -- set by hand so that the
    next launches' targets ((epoch + 1) * 8, * 16) straddle 2^32: four launches give the bits of the same four launches from the zeroed
    state, sync[15] stays 0, and the state ends at the closed form of E' + 4."""
    if direction == "forward":
        cases = [F.fwd_case("real", (128, 3), R, DEV, seed=10 + i) for i, R in enumerate((5, 32, 17, 1))]
        run = lambda c, s: (lambda k: k.z + k.coef)(F.launch_forward(c, s).check())
        closed = lambda E: F.fwd_sync_closed_form(E, 3, POLLS)
    else:
        cases = [F.bwd_case("real", 0, R, DEV, seed=10 + i) for i, R in enumerate((5, 32, 17, 1))]
        run = lambda c, s: (lambda k: [k.out[n] for n in sorted(k.out)])(F.launch_backward(c, s).check())
        closed = lambda E: F.bwd_sync_closed_form(E, 3, POLLS)
    zeroed = F.sync_block(POLLS)
    want = [run(c, zeroed) for c in cases]
    assert F.sync_words(zeroed) == closed(4)
    sync = F.sync_block(POLLS)
    F.sync_set(sync, closed(E0))
    assert F.sync_words(sync) == closed(E0)
    got = [run(c, sync) for c in cases]
    words = F.sync_words(sync)
    assert words[15] == 0, (what, words)
    assert words == closed(E0 + 4), (what, words)
    for i, (w, g) in enumerate(zip(want, got)):
        assert _same(w, g), (what, "launch", i)


# ---- the pool variants ---------------------------------------------------------------------------------------------------------------
POOL_CASES = [(B, N, None) for B, N in F.POOL_SHAPES] + [(5, 64, Co) for Co in F.POOL_OUT_WIDTHS] + [(32, 64, 96), (1, 128, 32), (3, 1024, 256)]


@pytest.mark.parametrize("B,N,Co", POOL_CASES, ids=["B%d-N%d-Co%s" % c for c in POOL_CASES])
def test_forward_pool_and_pool_out(B, N, Co):
    """sn_fc_chain_forward_pool (Co None) and _pool_out behind their real producer, sn_conv_stack_forward_bn with pooled = argsel = zsel =
    NULL: from the producer's last z in fp64 -- bn5's coefficients and running statistics under the bound of F.conv_stats_ref; argsel
    exactly the FIRST row of the maximum where the kernel's own scale is >= 0 and of the minimum otherwise, zsel = z[argsel] bit for
    bit; pooled within one rounding of relu(zsel scale + shift) from the kernel's own coefficients; the statistics accumulators left
    zero; the FC layers (and the output stage: no ReLU, y = z scale + shift) under the teacher-forced bounds."""
    from samplenet_amd._lib import lib

    assert F.pool_stack(B, N) is not None and F.pool_stack(1, 64) is None  # (B, N) = (1, 64): no conv stack runs 64 rows
    assert lib.sn_fc_chain_forward_pool_supported(B, N, 128, F.H, 3) == 1 and (Co is None or lib.sn_fc_chain_forward_pool_out_supported(B, N, 128, F.H, 3, Co))
    c = F.pool_case(B, N, DEV, Co)
    call = F.launch_pool(c, F.sync_block()).check()
    R, worst = B * N, {}
    # bn5 from the producer's z
    mean, var, E_mean, E_var = F.conv_stats_ref(call.z5, R)
    bn5 = F.bn_coef_ref(mean, var, E_mean, E_var, c.cg[-1], c.cbeta[-1], F.EPS, F.MOMENTUM, c.crm[-1], c.crv[-1], R / (R - 1.0))
    got = {"scale": call.coef5[0], "shift": call.coef5[1], "mean": call.coef5[2], "invstd": call.coef5[3], "running_mean": call.rm5,
           "running_var": call.rv5}
    for name, (ref, bnd) in bn5.items():
        worst["bn5 " + name] = under(got[name], ref, bnd, (call.what, "bn5", name))
    assert int(call.nbt5[0]) == 1 and int(call.nbt5[1]) == 0
    # the pick
    z = call.z5.view(B, N, 128)
    sc, sh = call.coef5[0], call.coef5[1]
    assert bool((sc < 0).any()) and bool((sc == 0).any()) and bool((sc > 0).any())
    zmax, zmin = z.max(1).values, z.min(1).values
    first = lambda hit: hit.int().argmax(1).int()  # (the first row that holds the extreme value)
    want_arg = torch.where(sc >= 0, first(z == zmax[:, None, :]), first(z == zmin[:, None, :]))
    want_z = torch.where(sc >= 0, zmax, zmin)
    assert torch.equal(call.argsel, want_arg), call.what
    assert torch.equal(call.zsel, want_z) and torch.equal(call.zsel, torch.gather(z, 1, call.argsel.long()[:, None, :])[:, 0]), call.what
    pre = call.zsel.double() * sc.double() + sh.double()
    worst["pooled"] = under(call.pooled, pre.clamp_min(0), F.U * pre.abs(), (call.what, "pooled"))  # relu(fmaf(.)): one rounding
    assert not bool(call.acc[:call.nsum].any()), (call.what, "statistics accumulators left zero")
    # the FC layers behind, teacher-forced from the kernel's pooled features
    worst_fc = {}
    for l in range(3):
        z_ref, bound = F.fwd_layer_z_ref(call.pooled, call.z[l - 1] if l else None, call.coef[l - 1] if l else None, c.W[l], c.bias[l])
        worst_fc["z"] = max(worst_fc.get("z", 0.0), under(call.z[l], z_ref, bound, (call.what, "z", l)))
        bn = F.bn_ref(call.z[l], c.gamma[l], c.beta[l], F.EPS, F.MOMENTUM, c.rm[l], c.rv[l], B)
        gotl = {"scale": call.coef[l][0], "shift": call.coef[l][1], "mean": call.coef[l][2], "invstd": call.coef[l][3],
                "running_mean": call.rm[l], "running_var": call.rv[l]}
        for name, (ref, bnd) in bn.items():
            worst_fc[name] = max(worst_fc.get(name, 0.0), under(gotl[name], ref, bnd, (call.what, name, l)))
        assert int(call.nbt[l][0]) == 1, (call.what, l)
    worst.update({"fc " + k: v for k, v in worst_fc.items()})
    if Co is not None:
        z_ref, bound = F.fwd_layer_z_ref(None, call.z[2], call.coef[2], c.oW, c.ob)
        worst["out z"] = under(call.zo, z_ref, bound, (call.what, "zo"))
        bn = F.bn_ref(call.zo, c.og, c.obeta, F.EPS, F.MOMENTUM, c.orm, c.orv, B)
        goto = {"scale": call.coef_o[0], "shift": call.coef_o[1], "mean": call.coef_o[2], "invstd": call.coef_o[3], "running_mean": call.orm,
                "running_var": call.orv}
        for name, (ref, bnd) in bn.items():
            worst["out " + name] = under(goto[name], ref, bnd, (call.what, "out", name))
        zs, zh = call.zo.double() * call.coef_o[0].double(), call.coef_o[1].double()
        worst["out y"] = under(call.y, zs + zh, F.U * (zs.abs() + zh.abs()), (call.what, "y"))  # fmaf, no ReLU: one rounding
        assert int(call.onbt[0]) == 1 and bool((call.y < 0).any())
    assert F.sync_words(call.sync) == F.fwd_sync_closed_form(1, 4 if Co is not None else 3), call.what
    print("\nfc_chain forward_pool%s B %d N %d Co %s stack %s: worst err / bound  %s" % ("_out" if Co else "", B, N, Co, "-".join(map(str, c.ch)),
                                                                                          "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))

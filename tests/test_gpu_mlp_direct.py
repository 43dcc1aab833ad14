"""The layer, BatchNorm and max-pool entries of csrc/pointnet_mlp.hip / pointnet_mlp_backward.hip called directly, table row by table
row (tests/mlp_ref.py), against fp64: sn_bn_finalize, sn_bn_eval_coef, sn_bn_batch_stats_twopass (and sn_bn_output_forward on top of
it), sn_bn_backward_coef, sn_pool_forward, sn_pool_backward, sn_pool_backward_bn, sn_layer_forward_bn, sn_conv_forward_bn_pool,
sn_layer_backward in its five routes, sn_layer_backward_in3, sn_linear_dgrad / sn_linear_wgrad alone in dz_mode 1 and 2, and
sn_conv_stack_forward_bn teacher-forced layer by layer.

Until now the BatchNorm and pool arithmetic reached the GPU only through the whole network (held to torch-fp32's own distance from
fp64) or with one HIP route compared with another, both sides sharing bn_finalize_channel, bn_backward_coefs, pool_fwd_kernel's pick
and pool_bwd_kernel's mask; the layer entries were pinned on small integers with power-of-two coefficients only.
Here every output and scratch buffer is a view into a sentinel-filled buffer of exactly the documented size (check(): nothing outside
it changed; filled(): every element of an output was written), EVERY element is compared -- integer data bit for bit, real data under
first-order bounds counted from the kernels' operations, picks and masks exactly (tests/test_mlp_host.py proves the data leaves no
decision near its threshold) -- and every case runs twice and must repeat bit for bit.  Run with -s for the figures of
profiles/mlp_direct/errors.txt."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
COEF_ROWS = ("scale", "shift", "mean", "invstd")


def under(got, ref, bound, what):
    """element by element |got - ref| <= bound; -> worst err / bound (0 where both are 0)"""
    err = (got.double() - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), (what, "worst err / bound", float((err / bound.clamp_min(1e-300))[~ok].max()), "at", int((~ok).flatten().nonzero()[0]))
    return float((err / bound.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0


def note(worst, name, value):
    worst[name] = max(worst.get(name, 0.0), value)


def report(entry, key, worst):
    if not worst:  # (an integer recipe: everything was compared bit for bit)
        return
    print("\nmlp_direct %s %s: worst err / bound  %s" % (entry, key, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def same_bits(a, b, what):
    """two launches of one case: every output bit for bit"""
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), (what, "not repeatable", name)


def _forward_outputs(call):
    out = {n: call.coef[i] for i, n in enumerate(COEF_ROWS)}
    out["running_mean"], out["running_var"] = call.rm, call.rv
    return out


def _check_bn_forward(c, call, ref, running, worst):
    """coef (4, C) and -- with running == "both" -- the running statistics under the reference's bounds; the counter incremented once
    and its neighbour left alone; running statistics not given (or only the variance given): both unchanged by a bit."""
    assert call.filled(call.coef), call.what
    got = _forward_outputs(call)
    for name, (val, bnd) in ref.items():
        note(worst, name, under(got[name], val, bnd, (call.what, name)))
    assert int(call.nbt[0]) == 8 and int(call.nbt[1]) == 0, (call.what, "num_batches_tracked")
    if running != "both":
        assert torch.equal(call.rm, c.rm) and torch.equal(call.rv, c.rv), (call.what, "running statistics touched")


@pytest.mark.parametrize("nblk", list(M.PARTIAL_SUMS_TABLE), ids=lambda n: "nblk%d" % n)
def test_bn_finalize(nblk):
    """sn_bn_finalize over partial_sums' branches x channel blockings, from synthetic partials (no GEMM in front) against fp64 of the same
    partials: a few U on every coefficient whatever |mean| / std (0, 3, 100, a constant channel: invstd = 1 / sqrt(eps)); the
    running-statistics update of torch.nn.BatchNorm1d (unbiased variance, momentum weights); R = 1 keeps the biased variance."""
    from samplenet_amd._lib import lib

    worst = {}
    cases = [M.finalize_case(nblk, C, M.ROWS_OF_NBLK[nblk], DEV) for C in M.PARTIAL_SUMS_C]
    assert lib.sn_linear_stats_blocks(M.ROWS_OF_NBLK[nblk]) == nblk
    if nblk == 1:
        cases.append(M.finalize_case(1, 8, 1, DEV))
    for c in cases:
        for running in ("both", "none", "var only"):
            call = M.launch_finalize(c, running).check()
            _check_bn_forward(c, call, M.finalize_ref(c, running == "both"), running, worst)
            again = M.launch_finalize(c, running).check()
            same_bits(_forward_outputs(call), _forward_outputs(again), call.what)
            if running == "both":
                first = call
            else:
                assert torch.equal(call.coef, first.coef), (call.what, "coef depends on the running statistics' pointers")
    report("sn_bn_finalize", "nblk %d (%s)" % (nblk, M.PARTIAL_SUMS_TABLE[nblk][0].split(":")[0]), worst)


@pytest.mark.parametrize("C", (5, 64, 72))
def test_bn_eval_coef(C):
    """sn_bn_eval_coef: coefficients from the running statistics (with eps under the root), fp32 arithmetic counted operation by
    operation; the mean row a copy."""
    c = M.eval_case(C, DEV)
    call = M.launch_eval_coef(c).check()
    assert call.filled(call.coef)
    worst = {}
    for i, name in enumerate(COEF_ROWS):
        val, bnd = M.eval_coef_ref(c)[name]
        note(worst, name, under(call.coef[i], val, bnd, (call.what, name)))
    assert torch.equal(call.coef[2], c.rm)
    assert torch.equal(M.launch_eval_coef(c).check().coef, call.coef), (call.what, "not repeatable")
    report("sn_bn_eval_coef", "C %d" % C, worst)


@pytest.mark.parametrize("R", list(M.TWOPASS_TABLE), ids=lambda r: "R%d" % r)
def test_bn_batch_stats_twopass(R):
    """sn_bn_batch_stats_twopass over its loop's branches x channel blockings against fp64 statistics of z: the bound carries NO
    conditioning factor (the channel with |mean| / std = 100 is held to the same few U as the one with mean 0 -- the case this entry
    exists for).  sn_bn_output_forward(training) on the same z: the same coefficients bit for bit, and y = z scale + shift to one
    rounding from the GPU's own coefficients, through its float4 kernel (C % 4 == 0) and its scalar kernel."""
    worst = {}
    for C in M.TWOPASS_C:
        c = M.twopass_case(R, C, DEV)
        for running in ("both", "none", "var only"):
            call = M.launch_twopass(c, running).check()
            _check_bn_forward(c, call, M.twopass_ref(c, running == "both"), running, worst)
            same_bits(_forward_outputs(call), _forward_outputs(M.launch_twopass(c, running).check()), call.what)
            if running == "both":
                first = call
        out = M.launch_twopass(c, "both", output=True).check()
        same_bits(_forward_outputs(first), _forward_outputs(out), (out.what, "against sn_bn_batch_stats_twopass"))
        assert out.filled(out.y)
        zs, sh = c.z.double() * out.coef[0].double(), out.coef[1].double()
        note(worst, "y", under(out.y, zs + sh, M.U * (zs.abs() + sh.abs()), (out.what, "y")))  # fmaf: one rounding
    report("sn_bn_batch_stats_twopass", "R %d (%s)" % (R, M.TWOPASS_TABLE[R][0].split(":")[0]), worst)


def _check_bn_backward(call, ref, worst, exact):
    for name in ("dgamma", "dbeta", "dbias", "kcoef"):
        if name not in call.out:
            continue
        assert call.filled(call.out[name]), (call.what, name)
        val, bnd = ref[name]
        if exact:
            assert torch.equal(call.out[name].double(), val), (call.what, name, "bit for bit")
        else:
            note(worst, name, under(call.out[name], val, bnd, (call.what, name)))


@pytest.mark.parametrize("recipe", ("integer", "real"))
@pytest.mark.parametrize("nblk", list(M.PARTIAL_SUMS_TABLE), ids=lambda n: "nblk%d" % n)
def test_bn_backward_coef(nblk, recipe):
    """sn_bn_backward_coef from synthetic partials against fp64 of the same partials: dgamma = invstd (sz - mean s) with |mean| / std up
    to 100 (the difference is taken in double: a few U), dbeta, k1 = scale, k2, k3, and dbias = k1 s + k2 R mean + R k3 (exactly the
    roundings of k2 and k3).  integer: R a power of two, every output bit for bit.  dbias == NULL: the rest bit-identical."""
    worst = {}
    for C in M.PARTIAL_SUMS_C:
        R = M.int_rows(nblk) if recipe == "integer" else M.ROWS_OF_NBLK[nblk]
        c = M.backward_coef_case(recipe, nblk, C, R, DEV)
        call = M.launch_backward_coef(c).check()
        _check_bn_backward(call, M.backward_coef_ref(c), worst, recipe == "integer")
        same_bits(call.out, M.launch_backward_coef(c).check().out, call.what)
        bare = M.launch_backward_coef(c, with_dbias=False).check()
        assert "dbias" not in bare.out
        same_bits(bare.out, call.out, (bare.what, "without dbias"))
    report("sn_bn_backward_coef", "nblk %d %s" % (nblk, recipe), worst)


@pytest.mark.parametrize("N", list(M.POOL_FWD_TABLE), ids=lambda n: "N%d" % n)
def test_pool_forward(N):
    """sn_pool_forward over its loops' branches x channel blockings: argsel EXACTLY the first row of the maximum (scale >= 0, the
    scales +0.0 and -0.0 included) or of the minimum (scale < 0), ties planted within one wave's row stride, across waves and across
    64-row blocks; zsel = z[argsel] bit for bit; pooled = relu(zsel scale + shift) to one rounding."""
    worst = {}
    for C in M.POOL_FWD_C:
        c = M.pool_case(N, C, DEV)
        call = M.launch_pool_forward(c).check()
        assert call.filled(call.pooled) and call.filled(call.zsel) and call.filled(call.argsel), call.what
        arg, zsel, pooled, bnd = M.pool_forward_ref(c.z, c.coef)
        assert torch.equal(call.argsel, arg), (call.what, "argsel", (call.argsel != arg).nonzero()[:4].tolist())
        assert torch.equal(call.zsel.view(torch.int32), zsel.view(torch.int32)), (call.what, "zsel")
        assert torch.equal(call.zsel, torch.gather(c.z, 1, call.argsel.long()[:, None, :])[:, 0]), (call.what, "zsel = z[argsel]")
        note(worst, "pooled", under(call.pooled, pooled, bnd, (call.what, "pooled")))
        assert bool((call.pooled == 0).any()) and bool((call.pooled > 0).any())
        for name, b, n0, n1, ch in c.ties:
            assert int(call.argsel[b, ch]) == n0, (call.what, "tie", name, b, n0, n1, ch)
        again = M.launch_pool_forward(c).check()
        same_bits({"pooled": call.pooled, "zsel": call.zsel, "argsel": call.argsel}, {"pooled": again.pooled, "zsel": again.zsel, "argsel": again.argsel},
                  call.what)
    report("sn_pool_forward", "N %d (%s)" % (N, M.POOL_FWD_TABLE[N][0].split(":")[0]), worst)


@pytest.mark.parametrize("B", list(M.POOL_BWD_TABLE), ids=lambda b: "B%d" % b)
def test_pool_backward(B):
    """pool_bwd_kernel called three ways -- sn_pool_backward alone (gsel + the two sums), sn_pool_backward_bn with R = B N (the
    BatchNorm under the pool averaged over B N rows, B carry a gradient) and with R < 0 (fixed statistics: k2 = k3 = 0, dbias = k1 s) --
    over its loops' branches x channel blockings: gsel = g [pooled > 0] bit for bit with pooled exactly 0 under a third of the
    non-zero gradients; the fp32 sums and everything derived from them under the counted bounds, the conditioning of sz - mean s
    included; integer data (B a power of two) bit for bit.  dbias == NULL: the rest bit-identical."""
    worst = {}
    for recipe in ("real",) + (("integer",) if B & (B - 1) == 0 else ()):
        for C in M.POOL_BWD_C:
            c = M.pool_backward_case(recipe, B, C, DEV)
            for way in ("alone", "bn", "fixed"):
                call = M.launch_pool_backward(c, way).check()
                ref = M.pool_backward_ref(c, rows=B * M.POOL_BWD_N if way == "bn" else None, fixed=way == "fixed")
                assert call.filled(call.out["gsel"]) and torch.equal(call.out["gsel"].view(torch.int32), ref["gsel"][0].view(torch.int32)), (call.what, "gsel")
                if way == "alone":
                    assert call.filled(call.out["stats"])
                    if recipe == "integer":
                        assert torch.equal(call.out["stats"].double(), ref["stats"][0]), (call.what, "stats")
                    else:
                        note(worst, "stats", under(call.out["stats"], ref["stats"][0], ref["stats"][1], (call.what, "stats")))
                else:
                    w = worst.setdefault(way, {})
                    _check_bn_backward(call, ref, w, recipe == "integer")
                    if way == "fixed":
                        assert not bool(call.out["kcoef"][1:].any()), (call.what, "k2 = k3 = 0")
                    bare = M.launch_pool_backward(c, way, with_dbias=False).check()
                    assert "dbias" not in bare.out
                    same_bits(bare.out, call.out, (bare.what, "without dbias"))
                same_bits(call.out, M.launch_pool_backward(c, way).check().out, call.what)
    flat = {"stats": worst.get("stats", 0.0)}
    for way in ("bn", "fixed"):
        flat.update({"%s %s" % (way, k): v for k, v in worst.get(way, {}).items()})
    report("sn_pool_backward[_bn]", "B %d (%s)" % (B, M.POOL_BWD_TABLE[B][0].split(":")[0]), flat)


_sid = lambda s: "R%d-Ci%d-Co%d-dz%d-npts%d" % s


@pytest.mark.parametrize("shape", [s for s, _ in M.SMALL_BWD_TABLE], ids=_sid)
def test_layer_backward_up_to_32_rows(shape):
    """sn_layer_backward's R <= 32 route (small_bwd_kernel) in the three dz_modes with real-valued kcoef and coef_prev, each with
    prev_bn_rows = 0 (the BatchNorm below saw these R rows), > 0 (it saw 64 R rows: the layer on top of the max-pool) and < 0 (fixed
    statistics): dYprev = [zprev scale + shift > 0] (dZ W) with a channel whose ReLU argument is exactly 0 under a non-zero gradient,
    dW, db, and the BatchNorm backward of the layer below, all under the counted bounds.  db == NULL / prev_dbias == NULL: the other
    outputs bit-identical."""
    for form in M.SMALL_BWD_FORMS:
        worst = {}
        c = M.layer_backward_case(shape, form, DEV)
        assert M.relu_margin(c) < 1.0
        call = M.launch_layer_backward(c).check()
        ref = M.layer_backward_ref(c)
        assert set(ref) == set(call.out), (call.what, sorted(set(ref) ^ set(call.out)))
        for name, (val, bnd) in ref.items():
            assert call.filled(call.out[name]), (call.what, name)
            note(worst, name, under(call.out[name], val, bnd, (call.what, name)))
        assert torch.equal(call.out["dyprev"] != 0, ref["dyprev"][0] != 0), (call.what, "the ReLU mask")
        assert torch.equal(call.out["prev_kcoef"][0], c.coef_prev[0]), (call.what, "k1 = scale")
        if form == "fixed":
            assert not bool(call.out["prev_kcoef"][1:].any()), (call.what, "k2 = k3 = 0")
        same_bits(call.out, M.launch_layer_backward(c).check().out, call.what)
        for want_db, want_dbias in ((False, True), (True, False), (False, False)):
            part = M.launch_layer_backward(c, want_db, want_dbias).check()
            assert ("db" in part.out) == want_db and ("prev_dbias" in part.out) == want_dbias
            same_bits(part.out, call.out, (part.what, "optional outputs"))
        report("sn_layer_backward", "%s prev_bn_rows %s (%s)" % (_sid(shape), form, dict(M.SMALL_BWD_TABLE)[shape]), worst)


_lid = lambda row: "%s-%s%s" % (row[1][0].replace("<=", "le").replace(">", "gt"), _sid(row[0][0]), "-db" if row[0][1] else "")


@pytest.mark.parametrize("row", M.LAYER_BWD_TABLE, ids=_lid)
def test_layer_backward_above_32_rows(row):
    """sn_layer_backward's four routes above 32 rows -- the fused convolution backward, the row-blocked launch (coefficients inside
    the launch up to 64 rows, bn_bwd_coef_kernel behind it above), the combined launch, and sn_linear_wgrad + sn_linear_dgrad -- each
    in every dz_mode it serves, real-valued kcoef and coef_prev, prev_bn_rows = 0 and < 0: dYprev with its ReLU mask exact, dW, db
    where asked for, and the BatchNorm backward of the layer below under the counted bounds (on the partial-sum routes dgamma, k2, k3
    carry the conditioning of sz - mean s).  prev_dbias == NULL, and db == NULL where that keeps the route: the rest bit-identical (dW too
    wherever the weight gradient's split count stays the same)."""
    from samplenet_amd._lib import lib

    (shape, want_db), (route, why) = row
    R, Ci, Co, mode, npts = shape
    assert lib.sn_linear_wgrad_splits(R, Ci, Co, int(want_db)) == M.wgrad_splits(R, Ci, Co, want_db, cus=torch.cuda.get_device_properties(0).multi_processor_count)
    for form in M.LAYER_BWD_FORMS:
        worst = {}
        c = M.layer_backward_case(shape, form, DEV)
        assert M.relu_margin(c) < 1.0
        call = M.launch_layer_backward(c, want_db).check()
        ref = M.layer_backward_ref(c, route, call.nsplit)
        if not want_db:
            del ref["db"]
        assert set(ref) == set(call.out), (call.what, sorted(set(ref) ^ set(call.out)))
        for name, (val, bnd) in ref.items():
            assert call.filled(call.out[name]), (call.what, name)
            note(worst, name, under(call.out[name], val, bnd, (call.what, name)))
        assert torch.equal(call.out["dyprev"] != 0, ref["dyprev"][0] != 0), (call.what, "the ReLU mask")
        assert torch.equal(call.out["prev_kcoef"][0], c.coef_prev[0]), (call.what, "k1 = scale")
        if form == "fixed":
            assert not bool(call.out["prev_kcoef"][1:].any()), (call.what, "k2 = k3 = 0")
        same_bits(call.out, M.launch_layer_backward(c, want_db).check().out, call.what)
        bare = M.launch_layer_backward(c, want_db, want_dbias=False).check()
        assert "prev_dbias" not in bare.out
        same_bits(bare.out, call.out, (bare.what, "without prev_dbias"))
        if want_db and M.layer_backward_route(R, Ci, Co, mode, npts, False) == route:
            # (the weight gradient's split count depends on db -- sn_linear_wgrad_splits(.., with_bias): 2 partials with the bias
            #  column against 4 without at (256, 64, 64) -- and with it dW's summation order: there dW is held to its bound instead)
            bare = M.launch_layer_backward(c, False).check()
            keep = [n for n in bare.out if n != "dW" or bare.nsplit == call.nsplit]
            same_bits({n: bare.out[n] for n in keep}, call.out, (bare.what, "without db"))
            note(worst, "dW", under(bare.out["dW"], *M.layer_backward_ref(c, route, bare.nsplit)["dW"], (bare.what, "dW")))
        elif want_db:
            # (db == NULL moves this shape to another route -- other kernels, other summation orders: no bit-identity to ask for; every
            #  remaining output is held to ITS route's bounds, the mask exactly)
            other = M.layer_backward_route(R, Ci, Co, mode, npts, False)
            bare = M.launch_layer_backward(c, False).check()
            oref = M.layer_backward_ref(c, other, bare.nsplit)
            assert set(bare.out) == set(oref) - {"db"}
            for name, t in bare.out.items():
                note(worst, "without db (%s) %s" % (other, name), under(t, *oref[name], (bare.what, other, name)))
            assert torch.equal(bare.out["dyprev"] != 0, oref["dyprev"][0] != 0), (bare.what, "the ReLU mask")
        report("sn_layer_backward", "%s %s prev_bn_rows %s (%s)" % (route, _sid(shape), form, why.split(":")[0]), worst)


@pytest.mark.parametrize("shape", M.ALONE_TABLE, ids=_sid)
def test_linear_dgrad_and_wgrad_alone(shape):
    """sn_linear_dgrad and sn_linear_wgrad called on their own in dz_mode 1 and 2 (the suite called them directly with dz_mode 0 only),
    on a tile-path shape and an R <= 32 shape, real-valued kcoef and coef_prev: dYprev and its mask, the BatchNorm-backward partials
    (summed over the blocks in double), dW and db; db == NULL: dW under the same bound (the split may differ)."""
    worst = {}
    c = M.layer_backward_case(shape, "rows", DEV)
    d = M.launch_linear_dgrad(c).check()
    ref = M.linear_dgrad_ref(c)
    assert d.filled(d.out["dyprev"]) and d.filled(d.out["stats"]), d.what
    note(worst, "dyprev", under(d.out["dyprev"], *ref["dyprev"], (d.what, "dyprev")))
    assert torch.equal(d.out["dyprev"] != 0, ref["dyprev"][0] != 0), (d.what, "the ReLU mask")
    note(worst, "stats", under(d.out["stats"].double().sum(0), *ref["stats"], (d.what, "stats")))
    same_bits(d.out, M.launch_linear_dgrad(c).check().out, d.what)
    for want_db in (True, False):
        w = M.launch_linear_wgrad(c, want_db).check()
        full = M.layer_backward_ref(c, "fallback", w.nsplit)
        for name in w.out:
            assert w.filled(w.out[name]), (w.what, name)
            note(worst, name, under(w.out[name], *full[name], (w.what, name)))
        same_bits(w.out, M.launch_linear_wgrad(c, want_db).check().out, w.what)
    report("sn_linear_dgrad / sn_linear_wgrad", _sid(shape), worst)


_fid = lambda row: "%s-R%d-Ci%d-Co%d" % ((row[1][0].replace(" ", "_"),) + row[0][0])


def _check_layer_forward(c, call, route, running, worst):
    assert call.filled(call.z) and call.filled(call.coef), call.what
    note(worst, "z", under(call.z, *M.layer_z_ref(c), (call.what, "z")))
    got = _forward_outputs(call)
    for name, (val, bnd) in M.layer_stats_ref(call.z, c, route, running).items():
        note(worst, name, under(got[name], val, bnd, (call.what, name)))
    assert int(call.nbt[0]) == 8 and int(call.nbt[1]) == 0, (call.what, "num_batches_tracked")
    if not running:
        assert torch.equal(call.rm, c.rm) and torch.equal(call.rv, c.rv), (call.what, "running statistics touched")


@pytest.mark.parametrize("row", M.LAYER_FWD_TABLE, ids=_fid)
def test_layer_forward_bn(row):
    """sn_layer_forward_bn route by route: z against the fp64 layer (every element), coef and the running statistics against fp64
    statistics of the GPU's own z -- two-pass in registers up to 64 rows (no conditioning factor), fp32 partials + bn_finalize_kernel
    above, where the bound on mean and var carries the conditioning of ss / R - mean^2.  Running statistics NULL: z and coef
    bit-identical, the counter still incremented."""
    (shape, with_prev, running), (route, why) = row
    worst = {}
    c = M.layer_forward_case(shape, with_prev, DEV)
    call = M.launch_layer_forward(c, running).check()
    _check_layer_forward(c, call, route, running, worst)
    again = M.launch_layer_forward(c, running).check()
    same_bits(dict(_forward_outputs(call), z=call.z), dict(_forward_outputs(again), z=again.z), call.what)
    other = M.launch_layer_forward(c, not running).check()
    assert torch.equal(other.z, call.z) and torch.equal(other.coef, call.coef), (other.what, "z / coef depend on the running statistics' pointers")
    report("sn_layer_forward_bn", "%s (%s)" % (_fid(row), why.split(":")[0]), worst)


@pytest.mark.parametrize("shape", [s for s, _ in M.CONV_POOL_TABLE], ids=lambda s: "R%d-npts%d-Ci%d-Co%d" % s)
def test_conv_forward_bn_pool(shape):
    """sn_conv_forward_bn_pool: z, coef and the running statistics as sn_layer_forward_bn's tile route; the pool outputs against the
    reference pool of THE GPU'S OWN z and coef: argsel exactly the first row of the selected extreme, zsel bit for bit, pooled to one
    rounding.  Input rows far out and duplicated -- inside one row wave of a tile (4, 9), across its two row waves (20, 52) and, where
    the cloud has them, across 64-row blocks (7, 77) -- make exact ties AT the extreme: asserted, with the earlier row returned."""
    R, npts, Ci, Co = shape
    worst = {}
    c = M.layer_forward_case((R, Ci, Co), True, DEV, seed=1)
    pairs = [(4, 9), (20, 52)] + ([(7, 77)] if npts > 64 else [])  # one row wave; the two row waves of a 64-row tile; two blocks
    for b in range(R // npts):
        for n0, n1 in pairs:
            c.ain[b * npts + n0] *= 6.0  # a row far out: its z is the cloud's maximum or minimum in most channels
            c.ain[b * npts + n1] = c.ain[b * npts + n0]
    call = M.launch_layer_forward(c, True, npts).check()
    _check_layer_forward(c, call, "tile big", True, worst)
    assert call.filled(call.pooled) and call.filled(call.zsel) and call.filled(call.argsel), call.what
    zb = call.z.view(R // npts, npts, Co)
    for n0, n1 in pairs:
        assert torch.equal(zb[:, n1], zb[:, n0]), "duplicated rows give bit-identical z: the ties are real"
    arg, zsel, pooled, bnd = M.pool_forward_ref(zb, call.coef)
    assert bool((call.coef[0] < 0).any()) and bool((call.coef[0] == 0).any())
    assert torch.equal(call.argsel, arg), (call.what, "argsel", (call.argsel != arg).nonzero()[:4].tolist())
    assert torch.equal(call.zsel.view(torch.int32), zsel.view(torch.int32)), (call.what, "zsel")
    note(worst, "pooled", under(call.pooled, pooled, bnd, (call.what, "pooled")))
    for n0, n1 in pairs:  # the tie rule IS exercised: each planted pair is the selected extreme somewhere, and the earlier row is returned
        hit = (call.argsel == n0) & (zb[:, n1] == call.zsel)
        assert int(hit.sum()) >= 4, (call.what, "pair", n0, n1, "selected in", int(hit.sum()), "(cloud, channel) places")
        assert not bool((call.argsel == n1).any()), (call.what, "the later row of a tie was returned", n0, n1)
    again = M.launch_layer_forward(c, True, npts).check()
    same_bits({"z": call.z, "coef": call.coef, "pooled": call.pooled, "zsel": call.zsel, "argsel": call.argsel},
              {"z": again.z, "coef": again.coef, "pooled": again.pooled, "zsel": again.zsel, "argsel": again.argsel}, call.what)
    report("sn_conv_forward_bn_pool", "R %d npts %d Ci %d Co %d" % shape, worst)


@pytest.mark.parametrize("shape,ok", [(s, ok) for s, ok, _ in M.IN3_TABLE], ids=lambda v: "R%d-Ci%d-Co%d" % v if isinstance(v, tuple) else str(v))
def test_layer_backward_in3(shape, ok):
    """sn_layer_backward_in3 on real data: dW and the xyz layer's BatchNorm backward as the fused route's, and dW_in under the bound counted
    from its closed form (fp32 partial moments of the cloud and of dYprev x, combined in double with the fp32 k1, k2, k3); prev_dbias
    NULL: the rest bit-identical.  The shapes for which sn_layer_backward_in3_stats_floats answers 0 are refused by the entry."""
    from samplenet_amd._lib import SampleNetHipError, lib

    R, Ci, Co = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.sn_layer_backward_in3_stats_floats(R, Ci, Co) == M.in3_stats_floats(R, Ci, Co, cus)
    if not ok:
        c = M.layer_backward_case((R, Ci, Co, 1, 0), "rows", DEV)
        c.x, c.W_in, c.b_in = torch.zeros(R, 3, device=DEV), torch.zeros(Ci, 3, device=DEV), torch.zeros(Ci, device=DEV)
        with pytest.raises(SampleNetHipError, match="shape not supported by the input-layer variant"):
            M.launch_layer_backward_in3(c)
        return
    worst = {}
    c = M.in3_case(R, DEV)
    call = M.launch_layer_backward_in3(c).check()
    ref = M.in3_ref(c, call.nsplit)
    assert set(ref) == set(call.out)
    for name, (val, bnd) in ref.items():
        assert call.filled(call.out[name]), (call.what, name)
        note(worst, name, under(call.out[name], val, bnd, (call.what, name)))
    same_bits(call.out, M.launch_layer_backward_in3(c).check().out, call.what)
    bare = M.launch_layer_backward_in3(c, want_dbias=False).check()
    same_bits(bare.out, call.out, (bare.what, "without prev_dbias"))
    report("sn_layer_backward_in3", "R %d" % R, worst)


@pytest.mark.parametrize("row", M.CONV_STACK_TABLE, ids=lambda r: "B%d-N%d-%s" % (r[0][0] + ("x".join(map(str, r[0][1])),)))
def test_conv_stack_forward_teacher_forced(row):
    """sn_conv_stack_forward_bn layer by layer: every z[l] against the fp64 layer applied to the GPU's own z[l-1] and coef[l-1] (z[0]:
    to the cloud); every coef[l] and running statistic against fp64 statistics of the GPU's own z[l], the bound with the fixed-point
    quantum; every counter incremented once; the pool against the reference pool of the GPU's own last z and coef (argsel, zsel
    exact); the statistics accumulators zero afterwards.  Where z[0] == NULL is admitted: the same call without z[0] gives every other
    output bit for bit (the rebuilt activation is the xyz layer's own expression), and z[1] holds its bound from the fp64 rebuild."""
    import ctypes

    from samplenet_amd._lib import lib

    ((B, N), ch), (z1free, why) = row
    n = len(ch) - 1
    chans = ctypes.cast((ctypes.c_int * (n + 1))(*ch), ctypes.c_void_p)
    assert lib.sn_conv_stack_forward_supported(B, N, n, chans) == 1 and lib.sn_conv_stack_z1_free_supported(B, N, n, chans) == int(z1free)
    c = M.conv_stack_case(B, N, ch, DEV)
    call = M.launch_conv_stack(c).check()
    worst = {}
    for l in range(n):
        lc = M.conv_stack_layer(c, l, call.z[l - 1] if l else None, call.coef[l - 1] if l else None)
        assert call.filled(call.z[l]) and call.filled(call.coef[l]), (call.what, l)
        note(worst, "z", under(call.z[l], *M.layer_z_ref(lc), (call.what, "z", l)))
        got = {nm: call.coef[l][i] for i, nm in enumerate(COEF_ROWS)}
        got["running_mean"], got["running_var"] = call.rm[l], call.rv[l]
        for name, (val, bnd) in M.conv_fx_stats_ref(call.z[l], lc).items():
            note(worst, name, under(got[name], val, bnd, (call.what, name, l)))
        assert int(call.nbt[l][0]) == 8 and int(call.nbt[l][1]) == 0, (call.what, "num_batches_tracked", l)
    arg, zsel, pooled, bnd = M.pool_forward_ref(call.z[-1].view(B, N, ch[-1]), call.coef[-1])
    assert bool((call.coef[-1][0] < 0).any()) and bool((call.coef[-1][0] == 0).any())
    assert torch.equal(call.argsel, arg) and torch.equal(call.zsel.view(torch.int32), zsel.view(torch.int32)), (call.what, "the pick")
    note(worst, "pooled", under(call.pooled, pooled, bnd, (call.what, "pooled")))
    assert not bool(call.acc[:call.nsum].any()), (call.what, "statistics accumulators left zero")
    outs = lambda k: dict([("z%d" % l, k.z[l]) for l in range(1, n)] + [("coef%d" % l, k.coef[l]) for l in range(n)] +
                          [("rm%d" % l, k.rm[l]) for l in range(n)] + [("rv%d" % l, k.rv[l]) for l in range(n)] +
                          [("pooled", k.pooled), ("zsel", k.zsel), ("argsel", k.argsel)])
    again = M.launch_conv_stack(c).check()
    same_bits(dict(outs(call), z0=call.z[0]), dict(outs(again), z0=again.z[0]), call.what)
    if z1free:
        free = M.launch_conv_stack(c, with_z0=False).check()
        same_bits(outs(free), outs(call), (free.what, "z[0] == NULL"))
        assert not bool(free.acc[:free.nsum].any()), (free.what, "statistics accumulators left zero")
        # z[1] from the cloud in fp64: the rebuilt z[0] carries the xyz layer's (3 + 8) U, seen through coef[0] and |W1|
        l0 = M.conv_stack_layer(c, 0, None, None)
        z0, E0 = M.layer_z_ref(l0)
        l1 = M.conv_stack_layer(c, 1, z0, free.coef[0])
        z1, E1 = M.layer_z_ref(l1)
        E1 = E1 + (E0 * free.coef[0][0].double().abs()) @ c.W[1].double().abs().t()
        # (an element of z[0] whose ReLU argument lies within its own bound of 0 moves by at most that bound: max(., 0) is 1-Lipschitz)
        note(worst, "z1 rebuilt", under(free.z[1], z1, E1, (free.what, "z[1] from the cloud")))
    report("sn_conv_stack_forward_bn", "B %d N %d %s (%s)" % (B, N, "-".join(map(str, ch)), why.split(":")[0]), worst)

"""sn_layer_forward_bn, sn_layer_backward, sn_linear_dgrad and sn_linear_wgrad at input widths that are no multiple of four:
Ci = 6, 131, 259 -- the 3 + C columns a set-abstraction level feeds the GEMMs (mlp_device.h: ld4_guard) --, R = 2 * 5 * 16 rows (two
clouds, five groups of 16 rows), Co = 64.  No row of tests/mlp_ref.py's tables has Ci % 4 != 0; the cases, the fp64 references and
the first-order bounds are that file's, the route of each shape is what its restated dispatch says."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
R, CO = 2 * 5 * 16, 64
WIDTHS = (6, 131, 259)
COEF_ROWS = ("scale", "shift", "mean", "invstd")


def under(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0
    print("odd_ci %s: worst err / bound %.3f" % (what, ratio))
    assert bool((err <= bound).all()), what


def same_bits(a, b, what):
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), (what, "not repeatable", name)


def _forward_outputs(call):
    out = {n: call.coef[i] for i, n in enumerate(COEF_ROWS)}
    out["running_mean"], out["running_var"], out["z"] = call.rm, call.rv, call.z
    return out


@pytest.mark.parametrize("with_prev", (False, True), ids=("raw", "bn_relu"))
@pytest.mark.parametrize("Ci", WIDTHS)
def test_layer_forward_bn(Ci, with_prev):
    shape = (R, Ci, CO)
    route = M.layer_forward_route(R, Ci, CO, with_prev)
    assert route == "tile big"
    c = M.layer_forward_case(shape, with_prev, DEV)
    call = M.launch_layer_forward(c, True).check()
    assert call.filled(call.z) and call.filled(call.coef), call.what
    under(call.z, *M.layer_z_ref(c), "forward Ci %d z" % Ci)
    got = _forward_outputs(call)
    for name, (val, bnd) in M.layer_stats_ref(call.z, c, route, True).items():
        under(got[name], val, bnd, "forward Ci %d %s" % (Ci, name))
    same_bits(got, _forward_outputs(M.launch_layer_forward(c, True).check()), call.what)


@pytest.mark.parametrize("mode,npts", ((1, 0), (2, 16)), ids=("dz_bn", "dz_pool"))
@pytest.mark.parametrize("Ci", WIDTHS)
def test_layer_backward(Ci, mode, npts):
    shape = (R, Ci, CO, mode, npts)
    route = M.layer_backward_route(R, Ci, CO, mode, npts, False)
    for form in M.LAYER_BWD_FORMS:
        c = M.layer_backward_case(shape, form, DEV)
        assert M.relu_margin(c) < 1.0
        call = M.launch_layer_backward(c, False).check()
        ref = M.layer_backward_ref(c, route, call.nsplit)
        del ref["db"]
        assert set(ref) == set(call.out), (call.what, sorted(set(ref) ^ set(call.out)))
        for name, (val, bnd) in ref.items():
            assert call.filled(call.out[name]), (call.what, name)
            under(call.out[name], val, bnd, "backward %s Ci %d mode %d %s %s" % (route, Ci, mode, form, name))
        assert torch.equal(call.out["dyprev"] != 0, ref["dyprev"][0] != 0), (call.what, "the ReLU mask")
        same_bits(call.out, M.launch_layer_backward(c, False).check().out, call.what)


@pytest.mark.parametrize("Ci", WIDTHS)
def test_linear_dgrad_and_wgrad(Ci):
    c = M.layer_backward_case((R, Ci, CO, 1, 0), "rows", DEV)
    d = M.launch_linear_dgrad(c).check()
    ref = M.linear_dgrad_ref(c)
    assert d.filled(d.out["dyprev"]) and d.filled(d.out["stats"]), d.what
    under(d.out["dyprev"], *ref["dyprev"], "dgrad Ci %d dyprev" % Ci)
    assert torch.equal(d.out["dyprev"] != 0, ref["dyprev"][0] != 0), (d.what, "the ReLU mask")
    under(d.out["stats"].double().sum(0), *ref["stats"], "dgrad Ci %d stats" % Ci)
    same_bits(d.out, M.launch_linear_dgrad(c).check().out, d.what)
    w = M.launch_linear_wgrad(c, False).check()
    full = M.layer_backward_ref(c, "fallback", w.nsplit)
    for name in w.out:
        assert w.filled(w.out[name]), (w.what, name)
        under(w.out[name], *full[name], "wgrad Ci %d %s" % (Ci, name))
    same_bits(w.out, M.launch_linear_wgrad(c, False).check().out, w.what)

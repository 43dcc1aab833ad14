"""Host-side tests of the pose-term feature (no GPU): the fp64 restatement tests/pose_ref.py is checked against closed forms and
a hand-computed case, its case table against the admission rule of the rot_err comparison, QuaternionTransform's container
methods on CPU tensors, the aggregates against a literal transcription of registration/main.py:461-483, and the three new entries
across header, prototype table and library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sn_pose_error_forward", "sn_pose_error_backward", "sn_chamfer_mean_per_cloud")


def test_norm_err_closed_form_on_unit_quaternions():
    """||R1 R2^T - I||_F^2 = 8 (1 - d^2) for unit quaternions (d their dot product): the matrix form the kernel computes against
    the closed form it must not use (it fails off the unit sphere -- second half).  The difference is the restatement's own fp64
    rounding, whole ulps of values up to 8 (8.9e-16 each): 6 ulps on these 1024 pairs, 7 (6.2e-15) on some samples of 4096."""
    rng = np.random.default_rng(0)
    q1, q2 = P._unit(rng, 1024), P._unit(rng, 1024)
    z = np.zeros((1024, 3))
    T = P.pose_terms(np.concatenate([q1, z], 1), np.concatenate([q2, z], 1))
    assert np.abs(T["norm_err"] - 8 * (1 - T["d"] ** 2)).max() < 6e-15
    # rot_err is the angle of R1 R2^T: trace = 3 - norm_err / 2 = 1 + 2 cos(angle); 2 acos(2 d^2 - 1) is TWICE that angle
    angle = np.arccos(np.clip((3 - T["norm_err"] / 2 - 1) / 2, -1, 1))
    folded = np.minimum(T["rot_err"], 2 * np.pi - T["rot_err"])  # cos(rot_err) = cos(2 angle)
    assert np.abs(np.cos(folded) - np.cos(2 * angle)).max() < 1e-12
    T3 = P.pose_terms(np.concatenate([3 * q1, z], 1), np.concatenate([q2, z], 1))
    assert np.abs(T3["norm_err"] - T["norm_err"]).max() < 1e-13  # normalised: the scale of est does not matter
    assert np.abs(8 * (1 - T3["d"] ** 2) - T3["norm_err"]).max() > 1.0


def test_hand_computed_quarter_turn_about_z():
    """est: 90 degrees about z, q = (cos 45, 0, 0, sin 45); gt: identity.  R = [[0,-1,0],[1,0,0],[0,0,1]], R - I has entries
    -1, -1, 1, -1: norm_err = 4; d = cos 45: x = 2 / 2 - 1 = 0, rot_err = 2 acos(0) = pi; dt = (1, -2, 0.5): trans_err = 3.5 / 3."""
    c = np.sqrt(0.5)
    est = np.array([[c, 0, 0, c, 1.0, -2.0, 0.5]])
    gt = np.array([[1.0, 0, 0, 0, 0, 0, 0]])
    T = P.pose_terms(est, gt)
    assert np.allclose(P.quat_to_matrix(est[:, :4])[0], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert abs(T["norm_err"][0] - 4) < 1e-14 and abs(T["rot_err"][0] - np.pi) < 1e-14 and abs(T["trans_err"][0] - 3.5 / 3) < 1e-15
    g = P.pose_backward(est, gt, g_trans_err=np.ones(1))
    assert np.array_equal(g[0, 4:], [1 / 3, -1 / 3, 1 / 3]) and np.array_equal(g[0, :4], np.zeros(4))


def test_analytic_gradient_equals_autograd_of_the_restatement():
    """pose_backward (the formulas the kernel follows) against torch autograd through pose_terms_torch, fp64."""
    for recipe in ("unit", "nonunit", "antipodal"):
        est, gt = P.make_case(recipe, 65)
        gm, gn, gt_ = P.upstream_case(65)
        e = torch.from_numpy(est).double().requires_grad_(True)
        _, nrm, trn = P.pose_terms_torch(e, torch.from_numpy(gt))
        wn = torch.from_numpy(gn).double() + float(gm[1]) / 65
        wt = torch.from_numpy(gt_).double() + float(gm[2]) / 65
        (ga,) = torch.autograd.grad((wn * nrm).sum() + (wt * trn).sum(), e)
        ref = P.pose_backward(est, gt, gm, gn, gt_)
        scale = np.abs(ref).max(1, keepdims=True) + 1e-300
        assert (np.abs(ga.numpy() - ref) / scale).max() < 1e-11, recipe


@pytest.mark.parametrize("B", P.BATCHES)
def test_value_recipes_keep_the_admission_cap(B):
    """At most 10 % of the rows of a recipe whose rot_err is compared by value fall outside |x| <= 1 - 2^-10."""
    for recipe, by_value in P.RECIPES.items():
        est, gt = P.make_case(recipe, B)
        assert est.shape == gt.shape == (B, 7) and est.dtype == np.float32
        if by_value:
            excluded = 1.0 - P.rot_admitted(P.pose_terms(est, gt)).mean()
            assert excluded <= P.ROT_EXCLUDED_CAP, (recipe, B, excluded)


def test_edge_recipes_sit_on_their_edges():
    T = P.pose_terms(*P.make_case("same", 64))
    assert np.abs(T["x"] - 1).max() < 1e-6 and T["norm_err"].max() < 1e-12 and not T["dt"].any()
    T = P.pose_terms(*P.make_case("negated", 64))
    assert np.abs(T["x"] - 1).max() < 1e-6 and T["norm_err"].max() < 1e-12
    T = P.pose_terms(*P.make_case("antipodal", 64))
    assert np.abs(T["x"] + 1).max() < 1e-6 and np.abs(T["norm_err"] - 8).max() < 1e-5
    est, gt = P.make_case("zero", 64)
    T = P.pose_terms(est, gt)
    assert np.isfinite(T["norm_err"]).all() and not P.pose_backward(est, gt, g_norm_err=np.ones(64))[:, :4].any()


def test_means_in_kernel_order_is_a_plain_sum_for_exact_values():
    v = np.arange(1, 701, dtype=np.float32)  # integers: every order gives the same float32
    assert P.means_in_kernel_order(v) == np.float32(v.sum() / 700)


# ------------------------------------------------------------------------------------------------ the container
def test_quaternion_transform_container_on_cpu():
    from samplenet_amd import QuaternionTransform, deg_to_rad, qinv, rad_to_deg

    est, _ = P.make_case("unit", 5)
    vec = torch.from_numpy(est)
    T = QuaternionTransform(vec)
    assert T.vec.shape == (5, 7) and torch.equal(T.quat(), vec[:, :4]) and torch.equal(T.trans(), vec[:, 4:]) and T.inversion() is False
    inv = T.inverse()
    assert inv.inversion() is True and torch.equal(inv.quat(), vec[:, :4] * torch.tensor([1.0, -1, -1, -1]))
    assert torch.equal(inv.trans(), -vec[:, 4:]) and torch.equal(qinv(vec[:, :4]), inv.quat())
    back = inv.inverse()
    assert back.inversion() is False and torch.equal(back.vec, vec)
    d = T.as_dict()
    assert set(d) == {"inversion", "vec"} and d["vec"] is T.vec
    again = QuaternionTransform.from_dict(inv.as_dict(), "cpu")
    assert again.inversion() is True and torch.equal(again.vec, inv.vec)
    q = vec[:, :4]
    assert torch.equal(QuaternionTransform.wxyz_to_xyzw(q), q[:, [1, 2, 3, 0]])
    assert torch.equal(QuaternionTransform.xyzw_to_wxyz(QuaternionTransform.wxyz_to_xyzw(q)), q)
    assert QuaternionTransform(vec.reshape(35)).vec.shape == (5, 7)
    assert abs(rad_to_deg(deg_to_rad(37.5)) - 37.5) < 1e-12 and abs(rad_to_deg(np.pi) - 180) < 1e-12
    # rotate (N,3) by a single transform: plain torch (task_features.qrot), a quarter turn about z takes x to y
    c = float(np.sqrt(0.5))
    one = QuaternionTransform(torch.tensor([c, 0, 0, c, 0, 0, 0]))
    assert torch.allclose(one.rotate(torch.tensor([[1.0, 0, 0], [0, 0, 2.0]])), torch.tensor([[0, 1.0, 0], [0, 0, 2.0]]), atol=1e-6)


def test_compute_errors_is_gpu_only():
    from samplenet_amd import QuaternionTransform, ops

    est, gt = (torch.from_numpy(a) for a in P.make_case("unit", 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        QuaternionTransform(est).compute_errors(QuaternionTransform(gt))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pose_errors(est, gt)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.chamfer_mean_per_cloud(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


# ------------------------------------------------------------------------------------------------ the aggregates
def test_aggregates_equal_the_transcription():
    from samplenet_amd.evaluation import registration_aggregates

    rng = np.random.default_rng(11)
    rot = rng.uniform(2, 170, 37).astype(np.float32).astype(np.float64)
    rot[:6] = [0.0, 0.5, 1.0, 179.5, 180.0, 12.5]  # exactly on grid points of arange(0, 180, 0.5) (and one behind its end)
    rot[6] = np.nan
    trans, cons, loss = (rng.uniform(0, 1, 37).astype(np.float32) for _ in range(3))
    with np.errstate(invalid="ignore"):
        got = registration_aggregates(rot.astype(np.float32), trans, cons, loss)
        ref = P.aggregates_transcribed(rot, trans.astype(np.float64), cons.astype(np.float64), loss.astype(np.float64))
    assert set(got) == set(ref)
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k]), equal_nan=True), k
    assert got["precision"].shape == (360,) and got["precision"][0] == 1 / 37 and got["precision"][1] == 2 / 37
    assert got["precision"][-1] == 35 / 37  # (the NaN and the 180.0 never count)
    clean = registration_aggregates(rot[:6], trans[:6], cons[:6], loss[:6])
    assert clean["auc"] == P.aggregates_transcribed(rot[:6], trans[:6], cons[:6])["auc"] and np.isfinite(clean["std_rotation_error"])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_in_header_prototypes_and_library():
    from samplenet_amd import _lib

    # declared in the INTERNAL header: the public one is held at its entry count by tests/test_cabi_and_host.py
    text = open(os.path.join(ROOT, "include", "samplenet_hip_internal.h")).read()
    assert not any(name in open(os.path.join(ROOT, "include", "samplenet_hip.h")).read() for name in ENTRIES)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:  # (their exact types: the compiler check of tests/test_cabi_and_host.py)
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "qdataset.py:62-95" in text and "main.py:540-555" in text
    # argument errors are reported before any device work; B = 0 is a no-op
    assert _lib.lib.sn_pose_error_forward(-1, None, None, None, None, None, None, None) == 10001
    assert _lib.lib.sn_pose_error_forward(0, None, None, None, None, None, None, None) == 0
    assert _lib.lib.sn_pose_error_backward(0, None, None, None, None, None, None, None) == 0
    assert _lib.lib.sn_pose_error_backward(3, None, None, None, None, None, None, None) == 10001
    assert _lib.lib.sn_chamfer_mean_per_cloud(0, 4, 4, None, None, None, None) == 0
    assert _lib.lib.sn_chamfer_mean_per_cloud(2, 0, 4, None, None, None, None) == 10001

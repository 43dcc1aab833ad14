"""evaluation.RegistrationEvaluator (eval_1 / test_1 of registration/main.py:364-483 on the device): 10 items of 128 points evaluated
(a) by add() in batches of 4, 4, 2, (b) by add() one item at a time, (c) by composing pcrnet_loss / sampling_consistency per item with
an .item() per value, as main.py:416-450 does.

What may differ between the routes, and the bound each comparison uses:
  * the pose kernel: every route's rot / norm / trans values are held against the fp64 terms of ITS OWN twists under the counted bounds
    of tests/pose_ref.py;
  * the networks: kernels of the sampler and of PCRNet may take another path at another row count, so the twists of two routes may
    differ by fp32 rounding -- held to the forward bar of tests/test_gpu_mlp.py::test_pcrnet_task_loss_matches_reference (rtol 1e-5,
    atol 1e-6); the OBSERVED twist difference dq is then propagated into the loss comparison through counted Lipschitz constants;
    this gate on the twists is a BORROWED bar, not a counted bound (counting the roundings of two networks is out of reach here);
    everything downstream of the twists is counted;
  * the Chamfer reductions (one workgroup per cloud against the loss entry's pair): the fixed-order sum bound, both ways.
Whether (a) and (b) agree bit for bit is printed as a finding (profiles/pose/errors.txt), not asserted."""
import numpy as np
import pytest
import torch

import pose_ref as P

pytestmark = pytest.mark.gpu

ITEMS, N, M = 10, 128, 32
DEG = 180 / np.pi


def _data():
    g = torch.Generator().manual_seed(7)
    p0 = torch.rand(ITEMS, N, 3, generator=g) - 0.5
    _, gt = P.make_case("unit", ITEMS)
    gt[:, 0] = np.abs(gt[:, 0]) + 2.0  # rotations of moderate angle (as the data set's: below 45 degrees an axis) ...
    gt[:, :4] /= np.linalg.norm(gt[:, :4].astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    gt[:, 4:] = 0  # ... and no translation (QuaternionFixedDataset draws none)
    igt = torch.from_numpy(gt).cuda()
    from samplenet_amd.task_features import qrot_cloud

    p0 = p0.cuda()
    p1 = qrot_cloud(igt[:, :4].contiguous(), p0) + 0.01 * (torch.rand(ITEMS, N, 3, generator=g) - 0.5).cuda()
    return p0, p1.contiguous(), igt


def _model():
    from samplenet_amd.task_features import PCRNet

    torch.manual_seed(21)
    return PCRNet(bottleneck_size=256, input_shape="bnc").cuda().eval()


def _sampler(kind):
    from samplenet_amd import FPSSampler, RandomSampler, SampleNet

    torch.manual_seed(4)
    if kind == "none":
        return None
    if kind == "fps":
        return FPSSampler(M, permute=False, input_shape="bnc", output_shape="bnc").cuda()
    if kind == "random":
        return RandomSampler(M, input_shape="bnc", output_shape="bnc").cuda()
    net = SampleNet(M, 128, group_size=4, input_shape="bnc", output_shape="bnc").cuda()
    net.train()
    with torch.no_grad():  # running statistics that are not the initial ones
        for _ in range(2):
            net(torch.rand(8, N, 3, device="cuda") - 0.5)
    return net.eval()


def _per_item_reference(model, sampler, nsc, p0, p1, igt):
    """main.py:416-450 at batch size 1 on this package's pieces: sample, compute_pcrnet_loss, consistency, an .item() per value."""
    from samplenet_amd.task_features import pcrnet_loss, sampling_consistency

    rows = []
    with torch.no_grad():
        for i in range(ITEMS):
            a, b, g = p0[i:i + 1], p1[i:i + 1], igt[i:i + 1]
            if sampler is not None:
                take = lambda x: (lambda o: o[1] if isinstance(o, tuple) else o)(sampler(x)).contiguous()  # noqa: E731
                b = take(b)
                if nsc == 2:
                    a = take(a)
            loss, info = pcrnet_loss(model, a, b, g, loss_type=0)
            cons = sampling_consistency(a, b, g)
            rows.append([info["rot_err"].item(), info["trans_err"].item(), cons.item(), loss.item()] + info["est_transform"].vec[0].tolist())
    t = np.array(rows, dtype=np.float64)
    return {"rotation_errors": t[:, 0], "trans_errs": t[:, 1], "consistency_errors": t[:, 2], "losses": t[:, 3], "twists": t[:, 4:]}


def _own_twist_checks(name, res, igt_np):
    """rot / trans of a route against the fp64 terms of its own twists, pose_ref's bounds (degrees: one more rounding)."""
    T = P.pose_terms(res["twists"].astype(np.float32), igt_np)
    ok = P.rot_admitted(T)
    err = np.abs(res["rotation_errors"] - T["rot_err"] * DEG)[ok]
    assert (err <= (P.bound_rot_err({k: v[ok] for k, v in T.items()}) + 2 * P.U * T["rot_err"][ok]) * DEG).all(), (name, err.max())
    assert np.isfinite(res["rotation_errors"]).all() and (res["rotation_errors"] >= 0).all() and (res["rotation_errors"] <= 360.0001).all()
    assert (np.abs(res["trans_errs"] - T["trans_err"]) <= P.bound_trans_err(T["trans_err"])).all(), name
    return T


@pytest.mark.parametrize("kind,nsc", [("none", 2), ("fps", 1), ("fps", 2), ("random", 1), ("samplenet", 1), ("samplenet", 2)])
def test_three_routes_agree(kind, nsc):
    from samplenet_amd import RegistrationEvaluator
    from samplenet_amd.evaluation import registration_aggregates

    p0, p1, igt = _data()
    igt_np = igt.cpu().numpy()
    model, sampler = _model(), _sampler(kind)
    if sampler is not None:
        model.sampler = sampler  # (main.py:296 hangs it there)
    was = (model.training, sampler.training if sampler is not None else None)
    routes = {}
    for name, cuts in (("batched", (0, 4, 8, 10)), ("one by one", tuple(range(ITEMS + 1)))):
        ev = RegistrationEvaluator(model, sampler, num_sampled_clouds=nsc, loss_type=0)
        torch.manual_seed(99)  # (RandomSampler draws per cloud, in item order on every route)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")  # add() must not synchronise
        try:
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                ev.add(p0[lo:hi], p1[lo:hi], igt[lo:hi] if lo else {"vec": igt[lo:hi], "inversion": torch.tensor([False])})
        finally:
            torch.cuda.set_sync_debug_mode("default")
        routes[name] = ev.result()
        assert (model.training, sampler.training if sampler is not None else None) == was
    torch.manual_seed(99)
    routes["per item"] = _per_item_reference(model, sampler, nsc, p0, p1, igt)

    res = routes["batched"]
    assert all(res[k].shape == (ITEMS,) and res[k].dtype == np.float64 for k in ("rotation_errors", "trans_errs", "consistency_errors", "losses"))
    # the aggregates: exactly the transcription of main.py:461-483 applied to the returned arrays
    ref = P.aggregates_transcribed(res["rotation_errors"], res["trans_errs"], res["consistency_errors"], res["losses"])
    for k, v in ref.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v)), k
    assert set(registration_aggregates(res["rotation_errors"], res["trans_errs"], res["consistency_errors"], res["losses"])) == set(ref)
    assert res["precision"].shape == (360,) and 0.0 <= res["auc"] <= 1.0

    terms = {name: _own_twist_checks(name, r, igt_np) for name, r in routes.items()}
    base, Tb = routes["batched"], terms["batched"]
    same = all(np.array_equal(base[k], routes["one by one"][k]) for k in ("rotation_errors", "trans_errs", "consistency_errors", "losses", "twists"))
    print("POSE_EVAL %-9s sampled clouds %d: batched (4, 4, 2) and one-by-one agree bit for bit: %s" % (kind, nsc, same))
    for name in ("one by one", "per item"):
        other, To = routes[name], terms[name]
        assert np.allclose(other["twists"], base["twists"], rtol=1e-5, atol=1e-6), name
        dq = np.abs(other["twists"] - base["twists"]).max(1)  # observed input difference of the loss stage, per item
        # consistency: the same sampled points (exact index selection) through the same scan; two fixed-order reductions of n = M or
        # N terms a side, and the scan's 5 U per squared distance
        c = base["consistency_errors"]
        n0 = M if (kind != "none" and nsc == 2) else N
        n1 = M if kind != "none" else N
        bc = 2 * (P.bound_chamfer_mean(n0, n1, c, c) + 1.01 * 5 * P.U * c)
        assert (np.abs(other["consistency_errors"] - c) <= bc).all(), (name, np.abs(other["consistency_errors"] - c).max())
        # loss = norm_err + chamfer(p1s, p1_est): both kernels' own bounds, + the twist difference dq carried through
        #   the normalisation (<= 2 dq a component), the matrix (a component's perturbation e moves an entry by <= 4 sqrt(2) e), the
        #   product with an orthogonal matrix (sqrt(3)) and sum D^2 (6 e_D sqrt(N) + 9 e_D^2);
        #   the rotation of points with |v| <= sqrt(3) / 2 (|d qrot / d q| <= 6 |v|) and the mean of squared nearest distances
        #   (<= 2 sqrt(mean d^2) dp + dp^2 a side)
        Nn = Tb["norm_err"]
        e_d = np.sqrt(3) * 4 * np.sqrt(2) * 2 * dq
        dp = 6 * (np.sqrt(3) / 2) * 2 * dq
        ch = np.maximum(base["losses"] - Nn, 0)
        lip = 6 * e_d * np.sqrt(Nn) + 9 * e_d ** 2 + 2 * (2 * np.sqrt(ch) * dp + dp ** 2)
        bl = 2 * (P.bound_norm_err(Nn) + P.bound_chamfer_mean(n1, n0, ch, ch) + 1.01 * 5 * P.U * ch) + lip + 2 * P.U * base["losses"]
        assert (np.abs(other["losses"] - base["losses"]) <= bl).all(), (name, np.abs(other["losses"] - base["losses"]).max(), bl.min())
        assert (np.abs(other["rotation_errors"] - base["rotation_errors"]) <=
                2 * (P.bound_rot_err(Tb) + 2 * P.U * Tb["rot_err"]) * DEG + np.abs(To["rot_err"] - Tb["rot_err"]) * DEG)[P.rot_admitted(Tb)].all(), name


def test_evaluator_argument_checks():
    from samplenet_amd import RegistrationEvaluator

    model = _model()
    with pytest.raises(ValueError):
        RegistrationEvaluator(model, num_sampled_clouds=3)
    with pytest.raises(RuntimeError, match="nothing was added"):
        RegistrationEvaluator(model).result()
    with pytest.raises(RuntimeError, match="GPU only"):
        RegistrationEvaluator(model).add(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, 7))
    ev = RegistrationEvaluator(model, loss_type=1)
    p0, p1, igt = _data()
    ev.add(p0[:3], p1[:3], igt[:3])
    r1 = ev.result()
    ev0 = RegistrationEvaluator(model, loss_type=0)
    ev0.add(p0[:3], p1[:3], igt[:3])
    r0 = ev0.result()
    T = P.pose_terms(r0["twists"].astype(np.float32), igt[:3].cpu().numpy())
    assert (np.abs((r0["losses"] - r1["losses"]) - T["norm_err"]) <= P.bound_norm_err(T["norm_err"]) + 2 * P.U * r0["losses"]).all()
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.result()

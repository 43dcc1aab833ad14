"""evaluation.ClassificationEvaluator (classification/evaluate_samplenet.py:156-277) and evaluation.ReconstructionEvaluator
(reconstruction/sampler/evaluate_samplenet.py:88-152, sampler_autoencoder.py:149-167) on small random-weight networks: 12 items of 128
points added as batches of 5, 4 and 3 with keep=True.  Every per-item value is held against fp64 terms of what the evaluator itself
kept (logits, reconstructions) under the counted bounds of tests/cls_terms_ref.py / tests/pose_ref.py (and tests/emd_ref.py's cost
bar); the aggregates against classification_aggregates and the restated script.  The networks' own accuracy is held by their own
tests; differences between batchings are not tested (the kernels choose routes by batch size)."""
import numpy as np
import pytest
import torch

import cls_terms_ref as R
import emd_ref as E
import pose_ref as P

pytestmark = pytest.mark.gpu

ITEMS, N, M, CLASSES = 12, 128, 16, 5
CUTS = (0, 5, 9, 12)


def _data():
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(ITEMS, N, 3, generator=g) - 0.5).cuda()
    labels = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0]).cuda()  # class 4 is never seen
    return x, labels


def _classifier(kind):
    from samplenet_amd import PointNetCls, PointNetClsBasic

    torch.manual_seed(2)
    net = (PointNetCls if kind == "full" else PointNetClsBasic)(num_classes=CLASSES, input_shape="bnc").cuda()
    if kind == "full":
        with torch.no_grad():  # a feature transform that is not the identity: the regulariser is not zero
            net.transform_net2.transform.weight.normal_(0, 0.01)
    return net.eval()


def _sampler(kind):
    from samplenet_amd import FPSSampler, SampleNet

    torch.manual_seed(4)
    if kind == "none":
        return None
    if kind == "fps":
        return FPSSampler(M, permute=False, input_shape="bnc", output_shape="bnc").cuda()
    net = SampleNet(M, 128, group_size=4, input_shape="bnc", output_shape="bnc").cuda()
    net.train()
    with torch.no_grad():  # running statistics that are not the initial ones
        for _ in range(2):
            net(torch.rand(8, N, 3, device="cuda") - 0.5)
    return net.eval()


def _add_all(ev, *tensors):
    mods = [m for m in (getattr(ev, "classifier", None), getattr(ev, "autoencoder", None), ev.sampler) if m is not None]
    for m in mods[:1]:
        m.train()  # one module arrives in training mode: add() must hand it back that way
    was = [m.training for m in mods]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # add() must not synchronise
    try:
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            ev.add(*[t[lo:hi] for t in tensors])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [m.training for m in mods] == was
    for m in mods:
        m.eval()
    return ev.result()


def _within(what, got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    i = np.argmax(err / np.maximum(bound, 1e-300))
    print("EVAL_ERR %-44s observed %.3e  bound %.3e  ratio %.3f" % (what, err.flat[i], np.broadcast_to(bound, err.shape).flat[i],
                                                                    err.flat[i] / max(np.broadcast_to(bound, err.shape).flat[i], 1e-300)))
    assert (err <= bound).all(), (what, err.max())


@pytest.mark.parametrize("cls_kind,samp_kind,match_output", [("full", "samplenet", True), ("full", "samplenet", False),
                                                             ("basic", "samplenet", True), ("basic", "none", True), ("full", "fps", True)])
def test_classification_evaluator(cls_kind, samp_kind, match_output):
    from samplenet_amd import ClassificationEvaluator, SampleNet, classification_aggregates
    from samplenet_amd.classifier import orthogonality_loss

    x, labels = _data()
    classifier, sampler = _classifier(cls_kind), _sampler(samp_kind)
    tag = "%s/%s/%s" % (cls_kind, samp_kind, "matched" if match_output else "simplified")
    res = _add_all(ClassificationEvaluator(classifier, sampler, match_output=match_output, reg_weight=0.001, keep=True), x, labels)
    lab = labels.cpu().numpy()
    points = N if samp_kind == "none" else M
    assert res["logits"].shape == (ITEMS, CLASSES) and res["clouds"].shape == (ITEMS, points, 3)
    assert np.array_equal(res["labels"], lab) and np.array_equal(res["batch_sizes"], np.diff(CUTS))
    # predictions: numpy's argmax of the logits the evaluator kept; losses: the fp64 terms of those logits
    assert np.array_equal(res["preds"], np.argmax(res["logits"], axis=1))
    T = R.terms(res["logits"], lab)
    _within(tag + " losses", res["losses"], T["ce"], R.bound_ce(T))
    # the classified clouds: the matched points are input points, n_unique = np.unique of the nearest-neighbour indices
    if isinstance(sampler, SampleNet):
        from samplenet_amd import ops

        with torch.no_grad():
            nn_idx = np.concatenate([ops.knn(1, x[lo:hi], sampler.sample_indices(x[lo:hi])[0], ops.BNC, ops.BNC,
                                             return_dist=False)[0].view(hi - lo, M).cpu().numpy() for lo, hi in zip(CUTS[:-1], CUTS[1:])])
        assert np.array_equal(res["n_unique"], [len(np.unique(r)) for r in nn_idx])
        if match_output:
            assert (np.abs(res["clouds"][:, :, None, :] - x.cpu().numpy()[:, None, :, :]).sum(-1).min(2) == 0).all()
    else:
        assert (res["n_unique"] == points).all()
    # the batch loss: the mean cross-entropy of the batch + the per-batch regulariser of the kept clouds' transform
    batches = []
    for j, (lo, hi) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        Tj = R.terms(res["logits"][lo:hi], lab[lo:hi])
        reg = 0.0
        if cls_kind == "full":
            with torch.no_grad():
                _lg, ep = classifier(torch.from_numpy(res["clouds"][lo:hi]).cuda())
                reg = 0.001 * float(orthogonality_loss(ep["transform"]))
        want = Tj["means"][0] + reg
        _within("%s batch loss %d" % (tag, j), res["batch_losses"][j:j + 1], np.array([want]),
                R.bound_mean_ce(Tj) + 2 * R.U * abs(want) + 3 * R.U * reg)
        batches.append((res["preds"][lo:hi], lab[lo:hi], res["batch_losses"][j], res["n_unique"][lo:hi]))
    if cls_kind == "full":
        assert reg > 0
    # the aggregates: classification_aggregates of the returned arrays = the restated script
    again = classification_aggregates(res["preds"], res["labels"], res["batch_sizes"], res["batch_losses"], res["n_unique"], CLASSES)
    ref = R.aggregates_restated(batches, CLASSES)
    for k, v in again.items():
        assert np.array_equal(np.asarray(res[k], dtype=np.float64), np.asarray(v, dtype=np.float64), equal_nan=True), k
    for k, v in ref.items():
        assert np.array_equal(np.asarray(res[k], dtype=np.float64), np.asarray(v, dtype=np.float64), equal_nan=True), k
    assert res["mean_loss"] == sum(float(l) * b for l, b in zip(res["batch_losses"], np.diff(CUTS))) / ITEMS
    assert np.isnan(res["class_accuracies"][4]) and np.isnan(res["avg_class_accuracy"]) and np.isfinite(res["avg_class_accuracy_seen"])
    assert res["total_seen"] == ITEMS and res["class_seen"].tolist() == [4, 3, 3, 2, 0]


def _chamfer_fp64(a, b):
    d = E.sqdist(a, b)
    return d.min(2).mean(1), d.min(1).mean(1)


def _chamfer_bound(n1, n2, m1, m2):
    # the fixed-order reduction (pose_ref) + the scan's 5 roundings per squared distance (as tests/test_gpu_evaluation.py)
    return P.bound_chamfer_mean(n1, n2, m1, m2) + 1.01 * 5 * P.U * (m1 + m2) + 2.0 ** -149


@pytest.mark.parametrize("samp_kind,loss", [("samplenet", "chamfer"), ("fps", "chamfer"), ("none", "chamfer"), ("samplenet", "emd")])
def test_reconstruction_evaluator(samp_kind, loss):
    from samplenet_amd import PointNetAE, ReconstructionEvaluator

    x, _ = _data()
    torch.manual_seed(6)
    ae = PointNetAE(n_pc_points=N, bottleneck_size=128, input_shape="bnc").cuda().eval()
    sampler = _sampler(samp_kind)
    res = _add_all(ReconstructionEvaluator(ae, sampler, loss=loss, with_reference=True, keep=True), x)
    xn = x.cpu().numpy()
    points = N if samp_kind == "none" else M
    assert res["sampled"].shape == (ITEMS, points, 3) and res["sample_idx"].shape == (ITEMS, points)
    assert res["reconstructions"].shape == (ITEMS, N, 3)
    assert np.array_equal(res["sampled"], np.stack([xn[b][res["sample_idx"][b]] for b in range(ITEMS)]))
    if samp_kind != "samplenet":  # (a SampleNet's count is that of the nearest neighbours BEFORE the completion)
        assert np.array_equal(res["n_unique"], [len(np.unique(r)) for r in res["sample_idx"]])
    assert ((res["n_unique"] >= 1) & (res["n_unique"] <= points)).all()
    with torch.no_grad():
        ref_rec = torch.cat([ae(x[lo:hi]) for lo, hi in zip(CUTS[:-1], CUTS[1:])]).cpu().numpy()
    tag = "%s/%s" % (samp_kind, loss)
    if loss == "chamfer":
        m1, m2 = _chamfer_fp64(res["reconstructions"], xn)
        _within(tag + " losses", res["losses"], m1 + m2, _chamfer_bound(N, N, m1, m2))
        r1, r2 = _chamfer_fp64(ref_rec, xn)
        _within(tag + " reference losses", res["reference_losses"], r1 + r2, _chamfer_bound(N, N, r1, r2))
    else:
        for name, rec in (("losses", res["reconstructions"]), ("reference_losses", ref_rec)):
            match, _ = E.approx_match_fp64(rec, xn)
            cost = E.match_cost_fp64(rec, xn, match)
            _within("%s %s" % (tag, name), res[name], cost, E.COST_REL * np.abs(cost))
    assert np.array_equal(res["nre"], np.divide(res["losses"], res["reference_losses"]))
    for k, a in (("mean_loss", "losses"), ("mean_reference_loss", "reference_losses"), ("mean_nre", "nre"), ("mean_unique", "n_unique")):
        assert res[k] == np.asarray(res[a], dtype=np.float64).mean()
    if samp_kind == "none":
        assert np.array_equal(res["losses"], res["reference_losses"]) and (res["nre"] == 1).all()


def _sync_warnings(fn):
    """fn() under torch's "warn" sync-debug mode -> (its value, how many synchronising calls torch reported)"""
    import warnings

    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            value = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # (torch's own once-only notice that the mode is a prototype speaks of synchronising too: only the per-call report counts)
    return value, sum("called a synchronizing" in str(w.message) for w in caught)


def test_result_makes_one_synchronising_call(monkeypatch):
    """result() of each of the seven evaluators, keep=True where it exists, after batches of 5, 4 and 3: exactly ONE synchronising
    call, the transfer.  Counted by torch's sync-debug mode "warn", after checking on a plain .cpu() of a device tensor that this
    torch build reports a blocking device-to-host copy there, once (it does on the ROCm build this was written on; a build that
    does not has the calls of torch.Tensor.cpu counted instead)."""
    from samplenet_amd import (ClassificationEvaluator, PointNetAE, ProgressiveClassificationEvaluator,
                               ProgressiveReconstructionEvaluator, ProgressiveRetrievalEvaluator, ReconstructionEvaluator,
                               RegistrationEvaluator, RetrievalEvaluator, SampleNetProgressive)
    from samplenet_amd.task_features import PCRNet

    x, labels = _data()
    g = torch.Generator().manual_seed(3)
    quat = torch.randn(ITEMS, 4, generator=g)
    igt = torch.cat([quat / quat.norm(dim=1, keepdim=True), torch.zeros(ITEMS, 3)], dim=1).cuda()
    classifier, sampler = _classifier("full"), _sampler("samplenet")
    torch.manual_seed(6)
    ae = PointNetAE(n_pc_points=N, bottleneck_size=128, input_shape="bnc").cuda().eval()
    pcr = PCRNet(bottleneck_size=256, input_shape="bnc").cuda().eval()
    ranker = SampleNetProgressive((8, M), 128, group_size=4, input_shape="bnc", output_shape="bnc").cuda().eval()
    cases = [(RegistrationEvaluator(pcr, sampler), (x, x.flip(1).contiguous(), igt)),
             (ClassificationEvaluator(classifier, sampler, keep=True), (x, labels)),
             (ReconstructionEvaluator(ae, sampler, keep=True), (x,)),
             (ProgressiveClassificationEvaluator(classifier, ranker, keep=True), (x, labels)),
             (ProgressiveReconstructionEvaluator(ae, ranker, keep=True), (x,)),
             (RetrievalEvaluator(classifier, sampler, keep=True), (x, labels)),
             (ProgressiveRetrievalEvaluator(classifier, ranker), (x, labels))]
    for ev, tensors in cases:
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            ev.add(*[t[lo:hi] for t in tensors])

    _, reported = _sync_warnings(lambda: torch.ones(1, device="cuda").cpu())
    print("EVAL_SYNC a plain .cpu(): %d synchronising call(s) reported by the sync-debug mode" % reported)
    calls = []
    if reported != 1:
        to_host = torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append(1) or to_host(self, *a, **k))
    for ev, _ in cases:
        del calls[:]
        res, warned = _sync_warnings(ev.result)
        count = warned if reported == 1 else len(calls)
        print("EVAL_SYNC %-36s %d synchronising call(s)" % (type(ev).__name__, count))
        assert count == 1, type(ev).__name__
        assert len(res["labels" if "labels" in res else "n_unique" if "n_unique" in res else "losses"]) == ITEMS


def test_result_before_add_raises_and_argument_checks():
    from samplenet_amd import ClassificationEvaluator, PointNetAE, ReconstructionEvaluator

    with pytest.raises(RuntimeError, match="nothing was added"):
        ClassificationEvaluator(_classifier("basic")).result()
    ae = PointNetAE(n_pc_points=N, bottleneck_size=128).cuda()
    with pytest.raises(RuntimeError, match="nothing was added"):
        ReconstructionEvaluator(ae).result()
    with pytest.raises(ValueError):
        ReconstructionEvaluator(ae, loss="l2")
    with pytest.raises(RuntimeError, match="GPU only"):
        ReconstructionEvaluator(ae).add(torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ClassificationEvaluator(_classifier("basic")).add(torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.long))

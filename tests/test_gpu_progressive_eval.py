"""Progressive-sampler inference on the device: SampleNetProgressive.rank against sample_indices (the earlier kernel) and against the
numpy route (sputils.nn_matching of the same knn indices), then ProgressiveClassificationEvaluator / ProgressiveReconstructionEvaluator
against the one-size evaluators fed the same prefixes -- the same kernels on the same input, so the same bits."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SIZES, N, CLASSES = (2, 8, 32, 128), 128, 5
CUTS = (0, 4, 7)  # a batch of 4 and a last batch of 3


def _ranker(shape="bnc", sizes=SIZES, warm=N):
    from samplenet_amd import SampleNetProgressive

    torch.manual_seed(4)
    net = SampleNetProgressive(sizes, 128, group_size=4, input_shape=shape, output_shape=shape).cuda()
    if warm:
        net.train()
        with torch.no_grad():  # running statistics that are not the initial ones
            for _ in range(2):
                x = torch.rand(8, warm, 3, device="cuda") - 0.5
                net(x if shape == "bnc" else x.permute(0, 2, 1).contiguous())
    return net.eval()


def _numpy_route(net, x, xin, simp):
    """sputils.nn_matching of the knn(1) indices of the simplified cloud: -> matched (B,M,3) float64, distinct counts."""
    from samplenet_amd import ops, sputils

    y = simp if net.output_shape == "bcn" else simp.permute(0, 2, 1)
    idx = ops.knn(1, x.permute(0, 2, 1).contiguous(), y.contiguous(), ops.BCN, ops.BCN, return_dist=False)[0]
    nn_idx = idx.squeeze(2).cpu().numpy()
    return sputils.nn_matching(x.cpu().numpy(), nn_idx, net.num_out_points), np.array([len(np.unique(r)) for r in nn_idx])


@pytest.mark.parametrize("shape", ["bnc", "bcn"])
@pytest.mark.parametrize("train_before", [False, True])
def test_rank_is_sample_indices_and_the_numpy_route(shape, train_before):
    net = _ranker(shape)
    x = torch.rand(3, N, 3, device="cuda") - 0.5
    x[:, N // 2:] = x[:, :N // 2]  # half of the points coincident
    xin = x if shape == "bnc" else x.permute(0, 2, 1).contiguous()
    net.train(train_before)
    simp, matched, out_idx, n_unique = net.sample_indices(xin)
    ordered, order, nun = net.rank(xin)
    assert net.training == train_before
    assert ordered.shape == matched.shape and order.dtype == torch.int32 and nun.dtype == torch.int32 and not ordered.requires_grad
    assert torch.equal(ordered, matched) and torch.equal(order, out_idx) and torch.equal(nun, n_unique)
    pts = ordered if shape == "bnc" else ordered.permute(0, 2, 1)
    assert torch.equal(pts, torch.gather(x, 1, order.long().unsqueeze(-1).expand(-1, -1, 3)))
    want, counts = _numpy_route(net, x, xin, simp)
    assert np.array_equal(pts.cpu().numpy().astype(np.float64), want) and np.array_equal(nun.cpu().numpy(), counts)
    for b in range(3):  # every one of the 64 distinct locations is taken before index 0 comes again
        assert len(np.unique(pts[b].cpu().numpy(), axis=0)) == N // 2


@pytest.mark.parametrize("shape", ["bnc", "bcn"])
def test_rank_of_2048_points_stays_on_the_device(shape):
    net = _ranker(shape, sizes=(32, 2048), warm=0)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 2048, 3, generator=g) - 0.5).cuda()
    xin = x if shape == "bnc" else x.permute(0, 2, 1).contiguous()
    simp = net.sample_indices(xin)[0]  # (its matching goes through the host at this size: only the simplified cloud is used)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # no host round trip
    try:
        ordered, order, nun = net.rank(xin)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pts = ordered if shape == "bnc" else ordered.permute(0, 2, 1)
    assert tuple(pts.shape) == (2, 2048, 3) and tuple(order.shape) == (2, 2048)
    want, counts = _numpy_route(net, x, xin, simp)
    assert np.array_equal(pts.cpu().numpy().astype(np.float64), want) and np.array_equal(nun.cpu().numpy(), counts)
    assert np.array_equal(np.sort(order.cpu().numpy(), axis=1), np.tile(np.arange(2048), (2, 1)))


# ------------------------------------------------------------------------------------------------ evaluators
def _data():
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(CUTS[-1], N, 3, generator=g) - 0.5).cuda()
    return x, torch.tensor([0, 1, 2, 3, 0, 1, 2]).cuda()


def _classifier(kind):
    from samplenet_amd import PointNetCls, PointNetClsBasic

    torch.manual_seed(2)
    net = (PointNetCls if kind == "full" else PointNetClsBasic)(num_classes=CLASSES, input_shape="bnc").cuda()
    if kind == "full":
        with torch.no_grad():  # a feature transform that is not the identity: the regulariser is not zero
            net.transform_net2.transform.weight.normal_(0, 0.01)
    return net.eval()


class _Prefix(nn.Module):
    """the first `size` ranked points as a sampler of the one-size evaluators"""

    def __init__(self, ranker, size):
        super().__init__()
        self.ranker, self.size, self.input_shape, self.output_shape = ranker, size, "bnc", "bnc"

    def forward(self, x):
        return self.ranker.rank(x)[0][:, :self.size].contiguous()


def _add_all(ev, *tensors, strict=True):
    torch.cuda.synchronize()
    if strict:
        torch.cuda.set_sync_debug_mode("error")  # add() must not synchronise
    try:
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            ev.add(*[t[lo:hi] for t in tensors])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return ev.result()


def _same(a, b, keys):
    for key in keys:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.dtype == v.dtype and np.array_equal(u, v, equal_nan=True), key


CLS_KEYS = ("preds", "labels", "losses", "batch_sizes", "batch_losses", "logits", "total_seen", "mean_loss", "accuracy", "class_seen",
            "class_correct", "class_accuracies", "avg_class_accuracy", "avg_class_accuracy_seen")


@pytest.mark.parametrize("cls_kind", ["basic", "full"])
def test_progressive_classification_evaluator(cls_kind):
    from samplenet_amd import ClassificationEvaluator, FPSSampler, ProgressiveClassificationEvaluator

    x, labels = _data()
    classifier, ranker = _classifier(cls_kind), _ranker()
    classifier.train()  # arrives in training mode: add() must hand it back that way
    res = _add_all(ProgressiveClassificationEvaluator(classifier, ranker, keep=True), x, labels)
    assert classifier.training and not ranker.training
    classifier.eval()
    assert res["sizes"] == list(SIZES) and sorted(res["by_size"]) == list(SIZES)
    ranked = [ranker.rank(x[lo:hi]) for lo, hi in zip(CUTS[:-1], CUTS[1:])]
    assert np.array_equal(res["n_unique"], torch.cat([r[2] for r in ranked]).cpu().numpy()) and res["n_unique"].dtype == np.int64
    assert res["mean_unique"] == res["n_unique"].astype(np.float64).sum() / CUTS[-1]
    assert np.array_equal(res["ordered"], torch.cat([r[0] for r in ranked]).cpu().numpy())
    assert np.array_equal(res["order"], torch.cat([r[1] for r in ranked]).cpu().numpy())
    for s in SIZES:
        one = _add_all(ClassificationEvaluator(classifier, _Prefix(ranker, s), keep=True), x, labels)
        _same(res["by_size"][s], one, CLS_KEYS)
        assert "n_unique" not in res["by_size"][s] and "mean_unique" not in res["by_size"][s]
        assert np.array_equal(one["clouds"], res["ordered"][:, :s])
    assert set(res["by_size"][SIZES[-1]]) == set(CLS_KEYS)

    # the farthest-point baseline: a prefix of the order of 128 points is the sample of that size
    fps = _add_all(ProgressiveClassificationEvaluator(classifier, FPSSampler(SIZES[-1], False, "bnc", "bnc"), SIZES, keep=True), x, labels)
    for s in SIZES:
        one = _add_all(ClassificationEvaluator(classifier, FPSSampler(s, False, "bnc", "bnc"), keep=True), x, labels)
        _same(fps["by_size"][s], one, ("preds", "logits"))
        assert np.array_equal(one["clouds"], fps["ordered"][:, :s])
    # ... and with the sampler's random permutation in front (one randperm per batch on either route: the same seed, the same clouds)
    torch.manual_seed(9)
    shuffled = _add_all(ProgressiveClassificationEvaluator(classifier, FPSSampler(SIZES[-1], True, "bnc", "bnc"), SIZES, keep=True), x, labels)
    xn = x.cpu().numpy()
    assert np.array_equal(shuffled["ordered"], np.stack([xn[b][shuffled["order"][b]] for b in range(CUTS[-1])]))
    assert not np.array_equal(shuffled["order"], fps["order"])
    for s in SIZES[1:3]:
        torch.manual_seed(9)
        # (the sampler itself indexes with its host permutation: a blocking transfer inside the one-size evaluator's add)
        one = _add_all(ClassificationEvaluator(classifier, FPSSampler(s, True, "bnc", "bnc"), keep=True), x, labels, strict=False)
        _same(shuffled["by_size"][s], one, ("preds", "logits"))
        assert np.array_equal(one["clouds"], shuffled["ordered"][:, :s])
    # the input order
    plain = _add_all(ProgressiveClassificationEvaluator(classifier, None, SIZES, keep=True), x, labels)
    _same(plain["by_size"][N], _add_all(ClassificationEvaluator(classifier, None, keep=True), x, labels), CLS_KEYS)
    assert np.array_equal(plain["ordered"], x.cpu().numpy()) and (plain["order"] == np.arange(N)).all()


REC_KEYS = ("losses", "mean_loss", "reference_losses", "nre", "mean_reference_loss", "mean_nre", "reconstructions")


@pytest.mark.parametrize("loss", ["chamfer", "emd"])
def test_progressive_reconstruction_evaluator(loss):
    from samplenet_amd import FPSSampler, PointNetAE, ProgressiveReconstructionEvaluator, ReconstructionEvaluator

    x, _ = _data()
    torch.manual_seed(6)
    ae = PointNetAE(n_pc_points=N, bottleneck_size=128, input_shape="bnc").cuda().eval()
    ranker = _ranker()
    res = _add_all(ProgressiveReconstructionEvaluator(ae, ranker, loss=loss, with_reference=True, keep=True), x)
    assert res["sizes"] == list(SIZES) and not ae.training
    ranked = [ranker.rank(x[lo:hi]) for lo, hi in zip(CUTS[:-1], CUTS[1:])]
    assert np.array_equal(res["n_unique"], torch.cat([r[2] for r in ranked]).cpu().numpy())
    assert res["mean_unique"] == res["n_unique"].astype(np.float64).mean()
    assert np.array_equal(res["order"], torch.cat([r[1] for r in ranked]).cpu().numpy())
    for s in SIZES:
        one = _add_all(ReconstructionEvaluator(ae, _Prefix(ranker, s), loss=loss, with_reference=True, keep=True), x)
        _same(res["by_size"][s], one, REC_KEYS)
        assert set(res["by_size"][s]) == set(REC_KEYS)
        assert np.array_equal(one["sampled"], res["ordered"][:, :s])
        assert np.array_equal(res["by_size"][s]["reference_losses"], res["by_size"][SIZES[0]]["reference_losses"])
        assert np.array_equal(res["by_size"][s]["nre"], np.divide(res["by_size"][s]["losses"], res["by_size"][s]["reference_losses"]))
    if loss == "chamfer":
        bare = _add_all(ProgressiveReconstructionEvaluator(ae, ranker, loss=loss, with_reference=False), x)
        for s in SIZES:
            assert set(bare["by_size"][s]) == {"losses", "mean_loss"}
            assert np.array_equal(bare["by_size"][s]["losses"], res["by_size"][s]["losses"])
        fps = _add_all(ProgressiveReconstructionEvaluator(ae, FPSSampler(SIZES[-1], False, "bnc", "bnc"), SIZES), x)
        for s in SIZES:
            one = _add_all(ReconstructionEvaluator(ae, FPSSampler(s, False, "bnc", "bnc")), x)
            _same(fps["by_size"][s], one, ("losses", "reference_losses", "nre"))
        plain = _add_all(ProgressiveReconstructionEvaluator(ae, None, SIZES), x)
        assert np.array_equal(plain["by_size"][N]["losses"], plain["by_size"][N]["reference_losses"])


def test_argument_checks_and_defaults():
    from samplenet_amd import FPSSampler, PointNetAE, ProgressiveClassificationEvaluator, ProgressiveReconstructionEvaluator, RandomSampler

    classifier, ranker = _classifier("basic"), _ranker(warm=0)
    assert ProgressiveClassificationEvaluator(classifier, ranker).sizes == list(SIZES)
    assert ProgressiveClassificationEvaluator(classifier, FPSSampler(16, False, "bnc", "bnc")).sizes == [16]
    assert ProgressiveClassificationEvaluator(classifier, ranker, (8, 2)).sizes == [2, 8]
    with pytest.raises(ValueError, match="sizes"):
        ProgressiveClassificationEvaluator(classifier, None)
    with pytest.raises(ValueError, match="sizes"):
        ProgressiveClassificationEvaluator(classifier, ranker, (4, 4))
    with pytest.raises(RuntimeError, match="nothing was added"):
        ProgressiveClassificationEvaluator(classifier, ranker).result()
    ae = PointNetAE(n_pc_points=N, bottleneck_size=128, input_shape="bnc").cuda()
    with pytest.raises(RuntimeError, match="nothing was added"):
        ProgressiveReconstructionEvaluator(ae, ranker).result()
    with pytest.raises(ValueError):
        ProgressiveReconstructionEvaluator(ae, ranker, loss="l2")
    with pytest.raises(RuntimeError, match="GPU only"):
        ProgressiveReconstructionEvaluator(ae, ranker).add(torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ProgressiveClassificationEvaluator(classifier, ranker).add(torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.long))
    x, labels = _data()
    with pytest.raises(TypeError, match="rank"):
        ProgressiveClassificationEvaluator(classifier, RandomSampler(16, "bnc", "bnc"), (16,)).add(x, labels)
    with pytest.raises(ValueError, match="exceeds"):
        ProgressiveClassificationEvaluator(classifier, ranker, (256,)).add(x, labels)
    with pytest.raises(ValueError, match="exceeds"):
        ProgressiveClassificationEvaluator(classifier, None, (256,)).add(x, labels)

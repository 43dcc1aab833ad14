"""RetrievalEvaluator / ProgressiveRetrievalEvaluator: the evaluator's figures are ops.retrieval_metrics (held to numpy by
tests/test_gpu_retrieval.py) on the descriptors the classifier gives for the same clouds one batch at a time, and
retrieval_aggregates of those; the progressive evaluator equals one plain evaluation per prefix size, bit for bit -- the same
kernels on the same input.  add() never synchronises and leaves the modules' training flags as found."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N, M, CLASSES, LEVELS = 128, 16, 5, 7
CUTS = (0, 8, 16, 24)  # 3 batches of 8 clouds
SIZES = (4, 8, 16)


def _data():
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(CUTS[-1], N, 3, generator=g) - 0.5).cuda()
    x[5] = x[2]  # two shapes with one descriptor: a zero distance
    labels = torch.arange(CUTS[-1]) % (CLASSES - 1)
    labels[7] = CLASSES - 1  # a class of one: that query is invalid
    return x, labels.cuda()


def _classifier(kind):
    from samplenet_amd import PointNetCls, PointNetClsBasic

    torch.manual_seed(2)
    net = (PointNetCls if kind == "full" else PointNetClsBasic)(num_classes=CLASSES, input_shape="bnc").cuda()
    if kind == "full":
        with torch.no_grad():  # a feature transform that is not the identity
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


class _Prefix(nn.Module):
    """the first `size` points of the ranked cloud (of the input order without a ranker) as a sampler of the plain evaluator"""

    def __init__(self, ranker, size):
        super().__init__()
        self.ranker, self.size, self.input_shape, self.output_shape = ranker, size, "bnc", "bnc"

    def forward(self, x):
        return (x if self.ranker is None else self.ranker.rank(x)[0])[:, :self.size].contiguous()


def _add_all(ev, x, labels, train=()):
    """every batch added with synchronisation forbidden; `train`: modules that arrive in training mode and must leave in it; every
    other module's flag must be left as found too"""
    for m in train:
        m.train()
    mods = [m for m in (ev.classifier, ev.sampler) if m is not None]
    was = [m.training for m in mods]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # add() must not synchronise
    try:
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            ev.add(x[lo:hi], labels[lo:hi])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(m.training for m in train) and [m.training for m in mods] == was
    for m in train:
        m.eval()
    return ev.result()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


@pytest.mark.parametrize("cls_kind", ["basic", "full"])
@pytest.mark.parametrize("sampler_kind", ["none", "fps", "samplenet"])
def test_retrieval_evaluator(cls_kind, sampler_kind):
    from samplenet_amd import RetrievalEvaluator, ops, retrieval_aggregates
    from samplenet_amd.evaluation import _sample_with_indices

    x, labels = _data()
    classifier, sampler = _classifier(cls_kind), _sampler(sampler_kind)
    res = _add_all(RetrievalEvaluator(classifier, sampler, levels=LEVELS, keep=True), x, labels, train=[classifier])

    # the same clouds through the same modules, one batch at a time
    with torch.no_grad():
        desc = torch.cat([classifier(_sample_with_indices(sampler, x[lo:hi])[1])[1]["retrieval_vectors"] for lo, hi in zip(CUTS[:-1], CUTS[1:])])
    n = CUTS[-1]
    assert tuple(desc.shape) == (n, 256) and np.array_equal(_bits(res["descriptors"]), _bits(desc.cpu().numpy()))
    ap, prec, nrel, order, _ = ops.retrieval_metrics(desc, labels, LEVELS, return_order=True)
    assert res["ap"].dtype == np.float64 and res["prec"].shape == (n, LEVELS) and res["n_relevant"].dtype == np.int64
    assert np.array_equal(res["ap"], ap.cpu().numpy().astype(np.float64), equal_nan=True)
    assert np.array_equal(res["prec"], prec.cpu().numpy().astype(np.float64), equal_nan=True)
    assert np.array_equal(res["n_relevant"], nrel.cpu().numpy()) and np.array_equal(res["labels"], labels.cpu().numpy())
    assert np.array_equal(res["order"], order.cpu().numpy()) and res["order"].shape == (n, n - 1)
    agg = retrieval_aggregates(res["ap"], res["prec"], res["n_relevant"])
    assert set(agg) == {"map", "pr_curve", "auc", "n_valid"}
    for key in agg:
        assert np.array_equal(res[key], agg[key]), key
    # shape 7 alone carries its label; shapes 2 and 5 are one cloud (for a sampler that does not shuffle: one descriptor)
    assert res["n_relevant"][7] == 0 and np.isnan(res["ap"][7]) and res["n_valid"] == n - 1 and 0 < res["map"] <= 1
    assert res["order"][2, 0] == 5 and res["order"][5, 0] == 2
    # the simplified cloud instead of the matched one, and no keeping
    if sampler_kind == "samplenet":
        simp = _add_all(RetrievalEvaluator(classifier, sampler, match_output=False, levels=LEVELS), x, labels)
        assert "order" not in simp and "descriptors" not in simp and not np.array_equal(simp["ap"], res["ap"], equal_nan=True)


@pytest.mark.parametrize("cls_kind", ["basic", "full"])
@pytest.mark.parametrize("sampler_kind", ["none", "fps", "samplenet"])
def test_progressive_retrieval_evaluator(cls_kind, sampler_kind):
    from samplenet_amd import FPSSampler, ProgressiveRetrievalEvaluator, RetrievalEvaluator

    x, labels = _data()
    classifier, sampler = _classifier(cls_kind), _sampler(sampler_kind)
    res = _add_all(ProgressiveRetrievalEvaluator(classifier, sampler, SIZES, levels=LEVELS), x, labels, train=[classifier])
    assert res["sizes"] == list(SIZES) and sorted(res["by_size"]) == list(SIZES)
    assert np.array_equal(res["labels"], labels.cpu().numpy())
    for s in SIZES:
        # (a prefix of a farthest-point order is the farthest-point sample of that size)
        one_sampler = FPSSampler(s, False, "bnc", "bnc") if sampler_kind == "fps" else _Prefix(sampler, s)
        one = _add_all(RetrievalEvaluator(classifier, one_sampler, levels=LEVELS), x, labels)
        got = res["by_size"][s]
        assert set(got) == {"ap", "prec", "map", "pr_curve", "auc", "n_valid"}
        for key in got:
            u, v = np.asarray(got[key]), np.asarray(one[key])
            assert u.dtype == v.dtype and np.array_equal(_bits(u), _bits(v)), (s, key)
        assert np.array_equal(res["n_relevant"], one["n_relevant"])
    assert not np.array_equal(res["by_size"][4]["ap"], res["by_size"][16]["ap"], equal_nan=True)


def test_argument_checks_and_defaults():
    from samplenet_amd import FPSSampler, ProgressiveRetrievalEvaluator, RetrievalEvaluator

    classifier = _classifier("basic")
    assert RetrievalEvaluator(classifier).levels == 20 and ProgressiveRetrievalEvaluator(classifier, None, (8, 2)).sizes == [2, 8]
    assert ProgressiveRetrievalEvaluator(classifier, FPSSampler(16, False, "bnc", "bnc")).sizes == [16]
    with pytest.raises(ValueError, match="sizes"):
        ProgressiveRetrievalEvaluator(classifier, None)
    with pytest.raises(RuntimeError, match="nothing was added"):
        RetrievalEvaluator(classifier).result()
    with pytest.raises(RuntimeError, match="nothing was added"):
        ProgressiveRetrievalEvaluator(classifier, None, (4,)).result()
    with pytest.raises(RuntimeError, match="GPU only"):
        RetrievalEvaluator(classifier).add(torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU only"):
        ProgressiveRetrievalEvaluator(classifier, None, (4,)).add(torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.long))
    x, labels = _data()
    ev = RetrievalEvaluator(classifier)
    ev.add(x[:8], labels[:8])
    ev.reset()
    with pytest.raises(RuntimeError, match="nothing was added"):
        ev.result()

"""The fp64 restatement of the segmentation terms (tests/seg_terms_ref.py) against CPU torch's fp64
F.cross_entropy(weight=, ignore_index=) with reduction 'none' and 'mean' and autograd's gradient; its prediction and counts against
numpy; evaluation.segmentation_aggregates against a plain per-cloud loop (the definitions its docstring gives); the segmentation
network's state_dict keys and shapes at a tiny table; segmentation_loss's label rewrite for an ignore_index inside the range.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_terms_ref as R

TINY_SA = ((16, 0.4, 4, (8, 16)), (8, 0.6, 4, (16, 16)), (4, 0.9, 4, (16, 32)), (2, 1.5, 2, (32, 32)))
TINY_FP = ((16, 16), (16, 16), (32, 16), (32, 32))


def _case_with_ignored(B, N, C, ignore_index, seed=0):
    x, lab = R.make_case("random", B, N, C, seed)
    rng = np.random.default_rng([seed, 9])
    lab = np.where(rng.random(B * N) < 0.3, ignore_index, lab).astype(np.int32)
    return x, lab


@pytest.mark.parametrize("weights", R.WEIGHTS)
@pytest.mark.parametrize("ignore_index", [-100, -1, 255])
@pytest.mark.parametrize("B,N,C", [(1, 1, 1), (3, 7, 13), (2, 100, 50), (2, 65, 130)])
def test_restatement_matches_torch_fp64(B, N, C, ignore_index, weights):
    x, lab = _case_with_ignored(B, N, C, ignore_index)
    w = R.make_weights(weights, C)
    T = R.terms(x, lab, N, w)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt = None if w is None else torch.from_numpy(w).double()
    lt = torch.from_numpy(lab).long()
    # reduction='none' returns w_label ce; the kernel's ce is unweighted: compare the unweighted call, then the weighted mean
    ce = F.cross_entropy(xt, lt, ignore_index=ignore_index, reduction="none")
    assert np.allclose(T["ce"], ce.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(T["ce"][lab == ignore_index], np.zeros(int((lab == ignore_index).sum())))
    wce = F.cross_entropy(xt, lt, weight=wt, ignore_index=ignore_index, reduction="none")
    assert np.allclose(T["t"], wce.detach().numpy(), rtol=1e-12, atol=1e-12)
    mean = F.cross_entropy(xt, lt, weight=wt, ignore_index=ignore_index, reduction="mean")
    assert np.isclose(T["means"][0], float(mean.detach()), rtol=1e-12, atol=1e-12, equal_nan=True)
    if not np.isfinite(float(mean.detach())):
        return
    gm, gce = R.upstream_case(B * N)
    for g_means, g_ce in ((gm, gce), (gm, None), (None, gce)):
        tot = 0.0 * xt.sum()
        if g_means is not None:
            tot = tot + float(g_means[0]) * mean
        if g_ce is not None:
            tot = tot + (ce * torch.from_numpy(g_ce).double()).sum()
        (g,) = torch.autograd.grad(tot, [xt], retain_graph=True)
        assert np.allclose(R.backward(T, g_means, g_ce), g.numpy(), rtol=1e-10, atol=1e-13)


def test_no_valid_point_gives_torchs_nan_mean():
    x, lab = R.make_case("all_ignored", 2, 5, 4)
    T = R.terms(x, lab, 5)
    mean = F.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(lab).long(), ignore_index=-100)
    assert np.isnan(float(mean)) and np.isnan(T["means"][0]) and T["means"][1] == 0 and T["means"][2] == 0
    assert not T["cloud_counts"].any() and not R.backward(T, np.ones(3, np.float32), None).any()


@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("B,N,C", [(3, 7, 13), (2, 100, 65), (2, 40, 130), (4, 3, 1)])
def test_restatement_pred_and_counts_are_numpys(recipe, B, N, C):
    x, lab = R.make_case(recipe, B, N, C)
    T = R.terms(x, lab, N)
    pred = np.argmax(x, axis=1)
    assert np.array_equal(T["pred"], pred)
    valid = (lab >= 0) & (lab < C)
    for b in range(B):
        sl = slice(b * N, (b + 1) * N)
        v, l, p = valid[sl], lab[sl], pred[sl]
        assert np.array_equal(T["cloud_counts"][b, :, 0], np.bincount(l[v], minlength=C))
        assert np.array_equal(T["cloud_counts"][b, :, 1], np.bincount(p[v], minlength=C))
        assert np.array_equal(T["cloud_counts"][b, :, 2], np.bincount(l[v & (p == l)], minlength=C))
    if recipe == "ties":
        assert (np.sort(x, axis=1)[:, -2:] == 3).all() or C == 1  # the maximum really is planted twice wherever two seams exist
    if recipe == "all_ignored":
        assert not T["cloud_counts"].any() and not T["ce"].any()
    if recipe == "cloud_ignored":
        assert not T["cloud_counts"][B - 1].any() and T["cloud_counts"][0].any()


def test_restatement_edge_rules():
    x, lab = R.make_case("nan_inf", 2, 10, 6)
    T = R.terms(x, lab, 10)
    assert np.isnan(T["ce"][[0, 5]]).all() and T["pred"][0] == 0 and T["pred"][5] == 1  # the first NaN is the prediction
    assert np.isposinf(T["ce"][[2, 12]]).all()                                           # the label's logit is -inf
    assert np.isnan(T["ce"][3]) and T["pred"][3] == 0                                     # a row of all -inf
    x, lab = R.make_case("random", 3, 2, 1)
    assert np.array_equal(R.terms(x, lab, 2)["ce"], np.zeros(6))


def test_the_counted_chain_covers_the_mapping():
    # 32 x 4096 rows of 13 classes: 16 lanes a row, 64 rows a workgroup, 2048 partials, 8 a thread in the closing launch
    assert R.group_lanes(13) == 16 and R.rows_per_block(13) == 64 and R.blocks(32 * 4096, 13) == 2048
    assert R.sum_chain(32 * 4096, 13) == 4 + 6 + 4 + 8 + 6 + 4
    assert [R.group_lanes(c) for c in R.CLASSES] == [1, 2, 16, 16, 32, 64, 64, 64, 64]


def _random_eval(seed, clouds, N, C, parts=None):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, (clouds, N))
    labels[rng.random((clouds, N)) < 0.2] = -100
    pred = np.where(rng.random((clouds, N)) < 0.6, np.clip(labels, 0, C - 1), rng.integers(0, C, (clouds, N)))
    counts = np.zeros((clouds, C, 3), dtype=np.int64)
    for b in range(clouds):
        v = labels[b] >= 0
        counts[b, :, 0] = np.bincount(labels[b][v], minlength=C)
        counts[b, :, 1] = np.bincount(pred[b][v], minlength=C)
        counts[b, :, 2] = np.bincount(labels[b][v & (pred[b] == labels[b])], minlength=C)
    return labels, pred, counts


def test_aggregates_match_the_per_cloud_loop():
    from samplenet_amd.evaluation import segmentation_aggregates

    C = 7
    labels, pred, counts = _random_eval(0, 6, 50, C)
    labels[labels == 5] = -100               # class 5: never labelled, still predicted -> accuracy 0, IoU 0, in the means
    labels[labels == 6] = 0
    pred[pred == 6] = 0                      # class 6: absent from both -> NaN, out of the means
    counts = np.zeros_like(counts)
    for b in range(6):
        v = labels[b] >= 0
        counts[b, :, 0] = np.bincount(labels[b][v], minlength=C)
        counts[b, :, 1] = np.bincount(pred[b][v], minlength=C)
        counts[b, :, 2] = np.bincount(labels[b][v & (pred[b] == labels[b])], minlength=C)
    means = np.array([[0.7, 0.5, 120.0], [np.nan, 0.0, 0.0], [1.9, 0.25, 33.5]])
    parts = {0: (0, 1, 2), 1: (3, 4), 2: (5, 6), 3: (6,)}
    cats = np.array([0, 1, 2, 0, 3, 1])
    got = segmentation_aggregates(counts, means, cats, parts)
    ref = R.aggregates_loop(pred, labels, C, means, cats, parts)
    for k in ("total_valid", "overall_accuracy", "mean_class_accuracy", "miou", "mean_loss", "instance_miou", "category_miou"):
        assert got[k] == pytest.approx(ref[k], rel=1e-14, abs=0), k
    for k in ("class_labelled", "class_predicted", "class_correct"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.allclose(got["cloud_iou"], ref["cloud_iou"], rtol=1e-14, atol=0)
    assert got["class_labelled"][5] == 0 and got["class_predicted"][5] > 0 and got["class_accuracies"][5] == 0 and got["class_iou"][5] == 0
    assert np.isnan(got["class_accuracies"][6]) and np.isnan(got["class_iou"][6])
    assert got["miou"] == pytest.approx(np.mean(got["class_iou"][:6]), rel=1e-14)
    assert got["mean_loss"] == pytest.approx((0.7 * 120.0 + 1.9 * 33.5) / 153.5, rel=1e-14)
    # category 3's one part (class 6) is absent from the labels and the predictions of its cloud: it scores 1
    assert got["cloud_iou"][4] == 1.0 and got["category_iou"][3] == 1.0
    # no parts table: the part figures are not formed
    assert "instance_miou" not in segmentation_aggregates(counts, means)


def test_aggregates_without_a_valid_point():
    from samplenet_amd.evaluation import segmentation_aggregates

    got = segmentation_aggregates(np.zeros((2, 3, 3), dtype=np.int64), np.array([[np.nan, 0.0, 0.0]]))
    assert got["total_valid"] == 0 and all(np.isnan(got[k]) for k in ("overall_accuracy", "mean_class_accuracy", "miou", "mean_loss"))


def test_network_state_dict_keys_and_shapes_at_a_tiny_table():
    from samplenet_amd.compat.pointnet2.models import PointNet2SemSegSSG

    net = PointNet2SemSegSSG(5, input_channels=3, sa=TINY_SA, fp=TINY_FP, head=16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    conv = {k: v for k, v in shapes.items() if k.endswith("conv.weight") or k.startswith("fc_layer")}
    assert conv == {
        "SA_modules.0.mlps.0.0.conv.weight": (8, 6, 1, 1), "SA_modules.0.mlps.0.1.conv.weight": (16, 8, 1, 1),
        "SA_modules.1.mlps.0.0.conv.weight": (16, 19, 1, 1), "SA_modules.1.mlps.0.1.conv.weight": (16, 16, 1, 1),
        "SA_modules.2.mlps.0.0.conv.weight": (16, 19, 1, 1), "SA_modules.2.mlps.0.1.conv.weight": (32, 16, 1, 1),
        "SA_modules.3.mlps.0.0.conv.weight": (32, 35, 1, 1), "SA_modules.3.mlps.0.1.conv.weight": (32, 32, 1, 1),
        "FP_modules.0.mlp.0.conv.weight": (16, 19, 1, 1), "FP_modules.0.mlp.1.conv.weight": (16, 16, 1, 1),
        "FP_modules.1.mlp.0.conv.weight": (16, 32, 1, 1), "FP_modules.1.mlp.1.conv.weight": (16, 16, 1, 1),
        "FP_modules.2.mlp.0.conv.weight": (32, 48, 1, 1), "FP_modules.2.mlp.1.conv.weight": (16, 32, 1, 1),
        "FP_modules.3.mlp.0.conv.weight": (32, 64, 1, 1), "FP_modules.3.mlp.1.conv.weight": (32, 32, 1, 1),
        "fc_layer.0.weight": (16, 16, 1), "fc_layer.1.weight": (16,), "fc_layer.1.bias": (16,), "fc_layer.1.running_mean": (16,),
        "fc_layer.1.running_var": (16,), "fc_layer.1.num_batches_tracked": (), "fc_layer.4.weight": (5, 16, 1), "fc_layer.4.bias": (5,)}
    # every conv of the levels has its BatchNorm beside it, and nothing else is in the state
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    levels = [k[:-len("conv.weight")] for k in conv if k.endswith("conv.weight")]
    assert set(shapes) == set(conv) | {p + "bn." + s for p in levels for s in bn}
    assert len(net.SA_modules) == 4 and len(net.FP_modules) == 4 and all(m.fused for m in net.FP_modules)
    assert not any(m.fused for m in PointNet2SemSegSSG(5, fused=False, sa=TINY_SA, fp=TINY_FP, head=16).FP_modules)
    # the default tables: no input features, the xyz columns alone feed the first level; the head is 128 -> 128 -> classes
    full = {k: tuple(v.shape) for k, v in PointNet2SemSegSSG(13).state_dict().items()}
    assert full["SA_modules.0.mlps.0.0.conv.weight"] == (32, 3, 1, 1) and full["SA_modules.3.mlps.0.2.conv.weight"] == (512, 256, 1, 1)
    assert full["FP_modules.0.mlp.0.conv.weight"] == (128, 128, 1, 1) and full["FP_modules.3.mlp.0.conv.weight"] == (256, 768, 1, 1)
    assert full["fc_layer.0.weight"] == (128, 128, 1) and full["fc_layer.4.weight"] == (13, 128, 1)


def test_an_ignore_index_inside_the_range_is_rewritten():
    from samplenet_amd.segmentation import fused_labels

    lab = torch.tensor([[0, 2, 4, 2], [2, 1, -100, 3]])
    out = fused_labels(lab, 5, ignore_index=2)
    assert torch.equal(out, torch.tensor([[0, -1, 4, -1], [-1, 1, -100, 3]])) and torch.equal(lab[0], torch.tensor([0, 2, 4, 2]))
    for outside in (-100, -1, 255, 5):
        assert fused_labels(lab, 5, ignore_index=outside) is lab  # the kernel ignores these already
    # the rewritten labels under the kernel's rule are torch's ignore_index=2
    x, _ = R.make_case("random", 2, 4, 5)
    w = R.make_weights("given", 5)
    T = R.terms(x, out.numpy().reshape(-1), 4, w)
    # (the label -100 is ignored by the kernel's rule; torch would refuse it beside ignore_index=2, so that point is left out)
    keep = lab.reshape(-1) != -100
    ref = F.cross_entropy(torch.from_numpy(x).double()[keep], lab.reshape(-1)[keep], weight=torch.from_numpy(w).double(), ignore_index=2)
    assert np.isclose(T["means"][0], float(ref), rtol=1e-12)


def test_the_ops_refuse_cpu_tensors():
    from samplenet_amd import ops, segmentation_loss

    x, lab = torch.randn(2, 4, 5), torch.zeros(2, 4, dtype=torch.long)
    for fn in (ops.segmentation_terms, ops.segmentation_mean_loss, lambda a, b: segmentation_loss(a, b, fused=True)):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(x, lab)
    # the torch route is torch's: it runs wherever the tensors are
    assert torch.isfinite(segmentation_loss(x, lab, fused=False))

"""The host layer of the segmentation terms on the GPU: ops.segmentation_terms / segmentation_mean_loss against the direct entries
bit for bit (the transposed-view input and the gradients through autograd included); segmentation_loss on both routes against fp64;
PointNet2SemSegSSG at a tiny table against its own modules called one by one, one training step, and run-to-run bits;
SegmentationEvaluator over three batches of unequal size against the numpy yardstick of tests/seg_terms_ref.py fed the same logits."""
import numpy as np
import pytest
import torch

import seg_terms_ref as R
from test_gpu_seg_terms import _within

pytestmark = pytest.mark.gpu

TINY_SA = ((16, 0.4, 4, (8, 16)), (8, 0.6, 4, (16, 16)), (4, 0.9, 4, (16, 32)), (2, 1.5, 2, (32, 32)))
TINY_FP = ((16, 16), (16, 16), (32, 16), (32, 32))


def _direct(x, lab, N, w, gm=None, gce=None):
    """the entries on plain device tensors -> ce, pred, counts, means, g_logits (numpy)"""
    from samplenet_amd._lib import check, lib

    R_, C = x.shape
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    dw = None if w is None else torch.from_numpy(w).cuda()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ce, pred = torch.empty(R_, device="cuda"), torch.empty(R_, device="cuda", dtype=torch.int32)
    counts, means = torch.empty(R_ // N, C, 3, device="cuda", dtype=torch.int32), torch.empty(3, device="cuda")
    ws = torch.empty(max(1, lib.sn_segmentation_terms_workspace_bytes(R_, C)), device="cuda", dtype=torch.uint8)
    check(lib.sn_segmentation_terms_forward(R_, N, C, p(dx), p(dl), p(dw), p(ce), p(pred), p(counts), p(means), p(ws), None), "forward")
    g = torch.empty(R_, C, device="cuda")
    dgm = None if gm is None else torch.from_numpy(gm).cuda()
    dgce = None if gce is None else torch.from_numpy(gce).cuda()
    check(lib.sn_segmentation_terms_backward(R_, C, p(dx), p(dl), p(dw), p(means), p(dgm), p(dgce), p(g), None), "backward")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (ce, pred, counts, means, g)]


@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("weights", ["none", "given"])
@pytest.mark.parametrize("B,N,C", [(3, 7, 13), (2, 257, 50), (2, 65, 65)])
def test_ops_are_the_direct_entries_bit_for_bit(B, N, C, weights, flipped):
    from samplenet_amd import ops

    x, lab = R.make_case("mixed_ignored", B, N, C)
    w = R.make_weights(weights, C)
    gm, gce = R.upstream_case(B * N)
    gm[1:] = 0  # (autograd hands the whole upstream vector over; only [0] is read)
    rows = torch.from_numpy(x).cuda().view(B, N, C)
    labels = torch.from_numpy(lab).cuda().view(B, N).long()
    dw = None if w is None else torch.from_numpy(w).cuda()
    leaf = (rows.transpose(1, 2) if flipped else rows).detach().requires_grad_(True)  # flipped: (B,C,N), a view of (B,N,C) memory
    assert leaf.shape == ((B, C, N) if flipped else (B, N, C)) and leaf.data_ptr() == rows.data_ptr()
    ce, pred, counts, means = ops.segmentation_terms(leaf, labels, dw)
    assert ce.shape == (B, N) and pred.shape == (B, N) and counts.shape == (B, C, 3) and means.shape == (3,)
    assert pred.dtype == torch.int32 and counts.dtype == torch.int32 and not pred.requires_grad and not counts.requires_grad
    ((ce * torch.from_numpy(gce).cuda().view(B, N)).sum() + float(gm[0]) * means[0] + 7.0 * means[1] + 3.0 * means[2]).backward()
    ref = _direct(x, lab, N, w, gm, gce)
    for name, a, b in zip(("ce", "pred", "counts", "means"), (ce, pred, counts, means), ref):
        assert np.array_equal(a.detach().cpu().numpy().reshape(b.shape), b, equal_nan=True), name
    grad = leaf.grad.transpose(1, 2) if flipped else leaf.grad
    assert leaf.grad.shape == leaf.shape and np.array_equal(grad.cpu().numpy().reshape(B * N, C), ref[4], equal_nan=True)
    # the mean loss alone: the same means[0], and the backward with the upstream scalar as g_means
    leaf2 = leaf.detach().clone().requires_grad_(True) if not flipped else rows.clone().transpose(1, 2).requires_grad_(True)
    loss = ops.segmentation_mean_loss(leaf2, labels, dw)
    assert loss.dim() == 0 and np.array_equal(loss.detach().cpu().numpy(), ref[3][0], equal_nan=True)
    (loss * 0.5).backward()
    ref2 = _direct(x, lab, N, w, np.array([0.5, 0, 0], dtype=np.float32), None)
    grad2 = leaf2.grad.transpose(1, 2) if flipped else leaf2.grad
    assert np.array_equal(grad2.cpu().numpy().reshape(B * N, C), ref2[4], equal_nan=True)


@pytest.mark.parametrize("ignore_index", [-100, 2])
@pytest.mark.parametrize("weights", ["none", "given"])
def test_segmentation_loss_on_both_routes_against_fp64(weights, ignore_index):
    from samplenet_amd import segmentation_loss

    B, N, C = 2, 257, 13
    x, lab = R.make_case("random", B, N, C)
    lab = np.where(np.random.default_rng(5).random(B * N) < 0.25, ignore_index, lab).astype(np.int32)
    w = R.make_weights(weights, C)
    T = R.terms(x, np.where(lab == ignore_index, -1, lab), N, w)
    dw = None if w is None else torch.from_numpy(w).cuda()
    labels = torch.from_numpy(lab).cuda().view(B, N).long()
    gm = np.array([1.0, 0, 0], dtype=np.float32)
    for fused in (True, False):
        for flipped in (False, True):
            rows = torch.from_numpy(x).cuda().view(B, N, C)
            leaf = (rows.transpose(1, 2) if flipped else rows).detach().requires_grad_(True)
            loss = segmentation_loss(leaf, labels, dw, ignore_index=ignore_index, fused=fused)
            loss.backward()
            grad = (leaf.grad.transpose(1, 2) if flipped else leaf.grad).cpu().numpy().reshape(B * N, C)
            tag = "segmentation_loss fused=%s flipped=%s w=%s ignore=%d" % (fused, flipped, weights, ignore_index)
            if fused:
                _within(tag, [float(loss.detach())], [T["means"][0]], R.bound_means(T)[0])
                _within(tag + " gradient", grad, R.backward(T, gm, None), R.bound_backward(T, gm, None))
            else:
                # torch's own fp32 route, whatever order it sums in: any order of R terms stays under gamma_(R-1) sum |t| / den, a
                # term within 16 roundings of its magnitudes (log-softmax, product), the division; the gradient's entries likewise
                mags = (np.abs(T["lse"]) + np.abs(T["ce"]) + np.abs(T["m"]))[T["valid"]]
                bound = (R._g(B * N + 16) * (np.abs(T["t"]).sum() + (T["w"][T["valid"]] * mags).sum()) / T["means"][2]
                         + R._g(B * N) * abs(T["means"][0]))
                _within(tag, [float(loss.detach())], [T["means"][0]], bound)
                k = np.where(T["valid"], T["w"] / T["means"][2], 0.0)
                _within(tag + " gradient", grad, R.backward(T, gm, None), R._g(B * N + 32) * k[:, None] + R.TINY)


def _tiny_net(fused, seed=0):
    from samplenet_amd.compat.pointnet2.models import PointNet2SemSegSSG

    torch.manual_seed(seed)
    return PointNet2SemSegSSG(5, input_channels=3, fused=fused, sa=TINY_SA, fp=TINY_FP, head=16).cuda()


def _tiny_batch(B=2, N=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    xyz, feats = torch.rand(B, N, 3, generator=g).cuda(), torch.randn(B, 3, N, generator=g).cuda()
    labels = torch.randint(0, 5, (B, N), generator=g)
    labels[torch.rand(B, N, generator=g) < 0.2] = -100
    return xyz, feats, labels.cuda()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_network_is_its_modules_called_one_by_one(fused, training):
    import torch.nn.functional as F

    net = _tiny_net(fused).train(training)
    xyz, feats, _labels = _tiny_batch()
    with torch.no_grad():
        state = {k: v.clone() for k, v in net.state_dict().items()}
        torch.manual_seed(7)
        logits = net(xyz, feats)
        net.load_state_dict(state)  # (the running statistics moved in training mode: the second pass starts where the first did)
        torch.manual_seed(7)
        l_xyz, l_f = [xyz], [feats]
        for sa in net.SA_modules:
            a, b = sa(l_xyz[-1], l_f[-1])
            l_xyz.append(a)
            l_f.append(b)
        assert [t.shape[1] for t in l_xyz] == [64, 16, 8, 4, 2]
        for j in (3, 2, 1, 0):
            l_f[j] = net.FP_modules[j](l_xyz[j], l_xyz[j + 1], l_f[j], l_f[j + 1], fused=fused)
        top = l_f[0]                                        # (B, 16, N)
        if fused:                                           # a view of (B, N, 16) rows, read by the head without a copy
            assert top.transpose(1, 2).is_contiguous()
        rows = top.transpose(1, 2).contiguous().view(2 * 64, 16)
        conv0, bn, act, drop, conv1 = net.fc_layer
        hidden = drop(act(bn(F.linear(rows, conv0.weight.squeeze(-1)))))
        mine = F.linear(hidden, conv1.weight.squeeze(-1), conv1.bias).view(2, 64, 5)
    assert logits.shape == (2, 5, 64) and logits.transpose(1, 2).is_contiguous()  # the original's shape on (B,N,C) memory
    assert torch.equal(logits.transpose(1, 2), mine) and bool(torch.isfinite(mine).all())


def _train_step(fused_loss, seed=0):
    from samplenet_amd import optim, segmentation_loss

    net = _tiny_net(True, seed).train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    xyz, feats, labels = _tiny_batch()
    torch.manual_seed(11)
    w = torch.linspace(0.5, 2.0, 5, device="cuda")
    loss = segmentation_loss(net(xyz, feats), labels, w, fused=fused_loss)
    loss.backward()
    grads = [p.grad.detach().clone() for p in net.parameters()]
    opt.step()
    return net, float(loss), grads


@pytest.mark.parametrize("fused_loss", [True, False])
def test_network_trains_one_step(fused_loss):
    before = [p.detach().clone() for p in _tiny_net(True).parameters()]
    net, loss, grads = _train_step(fused_loss)
    assert np.isfinite(loss) and loss > 0
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert all(float(g.abs().max()) > 0 for g in grads), [n for (n, _), g in zip(net.named_parameters(), grads) if float(g.abs().max()) == 0]
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))


def test_two_runs_from_one_seed_agree_bit_for_bit():
    _, loss_a, grads_a = _train_step(True)
    net_b, loss_b, grads_b = _train_step(True)
    assert loss_a == loss_b and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))


def test_evaluator_against_the_numpy_yardstick():
    from samplenet_amd import SegmentationEvaluator

    net = _tiny_net(True).eval()
    xyz, feats, labels = _tiny_batch(B=9, N=64, seed=3)
    labels[4] = -1                                   # one cloud entirely ignored
    labels[labels == 4] = 0                          # part 4 is labelled nowhere ...
    parts = {0: (0, 1), 1: (2, 3), 2: (4,), 3: (0, 1, 2, 3, 4)}
    cats = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 0], device="cuda")
    w = np.linspace(0.5, 2.0, 5).astype(np.float32)
    cuts = (0, 4, 7, 9)                              # batches of 4, 3 and 2 clouds
    ev = SegmentationEvaluator(net, 5, torch.from_numpy(w).cuda(), parts)
    net.train()                                      # add() must hand the network back in the mode it came in
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # add() must not synchronise
    try:
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ev.add(xyz[lo:hi], feats[lo:hi], labels[lo:hi], cats[lo:hi])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert net.training
    net.eval()
    res = ev.result()
    # the yardstick on the same logits
    lab_np, preds, batch_means, bound_num, den_sum = labels.cpu().numpy(), [], [], 0.0, 0.0
    with torch.no_grad():
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            lg = net(xyz[lo:hi], feats[lo:hi]).transpose(1, 2).contiguous().cpu().numpy().reshape(-1, 5)
            T = R.terms(lg, lab_np[lo:hi].reshape(-1), 64, w)
            preds.append(np.argmax(lg, axis=1).reshape(hi - lo, 64))
            batch_means.append(T["means"])
            # what a batch's numerator means[0] means[2] may be off by: the mean's bound and the weight sum's, each times the other
            b = R.bound_means(T)
            bound_num += b[0] * T["means"][2] + b[2] * abs(T["means"][0]) + 4 * R.U * abs(T["means"][0]) * T["means"][2]
            den_sum += T["means"][2]
            assert np.array_equal(res["cloud_counts"][lo:hi], T["cloud_counts"])
    ref = R.aggregates_loop(np.concatenate(preds), lab_np, 5, batch_means, cats.cpu().numpy(), parts)
    assert res["cloud_counts"].shape == (9, 5, 3) and res["cloud_counts"].dtype == np.int64 and not res["cloud_counts"][4].any()
    for k in ("class_labelled", "class_predicted", "class_correct"):
        assert np.array_equal(res[k], ref[k]), k
    for k in ("total_valid", "overall_accuracy", "mean_class_accuracy", "miou", "instance_miou", "category_miou"):
        assert res[k] == pytest.approx(ref[k], rel=1e-14, abs=0), k  # integer-derived: the same divisions in fp64
    assert np.allclose(res["cloud_iou"], ref["cloud_iou"], rtol=1e-14, atol=0)
    assert res["cloud_iou"][4] == 1.0                # every part of the ignored cloud is absent from labels and predictions
    l4, p4 = res["cloud_counts"][[2, 6], 4, 0], res["cloud_counts"][[2, 6], 4, 1]
    assert not l4.any() and np.array_equal(res["cloud_iou"][[2, 6]], np.where(p4 > 0, 0.0, 1.0))  # ... so it scores 1 unless predicted
    # the loss: the sum of the numerators' bounds over the sum of the weights (the denominators' error is inside bound_num)
    # and the batches' weight sums, each off by at most the longest chain's gamma (4 x 64 rows: the same chain for every batch)
    rel_den = R._g(R.sum_chain(4 * 64, 5))
    err = abs(res["mean_loss"] - ref["mean_loss"])
    bound = 1.01 * (bound_num / den_sum + (rel_den + 3 * R.U) * abs(ref["mean_loss"]))
    print("SEG_ERR evaluator mean_loss observed %.3e  bound %.3e  ratio %.3f" % (err, bound, err / bound))
    assert err <= bound

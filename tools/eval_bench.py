"""What the classification / reconstruction evaluators buy and what the fused classification terms cost.  Recorded, not gated.

    python tools/eval_bench.py > profiles/eval/eval_bench.txt

Shape: 256 items as batches of B = 32 clouds of N = 1024 points sampled to M = 64 (group size 7), random weights.
Part 1  ClassificationEvaluator (SampleNet inference branch -> matched cloud -> PointNetCls -> sn_classification_terms_forward, one
        result() at the end) beside the reference's pattern on the same networks (classification/evaluate_samplenet.py:182-258): the
        sampler with its host matching (idx.cpu(), numpy nn_matching), np.unique of the indices per item, the classifier, the loss'
        .item() and the logits' .cpu() argmax per batch.  Items per second, best of 3, the two routes alternated.
Part 2  ReconstructionEvaluator (chamfer, with the reference loss) beside the same pattern for reconstruction
        (reconstruction/sampler/evaluate_samplenet.py:88-152): host matching, the autoencoder per batch, get_loss_ae_per_pc's loop --
        the loss of ONE cloud and an .item() per item -- for the sampled and for the complete clouds.
Part 3  the captured classification step of tools/cls_bench.py (classification SampleNet, frozen PointNetCls, classification_loss +
        simplification + projection) with fused=True beside fused=False: ms per step (host clock around 200 replays ending in a
        synchronise, best of 3, alternated).  Launches per replay are NOT counted by this tool: a torch.profiler pass over the two
        replays ended in a segmentation fault of the host process while the profiler collected its trace, so the pass was taken
        out; the autograd nodes of the cross-entropy term on either route are printed instead.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, M, K, ITEMS, CLASSES = 32, 1024, 64, 7, 256, 40


def sync_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def networks():
    from samplenet_amd import PointNetAE, PointNetCls, SampleNet

    torch.manual_seed(0)
    net = SampleNet(M, 128, group_size=K, input_shape="bnc", output_shape="bnc", last_fc_batchnorm=True, min_sigma=0.0).cuda().eval()
    cls = PointNetCls(num_classes=CLASSES).cuda().eval().requires_grad_(False)
    with torch.no_grad():  # (transforms that differ from the identity, as a trained network's)
        cls.transform_net1.transform.weight.normal_(0, 0.005)
        cls.transform_net2.transform.weight.normal_(0, 0.002)
    ae = PointNetAE(n_pc_points=N).cuda().eval().requires_grad_(False)
    return net, cls, ae


def host_sample(net, x):
    """the reference's sampling step: the network, then the matching and the unique count on the host"""
    from samplenet_amd import ops

    net.device_matching = False
    try:
        simp, match = net(x)
    finally:
        net.device_matching = True
    idx = ops.knn(1, x, simp, ops.BNC, ops.BNC, return_dist=False)[0].view(x.shape[0], -1).cpu().numpy()
    return match, sum(np.size(np.unique(r)) for r in idx)


def report(name, ref_name, fast, slow):
    ta, tb = [], []
    for _ in range(3):  # alternated
        ta.append(sync_ms(fast, 3))
        tb.append(sync_ms(slow, 1))
    print("  %-44s %8.2f ms   %9.0f items / s   (runs: %s)" % (name, min(ta), ITEMS / min(ta) * 1e3, " ".join("%.2f" % t for t in ta)))
    print("  %-44s %8.2f ms   %9.0f items / s   (runs: %s)" % (ref_name, min(tb), ITEMS / min(tb) * 1e3, " ".join("%.2f" % t for t in tb)))
    print("  ratio                                        %.1f x" % (min(tb) / min(ta)))


def part1(net, cls, xs, labs):
    from samplenet_amd import ClassificationEvaluator, classification_loss

    print("Part 1 -- classification: %d items, batches of %d, %d -> %d points, PointNetCls (%d classes)" % (ITEMS, B, N, M, CLASSES))

    def device():
        ev = ClassificationEvaluator(cls, net)
        for x, lab in zip(xs, labs):
            ev.add(x, lab)
        return ev.result()

    def pattern():
        correct, loss_sum, unique = 0, 0.0, 0
        with torch.no_grad():
            for x, lab in zip(xs, labs):
                match, nu = host_sample(net, x)
                unique += nu
                logits, ep = cls(match)
                loss_sum += classification_loss(logits, lab, ep).item() * x.shape[0]
                correct += int(np.sum(np.argmax(logits.cpu().numpy(), 1) == lab.cpu().numpy()))
        return correct / ITEMS, loss_sum / ITEMS, unique / ITEMS

    ra, rb = device(), pattern()
    print("  the two routes: accuracy %.6f / %.6f, mean loss %.7f / %.7f, mean unique %.4f / %.4f"
          % (ra["accuracy"], rb[0], ra["mean_loss"], rb[1], ra["mean_unique"], rb[2]))
    report("ClassificationEvaluator, batches of %d" % B, "host matching, .cpu() per batch", device, pattern)


def part2(net, ae, xs):
    from samplenet_amd import ReconstructionEvaluator, reconstruction_loss

    print("Part 2 -- reconstruction: %d items, batches of %d, %d -> %d points, PointNetAE (%d points), Chamfer, with the reference loss"
          % (ITEMS, B, N, M, N))

    def device():
        ev = ReconstructionEvaluator(ae, net, loss="chamfer", with_reference=True)
        for x in xs:
            ev.add(x)
        return ev.result()

    def pattern():
        loss, ref = [], []
        with torch.no_grad():
            for x in xs:
                match, _nu = host_sample(net, x)
                rec, rec_full = ae(match), ae(x)
                for i in range(x.shape[0]):  # get_loss_ae_per_pc: one cloud at a time
                    loss.append(reconstruction_loss(rec[i:i + 1], x[i:i + 1]).item())
                    ref.append(reconstruction_loss(rec_full[i:i + 1], x[i:i + 1]).item())
        return np.array(loss), np.array(ref)

    ra, rb = device(), pattern()
    print("  largest difference of the per-item values between the two routes: loss %.3e (of %.3e), reference loss %.3e"
          % (np.abs(ra["losses"] - rb[0]).max(), ra["losses"].mean(), np.abs(ra["reference_losses"] - rb[1]).max()))
    report("ReconstructionEvaluator, batches of %d" % B, "host matching, batch-1 loss + .item()", device, pattern)


def part3(cls):
    from samplenet_amd import SampleNet, classification_loss
    from samplenet_amd.engine import SamplerTrainStep

    print("Part 3 -- the captured classification step (B = %d, %d -> %d, K = %d, frozen PointNetCls + classification_loss)" % (B, N, M, K))
    x = torch.rand(B, N, 3, device="cuda") - 0.5
    lab = torch.randint(0, CLASSES, (B,), device="cuda")
    steps = {}
    for name, fused in (("fused=False (F.cross_entropy)", False), ("fused=True (sn_classification_terms)", True)):
        def task(proj, fused=fused):
            y, ep = cls(proj)
            return classification_loss(y, lab, ep, fused=fused)

        torch.manual_seed(1)
        net = SampleNet(M, 128, group_size=K, input_shape="bnc", output_shape="bnc", last_fc_batchnorm=True, min_sigma=0.0).cuda().train()
        steps[name] = SamplerTrainStep(net, x, alpha=30.0, lmbda=1.0, task_loss=task, use_graph=True)
    for s in steps.values():
        sync_ms(lambda: s(x), 20)
    times = {n: [] for n in steps}
    for _ in range(3):  # alternated
        for n, s in steps.items():
            times[n].append(sync_ms(lambda: s(x), 200))
    for n in steps:
        print("  %-38s %.4f ms per step (runs: %s)" % (n, min(times[n]), " ".join("%.4f" % t for t in times[n])))
    names = list(steps)
    print("  difference %+.2f us" % ((min(times[names[1]]) - min(times[names[0]])) * 1e3))
    # what differs between the two replays: the autograd nodes of the cross-entropy term (no profiler pass: one over these replays
    # crashed in its trace collection)
    logits = torch.randn(B, CLASSES, device="cuda", requires_grad=True)
    for name, fused in (("fused=False", False), ("fused=True", True)):
        loss = classification_loss(logits, lab, {}, fused=fused)
        nodes, seen, stack = [], set(), [loss.grad_fn]
        while stack:
            f = stack.pop()
            if f is None or f in seen:
                continue
            seen.add(f)
            nodes.append(type(f).__name__)
            stack += [g for g, _ in f.next_functions]
        print("  %-12s autograd nodes of the cross-entropy term: %s" % (name, ", ".join(sorted(nodes))))
    print("  (ClassificationMeanLossFunctionBackward: sn_classification_terms_forward and _backward, one launch each)")


def main():
    print("device: %s, HIP %s, torch %s" % (torch.cuda.get_device_name(0), torch.version.hip, torch.__version__))
    g = torch.Generator().manual_seed(0)
    xs = [(torch.rand(B, N, 3, generator=g) - 0.5).cuda() for _ in range(ITEMS // B)]
    labs = [torch.randint(0, CLASSES, (B,), generator=g).cuda() for _ in range(ITEMS // B)]
    net, cls, ae = networks()
    part1(net, cls, xs, labs)
    part2(net, ae, xs)
    part3(cls)


if __name__ == "__main__":
    main()

"""Timings of the PointNet classifier (samplenet_amd/classifier.py) and its per-cloud transform kernels, hipEvents around graph replays.

    python tools/cls_bench.py [--replays 200] [--warmup 20] [--only-step]

(a) sn_cloud_transform_forward / _backward (dX + dT) beside torch.bmm on the same device at (B, N) = (32, 64), (32, 1024), (512, 64),
    (2048, 64) for K = 3 and K = 64; achieved bytes/s of the forward (X read, Y written).
(b) the frozen eval-mode classifier, forward + gradient to the input cloud, at B = 32 with 64 and 1024 points, its FC heads as the
    sn_skinny_linear composition (shipped) and on the layer walk (classifier.SKINNY_HEADS = False).
(c) the whole classification sampler step (classification SampleNet, K = 7, frozen PointNetCls, classification_loss + 30 simplification
    + projection, backward into the sampler), eager and captured (engine.SamplerTrainStep).
--only-step: (c) captured only, a few replays -- the run that rocprofv3 --kernel-trace --stats wraps.
Every figure is a median over the timed replays after untimed warm-up ones; min and max are printed beside it.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenet_amd import PointNetCls, SampleNet, classification_loss, classifier  # noqa: E402
from samplenet_amd._lib import check, lib, ptr, stream_of  # noqa: E402
from samplenet_amd.engine import SamplerTrainStep  # noqa: E402


def timed(fn, replays, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        keep = fn()
    g.keep = keep
    return g


def transforms(args):
    for K in (64, 3):
        for B, N in ((32, 64), (32, 1024), (512, 64), (2048, 64)):
            x, dy = torch.randn(B, N, K, device="cuda"), torch.randn(B, N, K, device="cuda")
            t = torch.randn(B, K, K, device="cuda")
            y, dx, dt = torch.empty_like(x), torch.empty_like(x), torch.empty_like(t)

            def fwd():
                check(lib.sn_cloud_transform_forward(B, N, K, ptr(x), ptr(t), ptr(y), stream_of(x)))

            def bwd():
                check(lib.sn_cloud_transform_backward(B, N, K, ptr(x), ptr(t), ptr(dy), ptr(dx), ptr(dt), stream_of(x)))

            res = []
            for fn in (fwd, lambda: torch.bmm(x, t), bwd, lambda: (torch.bmm(dy, t.transpose(1, 2)), torch.bmm(x.transpose(1, 2), dy))):
                res.append(timed(graphed(fn).replay, args.replays, args.warmup))
            print("transform K = %-2d B = %-4d N = %-4d  forward %7.2f us (min %.2f)  torch.bmm %7.2f us (min %.2f)  %5.2f TB/s |  "
                  "backward dX + dT %7.2f us (min %.2f)  2 x torch.bmm %7.2f us (min %.2f)"
                  % (K, B, N, res[0][0], res[0][1], res[1][0], res[1][1], 2 * x.numel() * 4 / (res[0][0] * 1e-6) / 1e12,
                     res[2][0], res[2][1], res[3][0], res[3][1]))


def frozen_classifier(args, cls):
    for N in (64, 1024):
        x = (torch.rand(32, N, 3, device="cuda") - 0.5).requires_grad_(True)
        w = torch.randn(32, 40, device="cuda")
        for skinny in (True, False):
            classifier.SKINNY_HEADS = skinny
            med, lo, hi = timed(graphed(lambda: torch.autograd.grad(cls(x)[0], x, w)[0]).replay, args.replays, args.warmup)
            print("frozen PointNetCls (eval), forward + input gradient, B = 32, N = %-4d heads: %-34s median %8.1f us (min %.1f, max %.1f)"
                  % (N, "sn_skinny_linear composition" if skinny else "layer walk (sn_linear_forward/_dgrad)", med, lo, hi))
        classifier.SKINNY_HEADS = True


def step(args, cls, modes):
    B = 32
    x = torch.rand(B, 1024, 3, device="cuda") - 0.5
    lab = torch.randint(0, 40, (B,), device="cuda")

    def task(proj):
        y, ep = cls(proj)
        return classification_loss(y, lab, ep)

    for use_graph in modes:
        torch.manual_seed(1)
        net = SampleNet(64, 128, group_size=7, input_shape="bnc", output_shape="bnc", last_fc_batchnorm=True, min_sigma=0.0).cuda().train()
        st = SamplerTrainStep(net, x, alpha=30.0, lmbda=1.0, task_loss=task, use_graph=use_graph)
        med, lo, hi = timed(lambda: st(x), max(20, args.replays // 4), 5)
        print("classification step, B = %d, 1024 -> 64, K = 7, frozen PointNetCls (eval) + classification_loss  %-8s median %8.1f us "
              "(min %.1f, max %.1f)  %.0f clouds/s" % (B, "captured" if use_graph else "eager", med, lo, hi, B / (med * 1e-6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-step", action="store_true")
    args = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
    torch.manual_seed(0)
    cls = PointNetCls().cuda().eval().requires_grad_(False)
    with torch.no_grad():  # (transforms that differ from the identity, as a trained network's)
        cls.transform_net1.transform.weight.normal_(0, 0.005)
        cls.transform_net2.transform.weight.normal_(0, 0.002)
    if args.only_step:
        step(args, cls, (True,))
        return
    transforms(args)
    frozen_classifier(args, cls)
    step(args, cls, (False, True))


if __name__ == "__main__":
    main()

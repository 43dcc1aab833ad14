"""Timings of the reconstruction autoencoder (samplenet_amd/autoencoder.py), hipEvents around graph replays.

    python tools/ae_bench.py [--replays 200] [--warmup 20] [--skip-step]

(a) decoder forward + data backward at B = 50 (128 -> 256 -> 256 -> 6144) as shipped: the per-layer sn_skinny_linear composition,
    captured into a graph, median of the replays; achieved bytes/s on W3 (read once forward, once backward).
(b) the whole reconstruction step (config3 sampler at B = 50, N = 2048, M = 64, K = 16 + frozen autoencoder + Chamfer | EMD
    + simplification + sigma, backward into the sampler), eager and captured (engine.SamplerTrainStep), with the figures of the two
    unconnected legs of the last committed BENCH_r06.json beside them.
Every figure is a median over the timed replays after untimed warm-up ones; min and max are printed beside it.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenet_amd import PointNetAE, SampleNet, reconstruction_loss  # noqa: E402
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


def decoder_graph(ae, B):
    z = torch.randn(B, ae.bottleneck_size, device="cuda").requires_grad_(True)
    w = torch.randn(B, ae.n_pc_points, 3, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            torch.autograd.grad(ae.decode(z), z, w)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gz = torch.autograd.grad(ae.decode(z), z, w)[0]
    return g, gz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
    torch.manual_seed(0)
    ae = PointNetAE().cuda().eval()
    for p in ae.parameters():
        p.requires_grad_(False)
    B = 50
    w3 = ae.fc3.weight.numel() * 4
    g, _ = decoder_graph(ae, B)
    med, lo, hi = timed(g.replay, args.replays, args.warmup)
    print("decoder fwd + data bwd, B = %d, sn_skinny_linear composition (6 launches): median %7.2f us  (min %.2f, max %.2f)   "
          "W3 traffic %.2f TB/s of 6.29 achievable" % (B, med, lo, hi, 2 * w3 / (med * 1e-6) / 1e12))
    if args.skip_step:
        return
    recon = dict(conv_widths=(64, 128, 128, 256), fc_widths=(256, 256), fc_batchnorm=False, temperature_floor=1e-2, min_sigma=0)
    for loss in ("chamfer", "emd"):
        x = torch.rand(B, 2048, 3, device="cuda") - 0.5
        for use_graph in (False, True):
            torch.manual_seed(1)
            net = SampleNet(64, 128, group_size=16, initial_temperature=0.5, input_shape="bnc", output_shape="bnc", **recon).cuda().train()
            step = SamplerTrainStep(net, x, task_loss=lambda proj: reconstruction_loss(ae(proj), x, loss), use_graph=use_graph)
            med, lo, hi = timed(lambda: step(x), max(20, args.replays // 4), 5)
            print("reconstruction step, B = %d, N = 2048, M = 64, K = 16, frozen AE (eval) + %-7s %-8s median %8.1f us (min %.1f, max %.1f)  "
                  "%.0f clouds/s" % (B, loss, "captured" if use_graph else "eager", med, lo, hi, B / (med * 1e-6)))


    print("context, BENCH_r06.json (two unconnected legs): config3_sampler 0.691 ms eager / 0.702 ms captured; config3_emd emd_loss 2.069 ms")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The feature-propagation level on the GPU (samplenet_amd/csrc/feature_rows.hip, samplenet_amd/feature_propagation.py, the pointnet2
stand-in's PointnetFPModule): HIP-event timing through the Python surface at the four layer shapes of DESIGN.md section 4.15's table,
batch 32, training mode, the columns of a row ALTERNATED inside one run (tools/sa_bench.py's timer), median and spread printed.

    module     forward and forward + backward, fused=True against the default route (torch weights, three_interpolate, cat, torch
               Conv2d / BatchNorm2d / ReLU)
    assembly   ops.interp_rows forward against torch weights + three_interpolate + cat + transpose (both behind one three_nn call
               made outside the timed region)
    backward   sn_interp_rows_backward against sn_weighted_gather_backward_inverted (channel-major), on one prebuilt inversion
    top        sn_bn_relu_backward_stats against sn_bn_relu_backward + the two torch sums, at the level's (rows, top width)

Output: profiles/fp_rows/fp_bench.txt (--out PATH to write elsewhere).

    python tools/fpm_bench.py [--calls 12] [--out PATH]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sa_bench import alternated, fmt, ratio_line  # noqa: E402
from samplenet_amd import ops  # noqa: E402
from samplenet_amd._lib import check, lib, ptr  # noqa: E402
from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM  # noqa: E402

B = 32
LEVELS = [  # (m, n, c2, c1, the MLP's widths behind c2 + c1: PointNet++ segmentation decoders as recalled)
    (16, 64, 512, 256, [256, 256]),
    (64, 256, 256, 128, [256, 256]),
    (256, 1024, 256, 64, [256, 128]),
    (1024, 4096, 128, 6, [128, 128, 128]),
]


def level_rows(lines, calls):
    st = torch.cuda.current_stream().cuda_stream
    for m, n, c2, c1, widths in LEVELS:
        torch.manual_seed(0)
        mod = PM.PointnetFPModule([c2 + c1] + widths).cuda().train()
        unknown, known = torch.rand(B, n, 3, device="cuda"), torch.rand(B, m, 3, device="cuda")
        kf = torch.randn(B, c2, m, device="cuda", requires_grad=True)
        sf = torch.randn(B, c1, n, device="cuda", requires_grad=True)
        lines.append("# %d x %d -> %d, c2 %d, c1 %d, mlp %s" % (B, m, n, c2, c1, [c2 + c1] + widths))
        with torch.no_grad():
            a, b_ = mod(unknown, known, sf, kf, fused=True), mod(unknown, known, sf, kf, fused=False)
        lines.append("#   fused against default, forward values: worst difference %.3g (of %.3g)" % (float((a - b_).abs().max()), float(b_.abs().max())))

        def fwd(fused):
            with torch.no_grad():
                mod(unknown, known, sf, kf, fused=fused)

        def step(fused):
            mod.zero_grad(set_to_none=True)
            kf.grad = sf.grad = None
            mod(unknown, known, sf, kf, fused=fused).sum().backward()

        res = alternated({"fused": lambda: fwd(True), "default": lambda: fwd(False)}, calls)
        lines.append("module forward   ms  " + fmt(res, ("fused", "default")))
        lines.append(ratio_line(res, "fused", "default"))
        res = alternated({"fused": lambda: step(True), "default": lambda: step(False)}, calls)
        lines.append("module fwd+bwd   ms  " + fmt(res, ("fused", "default")))
        lines.append(ratio_line(res, "fused", "default"))

        # the assembly alone, behind one query
        dist2, idx = ops.three_nn(unknown, known, return_dist2=True)
        dist = dist2.sqrt()
        kr, sr = kf.detach().transpose(1, 2).contiguous(), sf.detach().transpose(1, 2).contiguous()
        kfd, sfd = kf.detach(), sf.detach()

        def rows_fwd():
            ops.interp_rows(kr, sr, idx, dist2)

        def torch_fwd():
            r = 1.0 / (dist + 1e-8)
            w = r / torch.sum(r, dim=2, keepdim=True)
            torch.cat([ops.three_interpolate(kfd, idx, w), sfd], dim=1).transpose(1, 2).contiguous()

        res = alternated({"rows": rows_fwd, "torch": torch_fwd}, calls)
        lines.append("assembly forward ms  " + fmt(res, ("rows", "torch")))
        lines.append(ratio_line(res, "rows", "torch"))

        # the interpolation's gradient alone, on one prebuilt inversion
        start, order = ops.gather_invert(idx, m)
        w = torch.rand(B, n, 3, device="cuda")
        g_rows = torch.randn(B, n, c2 + c1, device="cuda")
        g_cm = g_rows[:, :, :c2].transpose(1, 2).contiguous()
        gk, gx = torch.empty(B, m, c2, device="cuda"), torch.empty(B, c2, m, device="cuda")

        def rows_bwd():
            check(lib.sn_interp_rows_backward(B, n, m, c2, c1, ptr(w), ptr(g_rows), ptr(start), ptr(order), ptr(gk), st))

        def cm_bwd():
            check(lib.sn_weighted_gather_backward_inverted(B, c2, m, n, 3, ptr(w), ptr(g_cm), ptr(start), ptr(order), ptr(gx), st))

        rows_bwd(), cm_bwd()
        lines.append("#   rows backward == channel-major inverted walk transposed: %s" % torch.equal(gk, gx.transpose(1, 2)))
        res = alternated({"rows": rows_bwd, "channel-major": cm_bwd}, calls)
        lines.append("interp backward  ms  " + fmt(res, ("rows", "channel-major")))
        lines.append(ratio_line(res, "rows", "channel-major"))

        # the top activation's backward with the BatchNorm sums
        R, C = B * n, widths[-1]
        z, g = torch.randn(R, C, device="cuda"), torch.randn(R, C, device="cuda")
        coef = torch.stack([torch.randn(C), torch.randn(C) * 0.3, torch.randn(C) * 0.1, torch.rand(C) + 0.5]).cuda().contiguous()
        dy = torch.empty(R, C, device="cuda")
        stats = torch.empty(lib.sn_bn_relu_stats_blocks(R), 2, C, device="cuda")

        def one_launch():
            check(lib.sn_bn_relu_backward_stats(R, C, ptr(z), ptr(coef), ptr(g), ptr(dy), ptr(stats), st))

        def sibling_and_sums():
            check(lib.sn_bn_relu_backward(R, C, ptr(z), ptr(coef), ptr(g), 0, ptr(dy), st))
            torch.stack((dy.sum(0), (dy * z).sum(0))).view(1, 2, C).contiguous()

        res = alternated({"stats": one_launch, "sibling+torch": sibling_and_sums}, calls)
        lines.append("top backward     ms  " + fmt(res, ("stats", "sibling+torch")) + "   (R %d, C %d)" % (R, C))
        lines.append(ratio_line(res, "stats", "sibling+torch"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp_rows", "fp_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.calls >= 10, "fpm_bench.py measures on a GPU, at least 10 calls per column"
    lines = ["# tools/fpm_bench.py on %s; HIP events; per column: median ms (min .. max) over %d calls, the columns of a row alternated"
             % (torch.cuda.get_device_name(0), args.calls)]
    level_rows(lines, args.calls)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

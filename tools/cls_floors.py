"""Measures the floors tests/test_gpu_classifier.py uses: the worst error of torch's own fp32 evaluation against fp64 over 16 seeds per
shape -- torch.bmm for the per-cloud transforms, the torch restatement of the classifier (tests/torch_cls.py) for the gradient handed
to the input cloud.  The library's kernels take no part (PointNetCls only supplies the parameter container).

    python tools/cls_floors.py > profiles/cls/floors.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_classifier as T  # noqa: E402

SEEDS = 16


def transform_floor(K):
    worst = {}
    for B, N in ((32, 64), (32, 1024), (3, 100), (1, 2500)):
        w = 0.0
        for seed in range(SEEDS):
            g = torch.Generator(device="cuda").manual_seed(1000 + seed * 31 + B + N + K)
            x = torch.rand(B, N, K, device="cuda", generator=g) - 0.5
            t = torch.randn(B, K, K, device="cuda", generator=g)
            dy = torch.randn(B, N, K, device="cuda", generator=g)
            ref = (torch.bmm(x, t), torch.bmm(dy, t.transpose(1, 2)), torch.bmm(x.transpose(1, 2), dy))
            for r, want in zip(ref, T._bmm64(x, t, dy)):
                w = max(w, float((r.double() - want).abs().max()) / float(want.abs().max()))
        worst[(B, N)] = w
    return worst


def in_grad_floor(mode, basic=False):
    worst = {}
    for B, N in ((32, 64), (32, 1024), (3, 64), (5, 100), (50, 64)):
        w = 0.0
        for seed in range(SEEDS):
            net = T._make(5000 + seed * 101 + B * 7 + N, mode, basic=basic, dropout=0.0)
            r32, r64 = T._refs(net, mode, basic, 0.0)
            x = T._clouds(B, N)
            wt = torch.randn(B, 40, device="cuda")
            x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
            (r32(x32)[0] * wt).sum().backward()
            (r64(x64)[0] * wt.double()).sum().backward()
            w = max(w, float((x32.grad.double() - x64.grad).norm()) / float(x64.grad.norm()))
        worst[(B, N)] = w
    return worst


if __name__ == "__main__":
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| %d seeds per shape" % SEEDS)
    for K in (3, 64):
        w = transform_floor(K)
        print("    transform K = %-2d  " % K + "  ".join("(%d,%d) %.2e" % (*k, v) for k, v in w.items()) + "   -> floor %.2e" % max(w.values()))
    for mode in ("eval", "train"):
        w = in_grad_floor(mode)
        print("    input gradient, %-5s  " % mode + "  ".join("(%d,%d) %.2e" % (*k, v) for k, v in w.items()) + "   -> floor %.2e" % max(w.values()))
    w = in_grad_floor("eval", basic=True)
    print("    input gradient, basic model, eval  " + "  ".join("(%d,%d) %.2e" % (*k, v) for k, v in w.items()) + "   -> floor %.2e" % max(w.values()))

#!/usr/bin/env python3
"""The per-point segmentation terms on the GPU (samplenet_amd/csrc/seg_terms.hip, ops.segmentation_terms, segmentation_loss,
SegmentationEvaluator, PointNet2SemSegSSG): HIP-event timing through the Python surface, the columns of a row ALTERNATED inside one
run (tools/sa_bench.py's timer), median and spread of the calls printed.

    terms      forward, and forward + backward of the mean loss, at (32 x 4096, 13) and (32 x 2048, 50):
                 seg     ops.segmentation_terms / ops.segmentation_mean_loss
                 torch   F.cross_entropy(weight=) + argmax + the per-cloud per-class bincounts (labelled, predicted, correct)
                 cls     ops.classification_terms / classification_mean_loss on the flattened rows (no weights, no counts: the
                         wave-per-row mapping on this many rows)
    evaluator  SegmentationEvaluator.add x 3 + result() beside the host pattern (argmax + .cpu() + numpy bincounts per batch), on a
               network that returns stored logits (the terms and the transfers alone)
    step       one training step of the default PointNet2SemSegSSG at 32 x 4096 (13 classes, xyz + 6 input channels), Adam, with
               segmentation_loss(fused=True) and (fused=False)

Output: profiles/seg/seg_bench.txt (--out PATH to write elsewhere).

    python tools/seg_bench.py [--calls 12] [--out PATH] [--no-step]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sa_bench import alternated, fmt, ratio_line  # noqa: E402
from samplenet_amd import SegmentationEvaluator, ops, optim, segmentation_loss  # noqa: E402
from samplenet_amd.compat.pointnet2.models import PointNet2SemSegSSG  # noqa: E402

SHAPES = ((32, 4096, 13), (32, 2048, 50))


def torch_terms(rows, labels, w):
    """the composition a user of the stand-in writes today: -> loss, pred, counts (B,C,3)"""
    B, N, C = rows.shape
    loss = F.cross_entropy(rows.transpose(1, 2), labels, weight=w, ignore_index=-100)
    pred = rows.argmax(dim=2)
    valid = labels >= 0
    base = (torch.arange(B, device=rows.device) * C).view(B, 1)
    lab = (labels.clamp_min(0) + base)[valid]
    prd = (pred + base)[valid]
    hit = lab[lab == prd]
    counts = torch.stack([torch.bincount(t, minlength=B * C) for t in (lab, prd, hit)], dim=1).view(B, C, 3)
    return loss, pred, counts


def terms_rows(lines, calls):
    for B, N, C in SHAPES:
        torch.manual_seed(0)
        rows = torch.randn(B, N, C, device="cuda") * 3
        labels = torch.randint(0, C, (B, N), device="cuda")
        labels[torch.rand(B, N, device="cuda") < 0.1] = -100
        w = torch.rand(C, device="cuda") + 0.5
        flat, flat_labels = rows.view(B * N, C), labels.clamp_min(0).view(B * N)
        lines.append("# %d x %d points, %d classes" % (B, N, C))
        _ce, pred, counts, means = ops.segmentation_terms(rows, labels, w)
        tl, tp, tc = torch_terms(rows, labels, w)
        lines.append("#   seg against torch: loss %.7g / %.7g, pred equal %s, counts equal %s"
                     % (float(means[0]), float(tl), torch.equal(pred.long(), tp), torch.equal(counts.long(), tc)))

        def fwd_seg():
            with torch.no_grad():
                ops.segmentation_terms(rows, labels, w)

        def fwd_torch():
            with torch.no_grad():
                torch_terms(rows, labels, w)

        def fwd_cls():
            with torch.no_grad():
                ops.classification_terms(flat, flat_labels)

        res = alternated({"seg": fwd_seg, "torch": fwd_torch, "cls": fwd_cls}, calls)
        lines.append("terms forward    ms  " + fmt(res, ("seg", "torch", "cls")))
        lines.append(ratio_line(res, "seg", "torch"))
        lines.append(ratio_line(res, "seg", "cls"))
        leaf = rows.clone().requires_grad_(True)
        leaf2 = flat.clone().requires_grad_(True)

        def step_seg():
            leaf.grad = None
            ops.segmentation_mean_loss(leaf, labels, w).backward()

        def step_torch():
            leaf.grad = None
            F.cross_entropy(leaf.transpose(1, 2), labels, weight=w, ignore_index=-100).backward()

        def step_cls():
            leaf2.grad = None
            ops.classification_mean_loss(leaf2, flat_labels).backward()

        res = alternated({"seg": step_seg, "torch": step_torch, "cls": step_cls}, calls)
        lines.append("loss fwd+bwd     ms  " + fmt(res, ("seg", "torch", "cls")))
        lines.append(ratio_line(res, "seg", "torch"))
        lines.append(ratio_line(res, "seg", "cls"))


class _Stored(torch.nn.Module):
    """a 'network' that returns stored logits: the evaluator's own work alone"""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, xyz, features=None):
        return self.logits.transpose(1, 2)


def evaluator_rows(lines, calls):
    for B, N, C in SHAPES:
        torch.manual_seed(0)
        rows = torch.randn(B, N, C, device="cuda") * 3
        labels = torch.randint(0, C, (B, N), device="cuda")
        xyz = torch.rand(B, N, 3, device="cuda")
        ev = SegmentationEvaluator(_Stored(rows), C)

        def device():
            ev.reset()
            for _ in range(3):
                ev.add(xyz, None, labels)
            return ev.result()

        def host():
            tot = np.zeros((C, 3), dtype=np.int64)
            loss = 0.0
            for _ in range(3):
                with torch.no_grad():
                    loss += float(F.cross_entropy(rows.transpose(1, 2), labels))
                    p, l = rows.argmax(dim=2).cpu().numpy().reshape(-1), labels.cpu().numpy().reshape(-1)
                tot[:, 0] += np.bincount(l, minlength=C)
                tot[:, 1] += np.bincount(p, minlength=C)
                tot[:, 2] += np.bincount(l[p == l], minlength=C)
            return tot, loss / 3

        a, (b, _) = device(), host()
        lines.append("# evaluator, 3 batches of %d x %d, %d classes: counts equal the host pattern's %s"
                     % (B, N, C, np.array_equal(np.stack([a["class_labelled"], a["class_predicted"], a["class_correct"]], 1), b)))
        res = alternated({"device": device, "host": host}, calls)
        lines.append("evaluator        ms  " + fmt(res, ("device", "host")))
        lines.append(ratio_line(res, "device", "host"))


def step_rows(lines, calls):
    B, N, C = 32, 4096, 13
    torch.manual_seed(0)
    net = PointNet2SemSegSSG(C, input_channels=6).cuda().train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    xyz, feats = torch.rand(B, N, 3, device="cuda"), torch.randn(B, 6, N, device="cuda")
    labels = torch.randint(0, C, (B, N), device="cuda")
    w = torch.rand(C, device="cuda") + 0.5

    def step(fused):
        opt.zero_grad(set_to_none=True)
        segmentation_loss(net(xyz, feats), labels, w, fused=fused).backward()
        opt.step()

    lines.append("# one training step of PointNet2SemSegSSG(13, input_channels=6), %d x %d, Adam" % (B, N))
    res = alternated({"fused loss": lambda: step(True), "torch loss": lambda: step(False)}, calls)
    lines.append("training step    ms  " + fmt(res, ("fused loss", "torch loss")))
    lines.append(ratio_line(res, "fused loss", "torch loss"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg", "seg_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.calls >= 10, "seg_bench.py measures on a GPU, at least 10 calls per column"
    lines = ["# tools/seg_bench.py on %s; HIP events; per column: median ms (min .. max) over %d calls, the columns of a row alternated"
             % (torch.cuda.get_device_name(0), args.calls)]
    terms_rows(lines, args.calls)
    evaluator_rows(lines, args.calls)
    if not args.no_step:
        step_rows(lines, args.calls)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The three-NN query of a PointNet++ feature-propagation layer on the GPU (samplenet_amd/csrc/feature_propagate.hip): HIP-event
timing of ops.three_nn (sn_three_nn: a lane owns an unknown point) beside ops.knn(3) (sn_knn: a wave owns a query) and torch's
cdist + topk, and of PointnetFPModule's feature assembly (three_nn + weights + three_interpolate + cat) forward and
forward + backward beside the same assembly on ops.knn(3) and a torch-only one, at the feature-propagation stack of a PointNet++
segmentation network at the reference's batch of 32 (layer widths AS RECALLED).  All columns of a shape are measured in ONE call,
alternated round by round; the table gives each column's median over the rounds and its spread (max - min).  Reports whether the
routes agree on the indices.  Output: profiles/fp/fp_bench.txt (or --out).

    python tools/fp_bench.py [--rounds 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenet_amd import ops  # noqa: E402

SHAPES = [  # (b, m known, n unknown, c2, c1): layer widths as recalled
    (32, 16, 64, 512, 256),
    (32, 64, 256, 256, 128),
    (32, 256, 1024, 256, 64),
    (32, 1024, 4096, 128, 6),
]


def timed(fn, target_s=0.15):
    """mean ms per call: 3 warm-up calls, then enough calls for ~target_s"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(10, min(2000, int(target_s * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _assemble(dist, idx, unknown_feats, known_feats):
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
    return torch.cat([ops.three_interpolate(known_feats, idx, weight), unknown_feats], 1)


def nn_propagate(unknown, known, unknown_feats, known_feats):
    """PointnetFPModule.forward without the MLP: ops.three_nn + torch weight ops + ops.three_interpolate + torch.cat"""
    dist, idx = ops.three_nn(unknown, known)
    return _assemble(dist, idx, unknown_feats, known_feats), idx


def knn_propagate(unknown, known, unknown_feats, known_feats):
    """the same on ops.knn(3), what a caller had before sn_three_nn"""
    idx, d2 = ops.knn(3, known, unknown, ref_layout=ops.BNC, query_layout=ops.BNC)
    return _assemble(torch.sqrt(d2), idx, unknown_feats, known_feats), idx


def torch_propagate(unknown, known, unknown_feats, known_feats):
    b, n, _ = unknown.shape
    c2 = known_feats.shape[1]
    dist, idx = torch.topk(torch.cdist(unknown, known), 3, dim=2, largest=False)
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
    f = torch.gather(known_feats, 2, idx.view(b, 1, n * 3).expand(b, c2, n * 3)).view(b, c2, n, 3)
    return torch.cat([(f * weight[:, None]).sum(-1), unknown_feats], 1), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fp", "fp_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fp_bench.py measures on a GPU"
    torch.manual_seed(0)
    lines = ["# tools/fp_bench.py on %s; HIP events, mean ms per call over >= 10 calls after 3 warm-up calls; %d rounds, the columns of a"
             % (torch.cuda.get_device_name(0), args.rounds),
             "# shape alternated inside every round; median over the rounds (max - min over the rounds)",
             "# shapes: the feature-propagation stack of a PointNet++ segmentation network at batch 32, layer widths AS RECALLED",
             "# assembly: query + torch weight ops + ops.three_interpolate + torch.cat (PointnetFPModule.forward without its MLP)",
             "%-44s %18s %18s %18s" % ("shape (b, m -> n, c2, c1)", "three_nn ms", "knn(3) ms", "torch ms")]
    for b, m, n, c2, c1 in SHAPES:
        unknown, known = torch.rand(b, n, 3, device="cuda") - 0.5, torch.rand(b, m, 3, device="cuda") - 0.5
        kf, uf = torch.randn(b, c2, m, device="cuda"), torch.randn(b, c1, n, device="cuda")
        g = torch.randn(b, c2 + c1, n, device="cuda")
        tag = "(%d, %d -> %d, %d, %d)" % (b, m, n, c2, c1)
        route = {"nn": nn_propagate, "knn": knn_propagate, "torch": torch_propagate}
        res = {name: fn(unknown, known, uf, kf) for name, fn in route.items()}
        lines.append("# %s  indices three_nn == knn(3): %s, == torch: %s; worst |three_nn - knn| %.3g, |three_nn - torch| %.3g"
                     % (tag, torch.equal(res["nn"][1], res["knn"][1]), torch.equal(res["nn"][1].long(), res["torch"][1]),
                        float((res["nn"][0] - res["knn"][0]).abs().max()), float((res["nn"][0] - res["torch"][0]).abs().max())))
        leaves = [kf.clone().requires_grad_(True), uf.clone().requires_grad_(True)]

        def step(name):
            for t in leaves:
                t.grad = None
            route[name](unknown, known, leaves[1], leaves[0])[0].backward(g)

        cols = {
            "q nn": lambda: ops.three_nn(unknown, known),
            "q knn": lambda: ops.knn(3, known, unknown, ref_layout=ops.BNC, query_layout=ops.BNC),
            "q torch": lambda: torch.topk(torch.cdist(unknown, known), 3, dim=2, largest=False),
            "f nn": lambda: nn_propagate(unknown, known, uf, kf), "f knn": lambda: knn_propagate(unknown, known, uf, kf),
            "f torch": lambda: torch_propagate(unknown, known, uf, kf),
            "fb nn": lambda: step("nn"), "fb knn": lambda: step("knn"), "fb torch": lambda: step("torch"),
        }
        times = {name: [] for name in cols}
        for _ in range(args.rounds):
            for name, fn in cols.items():
                times[name].append(timed(fn))

        def cell(name):
            t = times[name]
            return "%8.4f (%6.4f)" % (statistics.median(t), max(t) - min(t))

        lines.append("%-44s %18s %18s %18s" % ("query   " + tag, cell("q nn"), cell("q knn"), cell("q torch")))
        lines.append("%-44s %18s %18s %18s" % ("assembly forward", cell("f nn"), cell("f knn"), cell("f torch")))
        lines.append("%-44s %18s %18s %18s" % ("assembly fwd+bwd", cell("fb nn"), cell("fb knn"), cell("fb torch")))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The three-NN query of a PointNet++ feature-propagation layer on the GPU (samplenet_amd/csrc/feature_propagate.hip): HIP-event
timing of ops.three_nn (sn_three_nn: a lane owns an unknown point) beside ops.knn(3) (sn_knn: a wave owns a query) and torch's
cdist + topk, and of PointnetFPModule's feature assembly (three_nn + weights + three_interpolate + cat) forward and
forward + backward beside the same assembly on ops.knn(3) and a torch-only one, at the feature-propagation stack of a PointNet++
segmentation network at the reference's batch of 32 (layer widths AS RECALLED).  Then the interpolation's backward alone and
the assembly forward + backward on three routes of that backward: the inverted index (ops.three_interpolate: sn_gather_invert +
sn_weighted_gather_backward_inverted), the ordered route (WeightedGatherFunction: what ops.three_interpolate ran on before, and
its fallback now) and torch's gather / index_add; the inversion and the walk are also timed on their own.  All columns of a shape
are measured in ONE call, alternated round by round; the table gives each column's median over the rounds and its spread
(max - min).  Reports whether the routes agree on the indices and whether the two deterministic routes agree on every bit.
Output: profiles/fp/fp_bench.txt (or --out).

    python tools/fp_bench.py [--rounds 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenet_amd import ops  # noqa: E402
from samplenet_amd._lib import check, lib, ptr, stream_of  # noqa: E402

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


def _ordered_interpolate(features, idx, weight):
    """the route ops.three_interpolate had before the inverted index, and falls back to beyond sn_gather_invert_supported"""
    return ops.WeightedGatherFunction.apply(features, idx, weight)


def _torch_interpolate(features, idx, weight):
    b, n, _ = idx.shape
    c2 = features.shape[1]
    f = torch.gather(features, 2, idx.long().view(b, 1, n * 3).expand(b, c2, n * 3)).view(b, c2, n, 3)
    return (f * weight[:, None]).sum(-1)


def _assemble(dist, idx, unknown_feats, known_feats, interpolate=None):
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
    return torch.cat([(interpolate or ops.three_interpolate)(known_feats, idx, weight), unknown_feats], 1)


def nn_propagate(unknown, known, unknown_feats, known_feats):
    """PointnetFPModule.forward without the MLP: ops.three_nn + torch weight ops + ops.three_interpolate + torch.cat"""
    dist, idx = ops.three_nn(unknown, known)
    return _assemble(dist, idx, unknown_feats, known_feats), idx


def ordered_propagate(unknown, known, unknown_feats, known_feats):
    """nn_propagate with the interpolation on the ordered route"""
    dist, idx = ops.three_nn(unknown, known)
    return _assemble(dist, idx, unknown_feats, known_feats, _ordered_interpolate), idx


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


def backward_rows(lines, rounds, tag, unknown, known, kf, uf, g):
    """the interpolation's backward on its three routes: alone, inside the assembly's forward + backward, and in its two parts"""
    b, c2, m = kf.shape
    n = unknown.shape[1]
    dist, idx = ops.three_nn(unknown, known)
    recip = 1.0 / (dist + 1e-8)
    weight = (recip / torch.sum(recip, dim=2, keepdim=True)).contiguous()
    gi = g[:, :c2].contiguous()
    interp = {"inverted": ops.three_interpolate, "ordered": _ordered_interpolate, "torch": _torch_interpolate}
    leaf = kf.clone().requires_grad_(True)
    outs = {name: fn(leaf, idx, weight) for name, fn in interp.items()}   # the graphs are kept: the backward is timed alone
    grads = {name: torch.autograd.grad(o, [leaf], gi, retain_graph=True)[0] for name, o in outs.items()}
    lines.append("# %s  grad towards the features, inverted == ordered bit for bit: %s; worst |inverted - torch| %.3g"
                 % (tag, torch.equal(grads["inverted"].view(torch.int32), grads["ordered"].view(torch.int32)),
                    float((grads["inverted"] - grads["torch"]).abs().max())))
    leaves = [kf.clone().requires_grad_(True), uf.clone().requires_grad_(True)]
    route = {"inverted": lambda: _assemble(dist, idx, leaves[1], leaves[0]),
             "ordered": lambda: _assemble(dist, idx, leaves[1], leaves[0], _ordered_interpolate),
             "torch": lambda: _assemble(dist, idx, leaves[1], leaves[0], _torch_interpolate)}
    whole = {"inverted": nn_propagate, "ordered": ordered_propagate, "torch": torch_propagate}

    def step(fn):
        for t in leaves:
            t.grad = None
        fn().backward(g)

    start = torch.empty(b, m + 1, device="cuda", dtype=torch.int32)
    order = torch.empty(b, n * 3, device="cuda", dtype=torch.int32)
    gx = torch.empty_like(kf)
    idx32 = idx.contiguous()

    def invert():
        check(lib.sn_gather_invert(b, m, n * 3, ptr(idx32), ptr(start), ptr(order), stream_of(idx32)), "sn_gather_invert")

    def walk():
        check(lib.sn_weighted_gather_backward_inverted(b, c2, m, n, 3, ptr(weight), ptr(gi), ptr(start), ptr(order), ptr(gx),
                                                       stream_of(gx)), "sn_weighted_gather_backward_inverted")

    invert()
    cols = {"invert": invert, "walk": walk}
    for name in interp:
        cols["b " + name] = lambda name=name: torch.autograd.grad(outs[name], [leaf], gi, retain_graph=True)
        cols["ifb " + name] = lambda name=name: step(route[name])
        cols["fb " + name] = lambda name=name: step(lambda: whole[name](unknown, known, leaves[1], leaves[0])[0])
    times = {name: [] for name in cols}
    for _ in range(rounds):
        for name, fn in cols.items():
            times[name].append(timed(fn))

    def cell(name):
        t = times[name]
        return "%8.4f (%6.4f)" % (statistics.median(t), max(t) - min(t))

    lines.append("%-44s %18s %18s %18s" % ("  backward routes:", "inverted ms", "ordered ms", "torch ms"))
    lines.append("%-44s %18s %18s %18s" % ("interpolation backward alone", cell("b inverted"), cell("b ordered"), cell("b torch")))
    lines.append("%-44s %18s %18s %18s" % ("weights + interpolation + cat fwd+bwd", cell("ifb inverted"), cell("ifb ordered"), cell("ifb torch")))
    lines.append("%-44s %18s %18s %18s" % ("assembly fwd+bwd (own query each)", cell("fb inverted"), cell("fb ordered"), cell("fb torch")))
    lines.append("%-44s %18s %18s" % ("  sn_gather_invert | the walk", cell("invert"), cell("walk")))


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
        backward_rows(lines, args.rounds, tag, unknown, known, kf, uf, g)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

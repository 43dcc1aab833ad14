"""What ranking a batch of clouds costs (sn_rank_points) beside the earlier kernel and beside the host route.

    python tools/rank_bench.py [--out profiles/rank/rank_bench.txt]

Part 1 -- the entry alone at (B, N, k) = (32, 1024, 1024) [the classification ranking], (50, 2048, 2048) [the reconstruction ranking],
(32, 1024, 64) and (32, 2048, 64) [ordinary inference], on two inputs: idx = knn(1) of a seeded, untrained SampleNetProgressive's output
for a uniform cloud, and idx drawn with replacement.  Columns: sn_rank_points; sn_nn_matching_indexed(complete_fps = 1) where it takes
the shape (k <= 1024); the host route SampleNet.sample_indices takes beyond its cap (both transfers, sputils.nn_matching, the indices
recovered point by point).  Device columns: device events around REPS back-to-back calls, after a warm-up, the columns alternated
inside every one of ROUNDS rounds of one process; listed is the median round, with the lowest and highest round beside it.  The host
route: one call by the host clock (it is seconds long).
Part 2 -- sn_rank_points at every points-per-lane setting that holds the cloud in 1024 lanes (sn_rank_points_set_ppt), the same way:
the record behind the default (2 up to 1024 points, 4 up to 4096, 8 beyond).
Part 3 -- one ProgressiveClassificationEvaluator.add at B = 32, N = 1024, sizes 2 .. 1024 beside the same classification of every prefix
with the ranking done on the host.
Needs a GPU: fails without one.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((32, 1024, 1024), (50, 2048, 2048), (32, 1024, 64), (32, 2048, 64))
ROUNDS, REPS, WARM = 7, 5, 3


def make_ranker(k):
    from samplenet_amd import SampleNetProgressive, progressive_sizes

    torch.manual_seed(0)
    return SampleNetProgressive(progressive_sizes(2, k), 128, group_size=8, input_shape="bnc", output_shape="bnc").cuda().eval()


def make_inputs(B, N, k):
    """-> x (B,N,3) and {name: idx (B,k) int32} on the device"""
    from samplenet_amd import ops

    g = torch.Generator().manual_seed(1)
    x = (torch.rand(B, N, 3, generator=g) - 0.5).cuda()
    net = make_ranker(k)
    with torch.no_grad():
        y = net._features(x.permute(0, 2, 1), x)  # (B,3,k)
    idx = ops.knn(1, x, y.contiguous(), ops.BNC, ops.BCN, return_dist=False)[0].view(B, k)
    draws = torch.randint(0, N, (B, k), generator=g, dtype=torch.int32).cuda()
    return x, {"sampler": idx.contiguous(), "draws": draws}


def device_rounds(columns):
    """columns: {name: callable}; -> {name: (median, lowest, highest) ms per call over ROUNDS alternated rounds}"""
    for fn in columns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in columns}
    for _ in range(ROUNDS):
        for name, fn in columns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / REPS)
    return {name: (float(np.median(t)), min(t), max(t)) for name, t in times.items()}


def host_route(x, idx):
    """SampleNet.sample_indices' branch beyond the device cap, for given nearest-neighbour indices: -> (matched, out_idx, n_unique)"""
    from samplenet_amd import sputils

    k = idx.shape[1]
    pts = x.detach().cpu().numpy()
    nn = idx.cpu().numpy()
    picked, sel = sputils.nn_matching(pts, nn, k, complete_fps=True), []
    for b in range(pts.shape[0]):
        first = nn[b][np.sort(np.unique(nn[b], return_index=True)[1])]
        rest = [int(np.flatnonzero((pts[b] == p).all(1))[0]) for p in picked[b][len(first):]]
        sel.append(np.concatenate([first, np.asarray(rest, dtype=first.dtype)]))
    match = torch.as_tensor(picked, dtype=torch.float32).to(x.device)
    out_idx = torch.as_tensor(np.stack(sel).astype(np.int32)).to(x.device)
    n_unique = torch.as_tensor(np.array([len(np.unique(r)) for r in nn], dtype=np.int32)).to(x.device)
    torch.cuda.synchronize()
    return match, out_idx, n_unique


def fmt(t):
    return "%9.4f (%8.4f .. %8.4f)" % t


def part1(say):
    from samplenet_amd import ops

    say("part 1: one call, milliseconds: median round (lowest .. highest) of %d rounds of %d calls; host route: one call" % (ROUNDS, REPS))
    slower = []
    for B, N, k in SHAPES:
        x, inputs = make_inputs(B, N, k)
        for name, idx in inputs.items():
            columns = {"rank": lambda idx=idx: ops.rank_points(x, idx)}
            if k <= 1024:
                columns["old"] = lambda idx=idx: ops.nn_matching_indexed(x, idx, k)
            res = device_rounds(columns)
            new = ops.rank_points(x, idx)
            t0 = time.perf_counter()
            host = host_route(x, idx)
            t_host = (time.perf_counter() - t0) * 1e3
            same = all(torch.equal(a, b) for a, b in zip(new, host))
            if k <= 1024:
                same = same and all(torch.equal(a, b) for a, b in zip(new, ops.nn_matching_indexed(x, idx, k)))
            say("  B %3d N %5d k %5d  idx %-8s distinct %7.1f | sn_rank_points %s | sn_nn_matching_indexed %s | host route %10.1f | outputs equal: %s"
                % (B, N, k, name, float(new[2].float().mean()), fmt(res["rank"]),
                   fmt(res["old"]) if "old" in res else "        -- (k > 1024: refused)    ", t_host, same))
            if "old" in res and res["rank"][0] > res["old"][0]:
                slower.append("B %d N %d k %d idx %s: %.4f against %.4f ms" % (B, N, k, name, res["rank"][0], res["old"][0]))
    say("  sn_rank_points slower than sn_nn_matching_indexed (median): " + ("; ".join(slower) if slower else "nowhere"))


def part2(say):
    from samplenet_amd import ops
    from samplenet_amd._lib import lib

    say("part 2: sn_rank_points by points per lane (threads per workgroup), milliseconds as in part 1; * = the default")
    for B, N, k in SHAPES:
        x, inputs = make_inputs(B, N, k)
        idx = inputs["draws"]
        legal = [p for p in (1, 2, 4, 8) if N <= 1024 * p]

        def run(p):
            lib.sn_rank_points_set_ppt(p)
            ops.rank_points(x, idx)
            lib.sn_rank_points_set_ppt(0)

        res = device_rounds({p: (lambda p=p: run(p)) for p in legal})
        default = 2 if N <= 1024 else 4 if N <= 4096 else 8
        say("  B %3d N %5d k %5d  idx draws   " % (B, N, k) + " | ".join(
            "%d%s (%4d thr) %s" % (p, "*" if p == default else " ", (-(-N // p) + 63) // 64 * 64, fmt(res[p])) for p in legal))


def part3(say):
    from samplenet_amd import PointNetCls, ProgressiveClassificationEvaluator, ops
    from samplenet_amd.evaluation import _classify_batch

    B, N, k = 32, 1024, 1024
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(B, N, 3, generator=g) - 0.5).cuda()
    labels = torch.randint(0, 40, (B,), generator=g).cuda()
    torch.manual_seed(3)
    classifier = PointNetCls(num_classes=40, input_shape="bnc").cuda().eval()
    ranker = make_ranker(k)
    ev = ProgressiveClassificationEvaluator(classifier, ranker)

    def device_add():
        ev.reset()
        ev.add(x, labels)

    def host_add():
        with torch.no_grad():
            y = ranker._features(x.permute(0, 2, 1), x)
            idx = ops.knn(1, x, y.contiguous(), ops.BNC, ops.BCN, return_dist=False)[0].view(B, k)
            ordered = host_route(x, idx)[0]
            for s in ev.sizes:
                _classify_batch(classifier, ordered[:, :s].contiguous(), labels, 0.001)
        torch.cuda.synchronize()

    for _ in range(WARM):
        device_add()
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        device_add()
        torch.cuda.synchronize()
        t_dev.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    host_add()
    t_host = (time.perf_counter() - t0) * 1e3
    say("part 3: ProgressiveClassificationEvaluator.add, B %d N %d, %d sizes %d .. %d, PointNetCls, host clock to completion, milliseconds"
        % (B, N, len(ev.sizes), ev.sizes[0], ev.sizes[-1]))
    say("  ranked on the device %s | ranked on the host, classified size by size %10.1f (one call)"
        % (fmt((float(np.median(t_dev)), min(t_dev), max(t_dev))), t_host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rank", "rank_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench: no GPU (nothing is measured without one)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("tools/rank_bench.py on %s" % torch.cuda.get_device_name(0))
    part1(say)
    part2(say)
    part3(say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

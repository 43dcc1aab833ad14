"""What ranking and scoring a labelled set of shape descriptors costs (sn_retrieval_metrics) beside the host route.

    python tools/retrieval_bench.py [--out profiles/retrieval/retrieval_bench.txt]

Part 1 -- the entry alone at (S, n, C) = (1, 2468, 256) [ModelNet40's test split, one sampler] and (11, 2468, 256) [a progressive
sampler's sizes 2 .. 2048] on standard-normal descriptors with 40 labels, through ops.retrieval_metrics (its output allocations
included), with and without the ranking written out.  Device events around REPS back-to-back calls after a warm-up, ROUNDS rounds in
one process; listed is the median round with the lowest and highest beside it, and the call-level arithmetic rate 3 S n^2 C / time
(subtract, multiply, add per channel and pair; sort and scoring not counted).  Beside it the host route on the same descriptors, ONE
set, once, by the host clock: the transfer, numpy float64 distances in their quickest host form (|a|^2 + |b|^2 - 2 a.b through one
matrix product -- the form the kernel must not use), the stable argsort, and the rank loop of tests/retrieval_ref.py
(scores_by_loop); a progressive evaluation would pay it once per size.
Part 2 -- RetrievalEvaluator over 2468 clouds of 1024 points at batch 32 with a seeded PointNetCls: the adds (the classifier) and
result() (one launch, one transfer) by the host clock to completion.
Needs a GPU: fails without one.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1, 2468, 256), (11, 2468, 256))
ROUNDS, REPS, WARM, LEVELS = 7, 5, 3, 20


def device_rounds(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / REPS)
    return float(np.median(times)), min(times), max(times)


def host_route(desc, labels):
    """one set (n, C) on the device -> (ap, prec, n_relevant, order) and the seconds of each stage"""
    import retrieval_ref as R

    t = [time.perf_counter()]
    a, lab = desc.cpu().numpy(), labels.cpu().numpy()
    t.append(time.perf_counter())
    a64 = a.astype(np.float64)
    sq = (a64 * a64).sum(1)
    d = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (a64 @ a64.T), 0.0)  # (the quickest host form: one float64 matrix product)
    np.fill_diagonal(d, 0.0)
    t.append(time.perf_counter())
    order = R.ranking(d)
    t.append(time.perf_counter())
    ap, prec, rel = R.scores_by_loop(order, lab, LEVELS)
    t.append(time.perf_counter())
    return (ap, prec, rel, order), np.diff(t)


def fmt(t):
    return "%9.4f (%8.4f .. %8.4f)" % t


def part1(say):
    from samplenet_amd import ops

    say("part 1: one call, milliseconds: median round (lowest .. highest) of %d rounds of %d calls; host route: one set, one call" % (ROUNDS, REPS))
    for S, n, C in SHAPES:
        g = torch.Generator().manual_seed(S)
        desc = torch.randn(S, n, C, generator=g).cuda()
        labels = torch.randint(0, 40, (n,), generator=g, dtype=torch.int32).cuda()
        scores = device_rounds(lambda: ops.retrieval_metrics(desc, labels, LEVELS))
        ranked = device_rounds(lambda: ops.retrieval_metrics(desc, labels, LEVELS, return_order=True))
        ap, prec, rel, order, _ = [x.cpu().numpy() for x in ops.retrieval_metrics(desc, labels, LEVELS, return_order=True)]
        (hap, hprec, hrel, horder), stages = host_route(desc[0], labels)
        differ = int((order[0] != horder).any(axis=1).sum())
        say("  S %2d n %d C %d | scores %s = %6.2f TFLOP/s | scores and ranking %s | host route, ONE set: %8.1f ms (transfer %.1f, distances %.1f, "
            "argsort %.1f, rank loop %.1f)" % (S, n, C, fmt(scores), 3.0 * S * n * n * C / scores[0] * 1e-9, fmt(ranked),
                                               stages.sum() * 1e3, *(stages * 1e3)))
        say("       set 0 against the host's float64: n_relevant equal: %s; queries ranked differently (float32 near-ties): %d of %d; "
            "mean AP %.9f device, %.9f host" % (np.array_equal(rel, hrel), differ, n, np.nanmean(ap[0].astype(np.float64)), np.nanmean(hap)))


def part2(say):
    from samplenet_amd import PointNetCls, RetrievalEvaluator

    n, N, B = 2468, 1024, 32
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(n, N, 3, generator=g) - 0.5).cuda()
    labels = torch.randint(0, 40, (n,), generator=g).cuda()
    torch.manual_seed(3)
    ev = RetrievalEvaluator(PointNetCls(num_classes=40, input_shape="bnc").cuda().eval(), None, levels=LEVELS)

    def run():
        ev.reset()
        t0 = time.perf_counter()
        for lo in range(0, n, B):
            ev.add(x[lo:lo + B], labels[lo:lo + B])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = ev.result()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, res

    for _ in range(2):
        run()
    adds, results = zip(*[run()[:2] for _ in range(ROUNDS)])
    res = run()[2]
    say("part 2: RetrievalEvaluator, %d clouds of %d points, batch %d, PointNetCls, no sampler, host clock to completion, milliseconds" % (n, N, B))
    say("  %d adds %s | result() (one launch, one transfer) %s | map %.6f, n_valid %d"
        % (-(-n // B), fmt((float(np.median(adds)), min(adds), max(adds))), fmt((float(np.median(results)), min(results), max(results))),
           res["map"], res["n_valid"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval", "retrieval_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench: no GPU (nothing is measured without one)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("tools/retrieval_bench.py on %s" % torch.cuda.get_device_name(0))
    part1(say)
    part2(say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

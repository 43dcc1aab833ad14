#!/usr/bin/env python3
"""Farthest-point sampling on the GPU (sn_furthest_point_sample, samplenet_amd/csrc/sampling.hip): HIP-event timing of every
variant that takes the shape and of the auto choice, per call and per FPS step, at the shapes the reference's experiments
run; for two of them also the loop of torch ops a user would otherwise write.  Checks that every variant returns the same
indices.  Output: profiles/fps/fps_bench.txt.

    python tools/fps_bench.py            # the table
    python tools/fps_bench.py --quick    # one timed call per entry (for a rocprofv3 --kernel-trace --stats run)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenet_amd import ops  # noqa: E402
from samplenet_amd._lib import lib  # noqa: E402

SHAPES = [  # (B, N, M, what it is)
    (32, 1024, 64, "--sampler fps at main.py's batch"),
    (32, 1024, 1024, "full ordering"),
    (50, 2048, 2048, "the reconstruction sort"),
    (8, 16384, 1024, ""),
    (4, 65536, 2048, "streaming"),
    (1, 100000, 4096, "streaming"),
    (32, 256, 256, "auto rule: small clouds"),
    (2048, 1024, 64, "auto rule: clouds fill every SIMD"),
]
TORCH_LOOP = {(32, 1024, 64), (50, 2048, 2048)}
NAMES = {0: "auto", 1: "(a) wave", 2: "(b) group", 3: "(c) stream"}
MAX_N = {1: 2048, 2: 16384, 3: 1 << 30}
QUICK = "--quick" in sys.argv


def timed(fn, target_s=0.5):
    """mean ms per call: 2 warm-up calls, then enough calls for ~target_s (one with --quick)"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    one = e0.elapsed_time(e1)
    reps = 1 if QUICK else max(3, min(200, int(target_s * 1e3 / max(one, 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_loop_fps(x, m):
    """what a user without the kernel writes: one farthest-point step per iteration, in torch ops on the GPU"""
    B, N, _ = x.shape
    rows = torch.arange(B, device=x.device)
    idx = torch.zeros(B, m, dtype=torch.long, device=x.device)
    cur = torch.full((B, N), float("inf"), device=x.device)
    last = torch.zeros(B, dtype=torch.long, device=x.device)
    for j in range(1, m):
        d = ((x - x[rows, last][:, None, :]) ** 2).sum(-1)
        cur = torch.minimum(cur, d)
        last = cur.argmax(1)
        idx[:, j] = last
    return idx


def auto_pick(B, N):
    """the variant auto runs for (B, N), from the kernel name torch.profiler records (None without a profiler)"""
    x = torch.rand(B, N, 3, device="cuda")
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ops.furthest_point_sample(x, 2)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if "fps_" in e.name]
        for key, v in (("fps_wave_kernel", 1), ("fps_group_kernel", 2), ("fps_stream_kernel", 3)):
            if any(key in n for n in names):
                return v
    except Exception:  # pragma: no cover  (profiler unavailable: say so)
        pass
    return None


def main():
    torch.manual_seed(0)
    print("farthest-point sampling, MI355X, HIP events; ms per call (mean), ns per FPS step = call time / (M - 1)")
    print("%-18s %-34s %-11s %10s %10s  %s" % ("B, N, M", "what", "variant", "ms/call", "ns/step", "note"))
    for B, N, M, what in SHAPES:
        x = torch.rand(B, N, 3, device="cuda") - 0.5
        pick = None if QUICK else auto_pick(B, N)
        ref = None
        for v in (0, 1, 2, 3):
            if v and N > MAX_N[v]:
                continue
            prev = lib.sn_fps_set_variant(v)
            try:
                idx = ops.furthest_point_sample(x, M)
                ref = idx if ref is None else ref
                same = torch.equal(idx, ref)
                ms = timed(lambda: ops.furthest_point_sample(x, M))
            finally:
                lib.sn_fps_set_variant(prev)
            note = ("auto runs %s" % NAMES.get(pick, "?")) if v == 0 else ("" if same else "INDICES DIFFER FROM AUTO")
            print("%-18s %-34s %-11s %10.3f %10.1f  %s" % ("%d, %d, %d" % (B, N, M), what, NAMES[v], ms, ms * 1e6 / max(M - 1, 1), note))
            sys.stdout.flush()
        if (B, N, M) in TORCH_LOOP:
            ms = timed(lambda: torch_loop_fps(x, M), target_s=0.2)
            same = torch.equal(torch_loop_fps(x, M).int(), ref)
            print("%-18s %-34s %-11s %10.3f %10.1f  %s" % ("%d, %d, %d" % (B, N, M), "torch ops, one step per iteration",
                                                           "torch loop", ms, ms * 1e6 / max(M - 1, 1),
                                                           "same indices" if same else "indices differ (ties / rounding)"))
    print("peak memory %.1f MB" % (torch.cuda.max_memory_allocated() / 1e6))


if __name__ == "__main__":
    main()

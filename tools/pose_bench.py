"""What the pose-error terms cost and what the device evaluator buys.  Recorded, not gated.

    python tools/pose_bench.py > profiles/pose/pose_bench.txt

Shape: B = 32 clouds of N = 1024 points sampled to M = 64 (group size K = 8), PCRNet with its default bottleneck of 1024, frozen.
Part 1  the captured training step (engine.SamplerTrainStep on a pair-making DeviceBatchSource, sampler + frozen PCRNet): the task
        loss of `--loss-type 1` (pcrnet_chamfer_loss) beside `--loss-type 0` (pcrnet_loss(want_info=False) through task_loss_igt=True).  ms per step:
        host clock around 200 replays ending in a synchronise, best of 3, the two variants alternated.  Launches per replay and the
        gaps between consecutive kernels: one replay of each under torch.profiler (a run of its own, after the timing).
Part 2  evaluation of 256 items (SampleNet in its inference branch, both clouds sampled): RegistrationEvaluator.add in batches of 32
        and one result() at the end, against the reference's pattern (registration/main.py:416-450) on the same kernels -- batch 1,
        pcrnet_loss + sampling_consistency per item and an .item() for each of the three values.  Items per second, best of 3.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, P, L, M, K = 32, 1024, 2048, 512, 64, 8
ITEMS = 256


def sync_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def sampler():
    from samplenet_amd import SampleNet

    torch.manual_seed(0)
    return SampleNet(M, 128, group_size=K, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()


def pcrnet():
    from samplenet_amd.task_features import PCRNet

    torch.manual_seed(1)
    pcr = PCRNet(input_shape="bnc").cuda().eval()
    for p in pcr.parameters():
        p.requires_grad_(False)
    return pcr.static_weights(True)


def kernels_of(fn):
    """One call under the profiler -> (number of kernels, their names, median gap between consecutive kernels in us)."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = sorted((e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                  and "memset" not in e.name.lower()), key=lambda e: e.time_range.start)
    gaps = [b.time_range.start - a.time_range.end for a, b in zip(evs[:-1], evs[1:])]
    return len(evs), [e.name for e in evs], (float(np.median(gaps)) if gaps else float("nan"))


def part1(cloudset):
    from samplenet_amd import BatchRecipe, DeviceBatchSource
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.optim import Adam
    from samplenet_amd.parallel import FlatGradAllReducer
    from samplenet_amd.task_features import pcrnet_chamfer_loss, pcrnet_loss

    print("Part 1 -- the captured step, sampler + frozen PCRNet (B = %d, N = %d -> M = %d, K = %d; Adam inside)" % (B, N, M, K))
    rc = BatchRecipe(shuffle_points=True, unit_cube=True)
    pcr = pcrnet()
    steps = {}
    for name, kw in (("loss type 1", dict(task_loss=lambda proj, p1: pcrnet_chamfer_loss(pcr, proj, p1)[0])),
                     ("loss type 0", dict(task_loss=lambda proj, p1, igt: pcrnet_loss(pcr, proj, p1, igt, loss_type=0, want_info=False)[0], task_loss_igt=True))):
        net = sampler()
        src = DeviceBatchSource(cloudset, rc, B, N, seed=1, pair="fixed")
        steps[name] = SamplerTrainStep(net, src.at(0).p0, reducer=FlatGradAllReducer(net), optimizer=Adam(net.parameters(), lr=1e-3),
                                       input_source=src, **kw)
        assert len(steps[name]._ring_graphs[0]) == 1
    for s in steps.values():
        sync_ms(s.step, 20)
    times = {n: [] for n in steps}
    for _ in range(3):  # alternated
        for n, s in steps.items():
            times[n].append(sync_ms(s.step, 200))
    prof = {n: kernels_of(s.step) for n, s in steps.items()}
    for n in steps:
        print("  %-12s %.4f ms per step (runs: %s)   %d launches per replay, median gap between kernels %.2f us"
              % (n, min(times[n]), " ".join("%.4f" % t for t in times[n]), prof[n][0], prof[n][2]))
    d = min(times["loss type 0"]) - min(times["loss type 1"])
    print("  difference   %+.4f ms = %+.2f us; launches %+d; two median gaps of the loss-type-1 graph = %.2f us"
          % (d, d * 1e3, prof["loss type 0"][0] - prof["loss type 1"][0], 2 * prof["loss type 1"][2]))
    a, b = list(prof["loss type 1"][1]), list(prof["loss type 0"][1])
    for k in a:
        if k in b:
            b.remove(k)
    print("  kernels only in the loss-type-0 replay (%d): %s" % (len(b), "; ".join(b) or "none"))
    print("  expected: pose_error_fwd_kernel and pose_error_bwd_kernel (the feature), one elementwise add (norm_err + chamfer_loss, a 0-d")
    print("  tensor) and one three-element cat (the add's upstream scalar placed into sn_pose_error_backward's g_means vector).")


def part2(cloudset):
    from samplenet_amd import BatchRecipe, DeviceBatchSource, RegistrationEvaluator
    from samplenet_amd.task_features import pcrnet_loss, sampling_consistency

    print("Part 2 -- evaluating %d items (SampleNet inference branch, both clouds sampled, loss type 0)" % ITEMS)
    pcr, net = pcrnet(), sampler().eval()
    src = DeviceBatchSource(cloudset, BatchRecipe(shuffle_points=True, unit_cube=True), B, N, seed=2, pair="fixed")
    batches = [src.at(i * B) for i in range(ITEMS // B)]

    def batched():
        ev = RegistrationEvaluator(pcr, net, num_sampled_clouds=2, loss_type=0)
        for bt in batches:
            ev.add(bt.p0, bt.p1, bt.igt)
        return ev.result()

    def per_item():
        rot, trans, cons = [], [], []
        with torch.no_grad():
            for bt in batches:
                for i in range(B):
                    p0, p1, igt = bt.p0[i:i + 1], bt.p1[i:i + 1], bt.igt[i:i + 1]
                    p1s, p0s = net(p1)[1].contiguous(), net(p0)[1].contiguous()
                    _, info = pcrnet_loss(pcr, p0s, p1s, igt, loss_type=0)
                    cons.append(sampling_consistency(p0s, p1s, igt).item())
                    rot.append(info["rot_err"].item())
                    trans.append(info["trans_err"].item())
        return np.array(rot), np.array(trans), np.array(cons)

    ra, rb = batched(), per_item()
    print("  largest difference of the per-item values between the two routes: rotation %.3e deg, translation %.3e, consistency %.3e"
          % (np.abs(ra["rotation_errors"] - rb[0]).max(), np.abs(ra["trans_errs"] - rb[1]).max(), np.abs(ra["consistency_errors"] - rb[2]).max()))
    ta, tb = [], []
    for _ in range(3):  # alternated
        ta.append(sync_ms(batched, 3))
        tb.append(sync_ms(per_item, 1))
    print("  RegistrationEvaluator, batches of %d   %8.2f ms   %9.0f items / s" % (B, min(ta), ITEMS / min(ta) * 1e3))
    print("  batch 1, an .item() per value         %8.2f ms   %9.0f items / s" % (min(tb), ITEMS / min(tb) * 1e3))
    print("  ratio                                 %.1f x" % (min(tb) / min(ta)))


def main():
    from samplenet_amd import DeviceCloudSet

    print("device: %s, HIP %s, torch %s" % (torch.cuda.get_device_name(0), torch.version.hip, torch.__version__))
    rng = np.random.default_rng(0)
    cloudset = DeviceCloudSet(rng.standard_normal((L, P, 3), dtype=np.float32), rng.integers(0, 40, L))
    if "--only-eval" not in sys.argv:
        part1(cloudset)
    if "--only-step" not in sys.argv:
        part2(cloudset)


if __name__ == "__main__":
    main()

"""What feeding the sampler's training step costs: the device batch assembly (samplenet_amd.device_data, one launch) against the host
route (per-item ModelNetCls.__getitem__ + transform chain, collate, DeviceBatchRing.load), and the captured step with the source as
its first node against the captured step on a static input ring.  Recorded, not gated.

    python tools/input_bench.py > profiles/input/input_bench.txt

Shape: B = 32, N = 1024, P = 2048, L = 9840 (ModelNet40's training split; synthetic clouds of that size -- the cost does not depend on
the coordinates).  Two recipes:
    registration     shuffle_points + unit_cube + pair          (main.py: ModelNetCls(OnUnitCube) under QuaternionFixedDataset)
    classification   rotation about y + jitter                  (provider.py: rotate_point_cloud + jitter_point_cloud)
Part 1  assemble alone: `launch` = host clock around 200 launches ending in a synchronise; `graph` = 50 launches captured in one
        graph and replayed (device time per launch, no host launch path).
Part 2  host route for the same batches: the items are made by data.ModelNetCls.__getitem__ with a per-item transform in numpy
        (whole-array operations on one cloud: the stages' arithmetic, nothing else), stacked, and handed to DeviceBatchRing.load; ms
        per batch on ONE process, and the CPU count of this machine (a DataLoader divides the item cost by its workers at best).
Part 3  the captured step (engine.SamplerTrainStep, Adam inside): input_source= against an 8-entry static ring; ms per step.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, P, L, M, K = 32, 1024, 2048, 9840, 64, 8


def recipes():
    from samplenet_amd import BatchRecipe

    return {"registration": (BatchRecipe(shuffle_points=True, unit_cube=True), "fixed"),
            "classification": (BatchRecipe(rotate_axis=(0.0, 1.0, 0.0), jitter=(0.01, 0.05)), None)}


def sync_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def part1(cloudset):
    from samplenet_amd import DeviceBatchSource

    print("Part 1 -- the assemble launch alone (B = %d, N = %d, P = %d, L = %d), ms per batch" % (B, N, P, L))
    for name, (rc, pair) in recipes().items():
        src = DeviceBatchSource(cloudset, rc, B, N, seed=1, pair=pair)
        out = src._alloc()
        fn = lambda: src.next_into(out.p0, out.p1)  # noqa: E731
        sync_ms(fn, 20)
        launch = min(sync_ms(fn, 200) for _ in range(3))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(50):
                fn()
        g.replay()
        graph = min(sync_ms(g.replay, 10) for _ in range(3)) / 50
        print("  %-15s launch %.4f   graph %.4f   (%.0f k clouds/s from the graph figure)" % (name, launch, graph, B / graph))


def host_unit_cube(c):
    """(n, 3) float32 cloud -> the same cloud at unit largest extent with its centroid at the origin (numpy, one pass each)."""
    c = np.asarray(c, dtype=np.float32)
    extent = np.ptp(c, axis=0).max()
    c = c * np.float32(1.0 / extent)
    c -= c.sum(axis=0, dtype=np.float32) / np.float32(len(c))
    return torch.from_numpy(c)


def host_rotate_jitter(c, rng=np.random.default_rng(5)):
    """(n, 3) float32 cloud -> turned about y by a uniform angle, each coordinate moved by a clipped N(0, 0.01) offset (numpy)."""
    c = np.asarray(c, dtype=np.float32)
    turn = rng.random() * 2.0 * np.pi
    co, si = np.float32(np.cos(turn)), np.float32(np.sin(turn))
    out = np.empty_like(c)
    out[:, 0] = co * c[:, 0] + si * c[:, 2]
    out[:, 1] = c[:, 1]
    out[:, 2] = co * c[:, 2] - si * c[:, 0]
    out += np.clip(rng.standard_normal(c.shape, dtype=np.float32) * np.float32(0.01), -0.05, 0.05)
    return torch.from_numpy(out)


def part2(points, labels):
    from samplenet_amd.data import DeviceBatchRing, ModelNetCls

    print("Part 2 -- the host route, ONE process; this machine has %d CPUs (os.cpu_count), %d usable (affinity)"
          % (os.cpu_count(), len(os.sched_getaffinity(0))))
    chains = {"registration": host_unit_cube, "classification": host_rotate_jitter}
    quat = torch.randn(L, 4)
    quat = quat / quat.norm(dim=1, keepdim=True)
    ring = DeviceBatchRing(B, N, "cuda", depth=2)
    for name, chain in chains.items():
        ds = ModelNetCls.__new__(ModelNetCls)  # (the shards are synthetic: no files to read)
        ds.points, ds.labels, ds.transforms, ds.include_shapes, ds.shapes = points, labels[:, None], chain, False, []
        ds.set_num_points(N)
        order = np.random.permutation(L)

        def batch(t):
            items = [ds[int(i)] for i in order[t * B:(t + 1) * B]]
            p0 = torch.stack([c for c, _ in items])
            if name == "registration":  # QuaternionFixedDataset: rotate every cloud by its item's quaternion
                q, u = quat[order[t * B:(t + 1) * B], :1, None], quat[order[t * B:(t + 1) * B], None, 1:].expand(-1, N, -1)
                uv = torch.cross(u, p0, dim=2)
                p0 = p0 + 2 * (q * uv + torch.cross(u, uv, dim=2))
            ring.load(t % 2, p0)

        for t in range(3):
            batch(t)
        torch.cuda.synchronize()
        n, t0 = 20, time.perf_counter()
        for t in range(n):
            batch(3 + t)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        print("  %-15s %.3f ms per batch  (%.1f k clouds/s; %.1f us per item)" % (name, ms, B / ms, ms * 1e3 / B))


def part3(cloudset):
    from samplenet_amd import DeviceBatchSource, SampleNet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.optim import Adam
    from samplenet_amd.parallel import FlatGradAllReducer

    print("Part 3 -- the captured training step (B = %d, N = %d, M = %d; Adam inside), ms per step, best of 3 x 200" % (B, N, M))
    rc, _ = recipes()["registration"]

    def net():
        torch.manual_seed(0)
        return SampleNet(M, 128, group_size=K, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()

    src = DeviceBatchSource(cloudset, rc, B, N, seed=1)
    x0 = src.at(0).p0
    na, nb = net(), net()
    sa = SamplerTrainStep(na, x0, reducer=FlatGradAllReducer(na), optimizer=Adam(na.parameters(), lr=1e-3), input_source=src)
    ringt = [src.at(i * B).p0 for i in range(8)]
    sb = SamplerTrainStep(nb, x0, reducer=FlatGradAllReducer(nb), optimizer=Adam(nb.parameters(), lr=1e-3), input_ring=ringt)
    it = iter(range(10 ** 9))
    fa, fb = sa.step, (lambda: sb.replay(next(it) % 8))
    for f in (fa, fb):
        sync_ms(f, 20)
    ta, tb = [], []
    for _ in range(3):  # alternated
        ta.append(sync_ms(fa, 200))
        tb.append(sync_ms(fb, 200))
    print("  input_source (assembled inside the graph)  %.4f" % min(ta))
    print("  static 8-entry ring (no input work at all) %.4f" % min(tb))
    print("  difference                                 %+.4f" % (min(ta) - min(tb)))


def main():
    from samplenet_amd import DeviceCloudSet

    print("device: %s, HIP %s, torch %s" % (torch.cuda.get_device_name(0), torch.version.hip, torch.__version__))
    rng = np.random.default_rng(0)
    points = rng.standard_normal((L, P, 3), dtype=np.float32)
    labels = rng.integers(0, 40, L)
    cloudset = DeviceCloudSet(points, labels)
    part1(cloudset)
    part2(points, labels)
    part3(cloudset)


if __name__ == "__main__":
    main()

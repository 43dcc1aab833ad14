#!/usr/bin/env python3
"""Generate tests/golden/fps_reference.npz: farthest-point indices of the reference's in-tree GPU kernel
(farthestpointsamplingKernel, reconstruction/external/sampling/tf_sampling_g.cu:105-170), emulated literally in numpy:

  * one 512-thread block per cloud; thread t walks points t, t + 512, ... in ascending order and keeps its first maximum
    (strict >, starting from best = -1, besti = 0) of min(d, temp), temp starting at 1e38;
  * d = (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1) in float32, left to right;
  * a pairwise tree reduction over the 512 slots in which slot i1 = 2t << u takes slot i2 = (2t+1) << u only when strictly
    larger: equal values keep the lower SLOT, which is not always the lower point index.

That kernel breaks ties by slot first and its CUDA build may contract the distance to FMAs, so the clouds are chosen TIE-FREE:
at every step the largest running minimum beats the second by more than 8 float32 ulps.  There the arg-max does not depend on
either rule, and the fixture pins the farthest-point sequence itself (tests/test_fps_host.py, tests/test_gpu_fps.py).

    python tests/golden/make_fps_golden.py

Needs numpy only.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = 512


def intree_fps(xyz, m, check_gap=False):
    """xyz (N,3) float32 -> (idx (m,) int32, smallest top-1 / top-2 gap in ulps over the steps)."""
    n = xyz.shape[0]
    x, y, z = (xyz[:, c].astype(np.float32) for c in range(3))
    temp = np.full(n, 1e38, np.float32)
    rows = (n + THREADS - 1) // THREADS
    slot_k = np.arange(rows * THREADS).reshape(rows, THREADS)
    idx = np.zeros(m, np.int32)
    old, min_gap = 0, np.inf
    for j in range(1, m):
        x1, y1, z1 = x[old], y[old], z[old]
        d = (x - x1) * (x - x1) + (y - y1) * (y - y1) + (z - z1) * (z - z1)
        temp = np.minimum(d, temp)
        if check_gap and n > 1:
            top2 = np.sort(temp)[-2:]
            min_gap = min(min_gap, float((top2[1] - top2[0]) / np.spacing(top2[1])))
        grid = np.full(rows * THREADS, -np.inf, np.float32)
        grid[:n] = temp
        grid = grid.reshape(rows, THREADS)
        best = np.full(THREADS, -1.0, np.float32)
        besti = np.zeros(THREADS, np.int64)
        for r in range(rows):  # each thread's sequential walk
            take = grid[r] > best
            best = np.where(take, grid[r], best)
            besti = np.where(take, slot_k[r], besti)
        u = 0
        while (1 << u) < THREADS:  # the block's tree reduction
            t = np.arange(THREADS >> (u + 1))
            i1, i2 = (2 * t) << u, (2 * t + 1) << u
            take = best[i1] < best[i2]
            best[i1] = np.where(take, best[i2], best[i1])
            besti[i1] = np.where(take, besti[i2], besti[i1])
            u += 1
        old = int(besti[0])
        idx[j] = old
    return idx, min_gap


def tie_free_clouds(count, n, m, first_seed):
    clouds, idxs, seeds = [], [], []
    seed = first_seed
    while len(clouds) < count:
        xyz = np.random.default_rng(seed).random((n, 3), dtype=np.float32) * 2 - 1
        idx, gap = intree_fps(xyz, m, check_gap=True)
        if gap > 8:
            clouds.append(xyz)
            idxs.append(idx)
            seeds.append(seed)
        seed += 1
    return np.stack(clouds), np.stack(idxs), np.array(seeds)


def main():
    xa, ia, sa = tie_free_clouds(2, 2048, 2048, 1000)  # the reconstruction sort: full ordering, M = N = 2048
    xb, ib, sb = tie_free_clouds(4, 1024, 64, 2000)    # --sampler fps at num_out_points 64
    path = os.path.join(HERE, "fps_reference.npz")
    np.savez_compressed(path, xyz_full=xa, idx_full=ia, seeds_full=sa, xyz_64=xb, idx_64=ib, seeds_64=sb)
    print("wrote", path, "seeds", sa.tolist(), sb.tolist(), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Test helper for the cloud ranking (sn_rank_points; tests/test_rank_host.py, tests/test_gpu_rank_points.py): the numpy
restatement of the progressive sampler's inference ordering (first occurrences in order, then float64 farthest-point picks with
np.argmax: simple_projection_and_continued_fps / fps_from_given_indices, reconstruction/src/samplenet_progressive_pointnet_ae.py:546-600),
the input recipes and the shape table.  Lives in tests/ on purpose: nothing here is a product route."""
import functools

import numpy as np

# (B, N, k), one per branch of the kernel: a single point; one wave; two position chunks in one wave (100); 2 points per lane in 8 waves
# (1024); 4 points per lane in 5 / 8 / 10 waves (1025, 2048, 2500); 8 points per lane at the LDS limit (8192) and with a partly filled
# last wave (4100); k far below N; k above N (every point taken, then index 0 again)
SHAPES = ((1, 1, 1), (2, 64, 64), (3, 100, 100), (2, 1024, 1024), (1, 1025, 1025), (2, 2048, 2048), (1, 2500, 2500),
          (1, 8192, 8192), (2, 2048, 64), (1, 4100, 1500), (1, 16, 40))
RECIPES = ("draws", "near_tie", "distinct", "equal", "half", "coincident")


def rank_one(cloud, picks, k, dtype=np.float64):
    """One cloud (N,3) float32, picks (len,) in [0,N): -> (order (k,) int32, number of distinct picks).  The distinct picks in order of
    first occurrence, then farthest-point picks: squared distances to the chosen set in `dtype` as ((dx*dx + dy*dy) + dz*dz), np.argmax
    (first maximum).  dtype=np.float32 is the near_tie recipe's counter-example, not a reference."""
    pts = cloud.astype(dtype)

    def sqdist(p):
        d = pts[p] - pts
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    _, first = np.unique(picks, return_index=True)
    chosen = [int(p) for p in picks[np.sort(first)]]
    n_unique = len(chosen)
    dist = np.full(len(pts), np.inf, dtype=dtype)
    for p in chosen:
        dist = np.minimum(dist, sqdist(p))
    while len(chosen) < k:
        far = int(np.argmax(dist))
        chosen.append(far)
        dist = np.minimum(dist, sqdist(far))
    return np.asarray(chosen[:k], dtype=np.int32), n_unique


def _permutations(rng, B, N, k):
    """k indices per cloud without repetition while they last (k <= N), the permutation over again beyond."""
    return np.stack([np.resize(rng.permutation(N), k) for _ in range(B)])


def make_case(recipe, B, N, k, seed=0):
    """-> xyz (B,N,3) float32, idx (B,k) int32 in [0,N)."""
    rng = np.random.default_rng([seed, B, N, k, RECIPES.index(recipe)])
    xyz = rng.random((B, N, 3), dtype=np.float32) - 0.5
    if recipe == "draws":  # with replacement: at k = N about 63 % distinct -- both the seed pass and the farthest-point pass run long
        idx = rng.integers(0, N, (B, k))
    elif recipe == "near_tie":  # tells float64 distances from float32 ones (tests/test_rank_host.py): 1 + 2^-26 against 1
        xyz[:] = 0.0
        xyz[:, 1:, 0] = 1.0
        xyz[:, 2::2, 1] = 2.0 ** -13
        idx = np.zeros((B, k), dtype=np.int64)
    elif recipe == "distinct":  # a permutation: the farthest-point pass does not run (k <= N)
        idx = _permutations(rng, B, N, k)
    elif recipe == "equal":  # one seed
        idx = np.repeat(rng.integers(0, N, (B, 1)), k, axis=1)
    elif recipe == "half":  # every seed named twice, half a sample apart
        idx = _permutations(rng, B, N, k)
        idx[:, k // 2:] = idx[:, :k - k // 2]
    else:  # coincident: points exactly doubled, so ties of the farthest-point step go to the lowest index
        xyz[:, N // 2:] = xyz[:, :N - N // 2]
        idx = rng.integers(0, N, (B, k))
        idx[:, 1::2] = idx[:, 0:1]
    return xyz, idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(recipe, B, N, k):
    """make_case with its restated result, computed once and shared read-only: -> xyz, idx, order (B,k) int32, n_unique (B,) int32."""
    xyz, idx = make_case(recipe, B, N, k)
    ref = [rank_one(xyz[b], idx[b], k) for b in range(B)]
    out = (xyz, idx, np.stack([r[0] for r in ref]), np.array([r[1] for r in ref], dtype=np.int32))
    for a in out:
        a.setflags(write=False)
    return out

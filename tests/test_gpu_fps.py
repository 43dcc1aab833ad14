"""Farthest-point sampling on the GPU (samplenet_amd/csrc/sampling.hip): bit-exact against the numpy restatement of the contract
(tests/fps_numpy.py) over a sweep of shapes, tie-heavy clouds, every variant, the golden fixture of the reference's in-tree
kernel; the samplers over the compat shims against the reference's call pattern restated here; gather_operation's gradient;
hipGraph capture; edge cases."""
import importlib

import numpy as np
import pytest
import torch

from fps_numpy import fps_restated

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 64, 65, 1000, 1024, 2048, 2049, 8192, 16384, 16385, 40000]
BS = [1, 3, 32, 50]
WORK = 2.5e8  # B * N * M budget of one numpy restatement (~1-2 s)
VARIANT_MAX_N = {1: 2048, 2: 16384, 3: None}  # (a) wave per cloud, (b) workgroup per cloud, (c) streaming


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fps(x, m, layout=None):
    from samplenet_amd import ops

    return ops.furthest_point_sample(x, m, ops.BNC if layout is None else layout).cpu().numpy()


class forced:
    """with forced(v): sn_furthest_point_sample runs variant v (0 = auto); the hook is restored on exit."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from samplenet_amd._lib import lib

        self.prev = lib.sn_fps_set_variant(self.v)
        assert self.prev >= 0

    def __exit__(self, *exc):
        from samplenet_amd._lib import lib

        lib.sn_fps_set_variant(self.prev)


def fits(v, n):
    return v == 0 or VARIANT_MAX_N[v] is None or n <= VARIANT_MAX_N[v]


def sweep_cases(n):
    ms = [1, 2, 64, 512] if n > 16384 else [1, 2, 64, n, n + 5]
    cases = []
    for i, m in enumerate(dict.fromkeys(ms)):
        b = [b for b in BS[i % len(BS):] + BS[: i % len(BS)] if b * n * m <= WORK or b == 1][0]
        if n > 16384:
            b = min(b, 4)
        cases.append((b, m))
    return cases


# ---------------------------------------------------------------------------------------------------------------- 1. sweep
@pytest.mark.parametrize("n", NS)
def test_bit_exact_sweep_against_the_restatement(n):
    """Auto variant, both layouts, and a non-contiguous input: indices equal the restatement bit for bit."""
    from samplenet_amd import ops

    rng = np.random.default_rng(n)
    for b, m in sweep_cases(n):
        P = (rng.random((b, n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
        ref = fps_restated(P, m)
        x = dev(P)
        got = fps(x, m)
        assert got.shape == (b, m) and np.array_equal(got, ref), (b, n, m)
        assert np.array_equal(fps(x.transpose(1, 2).contiguous(), m, ops.BCN), ref), ("bcn", b, n, m)
        assert np.array_equal(fps(x.permute(0, 2, 1), m, ops.BCN), ref), ("bcn view", b, n, m)  # non-contiguous (B,3,N)
        wide = torch.zeros(b, n, 5, device="cuda")
        wide[:, :, 1:4] = x
        assert np.array_equal(fps(wide[:, :, 1:4], m), ref), ("strided", b, n, m)  # non-contiguous (B,N,3)


# ---------------------------------------------------------------------------------------------------------------- 2. ties
def _tie_clouds():
    rng = np.random.default_rng(7)
    grid = lambda b, n, r: rng.integers(-r, r + 1, (b, n, 3)).astype(np.float32)  # noqa: E731  exact in fp32 for |c| <= 64
    base = grid(3, 700, 64)
    return [
        ("grid64", grid(4, 1000, 64), 1005),
        ("grid64_2k", grid(3, 2048, 64), 1024),
        ("grid64_5k", grid(2, 5000, 64), 1024),
        ("grid2", grid(4, 1500, 2), 200),      # 125 distinct positions: M > distinct, then index 0 again
        ("dup", np.concatenate([base, base[:, ::-1]], axis=1), 1404),  # every point twice, M > N
        ("one_point", np.repeat(grid(2, 1, 64), 900, axis=1), 30),
        ("grid64_20k", grid(2, 20000, 64), 300),
    ]


@pytest.mark.parametrize("name,P,m", _tie_clouds(), ids=[c[0] for c in _tie_clouds()])
def test_tie_heavy_clouds(name, P, m):
    """Integer-grid coordinates (exact distances, many exact ties), duplicated points, M > N: every variant that takes the
    shape equals the restatement bit for bit; where sn_nn_matching takes the shape (N <= 8192, M <= 1024), its fp64
    farthest-point completion seeded with point 0 picks the same points."""
    from samplenet_amd import ops

    b, n, _ = P.shape
    ref = fps_restated(P, m)
    x = dev(P)
    for v in (0, 1, 2, 3):
        if fits(v, n):
            with forced(v):
                assert np.array_equal(fps(x, m), ref), (name, v)
                assert np.array_equal(fps(x.transpose(1, 2).contiguous(), m, ops.BCN), ref), (name, v, "bcn")
    if n <= 8192 and m <= 1024:
        pts = ops.nn_matching(x, torch.zeros(b, m, dtype=torch.int32, device="cuda"), m, True).cpu().numpy()
        assert np.array_equal(pts, np.take_along_axis(P, ref[:, :, None].astype(np.int64), axis=1)), name


# ------------------------------------------------------------------------------------------------------------- 3. variants
@pytest.mark.parametrize("b,n,m", [(32, 1024, 64), (5, 1, 3), (3, 64, 70), (7, 65, 65), (50, 2048, 2048), (4, 2047, 300),
                                   (2, 2049, 500), (3, 4096, 4096), (2, 4097, 333), (8, 8193, 1024), (2, 16384, 16389),
                                   (1, 16385, 700)])
def test_every_variant_gives_identical_indices(b, n, m):
    from samplenet_amd import ops

    rng = np.random.default_rng(b * 7 + n)
    x = dev(rng.standard_normal((b, n, 3)).astype(np.float32))
    xc = x.transpose(1, 2).contiguous()
    auto = fps(x, m)
    assert auto.min() >= 0 and auto.max() < n
    ran = 0
    for v in (1, 2, 3):
        if fits(v, n):
            with forced(v):
                assert np.array_equal(fps(x, m), auto), v
                assert np.array_equal(fps(xc, m, ops.BCN), auto), (v, "bcn")
            ran += 1
    assert ran >= 1 + (n <= 16384) + (n <= 2048)


def test_forced_variant_outside_its_range_is_refused():
    from samplenet_amd._lib import SampleNetHipError

    x = torch.rand(2, 2049, 3, device="cuda")
    with forced(1), pytest.raises(SampleNetHipError, match="variant 1"):
        fps(x, 8)


# --------------------------------------------------------------------------------------------------------------- 4. golden
def test_golden_fixture_of_the_in_tree_kernel(golden):
    from samplenet_amd import ops

    g = golden("fps_reference.npz")
    for key, m in (("full", 2048), ("64", 64)):
        x = dev(g["xyz_" + key])
        for v in (0, 1, 2, 3):
            with forced(v):
                assert np.array_equal(fps(x, m), g["idx_" + key]), (key, v)
        assert np.array_equal(fps(x.transpose(1, 2).contiguous(), m, ops.BCN), g["idx_" + key])


# ------------------------------------------------------------------------------------------------------- 5. samplers, shims
def _reference_fps_sampler_bnc(pu, x, m):
    # registration/src/fps.py:29-43 with permute=True, input_shape = output_shape = "bnc", call for call
    _, N, _ = x.shape
    x = x[:, torch.randperm(N), :]
    idx = pu.furthest_point_sample(x, m)
    x = x.permute(0, 2, 1).contiguous()
    y = pu.gather_operation(x, idx)
    return y.permute(0, 2, 1).contiguous()


def _reference_random_sampler_bnc(pu, x, m):
    # registration/src/random_sampling.py:27-46, input_shape = output_shape = "bnc", call for call
    x = x.permute(0, 2, 1).contiguous()
    B, _, N = x.shape
    idx = torch.zeros(B, m, dtype=torch.int32, device=x.device)
    for i in range(B):
        idx[i] = torch.randperm(N, dtype=torch.int32, device=x.device)[:m]
    y = pu.gather_operation(x, idx)
    return y.permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("b,n,m", [(32, 1024, 64), (4, 2048, 512), (2, 20000, 128)])
def test_samplers_equal_the_reference_call_pattern_over_the_shims(b, n, m):
    from samplenet_amd import FPSSampler, RandomSampler, compat

    compat.install()
    pu = importlib.import_module("pointnet2.utils.pointnet2_utils")
    x = torch.rand(b, n, 3, device="cuda") - 0.5
    for seed in (0, 1):
        torch.manual_seed(seed)
        ref = _reference_fps_sampler_bnc(pu, x, m)
        torch.manual_seed(seed)
        ours = FPSSampler(m, permute=True, input_shape="bnc", output_shape="bnc")(x)
        assert ours.shape == (b, m, 3) and torch.equal(ours, ref), ("fps", seed)
        torch.manual_seed(seed)
        ref = _reference_random_sampler_bnc(pu, x, m)
        torch.manual_seed(seed)
        ours = RandomSampler(m, input_shape="bnc", output_shape="bnc")(x)
        assert ours.shape == (b, m, 3) and torch.equal(ours, ref), ("random", seed)
    # without the permutation FPS picks the farthest-point sequence of the cloud itself
    y = FPSSampler(m, permute=False, input_shape="bnc", output_shape="bnc")(x)
    idx = fps_restated(x.cpu().numpy(), m) if n <= 2048 else fps(x, m)
    assert torch.equal(y.cpu(), torch.from_numpy(np.take_along_axis(x.cpu().numpy(), idx[:, :, None].astype(np.int64), axis=1)))


@pytest.mark.parametrize("permute", [False, True])
def test_bcn_samplers_equal_bnc_on_the_transposed_cloud(permute):
    from samplenet_amd import FPSSampler, RandomSampler

    x = torch.rand(6, 1500, 3, device="cuda")
    xt = x.transpose(1, 2).contiguous()
    for out in ("bcn", "bnc"):
        torch.manual_seed(3)
        a = FPSSampler(100, permute, input_shape="bnc", output_shape=out)(x)
        torch.manual_seed(3)
        c = FPSSampler(100, permute, input_shape="bcn", output_shape=out)(xt)
        assert torch.equal(a, c), ("fps", out)
        torch.manual_seed(4)
        a = RandomSampler(100, input_shape="bnc", output_shape=out)(x)
        torch.manual_seed(4)
        c = RandomSampler(100, input_shape="bcn", output_shape=out)(xt)
        assert torch.equal(a, c), ("random", out)
    assert FPSSampler(100, permute, "bcn", "bcn")(xt).shape == (6, 3, 100)


def _scatter_add_f64(shape, idx, go):
    g = np.zeros(shape, np.float64)
    for bi in range(shape[0]):
        np.add.at(g[bi].T, idx[bi].astype(np.int64), go[bi].T.astype(np.float64))
    return g


@pytest.mark.parametrize("case", ["fps_m_gt_n", "hand", "atomic_route"])
def test_gather_operation_gradient(case):
    """d out / d features of gather_operation (grouping_operation with one sample; its backward sums in order below
    kIndexAddOrderedWork and with float atomics above) against a float64 scatter-add, repeated indices included."""
    from samplenet_amd import ops

    rng = np.random.default_rng(11)
    if case == "fps_m_gt_n":
        B, C, N, M = 3, 5, 300, 700
        idx = ops.furthest_point_sample(torch.rand(B, N, 3, device="cuda"), M)  # every point, then index 0 over and over
    elif case == "hand":
        B, C, N, M = 2, 3, 50, 400
        idx = dev(rng.integers(0, 5, (B, M)).astype(np.int32))
    else:
        B, C, N, M = 1, 3, 16384, 300000  # (N / 64) * M index loads > 2^26
        idx = dev(rng.integers(0, N, (B, M)).astype(np.int32))
    feat = dev(rng.standard_normal((B, C, N)).astype(np.float32)).requires_grad_(True)
    out = ops.gather_operation(feat, idx)
    ih = idx.cpu().numpy()
    assert out.shape == (B, C, M)
    assert torch.equal(out.detach().cpu(), torch.from_numpy(np.take_along_axis(feat.detach().cpu().numpy(), ih[:, None, :].astype(np.int64).repeat(C, 1), axis=2)))
    go = rng.standard_normal((B, C, M)).astype(np.float32)
    (g,) = torch.autograd.grad(out, feat, dev(go))
    ref = _scatter_add_f64((B, C, N), ih, go)
    np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("b,n,m", [(32, 1024, 64), (2, 20000, 96)])
def test_graph_capture_replays_like_eager(b, n, m):
    from samplenet_amd import ops

    xs = torch.rand(b, n, 3, device="cuda")
    fs = torch.rand(b, 4, n, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.gather_operation(fs, ops.furthest_point_sample(xs, m))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx = ops.furthest_point_sample(xs, m)
        y = ops.gather_operation(fs, idx)
    for seed in (1, 2):
        g = torch.Generator(device="cuda").manual_seed(seed)
        xs.copy_(torch.rand(b, n, 3, device="cuda", generator=g))
        fs.copy_(torch.rand(b, 4, n, device="cuda", generator=g))
        graph.replay()
        torch.cuda.synchronize()
        ie = ops.furthest_point_sample(xs.clone(), m)
        assert torch.equal(idx, ie) and torch.equal(y, ops.gather_operation(fs.clone(), ie)), seed


# ---------------------------------------------------------------------------------------------------------------- 7. edges
def test_empty_work_and_cpu_tensors():
    from samplenet_amd import ops

    assert ops.furthest_point_sample(torch.rand(0, 10, 3, device="cuda"), 4).shape == (0, 4)
    assert ops.furthest_point_sample(torch.rand(3, 10, 3, device="cuda"), 0).shape == (3, 0)
    assert ops.furthest_point_sample(torch.rand(0, 3, 40000, device="cuda"), 5, ops.BCN).shape == (0, 5)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        ops.furthest_point_sample(torch.rand(2, 10, 3), 4)
    with pytest.raises(ValueError):
        ops.furthest_point_sample(torch.rand(2, 10, 4, device="cuda"), 4)
    x = torch.rand(2, 10, 3, device="cuda")
    x[0, 3, 1] = float("nan")
    x[1, 5] = float("inf")
    got = fps(x, 12)
    assert got.min() >= 0 and got.max() < 10 and np.array_equal(got, fps_restated(x.cpu().numpy(), 12))

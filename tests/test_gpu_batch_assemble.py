"""sn_batch_assemble / samplenet_amd.device_data on the GPU against the numpy restatement tests/batch_ref.py.

Integers (items, labels, point order, dropout's choice) bit for bit; float stages element by element against the fp64 restatement
under ITS OWN error bound, counted from the kernel's operations (batch_ref.V: one 2^-24 rounding per fp32 operation the header writes
out, inherited errors propagated) with each library call charged LIB_ULPS ulps.  Raw calls write into guarded buffers
(tests/skinny_ref.py) and the guards must stay intact."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref as R  # noqa: E402
import skinny_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

# Worst error of the device's logf / sqrtf / sincosf against fp64 over all 2^24 inputs the draws can produce, in ulps of the result
# (1 ulp = 2^-23 |result|): tools/batch_floors.py measures them (profiles/input/floors.txt) and the bar charges TWICE the measured
# worst, to cover another library build.  (None: not measured -- the call is then charged batch_ref.ULPS' default, twice the bound HIP's
# math API documents for it.)
LIB_ULPS = {"logf": 1.345914, "sqrtf": 0.5, "sincosf": 1.015133}
for _k, _v in LIB_ULPS.items():
    if _v is not None:
        R.ULPS[_k] = 2.0 * _v


def _recipe(rc):
    from samplenet_amd import BatchRecipe

    return BatchRecipe(**{k: getattr(rc, k) for k in ("order", "shuffle_points", "unit_cube", "scale", "rotate_axis", "perturb", "translate",
                                                       "jitter", "dropout", "pair_noise")})


def assemble(points, labels, rc, B, N, seed=0, position=0, rank=0, world=1, repeat=1, quat=None, layout=0, state=None):
    """One raw call into guarded outputs; synchronises, checks the guards.  -> dict of numpy arrays (p0 / p1 as (B, N, 3))."""
    import ctypes

    from samplenet_amd._lib import check, lib, ptr, stream_of

    L, P, _ = points.shape
    c = _recipe(rc).to_c()
    g = {"p0": S.Guarded(B * N * 3), "labels": S.Guarded(B * 2, torch.int64), "items": S.Guarded(B, torch.int32)}
    if quat is not None:
        g.update(p1=S.Guarded(B * N * 3), igt=S.Guarded(B * 7))
    v = {k: gb.view for k, gb in g.items()}
    check(lib.sn_batch_assemble(B, N, P, L, repeat, ptr(points), ptr(labels), ctypes.addressof(c), seed, rank, world, position,
                                ptr(state), ptr(quat), layout, ptr(v["p0"]), ptr(v.get("p1")), ptr(v["labels"]), ptr(v.get("igt")),
                                ptr(v["items"]), stream_of(points)), "sn_batch_assemble")
    torch.cuda.synchronize()
    for k, gb in g.items():
        assert gb.intact(), "write outside %s (B %d, N %d, P %d)" % (k, B, N, P)
    out = {k: t.cpu().numpy().copy() for k, t in v.items()}
    for k in ("p0", "p1"):
        if k in out:
            out[k] = out[k].reshape(B, 3, N).transpose(0, 2, 1) if layout else out[k].reshape(B, N, 3)
    if "igt" in out:
        out["igt"] = out["igt"].reshape(B, 7)
    return out


def _index_set(L, P):
    """points[l, p] = (l, p, 0): with every float stage off the output NAMES the item and the input point of every slot."""
    pts = torch.zeros(L, P, 3)
    pts[:, :, 0] = torch.arange(L)[:, None].float()
    pts[:, :, 1] = torch.arange(P)[None, :].float()
    return pts.cuda(), (torch.arange(L) * 3 + 1).cuda()


def _check_integers(got, ref, L, what):
    assert np.array_equal(got["items"], ref["items"]), what
    assert np.array_equal(got["labels"], ref["labels"]), what
    assert np.array_equal(got["p0"][:, :, 0], np.broadcast_to((ref["items"] % L)[:, None], ref["order"].shape)), what
    assert np.array_equal(got["p0"][:, :, 1], ref["order"]), what
    assert not got["p0"][:, :, 2].any(), what


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 256, 257, 1000, 2048])
def test_items_labels_and_point_order_bit_for_bit(N):
    """A single wave, one over a wave, one over the workgroup, non-powers of two and the sort's limit, at P = N and P = 2048, for
    B = 1, 3, 32; L = 7 so that B = 32 crosses four epoch ends."""
    L = 7
    rc = R.Recipe(shuffle_points=True)
    for P in sorted({N, 2048}):
        pts, labels = _index_set(L, P)
        for B in (1, 3, 32):
            got = assemble(pts, labels, rc, B, N, seed=21 + B, position=5)
            ref = R.batch(pts.cpu().numpy(), labels.cpu().numpy(), rc, B, N, seed=21 + B, position=5)
            _check_integers(got, ref, L, (N, P, B))


def test_epoch_ends_inside_a_batch_repeat_and_sequential():
    pts, labels = _index_set(5, 16)
    pn, ln = pts.cpu().numpy(), labels.cpu().numpy()
    rc = R.Recipe(shuffle_points=True)
    seen = []
    for step in range(4):  # Lset = 5, B = 3: positions 0..11, epoch ends inside the second and the fourth batch
        got = assemble(pts, labels, rc, 3, 9, seed=4, position=3 * step)
        _check_integers(got, R.batch(pn, ln, rc, 3, 9, seed=4, position=3 * step), 5, step)
        seen += got["items"].tolist()
    assert sorted(seen[:5]) == sorted(seen[5:10]) == list(range(5)) and seen[:5] != seen[5:10]
    quat = torch.from_numpy(R.fixed_pair_quaternions(10)).cuda()
    got = assemble(pts, labels, rc, 32, 9, seed=4, position=2, repeat=2, quat=quat)  # repeat = 2: Lset = 10, cloud = item mod 5
    ref = R.batch(pn, ln, rc, 32, 9, seed=4, position=2, repeat=2, pair_quat=quat.cpu().numpy())
    _check_integers(got, ref, 5, "repeat")
    assert got["items"].max() >= 5 and np.array_equal(got["igt"], ref["igt"])
    seq = R.Recipe(order="sequential")
    got = assemble(pts, labels, seq, 32, 16, seed=4, position=3)
    assert got["items"].tolist() == [(3 + b) % 5 for b in range(32)]
    _check_integers(got, R.batch(pn, ln, seq, 32, 16, seed=4, position=3), 5, "sequential")  # (order: the identity)
    big = torch.zeros(1, 3000, 3, device="cuda")  # without the shuffle any N <= P is served
    big[0, :, 1] = torch.arange(3000, device="cuda").float()
    got = assemble(big, labels[:1], seq, 2, 3000)
    assert np.array_equal(got["p0"][:, :, 1], np.broadcast_to(np.arange(3000.0), (2, 3000)))


STAGES = {
    "unit_cube": dict(unit_cube=True),
    "scale": dict(scale=(0.8, 1.25)),
    "rotate": dict(rotate_axis=(1.0, 2.0, 3.0)),
    "perturb": dict(perturb=(0.06, 0.18)),
    "translate": dict(translate=0.1),
    "jitter": dict(jitter=(0.01, 0.05)),
    "dropout": dict(dropout=0.875),
    "pair": dict(pair_noise=0.04),
    "all": dict(shuffle_points=True, unit_cube=True, scale=(0.8, 1.25), rotate_axis=(0.0, 1.0, 0.0), perturb=(0.06, 0.18), translate=0.1,
                jitter=(0.01, 0.05), dropout=0.875, pair_noise=0.04),
}


@pytest.fixture(scope="module")
def real_set():
    g = torch.Generator().manual_seed(8)
    pts = torch.randn(3, 1003, 3, generator=g) * torch.tensor([1.0, 0.4, 2.5]) + torch.tensor([0.5, -2.0, 0.1])
    return pts.cuda(), torch.tensor([4, 0, 39]).cuda(), torch.from_numpy(R.fixed_pair_quaternions(3, seed=1)).cuda()


def _check_floats(got, ref, what):
    worst = 0.0
    for k in ("p0", "p1"):
        if k not in ref:
            continue
        err, bound = np.abs(got[k].astype(np.float64) - ref[k]), ref[k + "_err"]
        ratio = err / np.maximum(bound, 1e-300)  # (a stage without arithmetic has a zero bound: the result is then exact)
        worst = max(worst, float(ratio.max()))
        assert np.all(err <= bound), (what, k, float(ratio.max()), float(err.max()))
    print("batch %s: worst error / bound %.3f" % (what, worst))


@pytest.mark.parametrize("N", [65, 1000])
@pytest.mark.parametrize("stage", list(STAGES))
def test_float_stages_element_by_element(real_set, stage, N):
    pts, labels, quat = real_set
    rc = R.Recipe(**STAGES[stage])
    q = quat if stage in ("pair", "all") else None
    got = assemble(pts, labels, rc, 2, N, seed=77, position=1, quat=q)
    ref = R.batch(pts.cpu().numpy(), labels.cpu().numpy(), rc, 2, N, seed=77, position=1, pair_quat=None if q is None else q.cpu().numpy())
    assert np.array_equal(got["items"], ref["items"]) and np.array_equal(got["labels"], ref["labels"])
    _check_floats(got, ref, (stage, N))
    if rc.dropout is not None:  # the choice of points is exact: a dropped point carries point 0's bits, the others (almost surely) do not
        same = (got["p0"] == got["p0"][:, :1, :]).all(-1)
        assert ref["dropped"].any() and np.array_equal(same | ref["dropped"], same) and (same & ~ref["dropped"])[:, 1:].sum() == 0


def test_clips_are_exact_and_bcn_layout(real_set):
    pts, labels, _ = real_set
    zero = torch.zeros_like(pts)
    got = assemble(zero, labels, R.Recipe(jitter=(1.0, 0.05)), 2, 1000, seed=3)  # std 1: ~96 % of the offsets sit on the clip
    clip = float(np.float32(0.05))
    assert np.abs(got["p0"]).max() == clip and (np.abs(got["p0"]) == clip).mean() > 0.9
    # sigma 1e6: every angle is +-clip exactly, so the cloud is one of the eight Rz Ry Rx of (+-clip)^3 applied to it
    rc = R.Recipe(perturb=(1e6, 0.18))
    got = assemble(pts, labels, rc, 2, 65, seed=3)
    ref = R.batch(pts.cpu().numpy(), labels.cpu().numpy(), rc, 2, 65, seed=3)
    for b, item in enumerate(ref["items"]):
        ang = R.cloud(pts[item].cpu().numpy(), int(item), 0, rc, 65, 3)["angles"]
        assert all(abs(float(a.v)) == float(np.float32(0.18)) and float(a.e) == 0.0 for a in ang)
    _check_floats(got, ref, "perturbation on the clip")
    # ... and the KERNEL's own angles, exactly.  Every cloud is (e_x, e_y, e_z): products with 1 and sums with 0 are exact, so with
    # S = sinf(+-a), C = cosf(+-a) of the cloud's angles about x, y, z the three plane rotations leave
    #   e_x -> (C_z C_y, S_z C_y, -S_y)      e_y -> (., ., C_y S_x)      e_z -> (., ., C_y C_x)         (one fp32 product each).
    # sinf is odd and cosf even bit for bit, so angles that are +-clip EXACTLY give |S| and C one bit pattern each over all clouds and
    # all three axes, and the signs are those of the restatement's draws; any angle off the clip by one ulp would show as another
    # pattern (sinf' = 0.98 at 0.18: one ulp of the angle moves S by an ulp).
    L = 8
    eye = torch.eye(3).repeat(L, 1, 1).cuda()
    rc = R.Recipe(order="sequential", perturb=(1e6, 0.18))
    got = assemble(eye, torch.arange(L).cuda(), rc, L, 3, seed=3)["p0"]
    bits = np.abs(got).view(np.int32)
    assert len(np.unique(bits[:, 0, 2])) == 1                                        # |S_y|
    assert len(np.unique(np.stack([bits[:, 0, 1], bits[:, 1, 2]]))) == 1             # |S_z| C_y = C_y |S_x|
    assert len(np.unique(np.stack([bits[:, 0, 0], bits[:, 2, 2]]))) == 1             # C_z C_y = C_y C_x
    sign = np.array([[np.sign(float(a.v)) for a in R.cloud(np.eye(3, dtype=np.float32), i, 0, rc, 3, 3)["angles"]] for i in range(L)])
    assert np.array_equal(np.sign(got[:, 0, 2]), -sign[:, 1]) and np.array_equal(np.sign(got[:, 0, 1]), sign[:, 2])
    assert np.array_equal(np.sign(got[:, 1, 2]), sign[:, 0]) and len(np.unique(sign[:, 1])) == 2
    # the one pattern is sinf / cosf of the fp32 clip: the library's allowance on S, two allowances and one rounding on the products
    a, lib = float(np.float32(0.18)), R.ULPS["sincosf"] * 2 * R.U
    assert abs(abs(float(got[0, 0, 2])) - np.sin(a)) <= lib * np.sin(a)
    assert abs(float(got[0, 0, 0]) - np.cos(a) ** 2) <= (2 * lib + lib * lib + R.U) * 1.001 * np.cos(a) ** 2
    assert abs(abs(float(got[0, 0, 1])) - np.sin(a) * np.cos(a)) <= (2 * lib + lib * lib + R.U) * 1.001 * np.sin(a) * np.cos(a)
    rc = R.Recipe(**STAGES["all"])
    a = assemble(pts, labels, rc, 3, 257, seed=5, layout=0)
    b = assemble(pts, labels, rc, 3, 257, seed=5, layout=1)  # (assemble() transposes the BCN result back)
    assert np.array_equal(a["p0"].view(np.int32), b["p0"].view(np.int32))


def _source(real_set, B, N=65, **kw):
    from samplenet_amd import BatchRecipe, DeviceBatchSource, DeviceCloudSet

    pts, labels, _ = real_set
    kw.setdefault("pair", "fixed")
    kw.setdefault("seed", 13)
    return DeviceBatchSource(DeviceCloudSet(pts, labels), BatchRecipe(**STAGES["all"]), B, N, **kw)


def test_cloudset_from_dataset(real_set):
    """from_dataset on the package's two dataset classes: the resident arrays, and a batch drawn from them."""
    from samplenet_amd import BatchRecipe, DeviceBatchSource, DeviceCloudSet
    from samplenet_amd.data import ModelNetCls, PointCloudDataSet

    pts = real_set[0].cpu().numpy()
    named = DeviceCloudSet.from_dataset(PointCloudDataSet(pts, labels=np.array(["a_0", "a_1", "b_0"]), init_shuffle=False))
    assert named.points.dtype == torch.float32 and named.labels.dtype == torch.int64 and named.device.type == "cuda"
    assert torch.equal(named.points, real_set[0]) and named.labels.tolist() == [0, 1, 2] and len(named) == 3
    numbered = DeviceCloudSet.from_dataset(PointCloudDataSet(pts.astype(np.float64), labels=np.array([4, 0, 39]), init_shuffle=False))
    assert torch.equal(numbered.points, real_set[0]) and numbered.labels.tolist() == [4, 0, 39]
    mn = ModelNetCls.__new__(ModelNetCls)  # (no shards on disk: the two arrays the loader leaves)
    mn.points, mn.labels = pts, np.array([[4], [0], [39]], dtype=np.uint8)
    resident = DeviceCloudSet.from_dataset(mn)
    assert torch.equal(resident.points, real_set[0]) and torch.equal(resident.labels, real_set[1])
    rc = BatchRecipe(order="sequential", unit_cube=True)
    a, b = DeviceBatchSource(resident, rc, 3, 65).at(0), DeviceBatchSource(DeviceCloudSet(*real_set[:2]), rc, 3, 65).at(0)
    assert torch.equal(a.p0.view(torch.int32), b.p0.view(torch.int32)) and a.labels.tolist() == b.labels.tolist() == [4, 0, 39]
    with pytest.raises(TypeError):
        DeviceCloudSet.from_dataset(pts)
    with pytest.raises(RuntimeError, match="GPU only"):
        DeviceCloudSet.from_dataset(mn, device="cpu")


def _same_batch(a, b, what=""):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), what


def _cat(*batches):
    return [torch.cat(ts) for ts in zip(*batches)]


def test_independence_of_batch_shape_rank_and_source(real_set):
    four = _source(real_set, 4).at(2)
    two = _source(real_set, 2)
    _same_batch(four, _cat(two.at(2), two.at(4)), "B = 4 against 2 x B = 2")
    r0, r1 = _source(real_set, 2, rank=0, world=2), _source(real_set, 2, rank=1, world=2)
    _same_batch(four, _cat(r0.at(2), r1.at(2)), "two ranks against one")
    _same_batch(_source(real_set, 4).at(2), four, "same seed, another source")
    assert not torch.equal(_source(real_set, 4, seed=14).at(2).p0, four.p0)


def test_state_block_advances_by_itself_also_under_graph_replay(real_set):
    src, B = _source(real_set, 3), 3
    want = [src.at(i * B) for i in range(3)]
    assert src.position == 0
    for i in range(3):
        _same_batch(src.next(), want[i], "launch %d" % i)
    assert src.position == 3 * B and src.epoch == 3  # (Lset = 3)
    # two ranks advance by B * world
    r1 = _source(real_set, 3, rank=1, world=2)
    r1.next()
    assert r1.position == 2 * B
    # the same launch captured once and replayed three times (one stream)
    src = _source(real_set, 3)
    out = src._alloc()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        src.next_into(*out)
    assert src.position == 0  # capturing draws nothing
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        _same_batch(out, want[i], "replay %d" % i)
    # resume in the middle of an epoch
    state = src.state_dict()
    assert state == {"seed": 13, "position": 9}
    other = _source(real_set, 3, seed=99)
    other.load_state_dict({"seed": 13, "position": 4})
    _same_batch(other.next(), src.at(4), "resumed")
    assert other.position == 7


# ---- the engine --------------------------------------------------------------------------------------------------------------------
EB, EN, EM = 4, 64, 8


def _engine_set():
    g = torch.Generator().manual_seed(2)
    return (torch.rand(5, 80, 3, generator=g) - 0.5).cuda(), torch.arange(5).cuda()


def _nets(n):
    from samplenet_amd import SampleNet

    torch.manual_seed(0)
    mk = lambda: SampleNet(EM, 128, group_size=4, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()  # noqa: E731
    nets = [mk()]
    sd = copy.deepcopy(nets[0].state_dict())
    for _ in range(n - 1):
        nets.append(mk())
        nets[-1].load_state_dict(sd)
    return nets


def test_engine_input_source_equals_feeding_the_same_batches():
    """B = 4, N = 64 -> M = 8, Lset = 5, three steps, optimizer= set.  (a) input_source= captured as the first node of the step's graph;
    (b) the same batches made by at() and fed to __call__(x).  The existing engine tests hold captured against eager bit for bit
    (tests/test_gpu_samplenet.py::test_graphed_step_equals_eager_step): inputs, losses, gradients and parameters here likewise."""
    from samplenet_amd import BatchRecipe, DeviceBatchSource, DeviceCloudSet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.optim import Adam
    from samplenet_amd.parallel import FlatGradAllReducer

    pts, labels = _engine_set()
    rc = BatchRecipe(shuffle_points=True, unit_cube=True, jitter=(0.01, 0.05))
    mk = lambda: DeviceBatchSource(DeviceCloudSet(pts, labels), rc, EB, EN, seed=6)  # noqa: E731
    src, twin = mk(), mk()
    na, nb = _nets(2)
    ra, rb = FlatGradAllReducer(na), FlatGradAllReducer(nb)
    oa, ob = Adam(na.parameters(), lr=1e-3), Adam(nb.parameters(), lr=1e-3)
    x0 = twin.at(0).p0
    sa = SamplerTrainStep(na, x0, reducer=ra, optimizer=oa, input_source=src)
    sb = SamplerTrainStep(nb, x0, reducer=rb, optimizer=ob)
    assert src.position == 0 and len(sa._ring_graphs[0]) == 1  # construction draws nothing; one graph carries launch, step and update
    with pytest.raises(RuntimeError):
        sa(x0)
    with pytest.raises(RuntimeError):
        sb.step()
    for i in range(3):
        x = twin.at(i * EB).p0
        la, lb = sa.step(), sb(x)
        torch.cuda.synchronize()
        assert torch.equal(sa.x.view(torch.int32), x.view(torch.int32)), i
        assert float(la) == float(lb), i
        assert torch.equal(ra.flat, rb.flat), i
        for p, q in zip(na.parameters(), nb.parameters()):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), i
    assert src.position == 3 * EB and oa._dev[0].step_count() == 3
    # eager: the launch is issued in front of the step
    nc = _nets(1)[0]
    sc = SamplerTrainStep(nc, x0, reducer=FlatGradAllReducer(nc), use_graph=False, input_source=mk())
    sc.step()
    torch.cuda.synchronize()
    assert torch.equal(sc.x, x0) and sc.source.position == EB
    with pytest.raises(ValueError):
        SamplerTrainStep(nc, x0, input_ring=[x0.clone(), x0.clone()], input_source=mk(), reducer=FlatGradAllReducer(nc))


def test_engine_pair_source_drives_the_pcrnet_task_loss():
    from samplenet_amd import BatchRecipe, DeviceBatchSource, DeviceCloudSet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer
    from samplenet_amd.task_features import PCRNet, pcrnet_chamfer_loss

    pts, labels = _engine_set()
    rc = BatchRecipe(shuffle_points=True, unit_cube=True)
    mk = lambda: DeviceBatchSource(DeviceCloudSet(pts, labels), rc, EB, EN, seed=6, pair="fixed")  # noqa: E731
    want = mk().at(0)
    torch.manual_seed(1)
    pcr = PCRNet(bottleneck_size=256, input_shape="bnc").cuda().eval()
    for p in pcr.parameters():
        p.requires_grad_(False)
    task = lambda proj, p1: pcrnet_chamfer_loss(pcr, proj, p1)[0]  # noqa: E731  (template = the sampled cloud, source = p1)
    na, nb = _nets(2)
    ra, rb = FlatGradAllReducer(na), FlatGradAllReducer(nb)
    sa = SamplerTrainStep(na, want.p0, reducer=ra, task_loss=task, use_graph=False, input_source=mk())
    sb = SamplerTrainStep(nb, want.p0, reducer=rb, task_loss=lambda proj: task(proj, want.p1), use_graph=False)
    la, lb = sa.step(), sb(want.p0)
    torch.cuda.synchronize()
    assert torch.equal(sa.x1.view(torch.int32), want.p1.view(torch.int32))
    assert float(la) == float(lb) and torch.isfinite(la) and torch.equal(ra.flat, rb.flat) and float(ra.flat.abs().sum()) > 0
    # captured: the launch fills x and x1 inside the graph, and the wrapped task loss reads the static x1 under replay -- two steps on
    # different batches against the captured step fed the same p0 by __call__ and the same p1 through a static tensor of its own
    nc, nd = _nets(2)
    rc_, rd = FlatGradAllReducer(nc), FlatGradAllReducer(nd)
    src, p1 = mk(), want.p1.clone()
    sc = SamplerTrainStep(nc, want.p0, reducer=rc_, task_loss=task, input_source=src)
    sd = SamplerTrainStep(nd, want.p0, reducer=rd, task_loss=lambda proj: task(proj, p1))
    assert src.position == 0 and len(sc._ring_graphs[0]) == 1
    seen = []
    for i in range(2):
        batch = mk().at(i * EB)
        p1.copy_(batch.p1)
        lc, ld = sc.step(), sd(batch.p0)
        torch.cuda.synchronize()
        assert torch.equal(sc.x.view(torch.int32), batch.p0.view(torch.int32)), i
        assert torch.equal(sc.x1.view(torch.int32), batch.p1.view(torch.int32)), i
        assert float(lc) == float(ld) and torch.isfinite(lc) and torch.equal(rc_.flat, rd.flat), i
        seen.append(float(lc))
    assert src.position == 2 * EB and seen[0] != seen[1]

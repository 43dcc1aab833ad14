"""Host-side checks of the device batch assembly (no GPU): the numpy restatement tests/batch_ref.py against published Philox vectors
and against the reference's own transforms (tests/golden/batch_reference.npz, written by tests/golden/make_batch_golden.py), the
item bijection, BatchRecipe.from_transforms, and sn_batch_assemble's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "batch_reference.npz"))


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    """The three vectors published with Random123 (kat_vectors: philox4x32 10)."""
    assert _hex(R.philox(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(R.philox(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(R.philox(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over the index, and the key split of a 64-bit seed
    a = R.draw(np.arange(4), 1, 7, 2, (0x299F31D0 << 32) | 0xA4093822)
    b = [R.philox(i, 1, 7, 2, 0xA4093822, 0x299F31D0) for i in range(4)]
    assert all(int(a[w][i]) == int(b[i][w]) for i in range(4) for w in range(4))


@pytest.mark.parametrize("lset", [1, 2, 3, 5, 37, 64, 65, 1025])
def test_item_order_is_a_permutation_per_epoch(lset):
    k = R.feistel_bits(lset)
    assert k % 2 == 0 and k >= 2 and (1 << k) >= lset and (k == 2 or (1 << (k - 2)) < lset)
    orders = []
    for epoch in range(4):
        got = [R.perm(11, epoch, x, lset) for x in range(lset)]
        assert sorted(i for i, _ in got) == list(range(lset)), (lset, epoch)
        assert max(s for _, s in got) <= (1 << k) - lset + 1  # the cycle walk's bound (header)
        orders.append([i for i, _ in got])
    if lset >= 37:  # (short sets have few permutations: epochs may coincide there)
        assert len({tuple(o) for o in orders}) == 4
        assert orders[0] != [R.perm(12, 0, x, lset)[0] for x in range(lset)]  # another seed, another order
    # positions run across epoch ends; sequential order counts up
    assert [R.item_at(11, g, lset)[1] for g in (0, lset - 1, lset, 3 * lset + 0)] == [0, 0, 1, 3]
    assert [R.item_at(11, g, lset, sequential=True)[0] for g in range(2 * lset)] == list(range(lset)) * 2


class PointcloudToTensor:
    pass


class OnUnitCube:
    pass


class PointcloudScale:
    lo, hi = 0.8, 1.25


class PointcloudRotate:
    axis = np.array([0.0, 1.0, 0.0])


class PointcloudRotatePerturbation:
    angle_sigma, angle_clip = 0.06, 0.18


class PointcloudTranslate:
    translate_range = 0.1


class PointcloudJitter:
    std, clip = 0.01, 0.05


class PointcloudRandomInputDropout:
    max_dropout_ratio = 0.875


class PointcloudFlip:
    pass


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms


def test_from_transforms():
    from samplenet_amd import BatchRecipe

    r = BatchRecipe.from_transforms(Compose([PointcloudToTensor(), OnUnitCube()]), shuffle_points=True)
    assert r == BatchRecipe(shuffle_points=True, unit_cube=True)
    full = [PointcloudToTensor(), PointcloudScale(), PointcloudRotate(), PointcloudRotatePerturbation(), PointcloudTranslate(),
            PointcloudJitter(), PointcloudRandomInputDropout()]
    r = BatchRecipe.from_transforms(full)
    assert r == BatchRecipe(scale=(0.8, 1.25), rotate_axis=(0.0, 1.0, 0.0), perturb=(0.06, 0.18), translate=0.1, jitter=(0.01, 0.05),
                            dropout=0.875)
    c = r.to_c()
    assert (c.scale, c.rotate, c.perturb, c.translate, c.jitter, c.dropout, c.unit_cube, c.pair_noise, c.order) == (1, 1, 1, 1, 1, 1, 0, 0, 0)
    assert (c.scale_lo, c.dropout_max, tuple(c.axis)) == (np.float32(0.8), np.float32(0.875), (0.0, 1.0, 0.0))
    with pytest.raises(ValueError, match="PointcloudFlip"):
        BatchRecipe.from_transforms([PointcloudToTensor(), PointcloudFlip()])
    with pytest.raises(ValueError, match="PointcloudScale after PointcloudJitter"):
        BatchRecipe.from_transforms([PointcloudJitter(), PointcloudScale()])
    with pytest.raises(ValueError, match="PointcloudJitter after PointcloudJitter"):
        BatchRecipe.from_transforms([PointcloudJitter(), PointcloudJitter()])
    with pytest.raises(ValueError):
        BatchRecipe(order="random").to_c()


def test_argument_errors_are_reported_without_a_gpu():
    from samplenet_amd import BatchRecipe
    from samplenet_amd._lib import lib

    BAD, UNSUPPORTED, p = 10001, 10002, ctypes.c_void_p(64)
    assert lib.sn_batch_state_bytes() == 64

    def call(B=2, N=8, P=16, L=4, repeat=1, points=p, labels=p, recipe=BatchRecipe(), rank=0, world=1, position=0, state=None,
             quat=None, layout=0, p0=p, p1=None, out_labels=None, igt=None, items=None):
        c = recipe.to_c() if recipe is not None else None
        return lib.sn_batch_assemble(B, N, P, L, repeat, points, labels, ctypes.byref(c) if c is not None else None, 5, rank, world,
                                     position, state, quat, layout, p0, p1, out_labels, igt, items, None)

    assert call(B=-1) == BAD and b"negative" in lib.sn_last_error_string()
    assert call(N=-1) == BAD and call(P=-1) == BAD and call(L=-1) == BAD and call(repeat=0) == BAD
    assert call(N=17) == BAD and b"N > P" in lib.sn_last_error_string()
    assert call(rank=1, world=1) == BAD and call(rank=-1) == BAD and call(rank=2, world=2) == BAD
    assert call(recipe=BatchRecipe(scale=(1.5, 0.5))) == BAD and b"scale_lo > scale_hi" in lib.sn_last_error_string()
    assert call(recipe=None) == BAD and call(points=None) == BAD and call(p0=None) == BAD
    assert call(position=-1, state=None) == BAD          # the self-advancing form needs the block
    assert call(p1=p) == BAD and call(igt=p) == BAD      # no quaternion table
    assert call(out_labels=p, labels=None) == BAD
    assert call(layout=2) == BAD and call(L=0) == BAD
    assert call(recipe=BatchRecipe(dropout=1.0)) == BAD and call(recipe=BatchRecipe(jitter=(-1.0, 0.1))) == BAD
    assert call(recipe=BatchRecipe(rotate_axis=(0.0, 0.0, 0.0))) == BAD
    assert call(N=2049, P=4096, recipe=BatchRecipe(shuffle_points=True)) == UNSUPPORTED
    assert call(B=0, points=None, p0=None) == 0          # empty batch: a no-op whatever the pointers
    assert call(B=0, N=17) == BAD                        # ... but sizes are still checked


def _f32_close(got, want, ulps=1.0, floor=0.0):
    """|got - want| <= ulps 2^-24 max(|want|, floor): `want` is an fp64 result rounded to fp32 (half an ulp = 2^-24 relative), `got`
    the restatement's fp64 value."""
    return np.all(np.abs(got - want.astype(np.float64)) <= ulps * U * np.maximum(np.abs(want), floor) + 1e-300)


def test_restatement_agrees_with_the_reference(gold):
    """unit_cube, the axis matrix, the perturbation matrix, qrot and the pair table against what the reference's own code gave.  The
    reference computes each in fp64 and casts to fp32, so the bar is one fp32 rounding of the (fp64) restatement's value: 2^-24 of
    the element itself wherever restatement and reference evaluate the same fp64 expression."""
    for c, want in zip(gold["clouds"], gold["unit_cube"]):
        got = R.unit_cube(R.V(c.astype(np.float64))).v
        assert _f32_close(got, want), np.abs(got - want).max()
    assert tuple(gold["axes"][0]) == (0.0, 1.0, 0.0)
    for axis, mats in zip(gold["axes"], gold["axis_R"]):
        exact_axis = tuple(axis) == (0.0, 1.0, 0.0)
        for ang, want in zip(gold["angles"], mats):
            M = R.axis_matrix(axis, R.V(np.sin(ang)), R.V(np.cos(ang)))
            got = np.array([[float(M[i][j].v) for j in range(3)] for i in range(3)])
            if exact_axis:  # the unit axis is exact in fp32: the same fp64 expression, one cast -- 2^-24 of each entry
                assert _f32_close(got, want), (axis, ang, np.abs(got - want).max())
                continue
            # (1, 2, 3): the restatement rounds the unit axis to fp32 as the kernel's host side does: a relative 2^-24 on each a_i,
            # so at most 2 x 2^-24 of (1 - c) a_i a_j <= 2 on the diagonal, 2^-24 (s a_k) + 2 x 2^-24 (|a_i a_j| <= 1/2) beside it:
            # 4 x 2^-24; plus the fixture's own cast of entries <= 1
            assert _f32_close(got, want, ulps=5.0, floor=1.0), (axis, ang, np.abs(got - want).max())
    for ang, want in zip(gold["perturb_angles"], gold["perturb_R"]):
        # the fixture multiplies the reference's three fp32-rounded elementary matrices in fp64: each factor is off by 2^-24 of its
        # entries, and the absolute row sums of the other two factors' product are at most 2: 3 x 2 x 2^-24
        assert np.abs(R.perturb_matrix(ang) - want).max() <= 6 * U
    for seed in (0, 1):
        want = gold["quat_seed%d" % seed]
        got = R.fixed_pair_quaternions(len(want), seed=seed)
        assert got.dtype == np.float32 and np.array_equal(got, want), seed  # same fp64 expression, same cast
    out = R.qrot(gold["qrot_q"], R.V(gold["clouds"][0].astype(np.float64))).v
    assert _f32_close(out, gold["qrot_out"], floor=np.abs(gold["clouds"][0]).max() * 3)


class _Recorder:
    """Stands in for the class in DeviceCloudSet.from_dataset: records what the constructor would be given."""

    def __init__(self, points, labels=None, device="cuda"):
        self.points, self.labels, self.device = points, labels, device


def test_from_dataset_selects_the_arrays():
    """Which arrays from_dataset hands to the constructor (the constructor itself needs the GPU: tests/test_gpu_batch_assemble.py)."""
    from samplenet_amd.data import ModelNetCls, PointCloudDataSet
    from samplenet_amd.device_data import DeviceCloudSet

    build = DeviceCloudSet.from_dataset.__func__
    pts = np.arange(3 * 4 * 3, dtype=np.float32).reshape(3, 4, 3)
    got = build(_Recorder, PointCloudDataSet(pts, labels=np.array([7, 5, 9]), init_shuffle=False), "cuda:0")
    assert np.array_equal(got.points, pts) and got.labels.tolist() == [7, 5, 9] and got.device == "cuda:0"
    got = build(_Recorder, PointCloudDataSet(pts, labels=np.array(["a_1", "a_2", "b_1"]), init_shuffle=False))
    assert np.array_equal(got.points, pts) and got.labels is None  # string labels: the constructor numbers the clouds
    got = build(_Recorder, PointCloudDataSet(pts, labels=np.array([0.5, 1.5, 2.5]), init_shuffle=False))
    assert got.labels is None                                      # ... and so do labels that are not integers
    mn = ModelNetCls.__new__(ModelNetCls)                          # (no shards on disk: the two arrays the loader leaves)
    mn.points, mn.labels = pts, np.array([[3], [1], [2]], dtype=np.uint8)
    got = build(_Recorder, mn)
    assert got.points is pts and got.labels.shape == (3,) and got.labels.tolist() == [3, 1, 2] and got.device == "cuda"
    with pytest.raises(TypeError, match="list"):
        build(_Recorder, [pts])


class _FakeSet:
    """What DeviceBatchSource.__init__ reads of a DeviceCloudSet before it touches the device."""

    class points:
        shape = (4, 4096, 3)

    device = "cuda"

    def __len__(self):
        return 4


def test_source_arguments_are_checked_before_the_device():
    from samplenet_amd import BatchRecipe, DeviceBatchSource
    from samplenet_amd.device_data import MAX_SHUFFLE_POINTS

    assert MAX_SHUFFLE_POINTS == 2048
    with pytest.raises(ValueError, match="at most 2048 points"):
        DeviceBatchSource(_FakeSet(), BatchRecipe(shuffle_points=True), 2, 2049)
    with pytest.raises(ValueError, match="4097 > the 4096 points"):
        DeviceBatchSource(_FakeSet(), BatchRecipe(), 2, 4097)
    with pytest.raises(ValueError, match="rank"):
        DeviceBatchSource(_FakeSet(), BatchRecipe(), 2, 8, rank=1, world=1)
    with pytest.raises(ValueError, match="layout"):
        DeviceBatchSource(_FakeSet(), BatchRecipe(), 2, 8, layout="cbn")
    with pytest.raises(ValueError, match="pair"):
        DeviceBatchSource(_FakeSet(), BatchRecipe(), 2, 8, pair="random")


def test_package_pair_table_equals_the_restatement():
    from samplenet_amd.device_data import fixed_pair_quaternions

    for seed in (0, 1):
        assert np.array_equal(fixed_pair_quaternions(9, seed=seed), R.fixed_pair_quaternions(9, seed=seed))


def test_restatement_is_self_consistent():
    """The draw layout's invariants, on the restatement alone: a cloud does not depend on the batch shape or the rank; the point
    order is a permutation; dropped points equal point 0; clips hold; error bounds are finite and small."""
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((5, 80, 3)).astype(np.float32)
    labels = np.arange(5) * 10
    rc = R.Recipe(shuffle_points=True, unit_cube=True, scale=(0.8, 1.25), rotate_axis=(0, 1, 0), perturb=(0.06, 0.18), translate=0.1,
                  jitter=(0.01, 0.05), dropout=0.875)
    quat = R.fixed_pair_quaternions(10)
    a = R.batch(pts, labels, rc, 4, 65, seed=9, position=3, repeat=2, pair_quat=quat)
    b0 = R.batch(pts, labels, rc, 2, 65, seed=9, position=3, repeat=2, pair_quat=quat)
    b1 = R.batch(pts, labels, rc, 2, 65, seed=9, position=3, repeat=2, pair_quat=quat, rank=1, world=2)
    for k in ("items", "labels", "order", "p0", "p1", "igt"):
        assert np.array_equal(a[k], np.concatenate([b0[k], b1[k]])), k
    assert all(sorted(o) == list(range(65)) for o in a["order"])
    assert np.array_equal(a["labels"], labels[a["items"] % 5])
    assert a["dropped"].any() and all(np.array_equal(p[d], np.tile(p[0], (d.sum(), 1))) for p, d in zip(a["p0"], a["dropped"]))
    assert np.isfinite(a["p0_err"]).all() and a["p0_err"].max() < 1e-4 and a["p1_err"].max() < 1e-4
    j = R.cloud(np.zeros((80, 3), np.float32), 1, 0, R.Recipe(jitter=(1.0, 0.05)), 80, 9)["p0"].v
    assert np.abs(j).max() == float(np.float32(0.05))

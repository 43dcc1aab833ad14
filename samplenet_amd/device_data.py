"""Training batches assembled on the device from an HBM-resident dataset (csrc/batch_assemble.hip: sn_batch_assemble).

The reference feeds its training loops from a torch DataLoader whose items are made one by one on the host: ModelNetCls.__getitem__
(registration/data/modelnet_loader_torch.py:114-125: a permutation of the points, a fancy-index copy, the Python transform chain of
src/pctransforms.py) and QuaternionFixedDataset (src/qdataset.py:133-179: a fixed rotation per item).  ModelNet40's whole training
split is 9840 x 2048 x 3 floats = 242 MB: it lives in HBM here, and a batch is ONE kernel launch driven by a counter-based random
generator -- the first node of the captured training step (engine.SamplerTrainStep(input_source=)), the way the Adam update is its
last.  A script swaps

    loader = DataLoader(QuaternionFixedDataset(ModelNetCls(1024, Compose([PointcloudToTensor(), OnUnitCube()]), train=True)), ...)
for
    source = DeviceBatchSource(DeviceCloudSet.from_dataset(modelnet), BatchRecipe.from_transforms(compose, shuffle_points=True),
                               batch=32, n_points=1024, pair="fixed")

The one difference from a DataLoader: batches run across epoch ends -- every epoch is a fresh permutation of the items, and there is
no "last partial batch".  A cloud's content depends on (seed, epoch, item, dataset, recipe) alone: not on the batch size, the slot,
the rank or the step.  The contract (item order, draw layout, stages) is written out in include/samplenet_hip_internal.h.

GPU only: there is no CPU fallback.
"""
import collections
import ctypes
import dataclasses
import math

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_of

_STATE_WORDS = lib.sn_batch_state_bytes() // 8
MAX_SHUFFLE_POINTS = 2048  # csrc/batch_assemble.hip: kMaxSort

Batch = collections.namedtuple("Batch", "p0 p1 labels igt items")


class _CRecipe(ctypes.Structure):  # include/samplenet_hip_internal.h: sn_batch_recipe
    _fields_ = [("order", ctypes.c_int), ("shuffle_points", ctypes.c_int), ("unit_cube", ctypes.c_int), ("scale", ctypes.c_int),
                ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float), ("rotate", ctypes.c_int), ("axis", ctypes.c_float * 3),
                ("perturb", ctypes.c_int), ("perturb_sigma", ctypes.c_float), ("perturb_clip", ctypes.c_float),
                ("translate", ctypes.c_int), ("translate_range", ctypes.c_float), ("jitter", ctypes.c_int),
                ("jitter_std", ctypes.c_float), ("jitter_clip", ctypes.c_float), ("dropout", ctypes.c_int),
                ("dropout_max", ctypes.c_float), ("pair_noise", ctypes.c_int), ("pair_noise_std", ctypes.c_float)]


# stage of the fixed pipeline each reference transform maps to (None: nothing to do on the device)
_STAGE = {"PointcloudToTensor": None, "OnUnitCube": 2, "PointcloudScale": 3, "PointcloudRotate": 4, "PointcloudRotatePerturbation": 5,
          "PointcloudTranslate": 6, "PointcloudJitter": 7, "PointcloudRandomInputDropout": 8}


@dataclasses.dataclass
class BatchRecipe:
    """The stages of the assembly as plain fields, in the pipeline's fixed order; None / False switches a stage off.
        order           "shuffled" (a fresh permutation of the items per epoch) or "sequential" (evaluation)
        shuffle_points  a random order of the cloud's first n_points points (ModelNetCls.__getitem__), n_points <= 2048
        unit_cube       OnUnitCube
        scale           (lo, hi)                 PointcloudScale
        rotate_axis     (x, y, z)                PointcloudRotate
        perturb         (angle_sigma, clip)      PointcloudRotatePerturbation
        translate       range                    PointcloudTranslate
        jitter          (std, clip)              PointcloudJitter
        dropout         max ratio                PointcloudRandomInputDropout
        pair_noise      std                      QuaternionFixedDataset(apply_noise=True) uses 0.04"""
    order: str = "shuffled"
    shuffle_points: bool = False
    unit_cube: bool = False
    scale: tuple = None
    rotate_axis: tuple = None
    perturb: tuple = None
    translate: float = None
    jitter: tuple = None
    dropout: float = None
    pair_noise: float = None

    @classmethod
    def from_transforms(cls, seq, **fields):
        """Reads a reference-style transform list (a list, or a Compose with .transforms): each object is recognised by its CLASS
        NAME and its attributes are copied.  ValueError for a transform the pipeline does not have, and for an order it cannot
        honour (the offending pair is named).  fields: the recipe's other fields (order, shuffle_points, pair_noise)."""
        seq = getattr(seq, "transforms", seq)
        rec, last = cls(**fields), None
        for t in seq:
            name = type(t).__name__
            if name not in _STAGE:
                raise ValueError("BatchRecipe.from_transforms: no device stage for transform %s" % name)
            stage = _STAGE[name]
            if stage is None:
                continue
            if last is not None and stage <= last[0]:
                raise ValueError("BatchRecipe.from_transforms: %s after %s -- the pipeline's order is fixed (%s)"
                                 % (name, last[1], " < ".join(n for n, s in sorted(_STAGE.items(), key=lambda kv: kv[1] or 0) if s)))
            last = (stage, name)
            if stage == 2:
                rec.unit_cube = True
            elif stage == 3:
                rec.scale = (float(t.lo), float(t.hi))
            elif stage == 4:
                rec.rotate_axis = tuple(float(a) for a in t.axis)
            elif stage == 5:
                rec.perturb = (float(t.angle_sigma), float(t.angle_clip))
            elif stage == 6:
                rec.translate = float(t.translate_range)
            elif stage == 7:
                rec.jitter = (float(t.std), float(t.clip))
            elif stage == 8:
                rec.dropout = float(t.max_dropout_ratio)
        return rec

    def to_c(self):
        if self.order not in ("shuffled", "sequential"):
            raise ValueError("BatchRecipe.order: 'shuffled' or 'sequential'")
        c = _CRecipe()
        c.order, c.shuffle_points, c.unit_cube = int(self.order == "sequential"), int(bool(self.shuffle_points)), int(bool(self.unit_cube))
        if self.scale is not None:
            c.scale, (c.scale_lo, c.scale_hi) = 1, self.scale
        if self.rotate_axis is not None:
            c.rotate, c.axis = 1, (ctypes.c_float * 3)(*self.rotate_axis)
        if self.perturb is not None:
            c.perturb, (c.perturb_sigma, c.perturb_clip) = 1, self.perturb
        if self.translate is not None:
            c.translate, c.translate_range = 1, self.translate
        if self.jitter is not None:
            c.jitter, (c.jitter_std, c.jitter_clip) = 1, self.jitter
        if self.dropout is not None:
            c.dropout, c.dropout_max = 1, self.dropout
        if self.pair_noise is not None:
            c.pair_noise, c.pair_noise_std = 1, self.pair_noise
        return c


class DeviceCloudSet:
    """The resident arrays: points (L, P, 3) float32 and labels (L,) int64 on `device`."""

    def __init__(self, points, labels=None, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("samplenet_amd.device_data runs on the GPU only (no CPU fallback): device %s" % device)
        points = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32) if isinstance(points, np.ndarray) else points)
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] < 1:
            raise ValueError("points must be (L, P, 3) with L >= 1, got %s" % (tuple(points.shape),))
        self.points = points.to(device=device, dtype=torch.float32).contiguous()
        if labels is None:
            labels = torch.arange(points.shape[0])
        labels = torch.as_tensor(np.asarray(labels).reshape(-1) if not isinstance(labels, torch.Tensor) else labels.reshape(-1))
        if labels.numel() != points.shape[0]:
            raise ValueError("%d labels for %d clouds" % (labels.numel(), points.shape[0]))
        self.labels = labels.to(device=device, dtype=torch.int64).contiguous()
        self.device = self.points.device  # (with its index: 'cuda' alone compares unequal to a tensor's 'cuda:0')

    def __len__(self):
        return self.points.shape[0]

    @classmethod
    def from_dataset(cls, ds, device="cuda"):
        """A data.ModelNetCls (points (L, 2048, 3), labels (L, 1)) or a data.PointCloudDataSet (point_clouds; its labels when
        they are integers, the example index otherwise -- the folder loaders label clouds with strings)."""
        if hasattr(ds, "point_clouds"):
            labels = np.asarray(ds.labels)
            return cls(ds.point_clouds, labels if labels.dtype.kind in "iu" else None, device)
        if hasattr(ds, "points") and hasattr(ds, "labels"):
            return cls(ds.points, np.asarray(ds.labels).reshape(len(ds.points)), device)
        raise TypeError("from_dataset: a ModelNetCls or a PointCloudDataSet (got %s)" % type(ds).__name__)


def fixed_pair_quaternions(lset, seed=0, max_rotation_deg=45.0):
    """The rotation table of QuaternionFixedDataset.__init__ (qdataset.py:122-145) as (lset, 4) float32 in (w, x, y, z) order:
    np.random.seed(seed); per item the Euler angles uniform(-max, max, [1, 3]) and the translation draw that the dataset never
    uses (it still advances the generator); Euler "xyz" to quaternion as quaternion.py:166-210 does -- the product qx qy qz, negated --
    in fp64, cast to float32.  Consumes numpy's GLOBAL generator, like the reference."""
    mx = math.pi / 180.0 * max_rotation_deg
    np.random.seed(seed)
    e = np.empty((lset, 3), dtype=np.float64)
    for i in range(lset):
        e[i] = np.random.uniform(-mx, mx, [1, 3])[0]
        np.random.uniform(-0.0, 0.0, [1, 3])
    c, s = np.cos(e / 2), np.sin(e / 2)

    def mul(q, r):  # Hamilton product of (w, x, y, z) rows
        return np.stack([q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3], q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2],
                         q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1], q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0]])

    z = np.zeros(lset)
    q = mul(mul(np.stack([c[:, 0], s[:, 0], z, z]), np.stack([c[:, 1], z, s[:, 1], z])), np.stack([c[:, 2], z, z, s[:, 2]]))
    return (-q.T).astype(np.float32)


class DeviceBatchSource:
    """Successive batches of a DeviceCloudSet, one launch each.
        batch, n_points   B clouds of the first n_points points of their items
        seed              key of every draw; rank / world: rank r takes positions [r B, (r + 1) B) of every world * B
        repeat            the set is `repeat` passes over the clouds, each with its own pair rotation (QuaternionFixedDataset)
        pair              None; "fixed" (fixed_pair_quaternions(len(set) * repeat, seed=0)); or a (len(set) * repeat, 4) table.
                          "fixed" RESEEDS numpy's global generator (np.random.seed(0), as QuaternionFixedDataset.__init__ does): a
                          script that seeded numpy before building the source must seed it again afterwards, or pass a table
        layout            "bnc" (B, N, 3) or "bcn" (B, 3, N)
    next_into / next launch on the current stream and never synchronise; reading `position` / `epoch` does."""

    def __init__(self, cloudset, recipe, batch, n_points, seed=0, rank=0, world=1, repeat=1, pair=None, layout="bnc"):
        if layout not in ("bnc", "bcn"):
            raise ValueError("layout: 'bnc' or 'bcn'")
        if batch < 0 or n_points < 0 or repeat < 1 or not 0 <= rank < world:
            raise ValueError("batch / n_points must be >= 0, repeat >= 1, 0 <= rank < world")
        if n_points > cloudset.points.shape[1]:
            raise ValueError("n_points = %d > the %d points a cloud holds" % (n_points, cloudset.points.shape[1]))
        if recipe.shuffle_points and n_points > MAX_SHUFFLE_POINTS:
            raise ValueError("shuffle_points sorts at most %d points per cloud, n_points = %d" % (MAX_SHUFFLE_POINTS, n_points))
        self.set, self.recipe, self.B, self.N = cloudset, recipe, int(batch), int(n_points)
        self.seed, self.rank, self.world, self.repeat = int(seed) & (2 ** 64 - 1), int(rank), int(world), int(repeat)
        self.layout, self.device = int(layout == "bcn"), cloudset.device
        self.lset = len(cloudset) * self.repeat
        self._c = recipe.to_c()
        if isinstance(pair, str):
            if pair != "fixed":
                raise ValueError("pair: None, 'fixed' or a quaternion table")
            pair = fixed_pair_quaternions(self.lset)
        if pair is not None:
            pair = torch.as_tensor(pair).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(pair.shape) != (self.lset, 4):
                raise ValueError("pair table must be (%d, 4), got %s" % (self.lset, tuple(pair.shape)))
        self.pair_quat = pair
        self._block = torch.zeros(_STATE_WORDS, dtype=torch.int64, device=self.device)

    @property
    def makes_pairs(self):
        return self.pair_quat is not None

    def shape(self):
        return (self.B, 3, self.N) if self.layout else (self.B, self.N, 3)

    def _target(self, t, shape, dtype, what):
        if t is None:
            return
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (what, dtype, tuple(shape), self.device))

    def _launch(self, position, p0, p1, labels, igt, items):
        self._target(p0, self.shape(), torch.float32, "p0")
        self._target(p1, self.shape(), torch.float32, "p1")
        self._target(labels, (self.B,), torch.int64, "labels")
        self._target(igt, (self.B, 7), torch.float32, "igt")
        self._target(items, (self.B,), torch.int32, "items")
        if p0 is None:
            raise ValueError("p0 is required")
        if (p1 is not None or igt is not None) and self.pair_quat is None:
            raise ValueError("p1 / igt need a source built with pair=")
        s = self.set
        check(lib.sn_batch_assemble(self.B, self.N, s.points.shape[1], len(s), self.repeat, ptr(s.points), ptr(s.labels),
                                    ctypes.addressof(self._c), self.seed, self.rank, self.world, position, ptr(self._block),
                                    ptr(self.pair_quat), self.layout, ptr(p0), ptr(p1), ptr(labels), ptr(igt), ptr(items),
                                    stream_of(p0)), "sn_batch_assemble")

    def next_into(self, p0, p1=None, labels=None, igt=None, items=None):
        """The next batch into caller-owned tensors: one launch; the device-side position advances by batch * world."""
        self._launch(-1, p0, p1, labels, igt, items)

    def _alloc(self):
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)  # noqa: E731
        pair = self.pair_quat is not None
        return Batch(e(self.shape(), torch.float32), e(self.shape(), torch.float32) if pair else None, e((self.B,), torch.int64),
                     e((self.B, 7), torch.float32) if pair else None, e((self.B,), torch.int32))

    def next(self):
        out = self._alloc()
        self._launch(-1, *out)
        return out

    def at(self, position):
        """The batch at an explicit global position (that of its rank-0 slot 0); the source's own position stays."""
        if position < 0:
            raise ValueError("position must be >= 0")
        out = self._alloc()
        self._launch(int(position), *out)
        return out

    @property
    def position(self):
        return int(self._block[0].item())  # synchronises

    @property
    def epoch(self):
        return self.position // self.lset

    def state_dict(self):
        return {"seed": self.seed, "position": self.position}

    def load_state_dict(self, state):
        if int(state["position"]) < 0:
            raise ValueError("position must be >= 0")
        self.seed = int(state["seed"]) & (2 ** 64 - 1)
        host = torch.zeros(_STATE_WORDS, dtype=torch.int64)
        host[0] = int(state["position"])
        self._block.copy_(host)

#!/usr/bin/env python3
"""Generate tests/golden/batch_reference.npz by RUNNING the reference's data-side code (itailang/SampleNet):
registration/src/pctransforms.py (OnUnitCube, angle_axis), src/quaternion.py (euler_to_quaternion, qrot) and
src/qdataset.py (create_random_transform), for tests/test_batch_host.py.

    SAMPLENET_REFERENCE=/path/to/SampleNet python tests/golden/make_batch_golden.py

The three files are copied into a scratch directory and imported from THERE (never in place: nothing is written beside the
reference, and its src/__init__.py -- which pulls in the CUDA extensions -- is not executed).  qdataset.py imports kornia for
functions this script never calls: two empty stand-in modules satisfy the import.

What the fixture holds
  clouds (3, 64, 3) float32        random clouds of different extents and offsets
  unit_cube (3, 64, 3) float32     OnUnitCube()(cloud as fp64), cast           -- computed in fp64, as the bar in the test assumes
  angles (6,), axes (2, 3)         given rotation angles and axes
  axis_R (2, 6, 3, 3) float32      angle_axis(angle, axis)                     -- fp64 inside, .float() at the end
  perturb_angles (4, 3)            given angle triples
  perturb_R (4, 3, 3) float64      Rz Ry Rx of angle_axis's three fp32 matrices, multiplied here in fp64
  quat_seed0 / quat_seed1 (8, 4)   np.random.seed(seed); eight create_random_transform(torch.float32, 45, 0) -> .quat()
  qrot_q (4,), qrot_out (64, 3)    quaternion.qrot of clouds[0] (fp64) by quat_seed0[3], cast
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SAMPLENET_REFERENCE")


def import_reference(scratch):
    src = os.path.join(scratch, "src")
    os.makedirs(src)
    for name in ("pctransforms.py", "quaternion.py", "qdataset.py"):
        shutil.copy(os.path.join(REF, "registration", "src", name), os.path.join(src, name))
    open(os.path.join(src, "__init__.py"), "w").close()
    for name in ("kornia", "kornia.geometry", "kornia.geometry.conversions", "kornia.geometry.linalg"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, scratch)
    import src.pctransforms as T
    import src.qdataset as D
    import src.quaternion as Q

    return T, Q, D


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set SAMPLENET_REFERENCE to a checkout of the reference")
    import torch

    scratch = tempfile.mkdtemp(prefix="batch_golden_")
    try:
        T, Q, D = import_reference(scratch)
        rng = np.random.default_rng(20)
        clouds = np.stack([(rng.random((64, 3)) * s + o).astype(np.float32)
                           for s, o in (((1.0, 1.0, 1.0), 0.0), ((0.3, 2.0, 0.7), -1.0), ((5.0, 0.01, 1.0), 10.0))])
        unit = np.stack([T.OnUnitCube()(torch.from_numpy(c.astype(np.float64))).numpy().astype(np.float32) for c in clouds])
        angles = np.array([0.0, 0.3, 1.0, 2.5, 4.0, 6.0])
        axes = np.array([[0.0, 1.0, 0.0], [1.0, 2.0, 3.0]])
        axis_R = np.stack([np.stack([T.angle_axis(a, ax).numpy() for a in angles]) for ax in axes])
        pang = np.array([[0.0, 0.0, 0.0], [0.18, -0.18, 0.05], [-0.01, 0.12, -0.18], [0.06, 0.06, 0.06]])
        ex, ey, ez = np.eye(3)
        perturb_R = np.stack([T.angle_axis(a[2], ez).double().numpy() @ T.angle_axis(a[1], ey).double().numpy()
                              @ T.angle_axis(a[0], ex).double().numpy() for a in pang])
        quats = {}
        for seed in (0, 1):
            np.random.seed(seed)
            quats[seed] = np.concatenate([D.create_random_transform(torch.float32, 45, 0).quat().numpy() for _ in range(8)])
        q = quats[0][3]
        rot = Q.qrot(torch.from_numpy(np.tile(q.astype(np.float64), (64, 1))), torch.from_numpy(clouds[0].astype(np.float64)))
        path = os.path.join(HERE, "batch_reference.npz")
        np.savez_compressed(path, clouds=clouds, unit_cube=unit, angles=angles, axes=axes, axis_R=axis_R.astype(np.float32),
                            perturb_angles=pang, perturb_R=perturb_R, quat_seed0=quats[0].astype(np.float32),
                            quat_seed1=quats[1].astype(np.float32), qrot_q=q.astype(np.float32),
                            qrot_out=rot.numpy().astype(np.float32))
        print("wrote", path, os.path.getsize(path), "bytes")
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()

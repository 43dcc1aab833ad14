"""QuaternionTransform -- the pose container of the registration task (drop-in for `registration/src/qdataset.py:8-119`):
a (B,7) tensor of rows [quaternion (w, x, y, z) | translation], its rotation of clouds on `sn_qrot_*` and its pose-error terms on
`sn_pose_error_*` (ops.pose_errors).  Two documented deviations from the reference's compute_errors, both only where the reference
returns NaN: the argument of rot_err's acos is clamped to [-1, 1], and the gradient of trans_err at a zero difference is 0.
"""
import math

import torch


def deg_to_rad(deg):
    return math.pi / 180 * deg


def rad_to_deg(rad):
    return 180 / math.pi * rad


def qinv(q):
    """Inverse of unit quaternions (*,4) in (w, x, y, z) order -- registration/src/quaternion.py:213-218."""
    return torch.cat([q[..., 0:1], -q[..., 1:]], dim=-1)


class QuaternionTransform:
    def __init__(self, vec, inverse=False):
        self._inversion = torch.tensor([bool(inverse)])  # (inversion: first apply the translation)
        self.vec = vec.view([-1, 7])

    @staticmethod
    def from_dict(d, device):
        return QuaternionTransform(d["vec"].to(device), bool(d["inversion"][0].item()))

    def inverse(self):
        vec = torch.cat([qinv(self.quat()), -self.trans()], dim=1)
        return QuaternionTransform(vec, inverse=(not self.inversion()))

    def as_dict(self):
        return {"inversion": self._inversion, "vec": self.vec}

    def quat(self):
        return self.vec[:, 0:4]

    def trans(self):
        return self.vec[:, 4:]

    def inversion(self):
        # (a data loader batches the flags of its items: the first item's stands for the batch, as in the reference)
        return self._inversion[0].item()

    @staticmethod
    def wxyz_to_xyzw(q):
        return q[..., [1, 2, 3, 0]]

    @staticmethod
    def xyzw_to_wxyz(q):
        return q[..., [3, 0, 1, 2]]

    def compute_errors(self, other):
        """-> (rot_err [radians], norm_err, trans_err), batch means as 0-d tensors (qdataset.py:62-95); norm_err and trans_err
        carry gradients to this transform's vec, rot_err is a metric."""
        from .ops import pose_error_means

        if not self.vec.is_cuda:
            raise RuntimeError("samplenet_amd ops run on the GPU only (got a %s tensor); no CPU fallback exists" % self.vec.device)
        return pose_error_means(self.vec, other.vec.to(self.vec.device))

    def rotate(self, p):
        """Rotation only (qdataset.py:97-119): p (B,N,3) by each cloud's own quaternion (one launch), or p (N,3) by a single one."""
        from .task_features import qrot, qrot_cloud

        if p.dim() == 2:
            assert self.vec.shape[0] == 1
            return qrot(self.quat().expand([p.shape[0], -1]), p)
        if p.dim() == 3:
            return qrot_cloud(self.quat(), p)
        raise ValueError("rotate: p must be (N,3) or (B,N,3)")

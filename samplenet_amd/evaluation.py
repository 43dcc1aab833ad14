"""Evaluation of the registration task on the device -- `eval_1` and `test_1` of `registration/main.py:364-483`.

The reference tests at batch_size 1 with an `.item()` per cloud and metric (main.py:128, 444-450).  Here a batch of any size goes
through the same steps -- sampling, PCRNet, the pose-error terms, the Chamfer term, the sampling consistency -- with every value
kept PER CLOUD on the device (ops.pose_errors, ops.chamfer_mean_per_cloud); `add` never synchronises and `result` makes one
transfer.  With everything in eval mode a cloud's values do not depend on the clouds it is batched with.
"""
import numpy as np
import torch

from . import ops
from .qtransform import qinv, rad_to_deg
from .task_features import _igt_vec, qrot_cloud


def registration_aggregates(rotation_errors, trans_errs, consistency_errors, losses=None):
    """The aggregates of main.py:461-483 from per-item arrays (rotation errors in degrees): the precision curve over
    arange(0, 180, 0.5) (the share of items with rotation error <= each threshold; a NaN error counts as a miss), its AUC, the
    means and standard deviations main.py prints (and the translation error's), and eval_1's two averages (main.py:406-407)."""
    # (float64, as the reference's arrays of .item() values are: the means and deviations accumulate in double)
    rot = np.asarray(rotation_errors, dtype=np.float64)
    trans, cons = np.asarray(trans_errs, dtype=np.float64), np.asarray(consistency_errors, dtype=np.float64)
    n_samples = len(rot)
    x = np.arange(0.0, 180.0, 0.5)
    y = np.sum(rot[None, :] <= x[:, None], axis=1) / n_samples
    out = {"thresholds": x, "precision": y, "auc": np.sum(y) / len(x),
           "mean_rotation_error": np.mean(rot), "std_rotation_error": np.std(rot),
           "mean_trans_error": np.mean(trans), "std_trans_error": np.std(trans),
           "mean_consistency_error": np.mean(cons), "std_consistency_error": np.std(cons),
           "ave_gloss": float(np.cumsum(rot)[-1]) / n_samples}  # (eval_1 adds item by item: a sequential sum)
    if losses is not None:
        out["ave_vloss"] = float(np.cumsum(np.asarray(losses, dtype=np.float64))[-1]) / n_samples
    return out


class RegistrationEvaluator:
    """model: a task_features.PCRNet on (B,N,3) clouds; sampler: a SampleNet (its inference branch: matched points), an FPSSampler /
    RandomSampler, or None (main.py:427-437); num_sampled_clouds 1: only the source p1 is sampled, 2: the template p0 as well
    (main.py:492-496, 514-526); loss_type as pcrnet_loss.  The sampler's own loss terms are zero in eval mode and not part of
    `losses` (the reference adds the inference branch's zeros, main.py:398)."""

    def __init__(self, model, sampler=None, num_sampled_clouds=2, loss_type=0):
        if num_sampled_clouds not in (1, 2) or loss_type not in (0, 1):
            raise ValueError("num_sampled_clouds: 1 or 2; loss_type: 0 or 1")
        if getattr(model, "input_shape", "bnc") != "bnc":
            raise ValueError("RegistrationEvaluator: the task network must take (B,N,3) clouds (input_shape='bnc')")
        self.model, self.sampler = model, sampler
        self.num_sampled_clouds, self.loss_type = num_sampled_clouds, loss_type
        self._rows = []  # (11, B) device tensors: rotation error [deg], translation error, consistency, loss, the estimated twist

    def reset(self):
        self._rows = []

    def _sample(self, p):
        out = self.sampler(p)
        return (out[1] if isinstance(out, tuple) else out).contiguous()  # (SampleNet: (simplified, matched))

    def add(self, p0, p1, igt):
        """One batch: p0 template, p1 source (B,N,3) on the GPU, igt (B,7) or the reference's dict.  No synchronisation."""
        if not (p0.is_cuda and p1.is_cuda):
            raise RuntimeError("samplenet_amd ops run on the GPU only (got a %s tensor); no CPU fallback exists" % p0.device)
        model, sampler = self.model, self.sampler
        states = [(m, m.training) for m in (model, sampler) if m is not None]
        for m, _ in states:
            m.eval()
        try:
            with torch.no_grad():
                vec = _igt_vec(igt, p1).float().contiguous()
                p0s, p1s = p0.contiguous(), p1.contiguous()
                if sampler is not None:
                    p1s = self._sample(p1s)
                    if self.num_sampled_clouds == 2:
                        p0s = self._sample(p0s)
                twist, _pre, _qnorm, _quat, p1_est = model.forward_with_qnorm(p0s, p1s, rotate=p0s)
                chamfer = ops.chamfer_mean_per_cloud(p1s, p1_est)
                rot, nrm, trn = ops.pose_errors(twist, vec)
                loss = nrm + chamfer if self.loss_type == 0 else chamfer
                cons = ops.chamfer_mean_per_cloud(p0s, qrot_cloud(qinv(vec[:, 0:4]), p1s))  # (main.py:540-555)
                self._rows.append(torch.cat([torch.stack([rad_to_deg(rot), trn, cons, loss]), twist.t()]))
        finally:
            for m, was in states:
                m.train(was)

    def result(self):
        """One device-to-host transfer -> dict: the per-item arrays rotation_errors (degrees), trans_errs, consistency_errors,
        losses, twists (items, 7: the estimated poses, main.py:595's est_transform), and registration_aggregates of the first four."""
        if not self._rows:
            raise RuntimeError("RegistrationEvaluator.result: nothing was added")
        table = torch.cat(self._rows, dim=1).cpu().numpy().astype(np.float64)  # (exact: what .item() returns per value)
        out = {"rotation_errors": table[0], "trans_errs": table[1], "consistency_errors": table[2], "losses": table[3],
               "twists": np.ascontiguousarray(table[4:11].T)}
        out.update(registration_aggregates(table[0], table[1], table[2], table[3]))
        return out

"""Evaluation of the three tasks on the device.  Registration: `eval_1` and `test_1` of `registration/main.py:364-483`
(RegistrationEvaluator, below first); classification: `classification/evaluate_samplenet.py:156-277` (ClassificationEvaluator);
reconstruction: `reconstruction/sampler/evaluate_samplenet.py:88-152` with `get_loss_ae_per_pc` of
`reconstruction/src/sampler_autoencoder.py:149-167` (ReconstructionEvaluator).  All three keep every value per cloud on the device,
never synchronise in `add`, and make one transfer in `result`.

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


# ------------------------------------------------------------------------------------------------ the sampling step, shared
def _sample_with_indices(sampler, x):
    """x (B,N,3) -> (simplified, matched, out_idx (B,M) int32, n_unique (B,) int32), clouds as (B,M,3).  SampleNet: its
    sample_indices; an FPSSampler / RandomSampler: its output as both clouds, the indices recovered as each sampled point's nearest
    (= coincident, lowest index) input point; None: the whole cloud."""
    from .samplenet import SampleNet

    B, N, _ = x.shape
    if sampler is None:
        idx = torch.arange(N, device=x.device, dtype=torch.int32).expand(B, N).contiguous()
        return x, x, idx, torch.full((B,), N, device=x.device, dtype=torch.int32)
    xin = x if sampler.input_shape == "bnc" else x.permute(0, 2, 1).contiguous()
    bnc = lambda t: (t if sampler.output_shape == "bnc" else t.permute(0, 2, 1)).contiguous()  # noqa: E731
    if isinstance(sampler, SampleNet):
        simp, match, idx, nun = sampler.sample_indices(xin)
        return bnc(simp), bnc(match), idx, nun
    out = sampler(xin)
    pts = bnc(out[1] if isinstance(out, tuple) else out)
    M = pts.shape[1]
    idx = ops.knn(1, x, pts, ops.BNC, ops.BNC, return_dist=False)[0].view(B, M)
    if M <= 1024 and N <= 8192:
        nun = ops.nn_matching_indexed(x, idx, M, complete_fps=False)[2]
    else:
        srt = idx.sort(dim=1).values
        nun = ((srt[:, 1:] != srt[:, :-1]).sum(1) + 1).int()
    return pts, pts, idx, nun


def _to_shape(t, module):
    return t if getattr(module, "input_shape", "bnc") == "bnc" else t.permute(0, 2, 1).contiguous()


class _EvalMode:
    """every given module in eval mode inside the block, its training flag restored afterwards"""

    def __init__(self, *modules):
        self.states = [(m, m.training) for m in modules if m is not None]

    def __enter__(self):
        for m, _ in self.states:
            m.eval()

    def __exit__(self, *exc):
        for m, was in self.states:
            m.train(was)


# ------------------------------------------------------------------------------------------------ classification
def classification_aggregates(preds, labels, batch_sizes, batch_losses, n_unique, num_classes):
    """The aggregates of classification/evaluate_samplenet.py:249-277 from per-item arrays and the per-batch (size, loss_val) pairs,
    accumulated in float64: mean_loss = sum_j loss_val_j B_j / total_seen (the regulariser inside loss_val is per batch, not per
    item, as in the reference), accuracy, class_seen / class_correct, class_accuracies (NaN for an unseen class: the reference's
    0 / 0), avg_class_accuracy (its np.mean: NaN when a class is unseen), mean_unique.  avg_class_accuracy_seen, the mean over the
    SEEN classes, is an addition: the reference has no such figure."""
    preds, labels = np.asarray(preds).astype(np.int64), np.asarray(labels).astype(np.int64)
    sizes, losses = np.asarray(batch_sizes, dtype=np.float64), np.asarray(batch_losses, dtype=np.float64)
    total_seen = len(labels)
    ok = (labels >= 0) & (labels < num_classes)
    seen = np.bincount(labels[ok], minlength=num_classes).astype(np.float64)
    correct = np.bincount(labels[ok & (preds == labels)], minlength=num_classes).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = correct / seen
    return {"total_seen": total_seen, "mean_loss": float(np.cumsum(losses * sizes)[-1]) / float(total_seen),
            "accuracy": float(np.sum(preds == labels)) / float(total_seen), "class_seen": seen.astype(np.int64),
            "class_correct": correct.astype(np.int64), "class_accuracies": acc, "avg_class_accuracy": float(np.mean(acc)),
            "avg_class_accuracy_seen": float(np.mean(acc[seen > 0])) if (seen > 0).any() else float("nan"),
            "mean_unique": float(np.sum(np.asarray(n_unique, dtype=np.float64))) / float(total_seen)}


class ClassificationEvaluator:
    """classifier: a PointNetCls / PointNetClsBasic; sampler: a SampleNet (sample_indices: the inference branch with its indices),
    an FPSSampler / RandomSampler, or None (the whole cloud); match_output: classify the matched cloud, else the simplified one
    (evaluate_samplenet.py:222-225); reg_weight as classification_loss; keep: result() also returns the logits and the classified
    clouds.  Clouds are (B,N,3)."""

    def __init__(self, classifier, sampler=None, match_output=True, reg_weight=0.001, keep=False):
        self.classifier, self.sampler = classifier, sampler
        self.match_output, self.reg_weight, self.keep = bool(match_output), float(reg_weight), bool(keep)
        self.reset()

    def reset(self):
        self._rows, self._sizes, self._losses, self._logits, self._clouds = [], [], [], [], []

    def add(self, x, labels):
        """One batch: x (B,N,3) and labels (B,) integer class indices on the GPU.  No synchronisation."""
        from .classifier import orthogonality_loss

        if not (x.is_cuda and labels.is_cuda):
            raise RuntimeError("samplenet_amd ops run on the GPU only (got a %s tensor); no CPU fallback exists" % x.device)
        with _EvalMode(self.classifier, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            simp, match, _idx, nun = _sample_with_indices(self.sampler, x)
            cloud = match if self.match_output else simp
            logits, end_points = self.classifier(_to_shape(cloud, self.classifier))
            ce, pred, _correct, means = ops.classification_terms(logits, labels)
            loss_val = means[0]
            t = end_points.get("transform")
            if t is not None:
                loss_val = loss_val + self.reg_weight * orthogonality_loss(t)
            # (class indices and counts are far below 2^24: exact as float32)
            self._rows.append(torch.stack([pred.float(), labels.float(), ce, nun.float()]))
            self._sizes.append(int(x.shape[0]))
            self._losses.append(loss_val.reshape(1))
            if self.keep:
                self._logits.append(logits.reshape(-1))
                self._clouds.append(cloud.reshape(-1))
            self._num_classes, self._cloud_points = int(logits.shape[1]), int(cloud.shape[1])

    def result(self):
        """One device-to-host transfer -> dict: the per-item arrays preds, labels (int64), losses (float64: the cross-entropy per
        item), n_unique (int64); batch_sizes, batch_losses; classification_aggregates of them (avg_class_accuracy_seen is an addition
        to the reference's figures); with keep=True also logits (items, classes) and clouds (items, points, 3)."""
        if not self._rows:
            raise RuntimeError("ClassificationEvaluator.result: nothing was added")
        n = sum(self._sizes)
        flat = torch.cat([torch.cat(self._rows, dim=1).reshape(-1)] + self._losses + self._logits + self._clouds).cpu().numpy()
        table = flat[:4 * n].reshape(4, n).astype(np.float64)
        nb, C, M = len(self._sizes), self._num_classes, self._cloud_points
        out = {"preds": table[0].astype(np.int64), "labels": table[1].astype(np.int64), "losses": table[2],
               "n_unique": table[3].astype(np.int64), "batch_sizes": np.asarray(self._sizes, dtype=np.int64),
               "batch_losses": flat[4 * n:4 * n + nb].astype(np.float64)}
        if self.keep:
            # (per batch the logits lie before the clouds' block: all logits first, then all clouds)
            o = 4 * n + nb
            out["logits"] = flat[o:o + n * C].reshape(n, C).copy()
            out["clouds"] = flat[o + n * C:o + n * C + n * M * 3].reshape(n, M, 3).copy()
        out.update(classification_aggregates(out["preds"], out["labels"], out["batch_sizes"], out["batch_losses"], out["n_unique"], C))
        return out


# ------------------------------------------------------------------------------------------------ reconstruction
class ReconstructionEvaluator:
    """autoencoder: a PointNetAE; sampler as ClassificationEvaluator's (the matched points are reconstructed from); loss "chamfer"
    (ops.chamfer_mean_per_cloud) or "emd" (ops.emd_loss' per-cloud costs): get_loss_ae_per_pc (sampler_autoencoder.py:149-167: the
    autoencoder loss one cloud at a time) for a batch; with_reference: also the autoencoder's loss on the complete cloud
    (evaluate_ae.py's ae_loss test_set file) and nre = loss / reference loss per cloud (evaluate_samplenet.py:145-152);
    keep: result() also returns sampled, sample_idx, reconstructions (the three arrays the reference script saves).  Clouds are (B,N,3)."""

    def __init__(self, autoencoder, sampler=None, loss="chamfer", with_reference=True, keep=False):
        if loss not in ("chamfer", "emd"):
            raise ValueError("loss: 'chamfer' or 'emd'")
        self.autoencoder, self.sampler = autoencoder, sampler
        self.loss, self.with_reference, self.keep = loss, bool(with_reference), bool(keep)
        self.reset()

    def reset(self):
        self._rows, self._kept = [], []

    def _per_cloud(self, recon, x):
        if self.loss == "chamfer":
            return ops.chamfer_mean_per_cloud(recon, x)
        return ops.emd_loss(recon, x)

    def add(self, x):
        """One batch: x (B,N,3) on the GPU.  No synchronisation."""
        if not x.is_cuda:
            raise RuntimeError("samplenet_amd ops run on the GPU only (got a %s tensor); no CPU fallback exists" % x.device)
        ae = self.autoencoder
        with _EvalMode(ae, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            _simp, sampled, idx, nun = _sample_with_indices(self.sampler, x)
            recon = ae(_to_shape(sampled, ae)).contiguous()
            loss = self._per_cloud(recon, x)
            ref = self._per_cloud(ae(_to_shape(x, ae)).contiguous(), x) if self.with_reference else torch.zeros_like(loss)
            self._rows.append(torch.stack([loss, ref, nun.float()]))
            if self.keep:
                self._kept.append((sampled.reshape(-1), idx.float().reshape(-1), recon.reshape(-1)))
            self._shape = (int(sampled.shape[1]), int(recon.shape[1]))

    def result(self):
        """One device-to-host transfer -> dict: the per-item float64 arrays losses, n_unique (int64) and, with_reference,
        reference_losses and nre (their quotient, np.divide as the reference); mean_loss, mean_unique, mean_reference_loss, mean_nre
        (evaluate_samplenet.py:143, 151-152); with keep=True sampled (items, M, 3), sample_idx (items, M) int64, reconstructions."""
        if not self._rows:
            raise RuntimeError("ReconstructionEvaluator.result: nothing was added")
        sizes = [r.shape[1] for r in self._rows]
        n = sum(sizes)
        parts = [torch.cat(self._rows, dim=1).reshape(-1)]
        for k in range(3):
            parts += [kept[k] for kept in self._kept]
        flat = torch.cat(parts).cpu().numpy()
        table = flat[:3 * n].reshape(3, n).astype(np.float64)
        out = {"losses": table[0], "n_unique": table[2].astype(np.int64), "mean_loss": float(table[0].mean()),
               "mean_unique": float(table[2].mean())}
        if self.with_reference:
            with np.errstate(invalid="ignore", divide="ignore"):
                nre = np.divide(table[0], table[1])
            out.update(reference_losses=table[1], nre=nre, mean_reference_loss=float(table[1].mean()), mean_nre=float(nre.mean()))
        if self.keep:
            M, R = self._shape
            o = 3 * n
            out["sampled"] = flat[o:o + n * M * 3].reshape(n, M, 3).copy()
            o += n * M * 3
            out["sample_idx"] = flat[o:o + n * M].astype(np.int64).reshape(n, M)
            o += n * M
            out["reconstructions"] = flat[o:o + n * R * 3].reshape(n, R, 3).copy()
        return out

"""Evaluation of the three tasks on the device.  Registration: `eval_1` and `test_1` of `registration/main.py:364-483`
(RegistrationEvaluator, below first); classification: `classification/evaluate_samplenet.py:156-277` (ClassificationEvaluator);
reconstruction: `reconstruction/sampler/evaluate_samplenet.py:88-152` with `get_loss_ae_per_pc` of
`reconstruction/src/sampler_autoencoder.py:149-167` (ReconstructionEvaluator).  All three keep every value per cloud on the device,
never synchronise in `add`, and make one transfer in `result`.  The progressive sampler's evaluation -- the cloud ranked once, the
task network run on every prefix (`classification/infer_samplenet_progressive.py:114,207-212` + `evaluate_samplenet.py`,
`reconstruction/sampler/evaluate_samplenet_progressive.py:105-141`) -- is ProgressiveClassificationEvaluator /
ProgressiveReconstructionEvaluator, over the same per-batch steps and aggregates.  Retrieval, the fourth application the reference
names (README.md:13) without a script for it, closes the file: RetrievalEvaluator / ProgressiveRetrievalEvaluator collect the
classifier's descriptors and rank and score all of them against each other in one launch (ops.retrieval_metrics).

The reference tests at batch_size 1 with an `.item()` per cloud and metric (main.py:128, 444-450).  Here a batch of any size goes
through the same steps -- sampling, PCRNet, the pose-error terms, the Chamfer term, the sampling consistency -- with every value
kept PER CLOUD on the device (ops.pose_errors, ops.chamfer_mean_per_cloud); `add` never synchronises and `result` makes one
transfer.  With everything in eval mode a cloud's values do not depend on the clouds it is batched with.  How the columns lie in
the one buffer that travels is known to _Collected.fetch alone: an evaluator names its columns and never counts an offset.
"""
import numpy as np
import torch

from . import ops
from .qtransform import qinv, rad_to_deg
from .task_features import _igt_vec, qrot_cloud


class _Collected:
    """What an evaluator keeps on the device, one column per key, until the one transfer of result()."""

    def __init__(self):
        self._columns = {}  # key -> (numpy dtype of the fetched array, the device tensors put under the key)

    def __bool__(self):
        return bool(self._columns)

    def put(self, key, tensor, dtype):
        """Record a device tensor whose leading dimension is the item axis -- (B,), (B, 7), (B, M, 3), (1,) for a value per batch --
        under `key` (any hashable); `dtype`: what fetch() returns the column as.  No device work, no synchronisation."""
        self._columns.setdefault(key, (dtype, []))[1].append(tensor)

    def on_device(self, key):
        """the column's pieces as one device tensor, in the dtype they were put in"""
        return torch.cat(self._columns[key][1])

    def fetch(self):
        """One torch.cat, one device-to-host transfer -> {key: array (items, *trailing)}, every array a copy of its own.  The
        carrier is float32: counts, class and point indices are far below 2^24, so they cross it exactly."""
        if not self._columns:
            return {}
        pieces = [p.reshape(-1).float() for _dtype, ps in self._columns.values() for p in ps]
        flat = torch.cat(pieces).cpu().numpy()
        out, o = {}, 0
        for key, (dtype, ps) in self._columns.items():
            shape = (sum(p.shape[0] for p in ps),) + tuple(ps[0].shape[1:])
            size = sum(p.numel() for p in ps)
            out[key] = flat[o:o + size].reshape(shape).astype(dtype)  # (astype copies: nothing keeps the carrier alive)
            o += size
        return out


def _need_added(collected, owner):
    if not collected:
        raise RuntimeError("%s.result: nothing was added" % owner)
    return collected


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
        self.reset()

    def reset(self):
        self._got = _Collected()

    def _sample(self, p):
        out = self.sampler(p)
        return (out[1] if isinstance(out, tuple) else out).contiguous()  # (SampleNet: (simplified, matched))

    def add(self, p0, p1, igt):
        """One batch: p0 template, p1 source (B,N,3) on the GPU, igt (B,7) or the reference's dict.  No synchronisation."""
        ops._need_gpu(p0, p1)
        with _EvalMode(self.model, self.sampler), torch.no_grad():
            vec = _igt_vec(igt, p1).float().contiguous()
            p0s, p1s = p0.contiguous(), p1.contiguous()
            if self.sampler is not None:
                p1s = self._sample(p1s)
                if self.num_sampled_clouds == 2:
                    p0s = self._sample(p0s)
            twist, _pre, _qnorm, _quat, p1_est = self.model.forward_with_qnorm(p0s, p1s, rotate=p0s)
            chamfer = ops.chamfer_mean_per_cloud(p1s, p1_est)
            rot, nrm, trn = ops.pose_errors(twist, vec)
            cons = ops.chamfer_mean_per_cloud(p0s, qrot_cloud(qinv(vec[:, 0:4]), p1s))  # (main.py:540-555)
            # (float64 is exact: what .item() returns per value)
            self._got.put("rotation_errors", rad_to_deg(rot), np.float64)
            self._got.put("trans_errs", trn, np.float64)
            self._got.put("consistency_errors", cons, np.float64)
            self._got.put("losses", nrm + chamfer if self.loss_type == 0 else chamfer, np.float64)
            self._got.put("twists", twist, np.float64)

    def result(self):
        """One device-to-host transfer -> dict: the per-item arrays rotation_errors (degrees), trans_errs, consistency_errors,
        losses, twists (items, 7: the estimated poses, main.py:595's est_transform), and registration_aggregates of the first four."""
        out = _need_added(self._got, "RegistrationEvaluator").fetch()
        out.update(registration_aggregates(out["rotation_errors"], out["trans_errs"], out["consistency_errors"], out["losses"]))
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


def _classify_batch(classifier, cloud, labels, reg_weight):
    """One batch of one cloud size through the classifier: -> (logits, pred (B,) int32, cross-entropy (B,), loss_val (1,)) with
    loss_val = the batch's mean cross-entropy plus the weighted orthogonality term (evaluate_samplenet.py:236-241)."""
    from .classifier import orthogonality_loss

    logits, end_points = classifier(_to_shape(cloud, classifier))
    ce, pred, _correct, means = ops.classification_terms(logits, labels)
    loss_val = means[0]
    t = end_points.get("transform")
    if t is not None:
        loss_val = loss_val + reg_weight * orthogonality_loss(t)
    return logits, pred, ce, loss_val.reshape(1)


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
        self._got, self._sizes = _Collected(), []

    def add(self, x, labels):
        """One batch: x (B,N,3) and labels (B,) integer class indices on the GPU.  No synchronisation."""
        ops._need_gpu(x, labels)
        with _EvalMode(self.classifier, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            simp, match, _idx, nun = _sample_with_indices(self.sampler, x)
            cloud = match if self.match_output else simp
            logits, pred, ce, loss_val = _classify_batch(self.classifier, cloud, labels, self.reg_weight)
            self._got.put("preds", pred, np.int64)
            self._got.put("labels", labels.clone(), np.int64)  # (a copy: the caller may refill its label buffer before result())
            self._got.put("losses", ce, np.float64)
            self._got.put("n_unique", nun, np.int64)
            self._got.put("batch_losses", loss_val, np.float64)
            # (without keep no logit travels: the empty slice carries the number of classes, which is host metadata)
            self._got.put("logits", logits if self.keep else logits[:0], np.float32)
            if self.keep:
                self._got.put("clouds", cloud, np.float32)
            self._sizes.append(int(x.shape[0]))

    def result(self):
        """One device-to-host transfer -> dict: the per-item arrays preds, labels (int64), losses (float64: the cross-entropy per
        item), n_unique (int64); batch_sizes, batch_losses; classification_aggregates of them (avg_class_accuracy_seen is an addition
        to the reference's figures); with keep=True also logits (items, classes) and clouds (items, points, 3)."""
        out = _need_added(self._got, "ClassificationEvaluator").fetch()
        num_classes = (out["logits"] if self.keep else out.pop("logits")).shape[1]
        out["batch_sizes"] = np.asarray(self._sizes, dtype=np.int64)
        out.update(classification_aggregates(out["preds"], out["labels"], out["batch_sizes"], out["batch_losses"], out["n_unique"],
                                             num_classes))
        return out


# ------------------------------------------------------------------------------------------------ reconstruction
def reconstruction_aggregates(losses, reference_losses=None):
    """losses, mean_loss and, with the autoencoder's losses on the complete clouds, reference_losses, nre (their quotient, np.divide as
    the reference), mean_reference_loss, mean_nre (evaluate_samplenet.py:143, 151-152) from per-item float64 arrays."""
    out = {"losses": losses, "mean_loss": float(losses.mean())}
    if reference_losses is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            nre = np.divide(losses, reference_losses)
        out.update(reference_losses=reference_losses, nre=nre, mean_reference_loss=float(reference_losses.mean()),
                   mean_nre=float(nre.mean()))
    return out


def _per_cloud_loss(loss):
    """the reconstruction loss by name -> the op (reconstruction, cloud) -> (B,) that computes it per cloud"""
    if loss not in ("chamfer", "emd"):
        raise ValueError("loss: 'chamfer' or 'emd'")
    return ops.chamfer_mean_per_cloud if loss == "chamfer" else ops.emd_loss


class ReconstructionEvaluator:
    """autoencoder: a PointNetAE; sampler as ClassificationEvaluator's (the matched points are reconstructed from); loss "chamfer"
    (ops.chamfer_mean_per_cloud) or "emd" (ops.emd_loss' per-cloud costs): get_loss_ae_per_pc (sampler_autoencoder.py:149-167: the
    autoencoder loss one cloud at a time) for a batch; with_reference: also the autoencoder's loss on the complete cloud
    (evaluate_ae.py's ae_loss test_set file) and nre = loss / reference loss per cloud (evaluate_samplenet.py:145-152);
    keep: result() also returns sampled, sample_idx, reconstructions (the three arrays the reference script saves).  Clouds are (B,N,3)."""

    def __init__(self, autoencoder, sampler=None, loss="chamfer", with_reference=True, keep=False):
        self._per_cloud = _per_cloud_loss(loss)
        self.autoencoder, self.sampler = autoencoder, sampler
        self.loss, self.with_reference, self.keep = loss, bool(with_reference), bool(keep)
        self.reset()

    def reset(self):
        self._got = _Collected()

    def add(self, x):
        """One batch: x (B,N,3) on the GPU.  No synchronisation."""
        ops._need_gpu(x)
        ae = self.autoencoder
        with _EvalMode(ae, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            _simp, sampled, idx, nun = _sample_with_indices(self.sampler, x)
            recon = ae(_to_shape(sampled, ae)).contiguous()
            self._got.put("n_unique", nun, np.int64)
            self._got.put("losses", self._per_cloud(recon, x), np.float64)
            if self.with_reference:
                self._got.put("reference_losses", self._per_cloud(ae(_to_shape(x, ae)).contiguous(), x), np.float64)
            if self.keep:
                self._got.put("sampled", sampled, np.float32)
                self._got.put("sample_idx", idx, np.int64)
                self._got.put("reconstructions", recon, np.float32)

    def result(self):
        """One device-to-host transfer -> dict: the per-item float64 arrays losses, n_unique (int64) and, with_reference,
        reference_losses and nre (their quotient, np.divide as the reference); mean_loss, mean_unique, mean_reference_loss, mean_nre
        (evaluate_samplenet.py:143, 151-152); with keep=True sampled (items, M, 3), sample_idx (items, M) int64, reconstructions."""
        out = _need_added(self._got, "ReconstructionEvaluator").fetch()
        out["mean_unique"] = float(out["n_unique"].mean())  # (integers: their float64 mean, whatever the order of the sum)
        out.update(reconstruction_aggregates(out["losses"], out.get("reference_losses")))
        return out


# ------------------------------------------------------------------------------------------------ progressive sampling
def _ranked_cloud(sampler, x, size):
    """x (B,N,3) -> (ordered (B,size,3), order (B,size) int32, n_unique (B,) int32): the first `size` points of the cloud in the
    sampler's order of importance.  A module with `rank` (SampleNetProgressive): its ranking, n_unique the distinct nearest
    neighbours before completion; an FPSSampler: the farthest-point order of `size` points (honouring its `permute`) -- a prefix
    of a farthest-point order is the farthest-point sample of that size; None: the input order.  For the latter two n_unique is
    `size`, the number of points taken."""
    from .samplers import FPSSampler

    B, N, _ = x.shape
    if sampler is None or isinstance(sampler, FPSSampler):
        if size > N:
            raise ValueError("the largest size (%d) exceeds the cloud's %d points" % (size, N))
        nun = torch.full((B,), size, device=x.device, dtype=torch.int32)
        if sampler is None:
            order = torch.arange(size, device=x.device, dtype=torch.int32).expand(B, size).contiguous()
            return x[:, :size].contiguous(), order, nun
        # (one randperm on the default device, as the sampler draws it; sent from pinned memory, so that add() does not synchronise)
        perm = torch.randperm(N).pin_memory().to(x.device, non_blocking=True) if sampler.permute else None
        src = x[:, perm, :].contiguous() if perm is not None else x
        order = ops.furthest_point_sample(src, size, ops.BNC)
        ordered = ops.group_point(src, order.unsqueeze(-1)).squeeze(2).contiguous()
        return ordered, (perm.int()[order.long()] if perm is not None else order), nun
    if not hasattr(sampler, "rank"):
        raise TypeError("sampler: a module with rank() (SampleNetProgressive), an FPSSampler or None")
    xin = x if sampler.input_shape == "bnc" else x.permute(0, 2, 1).contiguous()
    ordered, order, nun = sampler.rank(xin)
    if sampler.output_shape != "bnc":
        ordered = ordered.permute(0, 2, 1)
    if ordered.shape[1] < size:
        raise ValueError("the largest size (%d) exceeds the %d points the sampler ranks" % (size, ordered.shape[1]))
    return ordered[:, :size].contiguous(), order[:, :size].contiguous(), nun


def _default_sizes(sampler, sizes):
    if sizes is None:
        sizes = getattr(sampler, "sizes", None)
        if sizes is None and getattr(sampler, "num_out_points", None) is not None:
            sizes = [sampler.num_out_points]
    if sizes is None:
        raise ValueError("sizes: needed when the sampler has none of its own")
    sizes = sorted(int(s) for s in sizes)
    if not sizes or sizes[0] < 1 or len(set(sizes)) != len(sizes):
        raise ValueError("sizes must be distinct positive integers")
    return sizes


class ProgressiveClassificationEvaluator:
    """The classifier's figures at EVERY sample size from one ranking per batch (infer_samplenet_progressive.py:207-212 feeding
    evaluate_samplenet.py:156-277 once per size).  classifier, reg_weight, keep: as ClassificationEvaluator; sampler: a module with
    `rank` (SampleNetProgressive), an FPSSampler (the baseline curve) or None (the input order); sizes: default the sampler's.
    Clouds are (B,N,3)."""

    def __init__(self, classifier, sampler, sizes=None, reg_weight=0.001, keep=False):
        self.classifier, self.sampler = classifier, sampler
        self.sizes = _default_sizes(sampler, sizes)
        self.reg_weight, self.keep = float(reg_weight), bool(keep)
        self.reset()

    def reset(self):
        self._got, self._batch = _Collected(), []

    def add(self, x, labels):
        """One batch: x (B,N,3) and labels (B,) on the GPU: ranked once, classified once per size.  No synchronisation."""
        ops._need_gpu(x, labels)
        with _EvalMode(self.classifier, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            ordered, order, nun = _ranked_cloud(self.sampler, x, self.sizes[-1])
            for s in self.sizes:
                logits, pred, ce, loss_val = _classify_batch(self.classifier, ordered[:, :s].contiguous(), labels, self.reg_weight)
                self._got.put(("preds", s), pred, np.int64)
                self._got.put(("losses", s), ce, np.float64)
                self._got.put(("batch_losses", s), loss_val, np.float64)
                self._got.put(("logits", s), logits if self.keep else logits[:0], np.float32)  # (as ClassificationEvaluator.add)
            self._got.put("labels", labels.clone(), np.int64)  # (a copy, as there)
            self._got.put("n_unique", nun, np.int64)
            self._batch.append(int(x.shape[0]))
            if self.keep:
                self._got.put("ordered", ordered, np.float32)
                self._got.put("order", order, np.int64)

    def result(self):
        """One device-to-host transfer -> {"sizes", "n_unique" (items,) int64, "mean_unique", "by_size": {s: ...}}: by_size[s] holds
        what ClassificationEvaluator.result() holds for the first s ranked points (preds, labels, losses, batch_sizes, batch_losses,
        classification_aggregates of them) except the unique counts, which belong to the ranking; with keep=True by_size[s]["logits"]
        and, at the top, "ordered" (items, max size, 3) and "order" (items, max size) int64."""
        got = _need_added(self._got, "ProgressiveClassificationEvaluator").fetch()
        batch_sizes = np.asarray(self._batch, dtype=np.int64)
        out = {"sizes": list(self.sizes), "n_unique": got["n_unique"], "by_size": {}}
        for s in self.sizes:
            r = {"preds": got["preds", s], "labels": got["labels"], "losses": got["losses", s], "batch_sizes": batch_sizes,
                 "batch_losses": got["batch_losses", s]}
            if self.keep:
                r["logits"] = got["logits", s]
            r.update(classification_aggregates(r["preds"], r["labels"], batch_sizes, r["batch_losses"], out["n_unique"],
                                               got["logits", s].shape[1]))
            out["mean_unique"] = r.pop("mean_unique")  # (the ranking's, the same at every size)
            out["by_size"][s] = r
        if self.keep:
            out["ordered"], out["order"] = got["ordered"], got["order"]
        return out


class ProgressiveReconstructionEvaluator:
    """The autoencoder's per-cloud loss at EVERY sample size from one ranking per batch (evaluate_samplenet_progressive.py:105-141).
    autoencoder, loss, with_reference, keep: as ReconstructionEvaluator -- the reference loss (the autoencoder on the complete cloud)
    is computed once per batch, the nre per size; sampler, sizes: as ProgressiveClassificationEvaluator.  Clouds are (B,N,3)."""

    def __init__(self, autoencoder, sampler, sizes=None, loss="chamfer", with_reference=True, keep=False):
        self._per_cloud = _per_cloud_loss(loss)
        self.autoencoder, self.sampler = autoencoder, sampler
        self.sizes = _default_sizes(sampler, sizes)
        self.loss, self.with_reference, self.keep = loss, bool(with_reference), bool(keep)
        self.reset()

    def reset(self):
        self._got = _Collected()

    def add(self, x):
        """One batch: x (B,N,3) on the GPU: ranked once, reconstructed once per size.  No synchronisation."""
        ops._need_gpu(x)
        ae = self.autoencoder
        with _EvalMode(ae, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            ordered, order, nun = _ranked_cloud(self.sampler, x, self.sizes[-1])
            for s in self.sizes:
                recon = ae(_to_shape(ordered[:, :s].contiguous(), ae)).contiguous()
                self._got.put(("losses", s), self._per_cloud(recon, x), np.float64)
                if self.keep:
                    self._got.put(("reconstructions", s), recon, np.float32)
            if self.with_reference:
                self._got.put("reference_losses", self._per_cloud(ae(_to_shape(x, ae)).contiguous(), x), np.float64)
            self._got.put("n_unique", nun, np.int64)
            if self.keep:
                self._got.put("ordered", ordered, np.float32)
                self._got.put("order", order, np.int64)

    def result(self):
        """One device-to-host transfer -> {"sizes", "n_unique", "mean_unique", "by_size": {s: reconstruction_aggregates (losses,
        mean_loss and, with_reference, reference_losses -- the same array at every size --, nre, mean_reference_loss, mean_nre)}};
        with keep=True by_size[s]["reconstructions"] and, at the top, "ordered" and "order" (int64)."""
        got = _need_added(self._got, "ProgressiveReconstructionEvaluator").fetch()
        out = {"sizes": list(self.sizes), "n_unique": got["n_unique"], "mean_unique": float(got["n_unique"].mean()), "by_size": {}}
        for s in self.sizes:
            r = reconstruction_aggregates(got["losses", s], got.get("reference_losses"))
            if self.keep:
                r["reconstructions"] = got["reconstructions", s]
            out["by_size"][s] = r
        if self.keep:
            out["ordered"], out["order"] = got["ordered"], got["order"]
        return out


# ------------------------------------------------------------------------------------------------ retrieval
def retrieval_aggregates(ap, prec, n_relevant):
    """The figures of a retrieval experiment from the per-query arrays of ops.retrieval_metrics, in float64: ap (n,), prec (n, L),
    n_relevant (n,).  A query is valid when another shape carries its label (n_relevant > 0; its ap and prec are NaN otherwise) and
    only valid queries enter a mean: map = mean ap, pr_curve (L,) = mean precision at recall l / L, auc = mean of pr_curve (the
    normalised area on that recall grid), n_valid.  No valid query: NaN everywhere, n_valid 0."""
    ap, prec = np.asarray(ap, dtype=np.float64), np.asarray(prec, dtype=np.float64)
    valid = np.asarray(n_relevant) > 0
    n_valid = int(valid.sum())
    if n_valid == 0:
        curve = np.full(prec.shape[1], np.nan)
        return {"map": float("nan"), "pr_curve": curve, "auc": float("nan"), "n_valid": 0}
    curve = prec[valid].sum(axis=0) / n_valid
    return {"map": float(ap[valid].sum() / n_valid), "pr_curve": curve, "auc": float(curve.sum() / len(curve)), "n_valid": n_valid}


def _descriptors(classifier, cloud):
    """one batch of one cloud size through the classifier: its shape descriptor, end_points["retrieval_vectors"] (B, 256)"""
    return classifier(_to_shape(cloud, classifier))[1]["retrieval_vectors"].contiguous()


class RetrievalEvaluator:
    """Shape retrieval on the classifier's descriptor (end_points["retrieval_vectors"], pointnet_cls.py:111), all shapes added
    against each other.  classifier, sampler, match_output: as ClassificationEvaluator; levels: the recall grid l / levels of the
    precision-recall curve; keep: result() also returns the descriptors and the ranking.  Clouds are (B,N,3); at most 8192 in all."""

    def __init__(self, classifier, sampler=None, match_output=True, levels=20, keep=False):
        self.classifier, self.sampler = classifier, sampler
        self.match_output, self.levels, self.keep = bool(match_output), int(levels), bool(keep)
        self.reset()

    def reset(self):
        self._kept = _Collected()  # (result() takes these columns on the device, scores them there and fetches the scores)

    def add(self, x, labels):
        """One batch: x (B,N,3) and labels (B,) integer class indices on the GPU.  No synchronisation."""
        ops._need_gpu(x, labels)
        with _EvalMode(self.classifier, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            simp, match, _idx, _nun = _sample_with_indices(self.sampler, x)
            self._kept.put("descriptors", _descriptors(self.classifier, match if self.match_output else simp), np.float32)
            self._kept.put("labels", labels.reshape(-1).int(), np.int64)

    def result(self):
        """One launch and one device-to-host transfer -> dict: the per-query arrays ap (float64; NaN for a query without a relevant
        shape), prec (items, levels), n_relevant, labels (int64), retrieval_aggregates of them (map, pr_curve, auc, n_valid); with
        keep=True also descriptors (items, C) float32 and order (items, items - 1) int64, the ranking of every query."""
        kept = _need_added(self._kept, "RetrievalEvaluator")
        desc, labels = kept.on_device("descriptors"), kept.on_device("labels")
        scored = ops.retrieval_metrics(desc, labels, self.levels, return_order=self.keep)
        got = _Collected()
        got.put("ap", scored[0], np.float64)
        got.put("prec", scored[1], np.float64)
        got.put("n_relevant", scored[2], np.int64)
        got.put("labels", labels, np.int64)
        if self.keep:
            got.put("descriptors", desc, np.float32)
            got.put("order", scored[3], np.int64)
        out = got.fetch()
        out.update(retrieval_aggregates(out["ap"], out["prec"], out["n_relevant"]))
        return out


class ProgressiveRetrievalEvaluator:
    """The retrieval figures at EVERY sample size from one ranking per batch: the cloud is ranked once (_ranked_cloud), the classifier
    run on every prefix, the descriptors kept as (sizes, items, C) and scored in ONE launch.  classifier, levels: as
    RetrievalEvaluator; sampler, sizes: as ProgressiveClassificationEvaluator.  Clouds are (B,N,3)."""

    def __init__(self, classifier, sampler, sizes=None, levels=20):
        self.classifier, self.sampler = classifier, sampler
        self.sizes = _default_sizes(sampler, sizes)
        self.levels = int(levels)
        self.reset()

    def reset(self):
        self._kept = _Collected()  # (as RetrievalEvaluator's)

    def add(self, x, labels):
        """One batch: x (B,N,3) and labels (B,) on the GPU: ranked once, described once per size.  No synchronisation."""
        ops._need_gpu(x, labels)
        with _EvalMode(self.classifier, self.sampler), torch.no_grad():
            x = x.contiguous().float()
            ordered, _order, _nun = _ranked_cloud(self.sampler, x, self.sizes[-1])
            for s in self.sizes:
                self._kept.put(("descriptors", s), _descriptors(self.classifier, ordered[:, :s].contiguous()), np.float32)
            self._kept.put("labels", labels.reshape(-1).int(), np.int64)

    def result(self):
        """One launch for all sizes and one device-to-host transfer -> {"sizes", "labels", "n_relevant" (the labels alone decide
        it: the same at every size), "by_size": {s: ap, prec, retrieval_aggregates of them}}."""
        kept = _need_added(self._kept, "ProgressiveRetrievalEvaluator")
        labels = kept.on_device("labels")
        ap, prec, n_relevant = ops.retrieval_metrics(torch.stack([kept.on_device(("descriptors", s)) for s in self.sizes]), labels,
                                                     self.levels)
        got = _Collected()  # (ap (sizes, items) and prec (sizes, items, levels): here a size is an item of the column)
        got.put("ap", ap, np.float64)
        got.put("prec", prec, np.float64)
        got.put("n_relevant", n_relevant, np.int64)
        got.put("labels", labels, np.int64)
        got = got.fetch()
        out = {"sizes": list(self.sizes), "n_relevant": got["n_relevant"], "labels": got["labels"], "by_size": {}}
        for k, s in enumerate(self.sizes):
            r = {"ap": got["ap"][k], "prec": got["prec"][k]}
            r.update(retrieval_aggregates(r["ap"], r["prec"], out["n_relevant"]))
            out["by_size"][s] = r
        return out


# ------------------------------------------------------------------------------------------------ segmentation
def segmentation_aggregates(cloud_counts, means, categories=None, parts_of_category=None):
    """The figures of a per-point evaluation from cloud_counts (clouds, C, 3) = per cloud and class (points labelled c, valid points
    predicted c, valid points with pred == label == c) and the per-batch means (batches, 3) of ops.segmentation_terms, in int64 /
    float64.  A point whose label lies outside [0, C) is ignored: it is in no count.  With L_c, P_c, T_c the three columns summed
    over every cloud:
        total_valid        = sum_c L_c
        overall_accuracy   = sum_c T_c / total_valid                       (NaN without a valid point)
        class_accuracies_c = T_c / L_c, and 0 for a class that is predicted but never labelled (L_c = 0 < P_c)
        class_iou_c        = T_c / (L_c + P_c - T_c)
        both are NaN for a class absent from labels AND predictions (L_c = P_c = 0), and such a class is left out of
        mean_class_accuracy and miou, the plain means over the remaining classes (NaN when none remains)
        mean_loss          = sum_j means_j[0] means_j[2] / sum_j means_j[2]: the weighted mean loss over all valid points of all
                             batches (a batch without a valid point adds nothing)
    With parts_of_category (category -> the class indices of its parts) and categories (clouds,), the ShapeNet-part figures: only the
    cloud's own category's parts count; a part's IoU in a cloud is T / (L + P - T) of that cloud's counts and 1 when the part is
    absent from both its labels and its predictions (L = P = 0); cloud_iou = the mean over the category's parts;
    instance_miou = the mean of cloud_iou over the clouds; category_iou[k] = the mean of cloud_iou over the clouds of category k (NaN
    for a category without a cloud); category_miou = the mean over the categories that have a cloud.  A prediction outside the
    cloud's own parts is counted as it is: it belongs to no part of the category."""
    counts = np.asarray(cloud_counts).astype(np.int64)
    means = np.asarray(means, dtype=np.float64).reshape(-1, 3)
    L, P, T = (counts[:, :, k].sum(0) for k in range(3))
    present = (L + P) > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(present, T / np.maximum(L, 1), np.nan)
        iou = np.where(present, T / np.maximum(L + P - T, 1), np.nan)
        total = int(L.sum())
        den = means[:, 2]
        num = np.where(den > 0, means[:, 0] * den, 0.0)
        out = {"total_valid": total, "overall_accuracy": float(T.sum()) / total if total else float("nan"),
               "class_labelled": L, "class_predicted": P, "class_correct": T, "class_accuracies": acc, "class_iou": iou,
               "mean_class_accuracy": float(acc[present].mean()) if present.any() else float("nan"),
               "miou": float(iou[present].mean()) if present.any() else float("nan"),
               "mean_loss": float(num.sum() / den.sum()) if den.sum() > 0 else float("nan")}
    if parts_of_category is not None:
        cats = np.asarray(categories).astype(np.int64)
        cloud_iou = np.empty(len(cats), dtype=np.float64)
        for b, k in enumerate(cats):
            parts = np.asarray(parts_of_category[int(k)], dtype=np.int64)
            l, p, t = (counts[b, parts, j].astype(np.float64) for j in range(3))
            union = l + p - t
            cloud_iou[b] = np.where(union > 0, t / np.maximum(union, 1), 1.0).mean()
        keys = sorted(parts_of_category)
        cat_iou = np.array([cloud_iou[cats == k].mean() if (cats == k).any() else np.nan for k in keys])
        out.update({"cloud_iou": cloud_iou, "instance_miou": float(cloud_iou.mean()), "category_iou": dict(zip(keys, cat_iou)),
                    "category_miou": float(np.nanmean(cat_iou)) if np.isfinite(cat_iou).any() else float("nan")})
    return out


class SegmentationEvaluator:
    """network: a per-point network, network(xyz (B,N,3), features (B,Cf,N) or None) -> logits (B,num_classes,N) or (B,N,num_classes)
    (PointNet2SemSegSSG returns the first as a view of the second's memory, read without a copy); class_weights (num_classes,) or
    None: the loss's weights; parts_of_category: {category: the class indices of its parts} for the ShapeNet-part figures (add then
    takes the clouds' categories).  Labels outside [0, num_classes) are ignored points.  add() runs the network in eval mode under
    no_grad and makes ONE ops.segmentation_terms call; the per-cloud counts and the loss pieces stay on the device, nothing
    synchronises; result() makes one transfer and forms segmentation_aggregates (the definitions are in its docstring)."""

    def __init__(self, network, num_classes, class_weights=None, parts_of_category=None):
        self.network, self.num_classes = network, int(num_classes)
        self.class_weights = class_weights
        self.parts_of_category = None if parts_of_category is None else {int(k): tuple(int(p) for p in v)
                                                                       for k, v in dict(parts_of_category).items()}
        self.reset()

    def reset(self):
        self._got = _Collected()

    def add(self, xyz, features, labels, categories=None):
        """One batch: xyz (B,N,3), features (B,Cf,N) or None, labels (B,N) integer, categories (B,) integer (needed with
        parts_of_category).  No synchronisation."""
        ops._need_gpu(xyz, features, labels, categories)
        if self.parts_of_category is not None and categories is None:
            raise ValueError("SegmentationEvaluator.add: parts_of_category was given, so every batch needs its categories")
        with _EvalMode(self.network), torch.no_grad():
            logits = self.network(xyz, features)
            if logits.dim() != 3 or self.num_classes not in (logits.shape[1], logits.shape[2]):
                raise ValueError("SegmentationEvaluator.add: the network returned %s for %d classes" % (tuple(logits.shape), self.num_classes))
            _ce, _pred, counts, means = ops.segmentation_terms(logits, labels, self.class_weights)
            self._got.put("cloud_counts", counts, np.int64)
            self._got.put("means", means.reshape(1, 3), np.float64)
            if categories is not None:
                self._got.put("categories", categories.clone(), np.int64)

    def result(self):
        """One device-to-host transfer -> dict: cloud_counts (clouds, num_classes, 3) int64, means (batches, 3) float64, categories when
        given, and segmentation_aggregates of them."""
        out = _need_added(self._got, "SegmentationEvaluator").fetch()
        out.update(segmentation_aggregates(out["cloud_counts"], out["means"], out.get("categories"), self.parts_of_category))
        return out

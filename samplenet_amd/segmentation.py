"""The per-point (semantic / part segmentation) loss on the library's terms kernel.

    segmentation_loss(logits, labels, class_weights=None, ignore_index=-100, fused=FUSED_DEFAULT) -> 0-d loss

logits: (B,N,C), or (B,C,N) when that is a transposed view of (B,N,C) rows -- what PointNet2SemSegSSG returns as
`logits.transpose(1, 2)`; labels (B,N) integer class indices.  The loss is torch's
F.cross_entropy(weight=class_weights, ignore_index=ignore_index) with reduction 'mean': sum over the kept points of w_label ce,
divided by the sum of their weights.

fused=False is that torch call.  fused=True is ops.segmentation_mean_loss (sn_segmentation_terms_forward / _backward: one forward
pair and one backward launch, no float atomics, bit-identical from run to run).  The kernel ignores every label outside [0, C), so
an ignore_index outside that range (-100, -1, 255 with fewer classes) needs no work; one INSIDE the range is rewritten to -1 on the
device first.  A label that is neither a class nor ignore_index is an error in torch and an ignored point on the fused route.
"""
import torch.nn.functional as F

from . import ops

# Which route segmentation_loss takes when the caller does not say: the one tools/seg_bench.py's table shows ahead at both of its
# shapes beyond the larger spread, and torch otherwise.  profiles/seg/seg_bench.txt: the mean loss forward + backward took 0.157 /
# 0.158 ms fused against 0.136 / 0.139 ms with F.cross_entropy at (32 x 4096, 13) / (32 x 2048, 50) -- torch is ahead of the loss ALONE
# (the terms in one call, with argmax and counts, are 13x / 9.6x ahead of the torch composition: DESIGN 4.18).
FUSED_DEFAULT = False


def fused_labels(labels, num_classes, ignore_index=-100):
    """labels as the kernel's rule reads them: unchanged when ignore_index lies outside [0, num_classes) (the kernel ignores it
    already), otherwise a copy with ignore_index rewritten to -1.  On the labels' device, no synchronisation."""
    if 0 <= int(ignore_index) < int(num_classes):
        return labels.masked_fill(labels == int(ignore_index), -1)
    return labels


def segmentation_loss(logits, labels, class_weights=None, ignore_index=-100, fused=None):
    """The mean per-point cross-entropy (module docstring).  fused=None takes FUSED_DEFAULT."""
    fused = FUSED_DEFAULT if fused is None else fused
    if logits.dim() != 3 or labels.dim() != 2:
        raise ValueError("segmentation_loss: logits (B,N,C) or (B,C,N) and labels (B,N), got %s and %s"
                         % (tuple(logits.shape), tuple(labels.shape)))
    flipped = tuple(logits.shape[:2]) != tuple(labels.shape) or (
        logits.shape[1] == logits.shape[2] and not logits.is_contiguous() and logits.transpose(1, 2).is_contiguous())
    num_classes = logits.shape[1] if flipped else logits.shape[2]
    if fused:
        return ops.segmentation_mean_loss(logits, fused_labels(labels, num_classes, ignore_index), class_weights)
    per_class = logits if flipped else logits.transpose(1, 2)  # F.cross_entropy wants (B,C,N)
    return F.cross_entropy(per_class, labels.long(), weight=class_weights, ignore_index=int(ignore_index))

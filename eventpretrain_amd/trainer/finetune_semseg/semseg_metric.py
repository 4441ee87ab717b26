"""Segmentation metrics with the reference's names and signatures (reference trainer/finetune_semseg/semseg_metric.py). The confusion
table comes from ops.semseg_metrics (the logits are resized to the label's size inside the kernel); the two conversions are the
reference's double-precision formulas on whatever device the table is on."""
import torch

from ... import ops
from .semseg_loss import prediction_map


def semseg_compute_confusion(args, target, predict):
    """The reference's argument order, as ft_semseg_val calls it: `target` is the LOGITS (B, num_classes, h, w) of any spatial size and
    `predict` the LABEL map int64 (B, 1, H, W). -> int64 [num_classes, num_classes], rows = label, columns = argmax of the logits
    resized to (H, W), over the pixels whose label is not args.ignore_label."""
    if target.shape[1] != args.num_classes:
        raise ValueError(f"the logits have {target.shape[1]} channels, args.num_classes is {args.num_classes}")
    if getattr(args, "sample_mode", "bilinear") != "bilinear":
        raise NotImplementedError(f"sample_mode {args.sample_mode!r}: only 'bilinear'")
    m, B, h, w = prediction_map(target)
    confusion = torch.zeros(args.num_classes, args.num_classes, dtype=torch.int64, device=m.device)
    table = torch.zeros(1, 3, dtype=torch.float32, device=m.device)
    cursor = torch.zeros(1, dtype=torch.int64, device=m.device)
    ops.semseg_metrics(m, B, h, w, predict, args.ignore_label, table, cursor, confusion=confusion)
    return confusion


def _hits_rows_cols(confusion):
    t = confusion.to(torch.float64)
    return t.diagonal(), t.sum(1), t.sum(0)


def semseg_confusion_to_miou(confusion):
    """Mean over ALL classes (absent ones count as 0) of 100 * hits / max(labelled + predicted - hits, 1e-12), in double."""
    hits, rows, cols = _hits_rows_cols(confusion)
    return (100.0 * hits / torch.clamp(rows + cols - hits, min=1e-12)).mean()


def semseg_confusion_to_macc(confusion):
    """Mean over ALL classes of 100 * hits / max(labelled, 1e-12), in double."""
    hits, rows, _ = _hits_rows_cols(confusion)
    return (100.0 * hits / torch.clamp(rows, min=1e-12)).mean()

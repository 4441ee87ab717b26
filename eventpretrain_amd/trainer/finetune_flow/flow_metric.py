"""Flow metrics with the reference's names and signatures (reference trainer/finetune_flow/flow_metric.py), in plain torch on whatever
device the operands are on: they take predictions ALREADY at the label's size (resize_flow's result), as the reference's do.
flow_compute_metrics is the fused call on a low-resolution prediction (ops.flow_metrics: the resize and the scaling happen inside the
kernel), what ft_flow_val records per batch."""
import torch

from ... import ops
from ..finetune_semseg.semseg_loss import prediction_map


def flow_compute_mag(matrix, mask=None):
    """(B, 2, H, W) -> the L2 norm over the two components, (B, H, W), or its entries where mask == 1."""
    mag = torch.sum(matrix ** 2, dim=1).sqrt()
    return mag if mask is None else mag[mask == 1]


def flow_compute_epe(predict, target, mask=None):
    return flow_compute_mag(predict - target, mask=mask)


def flow_compute_aee(epe):
    return epe.view(-1).mean()


def flow_compute_outlier(epe, mag):
    """The share, in percent, of entries with epe > 3 and epe / mag > 0.05 (a zero magnitude gives inf, which counts)."""
    epe, mag = epe.view(-1), mag.view(-1)
    return ((epe > 3.0) & ((epe / mag) > 0.05)).float().mean() * 100


def flow_compute_aee_outlier(predict, target, mask=None):
    epe = flow_compute_epe(predict, target, mask=mask)
    mag = flow_compute_mag(target, mask=mask)
    return flow_compute_aee(epe), flow_compute_outlier(epe, mag)


def flow_compute_metrics(args, predict, target, target_valid, events_voxel_grid_org):
    """(B, 2, h, w) prediction of any spatial size, the labels, the unnormalised voxel grid (B, C, H, W) -> (l1, aee, outlier), 0-d
    float32 on the device: FlowLoss of resize_flow(predict), and flow_compute_aee_outlier over the reference's sparse mask
    (target_valid non-zero and an event at the pixel; reference ft_flow_trainer.py:194-203)."""
    if getattr(args, "sample_mode", "bilinear") != "bilinear":
        raise NotImplementedError(f"sample_mode {args.sample_mode!r}: only 'bilinear'")
    if predict.dim() != 4 or predict.shape[1] != 2:
        raise ValueError(f"expected a (B, 2, h, w) flow prediction, got shape {tuple(predict.shape)}")
    m, B, h, w = prediction_map(predict)
    table = torch.zeros(1, 3, dtype=torch.float32, device=m.device)
    cursor = torch.zeros(1, dtype=torch.int64, device=m.device)
    ops.flow_metrics(m, B, h, w, target, target_valid, args.max_flow, events_voxel_grid_org, table, cursor)
    return table[0, 0], table[0, 1], table[0, 2]

"""The flow objective with the reference's name and signature (reference trainer/finetune_flow/flow_loss.py:5-17 `FlowLoss`: the mean
of |predict - target| over both components of the pixels with target_valid >= 0.5 and |target| < args.max_flow). The reference runs
resize_flow (utils/reshape.py:45-54: bilinear resize to the label size, x times W / w, y times H / h) first and calls this on the
result; here `predict` may have ANY spatial size: the resize and the scaling happen inside the kernels (ops.FlowObjectiveFn), pixel by
pixel in registers, so the trainer hands over the heads' 14 x 14 predictions as they are."""
import torch.nn as nn

from ... import ops
from ..finetune_semseg.semseg_loss import prediction_map


class FlowLoss(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.sample_mode = getattr(args, "sample_mode", "bilinear")
        if self.sample_mode != "bilinear":
            raise NotImplementedError(f"sample_mode {self.sample_mode!r}: only 'bilinear' (what both of the reference's entry scripts set)")

    def forward(self, predict, target, target_valid):
        """predict (B, 2, h, w) of any spatial size, target float32 (B, 2, H, W), target_valid (B, 1, H, W) -> the L1 loss of
        resize_flow(predict, (H, W)); NaN, with a zero gradient, when no pixel is valid."""
        if predict.dim() != 4 or predict.shape[1] != 2:
            raise ValueError(f"expected a (B, 2, h, w) flow prediction, got shape {tuple(predict.shape)}")
        m, B, h, w = prediction_map(predict)
        return ops.FlowObjectiveFn.apply(m, B, h, w, target, target_valid, self.args.max_flow)

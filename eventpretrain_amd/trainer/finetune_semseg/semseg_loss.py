"""The segmentation objective with the reference's name and signature (reference trainer/finetune_semseg/semseg_loss.py:8-19
`SemsegLoss`: nn.CrossEntropyLoss(ignore_index) and the batch-wide Dice loss of :71-112). The reference resizes the heads' logits to
the label size first and calls this on the result; here `predict` may have ANY spatial size: the bilinear resize to the label's size
happens inside the kernels (ops.SemsegObjectiveFn), pixel by pixel in registers, so the trainer hands over the heads' 14 x 14
predictions as they are."""
import torch
import torch.nn as nn

from ... import ops


def prediction_map(predict):
    """(B, C, h, w) logits -> (token-major float32 [B*h*w, C], B, h, w). The permuted view a head returns (from_map of a map whose rows
    may be further apart than C) is consumed where it lies: no copy; any other layout is gathered into a contiguous map."""
    if predict.dim() != 4:
        raise ValueError(f"expected (B, C, h, w) logits, got shape {tuple(predict.shape)}")
    B, C, h, w = predict.shape
    if predict.dtype != torch.float32:
        predict = predict.float()
    return predict.permute(0, 2, 3, 1).reshape(B * h * w, C), B, h, w      # (reshape: a view wherever the strides allow one)


class SemsegLoss(nn.Module):
    def __init__(self, args, num_classes=13, ignore_index=None):
        super().__init__()
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.sample_mode = getattr(args, "sample_mode", "bilinear")
        if self.sample_mode != "bilinear":
            raise NotImplementedError(f"sample_mode {self.sample_mode!r}: only 'bilinear' (what both of the reference's entry scripts set)")

    def forward(self, predict, target):
        """predict (B, num_classes, h, w) logits of any spatial size, target int64 (B, 1, H, W) -> (ce_loss, dice_loss) of the logits
        resized to (H, W)."""
        if predict.shape[1] != self.num_classes:
            raise ValueError(f"predict has {predict.shape[1]} channels, the loss was built for {self.num_classes} classes")
        m, B, h, w = prediction_map(predict)
        return ops.SemsegObjectiveFn.apply(m, B, h, w, target, self.ignore_index)

#!/usr/bin/env python3
"""Fixture of the segmentation objective, made by the REFERENCE's own code on the CPU -> tests/golden/ft_semseg_objective.npz: its
`resize` (utils/reshape.py), `SemsegLoss` (trainer/finetune_semseg/semseg_loss.py) and `semseg_compute_confusion` / `_to_miou` /
`_to_macc` (semseg_metric.py) over the cases of tests/semseg_truth.py.

Runs where a checkout of the reference is at hand (EVP_REFERENCE=<its root>), never on the GPU machine. Nothing of the reference is
copied: the fixture holds recorded numbers. The inputs are closed-form (semseg_truth.case_inputs) and re-made by the tests.

Per case: the logits are fed in float64, so the Dice loss, its gradient in the low-resolution map, the confusion table, mIoU and mAcc are
float64 results; the reference casts to float32 in front of its cross entropy, so `ce` and its gradient carry float32 rounding."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import semseg_truth as st  # noqa: E402
from eventpretrain_amd.testing import make_args  # noqa: E402
from oracle import gen_golden  # noqa: E402  (the reference's import path)


def main():
    from trainer.finetune_semseg.semseg_loss import SemsegLoss
    from trainer.finetune_semseg.semseg_metric import semseg_compute_confusion, semseg_confusion_to_macc, semseg_confusion_to_miou
    from utils.reshape import resize
    out = {}
    for name, s in st.CASES.items():
        B, C, h, w = s["B"], s["C"], s["h"], s["w"]
        a = make_args(device="cpu", num_classes=C, ignore_label=st.IGNORE, sample_mode="bilinear")
        logits, label = st.case_inputs(name)
        x = logits.double().requires_grad_(True)
        predict = resize(input=x.view(B, h, w, C).permute(0, 3, 1, 2), size=label.shape[2:], mode=a.sample_mode)
        ce, dice = SemsegLoss(a, num_classes=C, ignore_index=st.IGNORE)(predict, label)
        (g_ce,) = torch.autograd.grad(ce, x, retain_graph=True)
        (g_dice,) = torch.autograd.grad(dice, x)
        confusion = semseg_compute_confusion(a, predict.detach(), label)
        out.update({f"{name}|ce": ce.detach().double().numpy(), f"{name}|dice": dice.detach().double().numpy(),
                    f"{name}|grad_ce": g_ce.double().numpy(), f"{name}|grad_dice": g_dice.double().numpy(),
                    f"{name}|confusion": confusion.numpy(), f"{name}|miou": semseg_confusion_to_miou(confusion).numpy(),
                    f"{name}|macc": semseg_confusion_to_macc(confusion).numpy()})
    out["cases"] = np.array(json.dumps(list(st.CASES)))
    path = os.path.join(ROOT, "tests", "golden", "ft_semseg_objective.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    if not os.path.isdir(gen_golden.REF):
        raise SystemExit("set EVP_REFERENCE to the root of a checkout of the reference")
    gen_golden._ref()
    torch.set_num_threads(1)
    main()

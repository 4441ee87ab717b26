#!/usr/bin/env python3
"""Fixture of the optical-flow objective, made by the REFERENCE's own code on the CPU -> tests/golden/ft_flow_objective.npz: its
`resize_flow` (utils/reshape.py), `FlowLoss` (trainer/finetune_flow/flow_loss.py) and `flow_compute_aee_outlier` (flow_metric.py) over
the cases of tests/flow_truth.py, with the sparse mask made as its validation loop makes it (ft_flow_trainer.py: the L2 norm of the
unnormalised voxel grid over channels > 0, logical_and with the valid map).

Runs where a checkout of the reference is at hand (EVP_REFERENCE=<its root>), never on the GPU machine. Nothing of the reference is
copied: the fixture holds recorded numbers. The inputs are closed-form (flow_truth.case_inputs) and re-made by the tests.

Per case: the map is fed in float64, so the loss, its gradient in the low-resolution map and aee are float64 results (the two scale
factors pass through the reference's float32 tensor); the outlier share goes through the reference's `.float()`."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flow_truth as ft  # noqa: E402
from eventpretrain_amd.testing import make_args  # noqa: E402
from oracle import gen_golden  # noqa: E402  (the reference's import path)


def main():
    from trainer.finetune_flow.flow_loss import FlowLoss
    from trainer.finetune_flow.flow_metric import flow_compute_aee_outlier
    from utils.reshape import resize_flow
    out = {}
    for name, s in ft.CASES.items():
        B, h, w = s["B"], s["h"], s["w"]
        a = make_args(device="cpu", max_flow=s["max_flow"], sample_mode="bilinear")
        flow_map, target, valid, org = ft.case_inputs(name)
        x = flow_map.double().requires_grad_(True)
        predict = resize_flow(a, input=x.view(B, h, w, 2).permute(0, 3, 1, 2), size=target.shape[2:], mode=a.sample_mode)
        l1 = FlowLoss(a)(predict, target.double(), valid)
        (g_l1,) = torch.autograd.grad(l1, x)
        events_mask = torch.linalg.norm(org, ord=2, dim=1, keepdims=False) > 0
        sparse = torch.logical_and(valid.squeeze(1), events_mask)
        aee, outlier = flow_compute_aee_outlier(predict.detach(), target.double(), mask=sparse)
        out.update({f"{name}|l1": l1.detach().double().numpy(), f"{name}|grad_l1": g_l1.double().numpy(),
                    f"{name}|aee": aee.double().numpy(), f"{name}|outlier": outlier.double().numpy(),
                    f"{name}|n_sparse": np.array(int(sparse.sum()))})
    out["cases"] = np.array(json.dumps(list(ft.CASES)))
    path = os.path.join(ROOT, "tests", "golden", "ft_flow_objective.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    if not os.path.isdir(gen_golden.REF):
        raise SystemExit("set EVP_REFERENCE to the root of a checkout of the reference")
    gen_golden._ref()
    torch.set_num_threads(1)
    main()

#!/usr/bin/env python3
"""Writes tests/golden/dense_label_views.npz: the label side of the dense fine-tuning datasets' view augmentation as the REFERENCE's own
functions compute it (dataset/augmentation/view_augment.py:65-134), in the order ft_dsec_dataset.py / ft_mvsec_dataset.py call them under
one sample seed:

  evg_augment(args, grid, size, mode='bilinear', seed=seed)  -> the time-flip flag
  semseg_label_augment(args, label.float(), (H, W), seed=seed)
  flow_label_augment(args, flow, (H, W), time_flip_flag, seed=seed)
  flow_label_valid_augment(args, valid, (H, W), seed=seed)          valid = (norm(flow) > 0) & (|fx| < 1000) & (|fy| < 1000), as the dataset

for labels of 11 x 14, 5 x 300, 44 x 64 and 26 x 35 and seeds 0..11 (48 cases). The inputs are tests/dense_input_truth.py's deterministic
fills (255 labels; exact zeros, +-1000, 999.99994 and 1e-6 flows planted) and are not stored; the crop rows each case was made under are
(oracle.augment_oracle.draw_evg_params on RandomState(seed)). Asserted below: the stored cases hold accepted crop boxes and all four flip
pairs. Data only: tests/test_dense_input_host.py holds the project's restatement (tests/dense_input_truth.py) to these arrays bit for bit.

    EVP_REFERENCE=/path/to/reference python tools/gen_dense_input_golden.py"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import augment_oracle as ao  # noqa: E402
from oracle import gen_golden  # noqa: E402
import dense_input_truth as truth  # noqa: E402

CROP_MIN, BINS = 0.8, 5


def main():
    gen_golden._ref()
    from dataset.augmentation.view_augment import evg_augment, flow_label_augment, flow_label_valid_augment, semseg_label_augment
    args = SimpleNamespace(num_bins=BINS, crop_min=CROP_MIN)
    arrays = {"shapes": np.asarray(truth.GOLDEN_SHAPES, np.int64), "seeds": np.asarray(truth.GOLDEN_SEEDS, np.int64)}
    boxes, flips = 0, set()
    for i, (H, W) in enumerate(truth.GOLDEN_SHAPES):
        label, flow = torch.from_numpy(truth.label_input(H, W)), torch.from_numpy(truth.flow_input(H, W))
        valid = ((torch.norm(flow, p=2, dim=0, keepdim=False) > 0) & (flow[0].abs() < 1000) & (flow[1].abs() < 1000)).float().unsqueeze(0)
        grid = torch.zeros(BINS, H, W)
        rows = []
        for seed in truth.GOLDEN_SEEDS:
            _, tflag = evg_augment(args, grid, (H, W), mode="bilinear", seed=seed)
            prm = ao.draw_evg_params(np.random.RandomState(seed), H, W, CROP_MIN)
            assert int(tflag) == prm[5], (H, W, seed)
            rows.append(prm)
            lab = semseg_label_augment(args, label.float(), (H, W), seed=seed)
            fl = flow_label_augment(args, flow, (H, W), tflag, seed=seed)
            va = flow_label_valid_augment(args, valid, (H, W), seed=seed)
            assert lab.dtype == torch.int64 and int(lab.max()) <= 255 and fl.dtype == torch.float32 and va.dtype == torch.float32
            arrays[f"label_{i}_{seed}"] = lab.numpy().astype(np.uint8)      # (values <= 255: the int64 bits are these, widened)
            arrays[f"flow_{i}_{seed}"] = fl.numpy()
            arrays[f"valid_{i}_{seed}"] = va.numpy().astype(np.uint8)       # (0.0 / 1.0)
            boxes += int(tuple(prm[:4]) != (0, 0, W, H))
            flips.add((prm[4], prm[5]))
        arrays[f"rows_{i}"] = np.asarray(rows, np.int32)
    assert boxes >= 8, f"only {boxes} accepted crop boxes among the stored cases"
    assert len(flips) == 4, f"flip pairs seen: {sorted(flips)}"
    print(f"{boxes} accepted boxes of {len(truth.GOLDEN_SHAPES) * len(truth.GOLDEN_SEEDS)} cases, flip pairs {sorted(flips)}")
    gen_golden.save("dense_label_views", **arrays)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/ft_sensor_recipe.npz: the sensor-resolution fine-tuning recipe (N-Caltech101, CIFAR10-DVS, DVS128-Gesture,
UCF101-DVS, ES-ImageNet with 5 bins: ft_n_caltech101_dataset.py:61-91 and siblings) as the REFERENCE's own functions compute it, on
non-square grids:

  validation  events_to_voxel_grid at the sensor's (H, W), unscaled, then view_resize to (S, S) in 'nearest' and 'bilinear' mode;
  train       seeded evg_augment(..., size=(S, S), mode=...) of the same grids, with the parameter rows
              oracle.augment_oracle.draw_evg_params gives for the same seeds.

(H, W, S) = (45, 60, 72) and (45, 62, 72): S = 72 keeps Hout + Wout > 128, the side on which ATen runs the generic bilinear kernel the
project restates (include/evtpretrain.h). The clips are sparse (a few hundred events) so that the compressed file stays small.
Data only: tests/test_ft_sensor_recipe_host.py holds the project's restatements (oracle.voxel_oracle.voxel_grid,
oracle.augment_oracle.evg_transform, tests/bilinear_truth.evg_bilinear) to these arrays bit for bit.

    EVP_REFERENCE=/path/to/reference python tools/gen_ft_sensor_golden.py"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden  # noqa: E402
from oracle.augment_oracle import draw_evg_params  # noqa: E402
from eventpretrain_amd.testing import synthetic_events  # noqa: E402

SHAPES = ((45, 60, 72), (45, 62, 72))
SEEDS = (3, 11, 29)
N_EVENTS = (260, 170)
MODES = ("nearest", "bilinear")


def main():
    gen_golden._ref()
    from dataset.augmentation.view_augment import evg_augment, view_resize
    from dataset.dataset_utils.events_to_voxel_grid import events_to_voxel_grid
    args = SimpleNamespace(num_bins=5, crop_min=0.8)
    arrays = {"shapes": np.asarray(SHAPES, np.int64), "seeds": np.asarray(SEEDS, np.int64)}
    for H, W, S in SHAPES:
        tag = f"{H}x{W}"
        clips = [synthetic_events(900 + 7 * W + i, n, width=W, height=H) for i, n in enumerate(N_EVENTS)]
        for i, ev in enumerate(clips):
            arrays[f"events_{tag}_{i}"] = ev
        grids = [events_to_voxel_grid(args, ev.copy(), (H, W)) for ev in clips]
        arrays[f"grid_{tag}"] = torch.stack(grids)
        for mode in MODES:
            arrays[f"val_{mode}_{tag}"] = torch.stack([view_resize(g, (S, S), mode) for g in grids])
            arrays[f"train_{mode}_{tag}"] = torch.stack([torch.stack([evg_augment(args, g, (S, S), mode=mode, seed=s)[0] for g in grids])
                                                         for s in SEEDS])
        arrays[f"params_{tag}"] = np.asarray([draw_evg_params(np.random.RandomState(s), H, W, args.crop_min) for s in SEEDS], np.int32)
    gen_golden.save("ft_sensor_recipe", **arrays)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/ft_ncars_recipe.npz: the N-Cars fine-tuning recipe (ft_n_cars_dataset.py:61-87) as the REFERENCE's own functions compute
it, in FinetuneNCarsDataset.__getitem__'s order under np.random.seed(s):

  get_random_index -> (H_c, W_c) = (int(max y) + 1, int(max x) + 1) of the window -> [train: events_augment(size=(H_c, W_c))] ->
  events_to_voxel_grid(size=(H_c, W_c)) -> [train: evg_augment(size=(S, S), mode) | val: view_resize((S, S), mode)]

with 5 bins, fix_events_num 300, validation windows that take the whole clip and S = 72 (Hout + Wout > 128: the side on which ATen runs the
generic bilinear kernel the project restates, include/evtpretrain.h). Five clips whose extents are 37 x 52, 48 x 64 (the capacity the tests
pad to), 9 x 13, 30 x 1 and 40 x 41, sparse (99 to 900 events) so that the compressed file stays small; two seeds per clip for training, both
resize modes. The seeds are chosen so that the stored samples hold an accepted crop box, both values of each flip coin, a clip too short
for erase / add (int(0.01 n) == 0) and an added row the per-clip bound actually moved -- asserted below.
Data only: tests/test_ft_ncars_host.py holds the project's restatement (a padded oracle.voxel_oracle.voxel_grid at the capacity,
oracle.augment_oracle.erase_add_apply / draw_evg_params on (H_c, W_c), evg_transform / tests/bilinear_truth.evg_bilinear) to these arrays
bit for bit.

    EVP_REFERENCE=/path/to/reference python tools/gen_ft_ncars_golden.py"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import augment_oracle as ao  # noqa: E402
from oracle import gen_golden  # noqa: E402
from eventpretrain_amd.testing import synthetic_events  # noqa: E402

EXTENTS = ((37, 52), (48, 64), (9, 13), (30, 1), (40, 41))      # (H, W) of the whole clip
N_EVENTS = (420, 900, 250, 99, 333)
SEEDS = (0, 5)
S, FIX, BINS = 72, 300, 5
MODES = ("nearest", "bilinear")


def clip(i):
    H, W = EXTENTS[i]
    ev = synthetic_events(1700 + i, N_EVENTS[i], width=W, height=H)
    ev[N_EVENTS[i] // 2, :2] = (W - 1, H - 1)       # the clip reaches its extent whatever the draw
    return ev


def main():
    gen_golden._ref()
    from dataset.augmentation.events_augment import events_augment, get_random_index
    from dataset.augmentation.view_augment import evg_augment, view_resize
    from dataset.dataset_utils.events_to_voxel_grid import events_to_voxel_grid
    args = SimpleNamespace(num_bins=BINS, crop_min=0.8, fix_events_num=FIX, val_fix_events_num=1000)
    arrays = {"extents": np.asarray(EXTENTS, np.int64), "seeds": np.asarray(SEEDS, np.int64),
              "recipe": np.asarray([S, FIX, BINS], np.int64)}
    boxes, flips, short, moved = 0, set(), 0, 0
    for i in range(len(EXTENTS)):
        ev = clip(i)
        arrays[f"events_{i}"] = ev
        for mode in MODES:
            # validation: the whole clip, no event augmentation, view_resize alone
            s0, s1 = get_random_index(args, ev, False)
            win = ev[s0:s1].copy()
            hw = int(win[:, 1].max()) + 1, int(win[:, 0].max()) + 1
            assert (s0, s1) == (0, ev.shape[0]) and hw == EXTENTS[i]
            grid = events_to_voxel_grid(args, win, size=hw)
            arrays[f"val_hw_{i}"] = np.asarray(hw, np.int64)
            arrays[f"val_grid_{i}"] = grid
            arrays[f"val_{mode}_{i}"] = view_resize(grid, (S, S), mode)
            for k, seed in enumerate(SEEDS):
                np.random.seed(seed)
                s0, s1 = get_random_index(args, ev, True)
                win = ev[s0:s1].copy()
                hw = int(win[:, 1].max()) + 1, int(win[:, 0].max()) + 1
                # the oracle's reading of the same stream: what the augmentation will draw for this window
                rs = np.random.RandomState(seed)
                assert ao.draw_window(rs, ev.shape[0], FIX) == (s0, s1)
                dec = ao.draw_erase_add(rs, win.shape[0])
                prm = ao.draw_evg_params(rs, hw[0], hw[1], args.crop_min)
                aug = events_augment(args, win.copy(), size=hw)
                grid = events_to_voxel_grid(args, aug.copy(), size=hw)
                view, _ = evg_augment(args, grid, (S, S), mode=mode)
                arrays[f"train_win_{i}_{k}"] = np.asarray([s0, s1], np.int64)
                arrays[f"train_hw_{i}_{k}"] = np.asarray(hw, np.int64)
                arrays[f"train_grid_{i}_{k}"] = grid
                arrays[f"train_{mode}_{i}_{k}"] = view
                if mode == MODES[0]:
                    boxes += int(tuple(prm[:4]) != (0, 0, hw[1], hw[0]))
                    flips.add(("h", prm[4])), flips.add(("t", prm[5]))
                    short += int(dec is None)
                    if dec is not None:
                        xy = win[dec[1], :2] + dec[2][:, :2]
                        moved += int(((xy[:, 0] > hw[1] - 1) | (xy[:, 1] > hw[0] - 1)).sum())
    assert boxes >= 1, "no accepted crop box among the stored samples"
    assert len(flips) == 4, f"a flip coin shows one value only: {sorted(flips)}"
    assert short >= 1, "no sample with int(0.01 n) == 0"
    assert moved >= 1, "no added row that the per-clip bound moved"
    print(f"{boxes} accepted boxes, flips {sorted(flips)}, {short} samples without erase / add, {moved} added rows moved by the per-clip bound")
    gen_golden.save("ft_ncars_recipe", **arrays)


if __name__ == "__main__":
    main()

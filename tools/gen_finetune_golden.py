#!/usr/bin/env python3
"""Fixture of the fine-tuning recipe's view augmentation: the REFERENCE's own evg_augment(args, v, size, mode='bilinear', seed=s)
(dataset/augmentation/view_augment.py:65-77) on a few small deterministic grids -> tests/golden/evg_augment_bilinear.npz.

Runs on the CPU where a checkout of the reference is at hand (EVP_REFERENCE=<its root>), never on the GPU machine. Nothing of
the reference is copied: the fixture holds seeds, shapes, the outputs and the time-flip flags; the inputs are re-made by the tests from
eventpretrain_amd.testing.det_normalish, the crop boxes and flip coins from draw_evg_params(RandomState(seed)) -- the draw order does not
depend on the resize mode. The seeds are chosen so that every flip combination and the "no box fits in ten tries" branch occur."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("EVP_REFERENCE")
sys.path.insert(0, ROOT)

from eventpretrain_amd.dataset.augmentation.view_augment import draw_evg_params  # noqa: E402
from eventpretrain_amd.testing import det_normalish, make_args  # noqa: E402

# tag, (C, H, W) of the grid, (Ho, Wo) of the view, crop_min. ATen's CPU op has TWO float32 bilinear kernels: the generic one, and a
# channels-last vector kernel that pre-multiplies the weights (1 ulp apart in about half the elements), which it also takes for a
# contiguous NCHW input when Ho + Wo <= 128 (and, single-threaded, when C == 3). A fine-tuning view is 5 x 224 x 224: the generic
# kernel, which is what evp_view_augment_bilinear_f32 restates. So the cases are small in BYTES but have Ho + Wo > 128 and C != 3
# (skinny outputs); only the identity case, exact in either kernel, is below that.
SHAPES = [("a", (5, 48, 64), (24, 106), 0.8), ("b", (5, 37, 53), (100, 30), 0.8), ("c", (4, 30, 30), (20, 110), 0.8),
          ("d", (5, 37, 53), (8, 300), 0.8), ("e", (6, 24, 40), (16, 113), 0.8), ("f", (5, 16, 16), (16, 16), 0.9999)]
assert all(tag == "f" or (size[0] + size[1] > 128 and shp[0] != 3) for tag, shp, size, _ in SHAPES)


def pick_seeds():
    """One seed per shape so that the cases together hold all four (hflip, tflip) pairs; case f (crop_min 0.9999 on a 16 x 16 grid: every
    try rounds to the full size) takes the 'no box fits' branch whatever the seed."""
    want = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 1), (1, 0)]
    seeds = []
    for (tag, shp, size, cmin), flips in zip(SHAPES, want):
        for s in range(1, 400):
            p = draw_evg_params(np.random.RandomState(s), shp[1], shp[2], cmin)
            full = (p[2], p[3]) == (shp[2], shp[1])
            if (p[4], p[5]) == flips and full == (tag == "f"):
                seeds.append(s)
                break
        else:
            raise SystemExit(f"no seed for case {tag}")
    return seeds


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set EVP_REFERENCE to the root of a checkout of the reference")
    sys.path.insert(0, REF)
    from dataset.augmentation.view_augment import evg_augment
    torch.set_num_threads(1)
    out, cases = {}, []
    for (tag, shp, size, cmin), seed in zip(SHAPES, pick_seeds()):
        a = make_args(crop_min=cmin, num_bins=shp[0])
        v = det_normalish(f"aug.bilinear.{tag}", shp)
        res, tflag = evg_augment(a, v.clone(), size=size, mode="bilinear", seed=seed)
        prm = draw_evg_params(np.random.RandomState(seed), shp[1], shp[2], cmin)
        assert int(bool(tflag)) == prm[5]
        out[f"{tag}_out"] = res.contiguous().numpy()
        out[f"{tag}_tflip"] = np.array(int(bool(tflag)))
        cases.append(dict(tag=tag, seed=seed, shape=list(shp), size=list(size), crop_min=cmin))
        print(tag, seed, prm)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(ROOT, "tests", "golden", "evg_augment_bilinear.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()

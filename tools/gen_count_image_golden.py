#!/usr/bin/env python3
"""Writes tests/golden/ft_count_images.npz: the event-count-image branches (args.num_bins 2 and 3) of the REFERENCE's classification
fine-tuning datasets, run as they are written. Each dataset class of dataset/finetune_cls/ is instantiated without its file listing
(object.__new__, load_events / get_label replaced by an in-memory clip) and its own __getitem__ runs under np.random.seed, for training
and for validation, with both representations. The names the dataset module imports from events_to_image.py, events_augment.py and
view_augment.py are wrapped where the module holds them, so that what flows between the stages is recorded beside the result:

  <case>_pre      the rows events_reshape received (or, where the branch has none, the rows events_to_image_* received)
  <case>_geom     int64 [7] = the counting grid (H, W) events_to_image_* was given, events_reshape's (input_w, sensor_w, input_h, sensor_h)
                  (1, 1, 1, 1 where the branch does not rescale), and the input size S
  <case>_raw      the raw image handed to the view stage (after / 255 and remove_hot_pixel_mem with 3 channels)
  <case>_row      the crop row {x0, y0, w, h, hflip, tflip} evg_augment drew (training; oracle.augment_oracle.draw_evg_params on a copy of
                  the generator state at its entry) or the full box (validation: view_resize alone)
  <case>_view     the view, <case>_out the dataset's normalised output
  <case>_margin   3 channels: the distance from remove_hot_pixel_mem's threshold to the nearest attainable k / 255, relative to the
                  threshold. A case below 1e-4 is refused here: the project takes the statistics as exact integers in float64 and the
                  reference in float32 sums, and the two may part only for a value within rounding of the threshold. This is a condition
                  on the INPUTS, checked on the CPU.

Sensors 24 x 32 (and 7 x 9); bilinear cases resize to 72 x 72 (Hout + Wout > 128: the side of ATen's generic bilinear kernel, which the
project's view kernel restates), nearest cases to 16 x 16. `hot_*`: a clip with one hot pixel that is removed and the largest count at
another pixel that is kept, and a clip whose view is all zero for the normalisation with and without the datasets' guard.
Data only; tests/test_count_image_host.py pins tests/count_image_truth.py to these arrays exactly.

    EVP_REFERENCE=/path/to/reference python tools/gen_count_image_golden.py"""
import importlib
import os
import sys
from types import SimpleNamespace

os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden  # noqa: E402
from oracle.augment_oracle import draw_evg_params  # noqa: E402
from eventpretrain_amd.testing import synthetic_events  # noqa: E402

SENSOR = (24, 32)
# dataset_type -> (module, class, prefix of its sensor arguments, resize mode / input size of the case)
DATASETS = {"n-imagenet": ("ft_n_imagenet_dataset", "FinetuneNImageNetDataset", "img", "bilinear", 72),
            "n-caltech101": ("ft_n_caltech101_dataset", "FinetuneNCaltech101Dataset", "cal", "bilinear", 72),
            "cifar10-dvs": ("ft_cifar10_dvs_dataset", "FinetuneCIFAR10DVSDataset", "cifar", "nearest", 16),
            "dvs128_gesture": ("ft_dvs128_gesture_dataset", "FinetuneDVS128GestureDataset", "gesture", "nearest", 16),
            "ucf101_dvs": ("ft_ucf101_dvs_dataset", "FinetuneUCF101DVSDataset", "ucf", "nearest", 16),
            # (its 2-channel branch counts UNSCALED rows on input_size x input_size: the input must hold the 24 x 32 sensor)
            "es-imagenet": ("ft_es_imagenet_dataset", "FinetuneESImageNetDataset", "esimg", "nearest", 32)}
N_ROWS, FIX, VAL_FIX = 420, 300, 360


def _clip(seed, n, hw, signed):
    ev = synthetic_events(seed, n, width=hw[1], height=hw[0], signed_polarity=signed)
    # a busy pixel, so that the common max and the hot-pixel statistics have something to look at
    ev[::9, 0], ev[::9, 1] = 5.0, 3.0
    return ev


def _find_class(mod, want):
    if hasattr(mod, want):
        return getattr(mod, want)
    found = [v for k, v in vars(mod).items() if isinstance(v, type) and k.startswith("Finetune") and v.__module__ == mod.__name__]
    assert len(found) == 1, (mod.__name__, found)
    return found[0]


def run_case(kind, num_bins, is_train, seed, sensor=SENSOR, events=None, mode=None, S=None):
    """One __getitem__ of the reference's dataset class for `kind`; -> dict of recorded arrays."""
    mod_name, cls_name, prefix, d_mode, d_S = DATASETS[kind]
    mode, S = mode or d_mode, S or d_S
    mod = importlib.import_module("dataset.finetune_cls." + mod_name)
    rec = {}
    saved = {}

    def wrap(name, fn):
        if hasattr(mod, name):
            saved[name] = getattr(mod, name)
            setattr(mod, name, fn(saved[name]))

    def w_reshape(f):
        def g(events, sensor_w, sensor_h, input_w, input_h):
            rec["pre"] = events.copy()
            rec["geom_scale"] = (input_w, sensor_w, input_h, sensor_h)
            return f(events, sensor_w, sensor_h, input_w, input_h)
        return g

    def w_image(f):
        def g(args, events, size, is_txyp=False):
            rec.setdefault("pre", events.copy())
            rec["size"] = (int(size[0]), int(size[1]))
            out = f(args, events, size, is_txyp)
            rec["raw"] = out.clone()
            return out
        return g

    def w_hot(f):
        def g(hist, *a, **k):
            rec["before_hot"] = hist.clone()
            out = f(hist, *a, **k)
            rec["raw"] = out.clone()
            return out
        return g

    def w_evg(f):
        def g(args, grid, size, mode="nearest", seed=None):
            state = np.random.get_state()
            rs = np.random.RandomState()
            rs.set_state(state)
            rec["row"] = np.asarray(draw_evg_params(rs, grid.shape[1], grid.shape[2], args.crop_min), np.int32)
            rec["raw"] = grid.clone()
            out, flag = f(args, grid, size=size, mode=mode, seed=seed)
            rec["view"] = out.clone()
            return out, flag
        return g

    def w_resize(f):
        def g(view, size, mode):
            rec["row"] = np.asarray([0, 0, view.shape[2], view.shape[1], 0, 0], np.int32)
            rec["raw"] = view.clone()
            out = f(view, size, mode)
            rec["view"] = out.clone()
            return out
        return g

    wrap("events_reshape", w_reshape)
    wrap("events_to_image_ecdp", w_image)
    wrap("events_to_image_mem", w_image)
    wrap("remove_hot_pixel_mem", w_hot)
    wrap("evg_augment", w_evg)
    wrap("view_resize", w_resize)
    try:
        a = SimpleNamespace(num_bins=num_bins, crop_min=0.8, input_size=S, resize_mode=mode, fix_events_num=FIX, val_fix_events_num=VAL_FIX,
                            val_event_noise=False, use_evrepsl=False)
        setattr(a, prefix + "_sensor_h", sensor[0])
        setattr(a, prefix + "_sensor_w", sensor[1])
        ds = object.__new__(_find_class(mod, cls_name))
        ds.args, ds.is_train = a, is_train
        clip = events if events is not None else _clip(4000 + seed, N_ROWS, sensor, signed=bool(seed & 1))
        ds.load_events = lambda name: clip.copy()
        ds.get_label = lambda name: 0
        ds.events_file_list = ["clip_0000000000000000000000000000.npy"]
        ds.events_file_path_list = ["dir/clip.npy"]
        np.random.seed(seed)
        item = ds[0]
    finally:
        for name, f in saved.items():
            setattr(mod, name, f)
    rec["out"] = item["events_voxel_grid"].clone()
    iw, sw, ih, sh = rec.get("geom_scale", (1, 1, 1, 1))
    # geom: the counting grid (H, W), then the rescale as the two quotients' operands (input_w, sensor_w, input_h, sensor_h; 1s = none)
    rec["geom"] = np.asarray([rec["size"][0], rec["size"][1], iw, sw, ih, sh, S], np.int64)
    if num_bins == 3:
        rec["margin"] = np.asarray(_margin(rec["before_hot"]))
    return rec


def _margin(hist):
    """Relative distance from the reference's own float32 threshold to the nearest attainable k / 255 (k = 0 .. max count + 1)."""
    thr = float(torch.mean(hist[0::2]) + 10 * torch.std(hist[0::2]))
    kmax = int(round(float(hist[0::2].max()) * 255)) + 1
    vals = (torch.arange(kmax + 1, dtype=torch.float32) / 255).double().numpy()
    return float(np.abs(vals - thr).min() / thr) if thr > 0 else 1.0


def _hot_clip(sensor):
    """A clip with a hot pixel (60 rows at (2, 1)) and, at (6, 4), the largest count the threshold still keeps (found by search)."""
    from count_image_truth import count_planes, hot_threshold
    base = synthetic_events(77, 180, width=sensor[1], height=sensor[0])
    base = base[~(((base[:, 0] == 2) & (base[:, 1] == 1)) | ((base[:, 0] == 6) & (base[:, 1] == 4)))]
    def build(k):
        extra = np.zeros((60 + k, 4))
        extra[:60, 0], extra[:60, 1] = 2.0, 1.0
        extra[60:, 0], extra[60:, 1] = 6.0, 4.0
        extra[:, 2], extra[:, 3] = np.linspace(0.0, 0.05, 60 + k), 1.0
        ev = np.concatenate([base, extra])
        return ev[np.argsort(ev[:, 2], kind="stable")]
    best = None
    for k in range(1, 60):
        planes, n_zero, _ = count_planes(build(k), sensor)
        thr = hot_threshold(planes[0], planes[1] if n_zero else planes[2])
        if np.float32(k) / np.float32(255) <= thr:
            best = k
    assert best is not None and best < 59
    return build(best), best


def main():
    gen_golden._ref()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    arrays, names = {}, []
    for kind in DATASETS:
        for nb in (2, 3):
            for is_train, seed in ((True, 3 if nb == 2 else 12), (False, 8)):
                name = f"{kind}_{nb}_{'train' if is_train else 'val'}"
                rec = run_case(kind, nb, is_train, seed + len(names))
                if nb == 3 and float(rec["margin"]) < 1e-4:
                    raise SystemExit(f"{name}: a value within 1e-4 of the hot-pixel threshold (margin {float(rec['margin']):.2e}); pick another seed")
                names.append(name)
                for k in ("pre", "geom", "raw", "row", "view", "out") + (("margin",) if nb == 3 else ()):
                    arrays[f"{name}_{k}"] = rec[k]
    # a grid that is no multiple of any tile, both representations, through N-Caltech101's branch (counts at the sensor's size)
    for nb in (2, 3):
        rec = run_case("n-caltech101", nb, True, 40 + nb, sensor=(7, 9), mode="nearest", S=16)
        name = f"small_{nb}"
        assert nb == 2 or float(rec["margin"]) >= 1e-4, rec["margin"]
        names.append(name)
        for k in ("pre", "geom", "raw", "row", "view", "out") + (("margin",) if nb == 3 else ()):
            arrays[f"{name}_{k}"] = rec[k]
    # the hot pixel: removed at (2, 1), kept at (6, 4) with the largest count the threshold allows
    ev, kept = _hot_clip(SENSOR)
    rec = run_case("n-caltech101", 3, False, 5, events=ev, mode="nearest", S=16)
    assert float(rec["margin"]) >= 1e-4, rec["margin"]
    got = (float(rec["before_hot"][0, 1, 2]) * 255, float(rec["raw"][0, 1, 2]), float(rec["raw"][0, 4, 6]) * 255)
    assert round(got[0]) >= 60 and got[1] == 0 and round(got[2]) == kept, (got, kept)
    arrays.update(hot_pre=rec["pre"], hot_raw=rec["raw"], hot_out=rec["out"], hot_margin=rec["margin"], hot_kept=np.asarray(kept))
    # an all-zero view: UCF101-DVS (guard) and CIFAR10-DVS (none) on a clip without rows of polarity 1 / 0 / -1
    empty = synthetic_events(5, 40, width=SENSOR[1], height=SENSOR[0])
    empty[:, 3] = 2.0
    for kind in ("ucf101_dvs", "cifar10-dvs"):
        rec = run_case(kind, 3, False, 6, events=empty)
        arrays[f"empty_{kind}_out"] = rec["out"]
    arrays["empty_pre"] = empty
    arrays["names"] = np.asarray(names)
    gen_golden.save("ft_count_images", **arrays)


if __name__ == "__main__":
    main()

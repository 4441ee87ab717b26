"""CPU-side checks of the event-count images (args.num_bins 2 and 3): tests/golden/ft_count_images.npz -- the reference's own dataset
branches, run as written by tools/gen_count_image_golden.py -- against the integer restatement the GPU tests lean on
(tests/count_image_truth.py) and the view restatements (oracle.augment_oracle.evg_transform, tests/bilinear_truth.evg_bilinear),
exactly; finetune_recipe's table per dataset and representation against the grids the reference's branches counted on; the refusals
that stay."""
import ctypes

import numpy as np
import pytest

from bilinear_truth import evg_bilinear
from conftest import load_golden
from count_image_truth import count_planes, hot_threshold, normalize, raw_image

KINDS = {"n-imagenet": "img", "n-caltech101": "cal", "cifar10-dvs": "cifar", "dvs128_gesture": "gesture", "ucf101_dvs": "ucf",
         "es-imagenet": "esimg"}
SENSOR = (24, 32)
GUARDED = {"ucf101_dvs", "es-imagenet"}


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    base = dict(phase="finetune_cls", input_size=16, fix_events_num=300, val_fix_events_num=360)
    base.update(kw)
    return make_args(**base)


def _case(g, name):
    geom = [int(v) for v in g[name + "_geom"]]
    size, (iw, sw, ih, sh), S = (geom[0], geom[1]), geom[2:6], geom[6]
    return size, (iw / sw, ih / sh), S


def _restate_view(raw, row, S):
    from oracle.augment_oracle import evg_transform
    fn = evg_bilinear if S == 72 else evg_transform               # (the generator's bilinear cases are the 72 x 72 ones)
    return fn(raw, tuple(int(v) for v in row), (S, S), negate=False)


def test_fixture_equals_the_integer_restatement_exactly():
    g = load_golden("ft_count_images")
    names = [str(n) for n in g["names"]]
    assert len(names) == 6 * 2 * 2 + 2
    flips, wrapped, minus = set(), 0, 0
    for name in names:
        nb = int(name.split("_")[-2]) if not name.startswith("small") else int(name.split("_")[1])
        kind = name.rsplit("_", 2)[0] if not name.startswith("small") else "n-caltech101"
        size, scale, S = _case(g, name)
        pre, raw, row, view, out = (g[f"{name}_{k}"] for k in ("pre", "raw", "row", "view", "out"))
        mine, outside = raw_image(pre, nb, size, scale)
        assert outside == 0 and raw.shape == (nb,) + size and raw.dtype == np.float32, name
        assert np.array_equal(mine, raw), name
        assert raw[0].sum() > 0 and raw[-1].sum() > 0, name
        minus += int((pre[:, 3] == -1).any())
        if nb == 3:
            assert float(g[name + "_margin"]) >= 1e-4, name
            assert not raw[1].any(), name
            planes, n_zero, _ = count_planes(pre, size, scale)
            # every case has a pixel the filter removed: counted, and zero in the image
            gone = ((planes[0] > 0) & (raw[0] == 0)) | ((planes[1 if n_zero else 2] > 0) & (raw[2] == 0))
            assert gone.any() or name.startswith("small"), name          # (63 cells under 300 rows: nothing stands out at 7 x 9)
        assert view.shape == (nb, S, S) and np.array_equal(_restate_view(raw, row, S), view), name
        flips.add((int(row[4]), int(row[5])))
        got, _ = normalize(view, guard=kind in GUARDED)
        assert np.array_equal(got, out), name
        assert np.isfinite(out).all() and (out.min() >= -1 if nb == 2 else abs(float(out[0::2].max()) - 1) < 1e-6), name
    assert len(flips) >= 3 and minus > 0, (flips, minus)


def test_recipe_table_per_dataset_and_representation():
    """finetune_recipe + GpuInputPipeline give, per dataset_type and num_bins, the grid the reference's own branch counted on and its
    rescale (read from the fixture's recorded events_to_image_* size and events_reshape arguments), and the guard where the file has one."""
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import finetune_recipe
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    g = load_golden("ft_count_images")
    seen = set()
    for kind, prefix in KINDS.items():
        for nb in (2, 3):
            for split in ("train", "val"):
                size, scale, S = _case(g, f"{kind}_{nb}_{split}")
                a = _args(dataset_type=kind, num_bins=nb, input_size=S, **{prefix + "_sensor_h": SENSOR[0], prefix + "_sensor_w": SENSOR[1]})
                r = finetune_recipe(a)
                assert set(r) == {"grid", "sensor", "rescale", "norm_guard"} and r["sensor"] == SENSOR, (kind, nb)
                assert r["norm_guard"] == (kind in GUARDED), kind
                p = GpuInputPipeline(a, representation="count", **r)
                assert p.count and (p.gh, p.gw) == size and p.scale == scale and p.sensor == SENSOR, (kind, nb, split, r)
                seen.add((r["grid"], r["rescale"]))
            # five bins: exactly what it was
            a5 = _args(dataset_type=kind, num_bins=5, **{prefix + "_sensor_h": SENSOR[0], prefix + "_sensor_w": SENSOR[1]})
            assert finetune_recipe(a5) == dict(grid="input" if kind == "n-imagenet" else "sensor", sensor=SENSOR), kind
            assert not GpuInputPipeline(a5, **finetune_recipe(a5)).count
    assert seen == {("input", True), ("input", False), ("sensor", True)}
    # ES-ImageNet with two channels: unscaled rows on the S x S grid, the added rows still clipped to the sensor
    a = _args(dataset_type="es-imagenet", num_bins=2, input_size=32, esimg_sensor_h=24, esimg_sensor_w=32)
    p = GpuInputPipeline(a, representation="count", **finetune_recipe(a))
    assert (p.gh, p.gw, p.scale, p.sensor) == (32, 32, (1.0, 1.0), (24, 32))
    # a pipeline of its own keeps binning voxel grids at any bin count (the pre-training chain's meaning of num_bins)
    assert not GpuInputPipeline(a).count
    with pytest.raises(ValueError, match="num_bins 2 or 3"):
        GpuInputPipeline(_args(num_bins=5), representation="count")


def test_hot_pixel_removed_and_the_largest_kept_count():
    g = load_golden("ft_count_images")
    pre, raw, kept = g["hot_pre"], g["hot_raw"], int(g["hot_kept"])
    assert float(g["hot_margin"]) >= 1e-4
    mine, outside = raw_image(pre, 3, SENSOR)
    assert outside == 0 and np.array_equal(mine, raw)
    planes, n_zero, _ = count_planes(pre, SENSOR)
    thr = hot_threshold(planes[0], planes[1])
    assert n_zero > 0 and planes[0, 1, 2] >= 60 and raw[0, 1, 2] == 0 and raw[2, 1, 2] == 0            # removed from both planes
    assert planes[0, 4, 6] == kept and raw[0, 4, 6] == np.float32(kept) / np.float32(255)               # kept ...
    assert np.float32(kept) / np.float32(255) <= thr < np.float32(kept + 1) / np.float32(255)           # ... and the next count would go
    assert np.array_equal(normalize(_restate_view(raw, (0, 0, SENSOR[1], SENSOR[0], 0, 0), 16))[0], g["hot_out"])


def test_all_zero_view_with_and_without_the_guard():
    g = load_golden("ft_count_images")
    raw, outside = raw_image(g["empty_pre"], 3, SENSOR)
    assert outside == 0 and not raw.any()                         # rows of another polarity are ignored
    view = _restate_view(raw, (0, 0, SENSOR[1], SENSOR[0], 0, 0), 16)
    guarded, n = normalize(view, guard=True)
    assert n == 1 and np.array_equal(guarded, g["empty_ucf101_dvs_out"]) and not guarded.any()
    plain, n = normalize(view, guard=False)
    want = g["empty_cifar10-dvs_out"]
    assert n == 1 and np.array_equal(plain, want, equal_nan=True) and np.isnan(want[0::2]).all() and not want[1].any()


def test_truth_counts_wrap_and_refuse_as_bincount_does():
    ev = np.array([[9.0, 0.0, 0.0, 1.0],        # x >= W on a 7 x 9 grid: wraps into row 1, column 0
                   [8.9, 6.9, 0.1, 1.0],        # truncation, the last cell
                   [-1.0, 1.0, 0.2, 0.0],       # a negative x with y >= 1 still lands inside: row 0, column 8
                   [0.0, 7.0, 0.3, 1.0],        # past the last row: outside
                   [-1.0, 0.0, 0.4, -1.0],      # a negative index: outside
                   [3.0, 3.0, 0.5, 0.5]])       # another polarity: ignored
    planes, n_zero, outside = count_planes(ev, (7, 9))
    assert (planes[0, 1, 0], planes[0, 6, 8], planes[1, 0, 8], n_zero, outside) == (1, 1, 1, 1, 2) and planes.sum() == 3
    # fractional coordinates under a rescale: the product is taken before the truncation
    planes, _, outside = count_planes(np.array([[5.0, 2.0, 0.0, 1.0]]), (4, 4), scale=(0.75, 0.75))
    assert planes[0, 1, 3] == 1 and outside == 0


def test_kept_refusals():
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader, finetune_recipe, ncars_recipe
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import GpuDenseLoader
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    for nb in (2, 3):
        a = _args(dataset_type="n-cars", num_bins=nb)
        with pytest.raises(NotImplementedError, match="count images"):
            finetune_recipe(a)
        with pytest.raises(NotImplementedError, match="count images"):
            GpuInputPipeline(a, representation="count", **ncars_recipe(a))
        with pytest.raises(NotImplementedError, match="count images"):
            GpuFinetuneLoader(a, [], 4, 1, True, **ncars_recipe(a))
        with pytest.raises(NotImplementedError, match="2- and 3-bin"):
            GpuDenseLoader(a, [], 4, 1, True, "semseg", (20, 30))
    with pytest.raises(NotImplementedError, match="EvRepSL"):
        GpuFinetuneLoader(_args(num_bins=3, use_evrepsl=True), [], 4, 1, True)


def test_new_symbols_are_declared_bound_and_validate_on_the_host():
    from eventpretrain_amd import _lib
    lib, p = _lib.load(), 4096 * 16
    for name in ("evp_event_image_count", "evp_event_image_finish", "evp_event_image_normalize"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.evp_event_image_finish(p, p, 4, 5, 8, 8, p, None) == -1 and b"C must be 2 or 3" in lib.evp_last_error()
    assert lib.evp_event_image_normalize(p, 4, 4, 8, 8, 0, p, None) == -1
    assert lib.evp_event_image_count(p, 10, p, 0, 10, 8, 8, 1.0, 1.0, p, p, p, None) == -2          # EVP_ESHAPE: no clips
    assert lib.evp_event_image_count(p, 10, p, 4, 10, 8, 8, 1.0, 1.0, None, p, p, None) == -1
    assert _lib.SIGNATURES["evp_event_image_count"][7:9] == [ctypes.c_double, ctypes.c_double]

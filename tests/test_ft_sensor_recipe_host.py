"""CPU-side checks of the sensor-resolution fine-tuning recipe: finetune_recipe's table, GpuInputPipeline's recipe keywords (crop rows
drawn on the sensor's non-square grid, the byte count, the refusals) and tests/golden/ft_sensor_recipe.npz -- the reference's own
events_to_voxel_grid / view_resize / evg_augment at 45 x 60 and 45 x 62 -> 72 x 72 -- against the restatements the GPU tests lean on
(oracle.voxel_oracle.voxel_grid, oracle.augment_oracle.evg_transform, tests/bilinear_truth.evg_bilinear), bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from bilinear_truth import evg_bilinear
from conftest import ROOT, load_golden

SENSORS = {"n-imagenet": ("input", "img", (480, 640)), "n-caltech101": ("sensor", "cal", (180, 240)),
           "cifar10-dvs": ("sensor", "cifar", (128, 128)), "dvs128_gesture": ("sensor", "gesture", (128, 128)),
           "ucf101_dvs": ("sensor", "ucf", (180, 240)), "es-imagenet": ("sensor", "esimg", (224, 224))}


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    base = dict(phase="finetune_cls", input_size=32, fix_events_num=2000, val_fix_events_num=3000)
    base.update(kw)
    return make_args(**base)


def test_finetune_recipe_maps_every_dataset_type():
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import finetune_recipe
    every = {}
    for i, (_, prefix, hw) in enumerate(SENSORS.values()):
        every[prefix + "_sensor_h"], every[prefix + "_sensor_w"] = hw[0] + i, hw[1] + 2 * i       # (distinct values: the right names are read)
    for i, (kind, (grid, _, hw)) in enumerate(SENSORS.items()):
        assert finetune_recipe(_args(dataset_type=kind, **every)) == dict(grid=grid, sensor=(hw[0] + i, hw[1] + 2 * i)), kind
    with pytest.raises(NotImplementedError, match=r"max\(x\) \+ 1"):
        finetune_recipe(_args(dataset_type="n-cars", cars_sensor_h=100, cars_sensor_w=120))
    with pytest.raises(ValueError):
        finetune_recipe(_args(dataset_type="bogus"))


def test_pipeline_draws_crop_rows_on_the_sensor_grid():
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    B, seed, step = 64, 9, 4
    a = _args()
    p = GpuInputPipeline(a, seed=seed, grid="sensor", sensor=(45, 60))
    assert p.sensor == (45, 60) and (p.gh, p.gw) == (45, 60) and p.scale == (1.0, 1.0) and p.fix == 2000
    windows, _, rows = p.draw(np.full(B, 2500), step, first_sample=3)
    assert np.array_equal(rows, va.draw_evg_params_batch(seed, step, B, 45, 60, 0.8, 3))
    assert (rows[:, 0] >= 0).all() and (rows[:, 1] >= 0).all() and (rows[:, 2] >= 1).all() and (rows[:, 3] >= 1).all()
    assert (rows[:, 0] + rows[:, 2] <= 60).all() and (rows[:, 1] + rows[:, 3] <= 45).all()
    assert (rows[:, 2] > 45).any()                                  # a box wider than the grid is high: drawn for 60 x 45, not for a square
    assert (windows[:, 1] - windows[:, 0] == 2000).all()
    # the defaults are what they were: the input grid, the args' sensor and window
    d = GpuInputPipeline(a, seed=seed)
    assert (d.grid, d.sensor, (d.gh, d.gw), d.scale, d.fix, d.view_augment, d.voxel_cells) == \
        ("input", (480, 640), (32, 32), (32 / 640, 32 / 480), 2000, True, "f32")
    assert np.array_equal(d.draw(np.full(B, 2500), step, first_sample=3)[2], va.draw_evg_params_batch(seed, step, B, 32, 32, 0.8, 3))
    # fix_events_num overrides the window length without touching args
    v = GpuInputPipeline(a, seed=seed, fix_events_num=a.val_fix_events_num, view_augment=False, voxel_cells="f64")
    w, dec, _ = v.draw(np.full(B, 5000), step)
    assert (w[:, 1] - w[:, 0] == 3000).all() and a.fix_events_num == 2000 and int(dec[0].max()) < 30


def test_pipeline_keyword_refusals_and_bytes():
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    a = _args()
    with pytest.raises(ValueError, match="grid"):
        GpuInputPipeline(a, grid="bogus")
    with pytest.raises(ValueError, match="voxel_cells"):
        GpuInputPipeline(a, voxel_cells="f16")
    n, raw, view = 150 * 32, 5 * 45 * 60 * 4.0 * 2, 5 * 32 * 32 * 4.0 * 2
    mk = lambda **kw: GpuInputPipeline(a, grid="sensor", sensor=(45, 60), **kw)
    assert mk().algorithmic_bytes([100, 50], fused=True) == n + view                                       # nearest: flushed through the view
    assert mk(resize_mode="bilinear").algorithmic_bytes([100, 50], fused=True) == n + 2 * raw + view
    assert mk(resize_mode="bilinear", view_augment=False).algorithmic_bytes([100, 50], fused=True) == n + 2 * raw + view
    assert mk().algorithmic_bytes([100, 50]) == 3 * n + 2 * raw + view
    same = GpuInputPipeline(a, resize_mode="bilinear", view_augment=False)                                 # S x S -> S x S: no view stage
    assert same.algorithmic_bytes([100, 50], fused=True) == n + view and same.algorithmic_bytes([100, 50]) == 3 * n + view


def test_new_symbol_is_declared_bound_and_exported():
    from eventpretrain_amd import _lib
    with open(os.path.join(ROOT, "include", "evtpretrain.h")) as f:
        header = f.read()
    assert "int evp_voxel_scatter_fused_algo_f32(const double *events, const int64_t *win_begin" in header
    assert "ft_n_caltech101_dataset.py:61-91" in header
    sig = _lib.SIGNATURES["evp_voxel_scatter_fused_algo_f32"]
    old = _lib.SIGNATURES["evp_voxel_scatter_fused_f32"]
    assert sig == old[:-1] + [ctypes.c_int, old[-1]]             # the same arguments plus `int algo` in front of the stream
    assert hasattr(_lib.load(), "evp_voxel_scatter_fused_algo_f32") and "evp_voxel_scatter_fused_algo_f32" in _lib.exported_symbols()


def test_unknown_algo_is_refused_before_any_launch():
    """algo is numbered as evp_voxel_scatter_f32's: 0 and 3 exist in the fused kernel, anything else is EVP_EINVAL (-1). Validated on
    the host (no device here); the pointers are never dereferenced, so any non-null value serves."""
    from eventpretrain_amd import _lib
    lib, p = _lib.load(), 4096 * 16
    for algo in (1, 2, 4, -1):
        rc = lib.evp_voxel_scatter_fused_algo_f32(p, p, p, 3, p, p, p, p, 3000, 5, 100, 224, 1.0, 1.0, None, 0, 0, 0, p, p, algo, None)
        assert rc == -1 and b"algo" in lib.evp_last_error(), algo


def test_fixture_equals_the_restatements_bit_for_bit():
    from oracle.augment_oracle import draw_evg_params, evg_transform
    from oracle.voxel_oracle import voxel_grid
    g = load_golden("ft_sensor_recipe")
    assert g["shapes"].tolist() == [[45, 60, 72], [45, 62, 72]] and len(g["seeds"]) == 3
    restate = {"nearest": evg_transform, "bilinear": evg_bilinear}
    for H, W, S in g["shapes"].tolist():
        tag = f"{H}x{W}"
        grids = g[f"grid_{tag}"]
        assert grids.shape == (2, 5, H, W) and grids.dtype == np.float32
        for i in range(2):
            assert np.array_equal(grids[i], voxel_grid(g[f"events_{tag}_{i}"], 5, (H, W))), (tag, i)
            assert np.abs(grids[i]).sum() > 0
        params = g[f"params_{tag}"]
        for k, seed in enumerate(g["seeds"].tolist()):
            assert tuple(params[k]) == draw_evg_params(np.random.RandomState(seed), H, W, 0.8), (tag, seed)
        assert any(tuple(p[:4]) != (0, 0, W, H) for p in params) and len({tuple(p[4:]) for p in params}) > 1, params
        for mode, fn in restate.items():
            val, train = g[f"val_{mode}_{tag}"], g[f"train_{mode}_{tag}"]
            assert val.shape == (2, 5, S, S) and train.shape == (3, 2, 5, S, S)
            for i in range(2):
                assert np.array_equal(val[i], fn(grids[i], (0, 0, W, H, 0, 0), (S, S))), (tag, mode, i)      # view_resize alone
                for k in range(3):
                    assert np.array_equal(train[k, i], fn(grids[i], params[k], (S, S))), (tag, mode, i, k)

"""CPU-side checks of the N-Cars fine-tuning recipe (grid="window": every clip's grid is its own window's extent, H_c = int(max y) + 1 by
W_c = int(max x) + 1): tests/golden/ft_ncars_recipe.npz -- the reference's own chain in FinetuneNCarsDataset.__getitem__'s order -- against
the restatement the GPU tests lean on (a PADDED oracle.voxel_oracle.voxel_grid at the capacity 48 x 64, erase_add_apply and draw_evg_params
on (H_c, W_c), evg_transform / tests/bilinear_truth.evg_bilinear on the padded grid under the clip's row), bit for bit; the per-clip form of
draw_evg_params_batch; ncars_recipe and the pipeline's refusals; the two new entry points' ABI. (A 1 x 1 window grid in bilinear mode is
outside every equality claim: ATen takes another path there and differs by 1 ulp.)"""
import ctypes
import os

import numpy as np
import pytest

from bilinear_truth import evg_bilinear
from conftest import ROOT, load_golden

CAP = (48, 64)
EXTENTS = [[37, 52], [48, 64], [9, 13], [30, 1], [40, 41]]


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    base = dict(phase="finetune_cls", input_size=32, fix_events_num=300, val_fix_events_num=4000)
    base.update(kw)
    return make_args(**base)


def _restate(mode):
    from oracle.augment_oracle import evg_transform
    return evg_bilinear if mode == "bilinear" else evg_transform


def test_fixture_equals_the_padded_restatement_bit_for_bit():
    from oracle import augment_oracle as ao
    from oracle.voxel_oracle import voxel_grid
    g = load_golden("ft_ncars_recipe")
    S, fix, bins = (int(v) for v in g["recipe"])
    assert g["extents"].tolist() == EXTENTS and (S, fix, bins) == (72, 300, 5) and len(g["seeds"]) == 2
    boxes, flips, short, moved, sizes = 0, set(), 0, 0, set()
    for i, (H, W) in enumerate(EXTENTS):
        ev = g[f"events_{i}"]
        # validation: the whole clip, no event augmentation, view_resize alone = the clip's full box on the padded grid
        assert g[f"val_hw_{i}"].tolist() == [H, W] == [int(ev[:, 1].max()) + 1, int(ev[:, 0].max()) + 1]
        pad = voxel_grid(ev, bins, CAP)
        assert pad.shape == (bins,) + CAP and np.array_equal(pad[:, :H, :W], g[f"val_grid_{i}"]), i
        assert not pad[:, H:].any() and not pad[:, :, W:].any(), i
        for mode in ("nearest", "bilinear"):
            assert np.array_equal(_restate(mode)(pad, (0, 0, W, H, 0, 0), (S, S)), g[f"val_{mode}_{i}"]), (i, mode)
        for k, seed in enumerate(g["seeds"].tolist()):
            rs = np.random.RandomState(seed)
            s0, s1 = ao.draw_window(rs, ev.shape[0], fix)
            assert [s0, s1] == g[f"train_win_{i}_{k}"].tolist()
            win = ev[s0:s1]
            Hc, Wc = int(win[:, 1].max()) + 1, int(win[:, 0].max()) + 1      # taken BEFORE the event augmentation
            assert [Hc, Wc] == g[f"train_hw_{i}_{k}"].tolist()
            sizes.add((Hc, Wc))
            dec = ao.draw_erase_add(rs, win.shape[0])
            rows = ao.erase_add_apply(win, dec, (Hc, Wc))
            prm = ao.draw_evg_params(rs, Hc, Wc, 0.8)
            pad = voxel_grid(rows, bins, CAP)
            assert np.array_equal(pad[:, :Hc, :Wc], g[f"train_grid_{i}_{k}"]), (i, k)
            assert not pad[:, Hc:].any() and not pad[:, :, Wc:].any(), (i, k)
            assert 0 <= prm[0] and prm[0] + prm[2] <= Wc and 0 <= prm[1] and prm[1] + prm[3] <= Hc
            for mode in ("nearest", "bilinear"):
                assert np.array_equal(_restate(mode)(pad, prm, (S, S)), g[f"train_{mode}_{i}_{k}"]), (i, k, mode)
            boxes += int(tuple(prm[:4]) != (0, 0, Wc, Hc))
            flips.add(("h", prm[4])), flips.add(("t", prm[5]))
            short += int(dec is None)
            if dec is not None:
                xy = win[dec[1], :2] + dec[2][:, :2]
                moved += int(((xy[:, 0] > Wc - 1) | (xy[:, 1] > Hc - 1)).sum())
    # what the fixture's seeds were chosen for
    assert boxes >= 1 and len(flips) == 4 and short >= 1 and moved >= 1, (boxes, flips, short, moved)
    assert len(sizes) >= 5


def test_crop_rows_per_clip_equal_the_scalar_calls():
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    B, seed, step, first = 12, 9, 4, 3
    H = np.array([37, 48, 9, 30, 40, 1, 48, 2, 17, 48, 5, 33])
    W = np.array([52, 64, 13, 1, 41, 1, 1, 64, 17, 63, 6, 7])
    rows = va.draw_evg_params_batch(seed, step, B, H, W, 0.8, first)
    assert rows.shape == (B, 6) and rows.dtype == np.int32
    for i in range(B):
        assert np.array_equal(rows[i], va.draw_evg_params_batch(seed, step, B, int(H[i]), int(W[i]), 0.8, first)[i]), i
    assert (rows[:, 0] >= 0).all() and (rows[:, 1] >= 0).all() and (rows[:, 2] >= 1).all() and (rows[:, 3] >= 1).all()
    assert (rows[:, 0] + rows[:, 2] <= W).all() and (rows[:, 1] + rows[:, 3] <= H).all()
    assert ((rows[:, 2] < W) & (rows[:, 3] < H)).any()                  # an accepted box
    # one array and one scalar broadcast; the shared-uniforms form agrees
    U = va.evg_uniforms(seed, step, B, first)
    assert np.array_equal(va.draw_evg_params_batch(seed, step, B, 48, W, 0.8, first, U=U),
                          va.draw_evg_params_batch(seed, step, B, np.full(B, 48), W, 0.8, first))
    with pytest.raises(ValueError):
        va.draw_evg_params_batch(seed, step, B, H[:5], W, 0.8, first)


def test_ncars_recipe_and_the_refusals():
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import finetune_recipe, ncars_recipe
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    assert ncars_recipe(_args(dataset_type="n-cars", cars_sensor_h=101, cars_sensor_w=123)) == dict(grid="window", sensor=(101, 123))
    assert ncars_recipe(_args(dataset_type="n-cars")) == dict(grid="window", sensor=(100, 120))       # the reference's defaults
    with pytest.raises(NotImplementedError, match="ncars_recipe"):
        finetune_recipe(_args(dataset_type="n-cars"))
    a = _args()
    p = GpuInputPipeline(a, seed=1, resize_mode="bilinear", **ncars_recipe(_args(cars_sensor_h=48, cars_sensor_w=64)))
    assert (p.grid, p.sensor, (p.gh, p.gw), p.scale, p.resize) == ("window", CAP, CAP, (1.0, 1.0), True)
    assert GpuInputPipeline(a, grid="window", sensor=(32, 32), view_augment=False).resize      # a window grid is never the view already
    off = np.array([0, 400, 900], np.int64)
    for call in (lambda: p.prepare(off, step=0), lambda: p.batch(None, off, 0), lambda: p.run(None, off, None, None, None),
                 lambda: p.run_prepared(None, None)):
        with pytest.raises(ValueError, match="captured self-driven chain"):
            call()
    with pytest.raises(ValueError, match="grid"):
        GpuInputPipeline(a, grid="bogus")
    with pytest.raises(ValueError, match="capacity"):
        GpuInputPipeline(a, grid="window")
    # the byte count prices a real resize at the capacity
    raw, view = 5 * 48 * 64 * 4.0 * 2, 5 * 32 * 32 * 4.0 * 2
    assert p.algorithmic_bytes([100, 50], fused=True) == 150 * 32 + 2 * raw + view


def test_new_symbols_are_declared_bound_and_exported():
    from eventpretrain_amd import _lib
    with open(os.path.join(ROOT, "include", "evtpretrain.h")) as f:
        header = f.read()
    assert "int evp_events_window_geometry(const double *events, const int64_t *win_begin, const int64_t *win_end, int n_clips" in header
    assert "int evp_events_build_added_hw_f64(const double *events, const int64_t *win_begin" in header
    assert "ft_n_cars_dataset.py:61-87" in header
    old, new = _lib.SIGNATURES["evp_events_build_added_f64"], _lib.SIGNATURES["evp_events_build_added_hw_f64"]
    assert new == old[:-2] + [ctypes.c_void_p] + old[-2:]              # the same arguments plus `clip_hw` in front of the output
    assert len(_lib.SIGNATURES["evp_events_window_geometry"]) == 16
    lib = _lib.load()
    for name in ("evp_events_window_geometry", "evp_events_build_added_hw_f64"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()


def test_bad_arguments_are_refused_before_any_launch():
    """Validated on the host (no device here); the pointers are never dereferenced, so any non-null 16-byte-aligned value serves."""
    from eventpretrain_amd import _lib
    lib, p = _lib.load(), 4096 * 16
    geom = lambda **kw: lib.evp_events_window_geometry(*[{**dict(events=p, wb=p, we=p, n=4, ch=48, cw=64, draw=1, cmin=0.8, seed=1, step=0, first=0,
                                                                sf=None, hw=p, prm=p, st=p, stream=None), **kw}[k]
                                                         for k in ("events", "wb", "we", "n", "ch", "cw", "draw", "cmin", "seed", "step", "first", "sf",
                                                                   "hw", "prm", "st", "stream")])
    EINVAL, ESHAPE = -1, -2
    for kw, rc, word in ((dict(events=None), EINVAL, b"null"), (dict(wb=None), EINVAL, b"null"), (dict(we=None), EINVAL, b"null"),
                         (dict(hw=None), EINVAL, b"null"), (dict(prm=None), EINVAL, b"null"), (dict(st=None), EINVAL, b"null"),
                         (dict(n=0), ESHAPE, b"n_clips"), (dict(n=-3), ESHAPE, b"n_clips"), (dict(ch=0), ESHAPE, b"capacity"),
                         (dict(cw=-1), ESHAPE, b"capacity"), (dict(cmin=0.0), EINVAL, b"crop_min"), (dict(cmin=1.5), EINVAL, b"crop_min"),
                         (dict(events=p + 8), EINVAL, b"aligned")):
        assert geom(**kw) == rc and word in lib.evp_last_error(), kw
    added = lambda *a: lib.evp_events_build_added_hw_f64(*a)
    assert added(None, p, 4, p, p, p, 3, 64.0, 48.0, p, p, None) == EINVAL and b"null" in lib.evp_last_error()
    assert added(p, p, 4, p, p, p, 3, 64.0, 48.0, p, None, None) == EINVAL
    assert added(p, p, 0, p, p, p, 3, 64.0, 48.0, p, p, None) == ESHAPE
    assert added(p, p, 4, p, p, p, 8193, 64.0, 48.0, None, p, None) == ESHAPE
    assert added(p, p, 4, p, p, p, 0, 64.0, 48.0, None, p, None) == 0          # nothing to add: no launch, with or without clip_hw
    # the scalar entry forwards: the same refusals
    assert lib.evp_events_build_added_f64(None, p, 4, p, p, p, 3, 64.0, 48.0, p, None) == EINVAL
    assert lib.evp_events_build_added_f64(p, p, 4, p, p, p, 8193, 64.0, 48.0, p, None) == ESHAPE

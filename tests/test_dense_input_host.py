"""Host side of the dense fine-tuning input: tests/dense_input_truth.py EQUALS the reference-made fixture tests/golden/dense_label_views.npz
(semseg_label_augment, flow_label_augment with evg_augment's time-flip flag, flow_label_valid_augment; 4 shapes x 12 seeds), the fixture's
crop rows are the oracle's draws, the new entries are in the built library and bound, the window rule's default is the Philox rule and
the dense loader's is the tail, and the rectify / mask / tail restatement does what its docstring says on a hand-checked case."""
import ctypes

import numpy as np
import pytest

import dense_input_truth as truth
from conftest import load_golden


@pytest.fixture(scope="module")
def views():
    return load_golden("dense_label_views")


def test_fixture_rows_are_the_reference_draws(views):
    from eventpretrain_amd.dataset.augmentation.view_augment import draw_evg_params
    from oracle import augment_oracle as ao
    assert tuple(map(tuple, views["shapes"])) == truth.GOLDEN_SHAPES and tuple(views["seeds"]) == truth.GOLDEN_SEEDS
    boxes, flips = 0, set()
    for i, (H, W) in enumerate(truth.GOLDEN_SHAPES):
        rows = views[f"rows_{i}"]
        assert rows.shape == (len(truth.GOLDEN_SEEDS), 6) and rows.dtype == np.int32
        for k, seed in enumerate(truth.GOLDEN_SEEDS):
            want = ao.draw_evg_params(np.random.RandomState(seed), H, W, 0.8)
            assert tuple(rows[k]) == tuple(want) == tuple(draw_evg_params(np.random.RandomState(seed), H, W, 0.8)), (H, W, seed)
            boxes += int(tuple(rows[k, :4]) != (0, 0, W, H))
            flips.add((int(rows[k, 4]), int(rows[k, 5])))
    assert boxes == 33 and len(flips) == 4


def test_truth_equals_the_reference_functions(views):
    n = 0
    for i, (H, W) in enumerate(truth.GOLDEN_SHAPES):
        label, flow = truth.label_input(H, W), truth.flow_input(H, W)
        assert label.max() == 255 and (flow == 0).any() and (np.abs(flow) == 1000).any() and (flow == truth.F32_BELOW_1000).any()
        for k, seed in enumerate(truth.GOLDEN_SEEDS):
            prm = views[f"rows_{i}"][k]
            lab = truth.semseg_label_view(label, prm, (H, W))
            fl, va = truth.flow_label_view(flow, prm, (H, W))
            what = (H, W, seed)
            assert lab.dtype == np.int64 and lab.shape == (1, H, W) and np.array_equal(lab, views[f"label_{i}_{seed}"].astype(np.int64)), what
            ref = views[f"flow_{i}_{seed}"]
            assert fl.dtype == ref.dtype == np.float32 and np.array_equal(fl, ref), what
            assert np.array_equal(fl.view(np.uint32) << 1, ref.view(np.uint32) << 1), what      # the bits, but for the sign of a zero
            assert va.dtype == np.float32 and va.shape == (1, H, W) and np.array_equal(va, views[f"valid_{i}_{seed}"].astype(np.float32)), what
            n += 1
    assert n == 48


def test_valid_rule_at_its_edges():
    flow = np.zeros((2, 1, 8), np.float32)
    flow[:, 0, :] = np.array([[1000, -1000, truth.F32_BELOW_1000, 1e-6, 0, 0, 3, -truth.F32_BELOW_1000],
                              [2, 0, 5, 0, -1e-6, 0, 1000, truth.F32_BELOW_1000]], np.float32)
    assert truth.flow_valid_mask(flow)[0, 0].tolist() == [0, 0, 1, 1, 1, 0, 0, 1]
    out, valid = truth.flow_label_view(flow, (2, 0, 4, 1, 1, 1), (1, 8))          # the box [2, 6) widened to 8, both flips
    assert valid[0, 0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert out[0, 0].tolist() == [0.0, 0.0, 0.0, 0.0, np.float32(1e-6) * 2, np.float32(1e-6) * 2, float(truth.F32_BELOW_1000 * np.float32(2)),
                                  float(truth.F32_BELOW_1000 * np.float32(2))]
    assert out[1, 0, 2:4].tolist() == [float(np.float32(1e-6)), float(np.float32(1e-6))] and out[1, 0, 6] == -5.0


def test_rectify_compact_truth_on_a_hand_checked_case():
    """Org sensor 2 x 3, kept extent 2 x 2: the map sends (x, y) = (0, 0) -> inside, (1, 0) -> x == W (drops), (2, 0) -> -0.0 (stays),
    (0, 1) -> NaN (drops), (1, 1) -> just below W and H (stays), (2, 1) -> negative (drops)."""
    nan, lo = np.float32(np.nan), np.nextafter(np.float32(2), np.float32(0))
    m = np.array([[[0.5, 1.0], [2.0, 0.0], [-0.0, 0.0]], [[nan, 0.0], [lo, lo], [-1.0, 1.0]]], np.float32)
    ev = np.array([[0, 0, 1, 1], [1, 0, 2, 0], [2, 0, 3, 1], [0, 1, 4, 0], [1, 1, 5, 1], [2, 1, 6, 0], [3, 0, 7, 1], [1.9, 1.2, 8, 0]], np.float64)
    rows, off, status = truth.rectify_compact(ev, [0, 8, 8, 8], (2, 2), 2, m)
    assert off.tolist() == [0, 2, 2, 2] and status.tolist() == [2, 1]                # clip 0 keeps its last 2 of 4; (3, 0) is outside the map
    assert rows[:, 2].tolist() == [5.0, 8.0] and rows[0, 0] == float(lo) and rows[1, :2].tolist() == [float(lo), float(lo)]
    rows, off, status = truth.rectify_compact(ev, [0, 8], (2, 2), 100, m)
    assert rows[:, 2].tolist() == [1.0, 3.0, 5.0, 8.0] and np.signbit(rows[1, 0]) and status.tolist() == [0, 1]
    # the DDD17 form: no map, mask first, tail second
    rows, off, status = truth.rectify_compact(ev, [0, 3, 8], (2, 2), 2)
    assert rows[:, 2].tolist() == [1.0, 2.0, 5.0, 8.0] and off.tolist() == [0, 2, 4] and status.tolist() == [0, 0]


def test_new_entries_are_built_and_bound():
    from eventpretrain_amd import _lib
    lib = _lib.load()
    for name, nargs in (("evp_semseg_label_augment", 9), ("evp_flow_label_augment_f32", 10), ("evp_events_rectify_compact_f64", 17),
                        ("evp_events_rectify_compact_ws_words", 2)):
        assert hasattr(lib, name) and name in _lib.exported_symbols() and len(_lib.SIGNATURES[name]) == nargs, name
    assert _lib.ABI_VERSION == 5 and _lib.RECTIFY_CHUNK_ROWS == 1024
    assert "#define EVP_RECTIFY_CHUNK_ROWS 1024" in open(_lib.CSRC + "/../../include/evtpretrain.h").read()
    assert _lib.call("evp_events_rectify_compact_ws_words", 64, 210_000) == 64 * 206 + 1
    # host-side refusals need no device
    assert lib.evp_semseg_label_augment(None, None, None, 1, 4, 4, 4, 4, None) == -1
    assert lib.evp_flow_label_augment_f32(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 4, 4, 0, 4, None) == -2
    assert lib.evp_events_rectify_compact_f64(None, 0, None, 1, 1, None, 0, 0, 1, 1, 1, None, 0, None, None, None, None) == -1
    p = ctypes.c_void_p(64)
    assert lib.evp_events_rectify_compact_f64(p, 8, p, 1, 8, None, 0, 0, 4, 4, 2, p, 8, p, p, p, None) == -1 and b"in place" in lib.evp_last_error()
    q = ctypes.c_void_p(128)
    assert lib.evp_events_rectify_compact_f64(p, 8, p, 70000, 8, None, 0, 0, 4, 4, 2, q, 8, p, p, p, None) == -2
    assert lib.evp_events_rectify_compact_f64(p, 8, p, 4096, 1 << 20, None, 0, 0, 4, 4, 2, q, 8, p, p, p, None) == -2 and b"2^31" in lib.evp_last_error()


def test_window_start_default_is_the_philox_rule_and_the_dense_one_the_tail():
    from eventpretrain_amd.dataset.augmentation.events_augment import philox_words
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import GpuDenseLoader
    from eventpretrain_amd.dataset.pretrain.gpu_event_loader import ClipWindowLoader
    base, dense = ClipWindowLoader.__new__(ClipWindowLoader), GpuDenseLoader.__new__(GpuDenseLoader)
    w0 = philox_words(21, 5, 8 + np.arange(6), 0, 1)[:, 0]
    for w, n in zip(w0, (1500, 5000, 2500, 3000, 2000, 4321)):
        fix = 2000
        want = (int(w) * (n - fix)) >> 32 if n > fix else 0          # tests/test_gpu_finetune_sensor_loader.py::_windows
        assert base._window_start(n, fix, int(w)) == want and 0 <= want <= max(n - fix, 0)
        assert dense._window_start(n, fix, int(w)) == max(n - fix, 0)
    assert any(base._window_start(n, 2000, int(w)) not in (0, n - 2000) for w, n in zip(w0, (5000, 5000, 5000, 5000, 5000, 5000)))


def test_dense_recipe_reads_the_reference_argument_names():
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import DDD17_MASK_MARGIN, dense_recipe
    from eventpretrain_amd.testing import make_args
    a = make_args(dataset_type="dsec", dsec_sensor_h=440, dsec_sensor_w=640, dsec_org_sensor_h=480, dsec_org_sensor_w=640)
    assert dense_recipe(a) == dict(task="semseg", sensor=(440, 640), org_sensor=(480, 640), rectify=True, raw_rows=None)
    a = make_args(dataset_type="ddd17", ddd17_sensor_h=200, ddd17_sensor_w=346, fix_events_num=3000, val_fix_events_num=5000)
    assert dense_recipe(a) == dict(task="semseg", sensor=(200, 346), org_sensor=None, rectify=False, raw_rows=5000 + DDD17_MASK_MARGIN)
    a = make_args(dataset_type="mvsec", mvsec_sensor_h=260, mvsec_sensor_w=346, max_events=7000)
    assert dense_recipe(a) == dict(task="flow", sensor=(260, 346), org_sensor=None, rectify=False, raw_rows=None, max_events=7000)
    with pytest.raises(ValueError, match="unknown dataset_type"):
        dense_recipe(make_args(dataset_type="n-cars"))

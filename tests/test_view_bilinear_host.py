"""The bilinear view augmentation without a GPU: the float32 restatement the GPU tests compare the kernel with (tests/bilinear_truth.py)
against the reference's own evg_augment(mode='bilinear') outputs (tests/golden/evg_augment_bilinear.npz, tools/gen_finetune_golden.py),
and the new entry point's declaration and binding."""
import os

import numpy as np
import pytest

from bilinear_truth import bilinear_resize, evg_bilinear, fmaf
from conftest import ROOT, jload, load_golden


def _cases():
    return jload(load_golden("evg_augment_bilinear")["cases"])


def test_fixture_covers_both_flips_and_the_full_view_branch():
    from eventpretrain_amd.dataset.augmentation.view_augment import draw_evg_params
    d = load_golden("evg_augment_bilinear")
    flips, full = set(), 0
    for c in _cases():
        C, H, W = c["shape"]
        p = draw_evg_params(np.random.RandomState(c["seed"]), H, W, c["crop_min"])
        assert int(d[c["tag"] + "_tflip"]) == p[5]
        flips.add((p[4], p[5]))
        full += (p[2], p[3]) == (W, H)
    assert flips == {(0, 0), (0, 1), (1, 0), (1, 1)} and full >= 1
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "evg_augment_bilinear.npz")) < \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "evg_augment.npz"))


@pytest.mark.parametrize("tag", [c["tag"] for c in _cases()] if os.path.exists(os.path.join(ROOT, "tests", "golden", "evg_augment_bilinear.npz")) else ["missing"])
def test_restatement_equals_the_reference_bit_for_bit(tag):
    from eventpretrain_amd.dataset.augmentation.view_augment import draw_evg_params
    from eventpretrain_amd.testing import det_normalish
    d = load_golden("evg_augment_bilinear")
    c = next(k for k in _cases() if k["tag"] == tag)
    C, H, W = c["shape"]
    v = det_normalish(f"aug.bilinear.{tag}", (C, H, W)).numpy()
    p = draw_evg_params(np.random.RandomState(c["seed"]), H, W, c["crop_min"])
    got = evg_bilinear(v, p, tuple(c["size"]), negate=C in (5, 6))
    want = d[tag + "_out"]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    n_diff = int((got != want).sum())
    print(f"{tag}: params {p}, {n_diff} of {want.size} elements differ, max |diff| {float(np.abs(got - want).max()):.3e}")
    assert np.array_equal(got, want)


def test_full_box_at_equal_size_is_the_identity():
    rng = np.random.default_rng(5)
    for shp in ((5, 32, 32), (3, 30, 30), (5, 224, 224), (1, 1, 7)):
        v = rng.standard_normal(shp).astype(np.float32)
        assert np.array_equal(bilinear_resize(v, shp[1:]), v)
        assert np.array_equal(evg_bilinear(v, (0, 0, shp[2], shp[1], 0, 0), shp[1:]), v)


def test_fmaf_emulation_rounds_once():
    """a * b + c whose float64 sum is a float32 tie while the exact sum is not: two roundings would go to the even neighbour."""
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)           # a * b = 1 + 2^-11 + 2^-24
    c = np.float32(2.0 ** -60)
    assert fmaf(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)           # above the tie: up
    assert fmaf(a, b, -c) == np.float32(1 + 2.0 ** -11)                       # below it: down
    assert fmaf(a, b, np.float32(0)) == np.float32(1 + 2.0 ** -11)            # the tie itself: to even


def test_mode_is_checked():
    from eventpretrain_amd.dataset.augmentation.view_augment import evg_augment_batch
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    from eventpretrain_amd.testing import make_args
    with pytest.raises(ValueError):
        evg_augment_batch(None, None, (8, 8), mode="bogus")
    with pytest.raises(ValueError):
        GpuInputPipeline(make_args(), resize_mode="bogus")
    assert GpuInputPipeline(make_args()).resize_mode == "nearest"
    assert GpuInputPipeline(make_args(resize_mode="bilinear")).resize_mode == "nearest"       # a keyword, never read from args
    p = GpuInputPipeline(make_args(), resize_mode="bilinear")
    grid = 5 * 224 * 224 * 4.0 * 2
    assert p.algorithmic_bytes([100, 50], fused=True) == 150 * 32 + 3 * grid
    assert GpuInputPipeline(make_args()).algorithmic_bytes([100, 50], fused=True) == 150 * 32 + grid


def test_symbol_is_declared_bound_and_exported():
    from eventpretrain_amd import _lib
    with open(os.path.join(ROOT, "include", "evtpretrain.h")) as f:
        header = f.read()
    assert "int evp_view_augment_bilinear_f32(const float *in, const int32_t *params, float *out" in header
    assert "main_finetune_cls.py:48" in header and "#define EVP_ABI_VERSION 5" in header
    assert _lib.SIGNATURES["evp_view_augment_bilinear_f32"] == _lib.SIGNATURES["evp_view_augment_f32"]
    assert hasattr(_lib.load(), "evp_view_augment_bilinear_f32")

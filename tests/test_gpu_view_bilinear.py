"""evp_view_augment_bilinear_f32 through evg_augment_batch(mode="bilinear") on the GPU: EQUAL (np.array_equal) to the reference's own
evg_augment(mode='bilinear') outputs (tests/golden/evg_augment_bilinear.npz) and to the float32 restatement that
tests/test_view_bilinear_host.py pins to them (tests/bilinear_truth.py), on boxes and shapes the fixture does not hold."""
import numpy as np
import pytest
import torch

from bilinear_truth import evg_bilinear
from conftest import jload, load_golden

pytestmark = pytest.mark.gpu


def _run(v, params, size, **kw):
    from eventpretrain_amd.dataset.augmentation.view_augment import evg_augment_batch
    out = evg_augment_batch(torch.from_numpy(np.ascontiguousarray(v)).cuda(), np.asarray(params, np.int32), size, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _grids(tag, B, C, H, W):
    from eventpretrain_amd.testing import det_normalish
    return det_normalish(f"gpu.bilinear.{tag}", (B, C, H, W)).numpy()


def test_equals_the_reference_fixture():
    from eventpretrain_amd.dataset.augmentation.view_augment import draw_evg_params
    from eventpretrain_amd.testing import det_normalish
    d = load_golden("evg_augment_bilinear")
    for c in jload(d["cases"]):
        C, H, W = c["shape"]
        v = det_normalish(f"aug.bilinear.{c['tag']}", (C, H, W)).numpy()
        p = draw_evg_params(np.random.RandomState(c["seed"]), H, W, c["crop_min"])
        got = _run(v[None], [p], c["size"], mode="bilinear")[0]
        want = d[c["tag"] + "_out"]
        print(c["tag"], p, "differing elements:", int((got != want).sum()), "of", want.size)
        assert np.array_equal(got, want), c["tag"]
        assert np.array_equal(got, evg_bilinear(v, p, c["size"], negate=C in (5, 6))), c["tag"]


# C, (H, W) -> (Ho, Wo), three rows {x0, y0, w, h, hflip, tflip} (a different one per sample)
CONFIGS = [
    # more than 256 output columns (the second block of a row, its tail masked): a box against the right and bottom borders, a
    # 1 x 1 box, a 1-row box
    ("wide", 5, (37, 53), (40, 300), [(20, 10, 33, 27, 0, 0), (5, 6, 1, 1, 0, 1), (3, 7, 40, 1, 1, 0)]),
    # boxes larger than the output (down-scale on both axes): the whole view, a box against the left and top borders, one inside
    ("down", 5, (37, 53), (16, 20), [(0, 0, 53, 37, 1, 1), (0, 0, 30, 20, 1, 0), (13, 5, 40, 32, 0, 1)]),
    # 3 bins (no negation on a time flip): the identity box time-flipped, an odd box with both flips, the last pixel alone
    ("c3", 3, (30, 30), (30, 30), [(0, 0, 30, 30, 0, 1), (2, 3, 25, 24, 1, 1), (29, 29, 1, 1, 0, 0)]),
    # 1-column box, up-scale by a non-integer factor, 6 bins (negated)
    ("c6", 6, (24, 40), (33, 47), [(39, 0, 1, 24, 1, 1), (0, 23, 40, 1, 0, 0), (7, 5, 19, 11, 0, 1)]),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_equals_the_restatement_on_edge_boxes(cfg):
    tag, C, (H, W), size, rows = cfg
    v = _grids(tag, 3, C, H, W)
    got = _run(v, rows, size, mode="bilinear")
    for b, p in enumerate(rows):
        want = evg_bilinear(v[b], p, size, negate=C in (5, 6))
        print(tag, p, "differing elements:", int((got[b] != want).sum()), "of", want.size)
        assert np.array_equal(got[b], want), (tag, p)
    assert {(p[4], p[5]) for c in CONFIGS for p in c[4]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if tag == "c3":           # the time flip of a 3-bin grid reverses the bins and does NOT negate; the identity box copies the pixels
        assert np.array_equal(got[0], v[0][::-1])
        explicit = _run(v, rows, size, mode="bilinear", negate=True)
        assert np.array_equal(explicit[0], -v[0][::-1])


def test_taps_are_clamped_at_the_crop_edge():
    """The pixels just outside the box hold 1e6: a tap clamped at the image's edge instead of the crop's would blend them in."""
    C, H, W, size = 5, 37, 53, (40, 300)
    v = _grids("clamp", 3, C, H, W)
    rows = [(10, 8, 30, 20, 0, 0), (10, 8, 30, 20, 1, 1), (1, 1, 51, 35, 0, 1)]
    poisoned = v.copy()
    for b, (x0, y0, w, h, _, _) in enumerate(rows):
        ring = np.zeros((H, W), bool)
        ring[y0 - 1:y0 + h + 1, x0 - 1:x0 + w + 1] = True
        ring[y0:y0 + h, x0:x0 + w] = False
        assert ring.sum() == 2 * (w + h) + 4
        poisoned[b][:, ring] = 1e6
    got = _run(poisoned, rows, size, mode="bilinear")
    assert float(np.abs(got).max()) < 1e3
    for b, p in enumerate(rows):
        assert np.array_equal(got[b], evg_bilinear(v[b], p, size)), p
    near = _run(poisoned, rows, size, mode="nearest")
    assert float(np.abs(near).max()) < 1e3


def test_nearest_mode_is_the_old_kernel():
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    C, H, W, size = 5, 37, 53, (40, 300)
    v = _grids("nearest", 3, C, H, W)
    rows = [(20, 10, 33, 27, 0, 0), (5, 6, 1, 1, 0, 1), (3, 7, 40, 1, 1, 0)]
    vd = torch.from_numpy(v).cuda()
    pd = torch.tensor(rows, dtype=torch.int32).cuda()
    want = torch.full((3, C, *size), 7.0, device="cuda")
    call("evp_view_augment_f32", ptr(vd), ptr(pd), ptr(want), 3, C, H, W, size[0], size[1], 1, stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_run(v, rows, size, mode="nearest"), want.cpu().numpy())
    assert np.array_equal(_run(v, rows, size), want.cpu().numpy())
    assert not np.array_equal(_run(v, rows, size, mode="bilinear"), want.cpu().numpy())
    with pytest.raises(ValueError):
        _run(v, rows, size, mode="bicubic")

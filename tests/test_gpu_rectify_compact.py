"""evp_events_rectify_compact_f64 on the GPU against tests/dense_input_truth.rectify_compact (the line-by-line restatement of
ft_dsec_dataset.py:211-226 and ft_ddd17_dataset.py:116-127): rows, offsets and both status words EQUAL. Org sensor 6 x 8, kept extent
5 x 8, a map holding -0.0, NaNs, values equal to W and H, values just below them and negative values; clips whose lengths sit on the
edges of a wave's run (64) and of a chunk (RECTIFY_CHUNK_ROWS), an empty clip, a clip that loses every row and one that loses none;
keep_last below, equal to and above the survivor counts; the map = NULL form (DDD17's mask); rows past offsets_out[B] are left alone."""
import numpy as np
import pytest
import torch

import dense_input_truth as truth

pytestmark = pytest.mark.gpu

ORG, EXTENT = (6, 8), (5, 8)
SENTINEL = -7.0


def _chunk():
    from eventpretrain_amd._lib import RECTIFY_CHUNK_ROWS
    return RECTIFY_CHUNK_ROWS


def _map():
    H, W = EXTENT
    m = np.zeros(ORG + (2,), np.float32)
    for y in range(ORG[0]):
        for x in range(ORG[1]):
            m[y, x] = (x + 0.25, y * 0.8)                    # rows 1..4 of the org sensor land inside
    nan = np.float32(np.nan)
    m[0] = [(-0.0, 0.0), (nan, 1.0), (W, 1.0), (np.nextafter(np.float32(W), np.float32(0)), np.nextafter(np.float32(H), np.float32(0))),
            (1.0, H), (-1e-3, 2.0), (3.0, -2.0), (2.0, nan)]
    m[5, :, 1] = 5.5                                         # the bottom row of the org sensor leaves the kept extent
    return m


def _clip(rng, n, kind="mixed"):
    x = np.floor(rng.uniform(0, ORG[1], n))
    y = {"none": np.full(n, 5.0), "all": np.floor(rng.uniform(1, 5, n))}.get(kind, np.floor(rng.uniform(0, ORG[0], n)))
    frac = rng.uniform(0, 1, n) < 0.25                       # (int) truncates: x + 0.75 names the same cell
    x, y = x + 0.75 * frac, y + 0.5 * frac
    if kind == "outside" or n == 2049:                       # rows that name no cell of the map: dropped and counted
        k = np.arange(5, n, 397)
        x[k[0::4]], x[k[1::4]], y[k[2::4]], y[k[3::4]] = ORG[1], -1.0, ORG[0], np.nan
    return np.stack([x, y, np.arange(n, dtype=np.float64) * 1e-3 + 1.0, (rng.uniform(0, 1, n) < 0.5).astype(np.float64)], 1)


def _batches():
    C = _chunk()
    rng = np.random.default_rng(77)
    one = [_clip(rng, 0), _clip(rng, 1, "all"), _clip(rng, C - 1, "none"), _clip(rng, C, "all"), _clip(rng, 3 * C + 7)]
    two = [_clip(rng, n) for n in (63, 64, 65, 2049, 5000)]
    return one, two


def _run(clips, keep_last, rectify_map, extra_rows=9):
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import rectify_compact_batch
    ev = np.concatenate(clips, 0)
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
    want_rows, want_off, want_status = truth.rectify_compact(ev, off, EXTENT, keep_last, rectify_map)
    cap = min(ev.shape[0], len(clips) * keep_last) + extra_rows
    out = torch.full((cap, 4), SENTINEL, dtype=torch.float64, device="cuda")
    off_out = torch.full((len(clips) + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_map = None if rectify_map is None else torch.from_numpy(rectify_map).cuda()
    rectify_compact_batch(torch.from_numpy(ev).cuda(), torch.from_numpy(off).cuda(), max(c.shape[0] for c in clips), keep_last, EXTENT, out, off_out,
                          status, rectify_map=d_map)
    torch.cuda.synchronize()
    got, got_off, got_status = out.cpu().numpy(), off_out.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(got_off, want_off), (got_off, want_off)
    assert np.array_equal(got_status, want_status), (got_status, want_status)
    m = int(want_off[-1])
    assert np.array_equal(got[:m], want_rows)
    assert np.array_equal(np.signbit(got[:m, :2]), np.signbit(want_rows[:, :2]))       # -0.0 stays -0.0
    assert (got[m:] == SENTINEL).all()                                                  # nothing past offsets_out[B] is touched
    return want_off, want_status


@pytest.mark.parametrize("which", [0, 1])
def test_rectified_survivors_equal_the_truth(which):
    C = _chunk()
    clips = _batches()[which]
    m = _map()
    survivors, _ = _run(clips, 10 ** 6, m)                   # above every count: all survivors, in order
    T = np.diff(survivors)
    if which == 0:
        assert T.tolist()[:4] == [0, 1, 0, C] and 0 < T[4] < 3 * C + 7
    else:
        assert all(0 < t < c.shape[0] for t, c in zip(T, clips))
    # below, equal to (clip 3 of the first batch keeps exactly C rows; the largest count of the second) and just above a count
    for keep in (7, C if which == 0 else int(T.max()), int(T.max()) + 1, 1):
        off, status = _run(clips, keep, m)
        assert np.diff(off).tolist() == np.minimum(T, keep).tolist()
        assert status.tolist() == [2, 0] if which == 0 else (status[0] == 0 and status[1] > 0)


def test_rows_outside_the_map_are_dropped_and_counted():
    rng = np.random.default_rng(5)
    clips = [_clip(rng, 900, "outside"), _clip(rng, 130)]
    _, status = _run(clips, 500, _map())
    assert status.tolist() == [0, 3]                         # rows 5, 402, 799 of the first clip


def test_plain_mask_form_without_a_map():
    """DDD17: map = NULL, the mask on the raw coordinates, then the tail."""
    C = _chunk()
    rng = np.random.default_rng(11)
    clips = []
    for n in (C + 1, 2 * C, 70, 0, 1):
        x, y = np.floor(rng.uniform(-1, 10, n) * 2) / 2, np.floor(rng.uniform(-1, 7, n) * 2) / 2
        if n >= 70:
            x[3], x[4], x[5], y[6], y[7] = np.nan, -0.0, EXTENT[1], EXTENT[0], -0.0
        clips.append(np.stack([x, y, np.arange(n, dtype=np.float64), np.ones(n)], 1))
    clips[-1][0, :2] = (EXTENT[1], 0.0)                      # a one-row clip that loses its row
    for keep in (10 ** 6, 40, 1):
        off, status = _run(clips, keep, None)
        assert status.tolist() == [2, 0]
    assert np.diff(off).tolist() == [1, 1, 1, 0, 0]


def test_offsets_that_leave_the_buffer_are_counted_not_read():
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import rectify_compact_batch
    rng = np.random.default_rng(3)
    ev = torch.from_numpy(_clip(rng, 200, "all")).cuda()
    out = torch.full((300, 4), SENTINEL, dtype=torch.float64, device="cuda")
    off_out, status = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    # clip 0 holds more rows than max_rows_per_clip says (the first 64 are read), clip 1 runs past the 200 rows of the buffer
    rectify_compact_batch(ev, torch.tensor([0, 100, 260], device="cuda"), 64, 1000, EXTENT, out, off_out, status)
    assert off_out.tolist() == [0, 64, 128] and status.tolist() == [0, 2]
    got = out.cpu().numpy()
    assert np.array_equal(got[:64, 2], ev[:64, 2].cpu().numpy()) and np.array_equal(got[64:128, 2], ev[100:164, 2].cpu().numpy()) and (got[128:] == SENTINEL).all()

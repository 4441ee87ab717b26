"""evp_voxel_scatter_fused_algo_f32 on the GPU, through the C-ABI: the fused K1 (window rows - erased rows + added rows) with float64
cells in its LDS tile (algo 3) against the CPU oracle, against the float32-cell entry, against itself (two launches must agree bit for
bit: the float64 sum does not depend on the order the atomics arrive in) and, flushed through the nearest view, against the
restatement of the view on its own raw grids.

Grids 100 x 224 and 100 x 222 with bins 5: float64 cells give two y-tiles (91 rows of 224 float64 fit beside the bitmap) where float32
cells give one, and 222 takes the scalar flush. Three clips and eight: the two workgroup-to-clip maps."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, BINS, N_WIN, MAX_WINDOW = 100, 5, 3000, 3000
K1_TOL = 1e-5                    # the project's K1 bound against the oracle's sequential float32 sum
VIEW = (72, 72)


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _case(W):
    """Eight clips on a 100 x W sensor with explicit decisions, and the oracle's grids for them (computed once per width).
    clip 1: two stamps swapped across bin regions (the verified fast pass flags it, the repair pass scans it whole);
    clip 2: 3400 rows against max_window = 3000, erased rows behind the bitmap (the erase-list search path);
    clip 3: an empty window; the others: 3000 rows, ~20 erased, ~20 added."""
    from eventpretrain_amd.testing import synthetic_events
    from oracle import augment_oracle as ao
    from oracle.voxel_oracle import voxel_grid
    rng = np.random.default_rng(1000 + W)
    wins, ers, adds, want = [], [], [], []
    for c in range(8):
        n = {2: 3400, 3: 0}.get(c, N_WIN)
        win = synthetic_events(300 + 8 * W + c, n, width=W, height=H) if n else np.zeros((0, 4))
        if c == 1:
            win[[500, 2500], 2] = win[[2500, 500], 2]
        if n:
            er = np.sort(rng.choice(np.setdiff1d(np.arange(n), [500, 2500]), 18 + c, replace=False))
            if c == 2:
                er = np.unique(np.concatenate([er, [3001, 3100, 3398, 3399]]))        # behind the bitmap, the last two rows among them
            ai = rng.choice(n, 17 + c, replace=False)
            nz = rng.normal(0, 1, (ai.size, 3)) * [1.5, 1.5, 0.001]
        else:
            er, ai, nz = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
        # the added rows by hand (events_augment.py:40-49): copies plus noise, clipped to the sensor, time-sorted
        add = win[ai].copy()
        add[:, :3] += nz
        add[:, 0], add[:, 1] = np.clip(add[:, 0], 0, W - 1), np.clip(add[:, 1], 0, H - 1)
        add = add[np.argsort(add[:, 2], kind="stable")]
        rows = ao.erase_add_apply(win, (er, ai, nz), (H, W)) if n else win
        wins.append(win), ers.append(er.astype(np.int64)), adds.append(add)
        want.append(voxel_grid(rows, BINS, (H, W)) if n else np.zeros((BINS, H, W), np.float32))
    return wins, ers, adds, want


def _launch(W, clips, algo, view_params=None, entry="evp_voxel_scatter_fused_algo_f32"):
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    wins, ers, adds, _ = _case(W)
    wins, ers, adds = [wins[c] for c in clips], [ers[c] for c in clips], [adds[c] for c in clips]
    nc = len(clips)
    cum = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    off, e_off, a_off = cum(wins), cum(ers), cum(adds)
    ev = _dev(np.concatenate(wins, 0), torch.float64)
    d_wb, d_we, d_eo, d_ao = _dev(off[:-1]), _dev(off[1:]), _dev(e_off), _dev(a_off)
    d_er = _dev(np.concatenate(ers + [np.zeros(1, np.int64)]))
    d_add = _dev(np.concatenate(adds + [np.zeros((1, 4))], 0), torch.float64)
    shape = (nc, BINS, H, W) if view_params is None else (nc, BINS) + VIEW
    out = torch.full(shape, 7.0, device="cuda")
    kws = torch.zeros(nc * (BINS + 5), dtype=torch.int64, device="cuda")
    prm = None if view_params is None else _dev(view_params, torch.int32)
    tail = (ptr(kws), ptr(out)) + ((algo,) if entry.endswith("algo_f32") else ()) + (stream_ptr(),)
    call(entry, ptr(ev), ptr(d_wb), ptr(d_we), nc, ptr(d_er), ptr(d_eo), ptr(d_add), ptr(d_ao), MAX_WINDOW, BINS, H, W, 1.0, 1.0,
         ptr(prm), VIEW[0] if prm is not None else 0, VIEW[1] if prm is not None else 0, 1 if prm is not None else 0, *tail)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("clips", [(1, 2, 3), tuple(range(8))], ids=["3clips", "8clips"])
@pytest.mark.parametrize("W", [224, 222])
def test_float64_cells_against_oracle_float32_cells_and_itself(W, clips):
    want = _case(W)[3]
    got = _launch(W, clips, 3)
    again = _launch(W, clips, 3)
    f32 = _launch(W, clips, 0)
    old = _launch(W, clips, 0, entry="evp_voxel_scatter_fused_f32")
    for i, c in enumerate(clips):
        err, d32 = float(np.abs(got[i] - want[c]).max()), float(np.abs(got[i] - f32[i]).max())
        print(f"W {W} clip {c}: |f64 cells - oracle| {err:.3e}, |f64 - f32 cells| {d32:.3e}, |f32 cells - oracle| {float(np.abs(f32[i] - want[c]).max()):.3e}")
        assert err <= K1_TOL, (W, c, err)
        assert d32 <= 2 * K1_TOL, (W, c, d32)
        assert float(np.abs(old[i] - want[c]).max()) <= K1_TOL, (W, c)            # the forwarding entry is the float32 kernel
    assert np.array_equal(got, again), int((got != again).sum())
    empty = clips.index(3)
    assert float(np.abs(got[empty]).max()) == 0.0 and all(float(np.abs(got[i]).sum()) > 0 for i in range(len(clips)) if i != empty)


@pytest.mark.parametrize("clips", [(1, 2, 3), tuple(range(8))], ids=["3clips", "8clips"])
def test_float64_cells_flushed_through_the_nearest_view(clips):
    """100 x 224 -> 72 x 72: every output pixel reads one cell of the float64 tile, rounded to float32 there -- the result EQUALS the
    view restatement applied to the algo-3 raw grids (crops, both flips and the time flip's negation among the rows)."""
    from oracle.augment_oracle import evg_transform
    rows = np.array([(5, 3, 200, 90, 1, 0), (0, 0, 224, 100, 0, 1), (10, 7, 150, 80, 1, 1), (30, 0, 194, 100, 0, 0),
                     (0, 49, 224, 51, 0, 1), (1, 1, 77, 97, 1, 0), (100, 20, 124, 33, 0, 0), (0, 0, 224, 100, 1, 1)], np.int32)[:len(clips)]
    raw = _launch(224, clips, 3)
    got = _launch(224, clips, 3, view_params=rows)
    for i in range(len(clips)):
        assert np.array_equal(got[i], evg_transform(raw[i], tuple(int(v) for v in rows[i]), VIEW, negate=True)), (clips[i], rows[i])
    assert float(np.abs(got).sum()) > 0


def test_unknown_algo_is_refused():
    from eventpretrain_amd import _lib
    p = 4096 * 16                  # validated on the host before any launch: never dereferenced
    rc = _lib.load().evp_voxel_scatter_fused_algo_f32(p, p, p, 3, p, p, p, p, 3000, 5, 100, 224, 1.0, 1.0, None, 0, 0, 0, p, p, 1, None)
    assert rc == -1 and b"algo" in _lib.load().evp_last_error()

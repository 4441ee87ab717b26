#!/usr/bin/env python3
"""One SHA-256 per K1 case of the grid with float64 cells (algo 3): run it from two checkouts on the same GPU and compare the lists
line by line. With float64 cells every cell is rounded to float32 once, at the flush, so a launch repeats bit for bit and a change
that keeps the per-row arithmetic keeps every digest. Float32 cells (algo 0) cannot be digested -- the LDS atomics arrive in another
order per launch -- so each line also carries max |algo 0 - algo 3| of the same tree (the project's bound between cell types: 2e-5).

Plain form (voxel_grid_batch): tile_rows 0 / 1 / 5, both column orders, verified / trust / unsorted. Fused form
(evp_voxel_scatter_fused_algo_f32): without decisions, with erased and added rows, raw and flushed through the nearest view.
Inputs: the small shapes below (tests/test_gpu_voxel_forms.py takes them from here) and one full-size batch, 64 clips x 100 k events
-> 5 x 224 x 224."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from eventpretrain_amd._lib import call, ptr, stream_ptr  # noqa: E402
from eventpretrain_amd.dataset.dataset_utils.events_to_voxel_grid import voxel_grid_batch  # noqa: E402
from eventpretrain_amd.testing import synthetic_events  # noqa: E402

H = 100
MAX_WINDOW = 3000


def sensor_clips(W):
    """Eight clips on a 100 x W sensor. clip 1: two stamps swapped across bin regions (the verified fast pass flags it, the repair pass
    scans it whole); clip 2: 3400 rows against max_window = 3000 (rows behind the bitmap); clip 3: empty; the others: 3000 rows."""
    clips = []
    for c in range(8):
        n = {2: 3400, 3: 0}.get(c, 3000)
        ev = synthetic_events(300 + 8 * W + c, n, width=W, height=H) if n else np.zeros((0, 4))
        if c == 1:
            ev[[500, 2500], 2] = ev[[2500, 500], 2]
        clips.append(ev)
    return clips


def tiny_clips():
    """Three 500-row clips on a 20 x 24 grid: one workgroup per clip at bins 2 (two jobs), five at bins 6 (an even count)."""
    return [synthetic_events(900 + c, 500, width=24, height=20) for c in range(3)]


def decisions(clips, size):
    """Per clip an ascending erase list (every 97th row, and for a window behind the bitmap its last two rows) and time-sorted added
    rows (every 131st row, moved and clipped to the sensor); nothing for an empty clip."""
    ers, adds = [], []
    for ev in clips:
        n = ev.shape[0]
        er = np.unique(np.concatenate([np.arange(3, n, 97), np.arange(max(n - 2, MAX_WINDOW), n)])).astype(np.int64)
        add = ev[5::131].copy()
        add[:, :3] += [1.25, -0.75, 1e-4]
        add[:, 0], add[:, 1] = np.clip(add[:, 0], 0, size[1] - 1), np.clip(add[:, 1], 0, size[0] - 1)
        ers.append(er), adds.append(add[np.argsort(add[:, 2], kind="stable")])
    return ers, adds


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _cum(xs):
    return np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)


def run_plain(clips, bins, size, algo, **kw):
    """The plain form on the clips as one batch -> numpy [n_clips, bins, H, W]."""
    return voxel_grid_batch(_dev(np.concatenate(clips, 0), torch.float64), _dev(_cum(clips)), bins, size, algo=algo, **kw).cpu().numpy()


def run_fused(clips, bins, sensor, algo, max_window=MAX_WINDOW, scale=(1.0, 1.0), ers=None, adds=None, view_params=None, view=(0, 0)):
    """The fused form on the clips as windows of one event array; ers / adds None: no decisions (all-zero offsets, one-element dummy
    arrays). sensor: the grid (H, W) the scaled rows fall into. view_params [n_clips, 6]: flushed through the nearest view."""
    nc = len(clips)
    ers = ers if ers is not None else [np.zeros(0, np.int64)] * nc
    adds = adds if adds is not None else [np.zeros((0, 4))] * nc
    off = _cum(clips)
    ev, d_wb, d_we = _dev(np.concatenate(clips, 0), torch.float64), _dev(off[:-1]), _dev(off[1:])
    d_er, d_eo = _dev(np.concatenate(list(ers) + [np.zeros(1, np.int64)])), _dev(_cum(ers))
    d_add, d_ao = _dev(np.concatenate(list(adds) + [np.zeros((1, 4))], 0), torch.float64), _dev(_cum(adds))
    prm = None if view_params is None else _dev(view_params, torch.int32)
    out = torch.full((nc, bins) + (tuple(sensor) if prm is None else tuple(view)), 7.0, device="cuda")
    ws = torch.zeros(nc * (bins + 5), dtype=torch.int64, device="cuda")
    call("evp_voxel_scatter_fused_algo_f32", ptr(ev), ptr(d_wb), ptr(d_we), nc, ptr(d_er), ptr(d_eo), ptr(d_add), ptr(d_ao), int(max_window),
         bins, int(sensor[0]), int(sensor[1]), float(scale[0]), float(scale[1]), ptr(prm), int(view[0]), int(view[1]), 1 if prm is not None else 0,
         ptr(ws), ptr(out), algo, stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def shapes():
    """(tag, clips, bins, grid (H, W), scale or None, max_window): the shapes of tests/test_gpu_voxel_forms.py."""
    out = []
    for W in (224, 222):
        clips = sensor_clips(W)
        out.append((f"100x{W} 3 clips", clips[1:4], 5, (H, W), None, MAX_WINDOW))
        out.append((f"100x{W} 8 clips", clips, 5, (H, W), None, MAX_WINDOW))
    out.append(("20x24 bins 2", tiny_clips(), 2, (20, 24), None, 512))
    out.append(("20x24 bins 6", tiny_clips(), 6, (20, 24), None, 512))
    out.append(("100x224 -> 50x112 scaled", sensor_clips(224)[1:4], 5, (50, 112), (0.5, 0.5), MAX_WINDOW))
    return out


def _line(tag, fn):
    g3, g0 = fn(3), fn(0)
    assert np.array_equal(g3, fn(3)), tag + ": two algo-3 launches differ"
    print(f"{tag:72s} {hashlib.sha256(np.ascontiguousarray(g3).tobytes()).hexdigest()}  |algo 0 - algo 3| {float(np.abs(g0 - g3).max()):.3e}", flush=True)


def main():
    txyp = lambda clips: [np.ascontiguousarray(ev[:, [2, 0, 1, 3]]) for ev in clips]
    full = [synthetic_events(i) for i in range(64)]
    for tag, clips, bins, size, scale, mw in shapes() + [("224x224 64 clips x 100k", full, 5, (224, 224), None, 100_000)]:
        small = len(clips) < 64
        for order, cl in (("xytp", clips), ("txyp", txyp(clips))):
            for mode, srt in (("verified", True), ("trust", "trust"), ("unsorted", False)):
                for t in (0, 1, 5) if small else (0,):
                    _line(f"plain {tag} {order} {mode} tile_rows {t}",
                          lambda a: run_plain(cl, bins, size, a, is_txyp=order == "txyp", assume_sorted=srt, tile_rows=min(t, size[0]), scale=scale))
        sc = scale or (1.0, 1.0)
        view = (72, 72) if small else (224, 224)
        prm = np.array([(3 * c % 7, c % 5, size[1] - 3 * c % 7 - c % 3, size[0] - c % 5 - c % 4, c & 1, (c >> 1) & 1) for c in range(len(clips))], np.int32)
        sensor = (int(round(size[0] / sc[1])), int(round(size[1] / sc[0])))
        for dtag, (ers, adds) in (("no decisions", (None, None)), ("erase + add", decisions(clips, sensor))):
            _line(f"fused {tag} {dtag} raw", lambda a: run_fused(clips, bins, size, a, mw, sc, ers, adds))
            _line(f"fused {tag} {dtag} view {view[0]}x{view[1]}", lambda a: run_fused(clips, bins, size, a, mw, sc, ers, adds, prm, view))


if __name__ == "__main__":
    main()

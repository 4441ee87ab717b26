"""numpy restatement of MVSEC's ground-truth flow label (the reference's FinetuneMVSECSeqDataset.gen_correspond_gt_flow with the two
searchsorted calls in front of it, dataset/finetune_flow/ft_mvsec_dataset.py:121-188, :264-272) as a hop schedule plus a per-pixel rule
-- what evp_mvsec_flow_propagate (include/evtpretrain.h K29) computes, and what tests/golden/mvsec_gt_flow.npz (made by the reference's
own function, tools/gen_mvsec_flow_golden.py) pins bit for bit.

The schedule (float64): left = searchsorted(ts, t1, 'right') - 1, right = searchsorted(ts, t2, 'right'), F = right - left frames and
F + 1 timestamps from `left` on. Direct iff t1 > ts[left] and t2 <= ts[left + 1]: the label is frame `left` times (t2 - t1) / (ts[left + 1]
- ts[left]), the product in float64, rounded once into the frame's dtype. Otherwise the hops are (left, (ts[left+1] - t1) / (ts[left+1] -
ts[left])), (left + i, 1.0) for i = 1 .. F - 2, (right - 1, (t2 - ts[right-1]) / (ts[right] - ts[right-1])) -- two hops through the same
frame when F = 1.

The rule, per pixel: x, y float32 from the pixel's own column and row; per hop (f, s): ix = rint(x), iy = rint(y) (half to even), ax,
ay = frame f's two planes at (iy, ix) -- BOTH at the position before the update, 0 outside the frame or for a NaN --, x_ok &= ax != 0,
y_ok &= ay != 0, x = float32(float64(x) + float64(ax) * s) with the product and the sum each rounded to float64, likewise y. The label is
(x - x0, y - y0) in float32, a component zeroed where its flag fell.

ROUNDING: rint's half-to-even is OpenCV's cvRound as remap's nearest mode uses it, stated from its source; the fixture was made with an
in-memory stand-in for cv2.remap that states the same rule (cv2 is not installed where the fixture was made), so the fixture pins the
arithmetic and the order of reads, NOT that rule against a real OpenCV.

`variant` names a deliberate mutation of the rule (MUTATIONS); tests/test_mvsec_flow_host.py holds that each fails the fixture."""
from fractions import Fraction

import numpy as np

SHAPE = (13, 17)                   # odd, no multiple of 64
N_SEQ = 10                         # frames of a case's sequence
MAX_HOPS = 8
MUTATIONS = ("half_away", "x_first", "shared_mask", "f32_product", "fma")
DTYPES = ("f32", "f64")
# the frames a sample slices and how (case_times); each kind with float32 and with float64 frames
KINDS = ("F1_direct", "F1_two_hop", "F2", "F2_edge_direct", "F2_real", "F3", "F4", "F6")
CASES = [f"{k}.{d}" for k in KINDS for d in DTYPES]


# ------------------------------------------------------------------------------------------------------------------ schedule
def flow_slice(flow_ts, t1, t2):
    ts = np.asarray(flow_ts, np.float64)
    return int(np.searchsorted(ts, t1, side="right")) - 1, int(np.searchsorted(ts, t2, side="right"))


def hops(flow_ts, t1, t2):
    """-> (frames int64 [n], scales float64 [n], n_hops): n_hops = 0 is the direct branch, whose frame and scale are row 0."""
    ts = np.asarray(flow_ts, np.float64)
    t1, t2 = np.float64(t1), np.float64(t2)
    left, right = flow_slice(ts, t1, t2)
    F = right - left
    assert 0 <= left and F >= 1 and right < ts.shape[0], (left, right, ts.shape[0])
    if t1 > ts[left] and t2 <= ts[left + 1]:
        return np.array([left], np.int64), np.array([(t2 - t1) / (ts[left + 1] - ts[left])], np.float64), 0
    frames = [left] + [left + i for i in range(1, F - 1)] + [right - 1]
    scales = [(ts[left + 1] - t1) / (ts[left + 1] - ts[left])] + [1.0] * (F - 2) + [(t2 - ts[right - 1]) / (ts[right] - ts[right - 1])]
    return np.array(frames, np.int64), np.array(scales, np.float64), len(frames)


# ------------------------------------------------------------------------------------------------------------------ the rule
def _round(v, variant):
    if variant == "half_away":
        return np.where(np.isnan(v), v, np.sign(v) * np.floor(np.abs(v) + np.float32(0.5)))
    return np.rint(v)


def _gather(plane, ix, iy):
    """plane[iy, ix] where (iy, ix) names a cell, else 0 (a NaN names none); ix, iy hold rounded floats."""
    H, W = plane.shape
    ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    out = np.zeros(ix.shape, plane.dtype)
    out[ok] = plane[iy[ok].astype(np.int64), ix[ok].astype(np.int64)]
    return out, ok


def _round_f32(r):
    """Fraction -> the nearest float32, ties to the even mantissa."""
    f = np.float32(float(r))
    cands = (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf)))
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - r), int(c.view(np.uint32)) & 1))


def _advance(pos, a, s, variant):
    if variant == "f32_product":
        return pos + a.astype(np.float32) * np.float32(s)
    if variant == "fma":                                  # one rounding of the exact pos + a * s
        flat = [_round_f32(Fraction(float(p)) + Fraction(float(v)) * Fraction(float(s))) for p, v in zip(pos.ravel(), a.ravel())]
        return np.array(flat, np.float32).reshape(pos.shape)
    return (pos.astype(np.float64) + a.astype(np.float64) * np.float64(s)).astype(np.float32)


def propagate(frames, hop_frames, hop_scales, n_hops, variant=None, stats=None):
    """frames [N,2,H,W] float32 | float64; hop_frames index them. -> the label: the frames' dtype in the direct branch (n_hops = 0),
    float32 otherwise. `stats` (a dict) collects what the walk met: pixels that left the frame on the first / a later hop, ties met per
    parity, zeros read."""
    frames = np.asarray(frames)
    H, W = frames.shape[2:]
    if n_hops == 0:
        a = frames[int(hop_frames[0])]
        return (a.astype(np.float64) * np.float64(hop_scales[0])).astype(a.dtype)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = xx.astype(np.float32), yy.astype(np.float32)
    x0, y0 = x.copy(), y.copy()
    x_ok, y_ok = np.ones((H, W), bool), np.ones((H, W), bool)
    inside = np.ones((H, W), bool)
    for k in range(int(n_hops)):
        f, s = int(hop_frames[k]), np.float64(hop_scales[k])
        ix, iy = _round(x, variant), _round(y, variant)
        ax, ok = _gather(frames[f, 0], ix, iy)
        if variant == "x_first":
            x_new = _advance(x, ax, s, variant)
            ay, _ = _gather(frames[f, 1], _round(x_new, variant), iy)
        else:
            ay, _ = _gather(frames[f, 1], ix, iy)
        if stats is not None:
            key = "left_first" if k == 1 else "left_later"        # (a pixel that leaves on hop 0 is seen outside at hop 1)
            stats[key] = stats.get(key, 0) + int((inside & ~ok).sum())
            inside &= ok
            for v in (x, y):
                tie = (np.abs(v - np.trunc(v)) == 0.5) & ok
                stats["tie_even"] = stats.get("tie_even", 0) + int((tie & (np.trunc(v) % 2 == 0)).sum())
                stats["tie_odd"] = stats.get("tie_odd", 0) + int((tie & (np.trunc(v) % 2 == 1)).sum())
            stats["zero_x_only"] = stats.get("zero_x_only", 0) + int((ok & (ax == 0) & (ay != 0)).sum())
            stats["zero_y_only"] = stats.get("zero_y_only", 0) + int((ok & (ay == 0) & (ax != 0)).sum())
        if variant == "shared_mask":
            x_ok &= (ax != 0) & (ay != 0)
            y_ok &= (ax != 0) & (ay != 0)
        else:
            x_ok &= ax != 0
            y_ok &= ay != 0
        x, y = _advance(x, ax, s, variant), _advance(y, ay, s, variant)
    out = np.stack([x - x0, y - y0]).astype(np.float32)
    out[0][~x_ok] = 0
    out[1][~y_ok] = 0
    return out


def label(frames, flow_ts, t1, t2, variant=None, stats=None):
    """The whole label of one sample: the schedule, then the rule."""
    hf, hs, n = hops(flow_ts, t1, t2)
    return propagate(frames, hf, hs, n, variant, stats)


def label_f32(frames, flow_ts, t1, t2):
    """What the loader's contract asks for: float32 [2,H,W] (a float64 frame in the direct branch is rounded once more)."""
    return np.ascontiguousarray(label(frames, flow_ts, t1, t2), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ the cases
def _ts(family):
    i = np.arange(N_SEQ, dtype=np.float64)
    if family == "dyadic":                                # spacing 2^-4 from 1024: halves and quarters of a gap are exact
        return 1024.0 + 0.0625 * i
    if family == "even":                                  # 0, 2, 4, ...: lets a scale of 0.5 + 2^-51 be written down exactly
        return 2.0 * i
    from eventpretrain_amd.testing import det_uniform
    jitter = det_uniform("mvsec.gt.ts", (N_SEQ,), -0.004, 0.004).double().numpy()
    return 1506117923.86 + 0.05 * i + jitter              # "real": MVSEC's magnitudes, 20 Hz with jitter


def case_times(kind):
    """-> (flow_ts float64 [N_SEQ], t1, t2, first-hop scale or None)."""
    if kind == "F1_direct":
        ts = _ts("real")
        return ts, ts[3] + 0.0113, ts[3] + 0.0335, None
    if kind == "F1_two_hop":                              # t1 == ts[left]: not direct; both hops go through frame `left`
        ts = _ts("real")
        return ts, ts[3], ts[3] + 0.0223, 1.0
    if kind == "F2":
        ts = _ts("dyadic")
        return ts, ts[2] + 0.03125, ts[3] + 0.0625 * 0.3, 0.5
    if kind == "F2_edge_direct":                          # t2 == ts[left + 1]: 'right' counts it, F = 2, and the branch test says direct
        ts = _ts("real")
        return ts, ts[4] + 0.0071, ts[5], None
    if kind == "F2_real":
        ts = _ts("real")
        return ts, ts[4] + 0.0171, ts[5] + 0.0093, None
    if kind == "F3":                                      # first scale (6 - t1) / 2 = 0.5 + 2^-51
        ts = _ts("even")
        return ts, 5.0 - 2.0 ** -50, 9.3, 0.5
    if kind == "F4":
        ts = _ts("real")
        return ts, ts[2], ts[5] + 0.0312, 1.0
    if kind == "F6":
        ts = _ts("dyadic")
        return ts, ts[1] + 0.03125, ts[6] + 0.0625 * 0.77, 0.5
    raise KeyError(kind)


def case_inputs(name):
    """-> (frames [N_SEQ,2,H,W] float32 | float64, flow_ts, t1, t2), re-made from testing.det_uniform; what is planted:
      every frame   x-plane zero at rows 2:4, cols 3:6, y-plane zero at rows 3:5, cols 5:8 (a zero in one plane only, and in both)
      frame `left`  +20 px at rows 0:2, cols 12:15 (gone on the first hop); at row 8, cols 4 and 5 an x-flow that lands on c + 0.5
                    under the first scale (an even and an odd tie), at col 10, rows 6 and 7 the same in y; at (10, 4) an x-flow of
                    2^-21: under F3's first scale 0.5 + 2^-51 the exact 4 + 2^-22 + 2^-72 lies above a float32 midpoint that the
                    float64 sum lands on exactly, so one rounding and two give different floats."""
    from eventpretrain_amd.testing import det_uniform
    kind, d = name.split(".")
    H, W = SHAPE
    ts, t1, t2, s0 = case_times(kind)
    a = det_uniform(f"mvsec.gt.frames.{kind}", (N_SEQ, 2, H, W), -3.0, 3.0).numpy()
    if d == "f64":
        a = a.astype(np.float64) + det_uniform(f"mvsec.gt.low.{kind}", (N_SEQ, 2, H, W), -1.0, 1.0).numpy().astype(np.float64) * 2.0 ** -30
    a[:, 0, 2:4, 3:6] = 0
    a[:, 1, 3:5, 5:8] = 0
    left, _ = flow_slice(ts, t1, t2)
    a[left, 0, 0:2, 12:15] = 20.0
    tie = 0.5 if s0 == 1.0 else 1.0
    a[left, 0, 8, 4:6] = tie
    a[left, 1, 8, 4:6] = 0.25
    a[left, 1, 6:8, 10] = tie
    a[left, 0, 6:8, 10] = 0.25
    a[left, :, 10, 4] = 2.0 ** -21
    return a, ts, np.float64(t1), np.float64(t2)

#!/usr/bin/env python3
"""The N-Cars recipe's loader chain beside the sensor-resolution one, one process, one box: 64 clips on a 100 x 120 grid (the reference's
cars_sensor_h / _w), 3000-row windows (main_finetune_cls.py's fix_events_num), 5 x 100 x 120 grids -> 5 x 224 x 224 views, bilinear.

  sensor chain   the self-driven captured chain, grid="sensor", sensor=(100, 120): plan, draw, build added rows, fused K1 (float32
                 cells) -> raw grids, bilinear view kernel under crop rows drawn on 100 x 120;
  window chain   the same with grid="window", sensor=(100, 120) as the capacity: one more launch (evp_events_window_geometry) between the
                 plan and the draw, the added rows bounded per clip, the crop rows drawn on each clip's own extent.

Device events around 24 replays per round, five alternating rounds. With `--trace-only N` the process just replays the window chain N
times, for a `rocprofv3 --kernel-trace --stats` run that gives the geometry kernel's own time."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
from eventpretrain_amd.testing import make_args, synthetic_events

B, S, CAP, FIX, ROUNDS, N_CLIP = 64, 224, (100, 120), 3000, 5, 5000
H, W = CAP


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def spread(v):
    return f"min {min(v):.1f}, median {sorted(v)[len(v) // 2]:.1f}, max {max(v):.1f} us (rounds: {', '.join('%.1f' % x for x in v)})"


pa = make_args(crop_min=0.8, input_size=S, fix_events_num=FIX, val_fix_events_num=FIX, device="cuda")
# clips of their own extents inside the capacity (the window chain's grids differ per clip; the sensor chain bins the same rows at 100 x 120)
clips = [synthetic_events(4242 + i, N_CLIP, width=W - (7 * i) % 60, height=H - (5 * i) % 50) for i in range(B)]
ev = torch.from_numpy(np.concatenate(clips, 0)).cuda()
off = np.arange(0, (B + 1) * N_CLIP, N_CLIP, dtype=np.int64)
kw = dict(seed=1, resize_mode="bilinear", sensor=CAP)
window = GpuInputPipeline(pa, grid="window", **kw).capture(ev, B, clip_offsets=off)
if len(sys.argv) > 2 and sys.argv[1] == "--trace-only":
    for _ in range(int(sys.argv[2])):
        window.run_next()
    torch.cuda.synchronize()
    assert int(window.geom_status.item()) == 0
    sys.exit(0)
sensor = GpuInputPipeline(pa, grid="sensor", **kw).capture(ev, B, clip_offsets=off)

forms = {"sensor chain (grid='sensor', 100 x 120)": sensor.run_next, "window chain (grid='window', capacity 100 x 120)": window.run_next}
for fn in forms.values():
    timed(fn, 3)
res = {k: [] for k in forms}
for rnd in range(ROUNDS):
    for k, fn in forms.items():
        res[k].append(timed(fn, 24))
print(f"B = {B}, capacity {H} x {W} -> {S} x {S}, bilinear, windows of {FIX} rows out of {N_CLIP}-row clips; per batch, 24 replays per round, "
      f"{ROUNDS} alternating rounds")
for k, v in res.items():
    print(f"{k}: {spread(v)}")
a, b = res["sensor chain (grid='sensor', 100 x 120)"], res["window chain (grid='window', capacity 100 x 120)"]
print(f"window - sensor: {min(b) - min(a):+.1f} us per batch (min over min), {sorted(b)[ROUNDS // 2] - sorted(a)[ROUNDS // 2]:+.1f} us (median over median); "
      f"spread between rounds: sensor {max(a) - min(a):.1f} us, window {max(b) - min(b):.1f} us")
ext = window.ext.cpu().numpy()
print(f"extents of the last batch: H_c {ext[:, 0].min()}..{ext[:, 0].max()}, W_c {ext[:, 1].min()}..{ext[:, 1].max()}; refused windows: "
      f"{int(window.geom_status.item())}")

#!/usr/bin/env python3
"""The fine-tuning recipe's loader chain beside the pre-training one, same process, same box (bench.py's `loader_chain` workload: 64 clips
of 150 k events on a 640 x 480 sensor, 100 k-event windows, 5 x 224 x 224 views):

  chains   the self-driven captured chain per batch (device events around 24 replays, three alternating rounds): nearest-fused with
           frame targets (the configuration bench.py times), nearest-fused without frames, bilinear (K1 -> raw grids -> bilinear view
           kernel) without frames -- a fine-tuning batch has labels, not frame targets;
  kernels  evp_view_augment_f32 and evp_view_augment_bilinear_f32 alone on 64 raw grids, 20 launches each: event-timed here; run
           `--kernels-only` under `rocprofv3 --kernel-trace --stats` for the profiler's own per-kernel figures."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eventpretrain_amd.dataset.augmentation import view_augment as va
from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
from eventpretrain_amd.testing import make_args, synthetic_events

ap = argparse.ArgumentParser()
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--batch", type=int, default=64)
ns = ap.parse_args()
B, S = ns.batch, 224


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


pa = make_args(crop_min=0.8, input_size=S, fix_events_num=100_000, img_sensor_w=640, img_sensor_h=480, device="cuda")
clip = synthetic_events(4242, 150_000, width=640, height=480)
ev = torch.from_numpy(np.concatenate([clip] * B, 0)).cuda()
off = np.arange(0, (B + 1) * 150_000, 150_000, dtype=np.int64)

# ---- the two view kernels alone, on real grids under the crop rows the chain's stream draws
pipe_b = GpuInputPipeline(pa, seed=1, resize_mode="bilinear")
chain_b = pipe_b.capture(ev, B, clip_offsets=off)
chain_b.run_next()
torch.cuda.synchronize()
raw = chain_b.raw.clone()
prm = torch.from_numpy(va.draw_evg_params_batch(1, 0, B, S, S, 0.8)).cuda()
out = torch.empty_like(raw)
for mode in ("nearest", "bilinear"):
    fn = lambda: va.evg_augment_batch(raw, prm, (S, S), out=out, mode=mode)
    timed(fn, 3)
    us = timed(fn, 20)
    moved = 2 * raw.numel() * 4
    print(f"view kernel {mode}: {us:.1f} us per launch (B = {B}, 5 x {S} x {S}; {moved / 1e6:.0f} MB at most read + written = {moved / us / 1e6:.2f} TB/s)")
if ns.kernels_only:
    sys.exit(0)

# ---- the captured chains
frames = torch.randn(B, 1, 480, 640, device="cuda")
pipe_n = GpuInputPipeline(pa, seed=1)
chains = {"nearest fused + frame targets": pipe_n.capture(ev, B, frames=frames, clip_offsets=off),
          "nearest fused": pipe_n.capture(ev, B, clip_offsets=off),
          "bilinear (K1 -> raw -> view)": chain_b}
for c in chains.values():
    timed(c.run_next, 3)
res = {k: [] for k in chains}
for rnd in range(3):
    for k, c in chains.items():
        res[k].append(timed(c.run_next, 24))
for k, v in res.items():
    print(f"chain {k}: {min(v):.1f} us per batch (rounds: {', '.join('%.1f' % x for x in v)})")
for k, p in (("nearest fused", pipe_n), ("bilinear (K1 -> raw -> view)", pipe_b)):
    print(f"algorithmic bytes {k}: {p.algorithmic_bytes(np.full(B, 100_000), fused=True) / 1e6:.0f} MB per batch")

#!/usr/bin/env python3
"""The sensor-resolution fine-tuning recipe's loader forms beside each other, one process, one box: 64 clips of 150 k events on a 180 x 240
sensor (N-Caltech101 / UCF101-DVS), 100 k-event windows, 5 x 180 x 240 grids -> 5 x 224 x 224 views, bilinear.

  train        the self-driven captured chain, grid="sensor": plan, draw, build added rows, fused K1 (float32 cells) -> raw grids,
               bilinear view kernel under the drawn crop rows;
  clean val    what GpuFinetuneLoader runs per clean validation batch: K1 algo 3 on the windows + the bilinear view kernel under the
               full-box rows (eager launches, not a graph);
  noisy val    the self-driven captured chain with view_augment=False, fused K1 with float32 cells and with float64 cells.

Device events around 24 replays / calls per round, five alternating rounds; then the fused K1 entry alone on the noisy chain's tables,
algo 0 against algo 3, 20 launches per round, five alternating rounds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eventpretrain_amd._lib import call, ptr, stream_ptr
from eventpretrain_amd.dataset.augmentation import view_augment as va
from eventpretrain_amd.dataset.dataset_utils.events_to_voxel_grid import voxel_grid_batch
from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
from eventpretrain_amd.testing import make_args, synthetic_events

B, S, SENSOR, FIX, ROUNDS = 64, 224, (180, 240), 100_000, 5
H, W = SENSOR


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
clip = synthetic_events(4242, 150_000, width=W, height=H)
ev = torch.from_numpy(np.concatenate([clip] * B, 0)).cuda()
off = np.arange(0, (B + 1) * 150_000, 150_000, dtype=np.int64)
kw = dict(seed=1, resize_mode="bilinear", grid="sensor", sensor=SENSOR)
train = GpuInputPipeline(pa, **kw).capture(ev, B, clip_offsets=off)
noisy = {c: GpuInputPipeline(pa, fix_events_num=pa.val_fix_events_num, view_augment=False, voxel_cells=c, **kw).capture(ev, B, clip_offsets=off)
         for c in ("f32", "f64")}

# clean validation: the windows as the loader uploads them (contiguous), K1 algo 3 into static raw grids, the view kernel under the full box
ev_val = torch.from_numpy(np.concatenate([clip[:FIX]] * B, 0)).cuda()
off_val = torch.arange(0, (B + 1) * FIX, FIX, dtype=torch.int64, device="cuda")
raw = torch.zeros(B, 5, H, W, device="cuda")
out = torch.zeros(B, 5, S, S, device="cuda")
full = torch.tensor([[0, 0, W, H, 0, 0]] * B, dtype=torch.int32, device="cuda")


def clean_val():
    voxel_grid_batch(ev_val, off_val, 5, SENSOR, out=raw, algo=3)
    va.evg_augment_batch(raw, full, (S, S), out=out, mode="bilinear")


forms = {"train chain (fused K1 f32 -> raw -> bilinear view)": train.run_next,
         "clean val pair (K1 algo 3 + bilinear resize, eager)": clean_val,
         "noisy val chain, float32 cells": noisy["f32"].run_next,
         "noisy val chain, float64 cells": noisy["f64"].run_next}
for fn in forms.values():
    timed(fn, 3)
res = {k: [] for k in forms}
for rnd in range(ROUNDS):
    for k, fn in forms.items():
        res[k].append(timed(fn, 24))
print(f"B = {B}, {H} x {W} -> {S} x {S}, bilinear, windows of {FIX} rows; per batch, 24 per round, {ROUNDS} alternating rounds")
for k, v in res.items():
    print(f"{k}: {spread(v)}")
a, b = res["noisy val chain, float32 cells"], res["noisy val chain, float64 cells"]
print(f"noisy val chain, float64 / float32 cells: {min(b) / min(a):.3f} x (min over min), +{min(b) - min(a):.1f} us per batch")

# ---- the fused K1 entry alone, on the tables the float64 chain's last replay planned: float32 cells (algo 0) against float64 (algo 3)
ch = noisy["f64"]
tabs = ch.d_tab[:5 * (B + 1)].view(5, B + 1)
kws = torch.zeros_like(ch.kws)


def fused(algo):
    call("evp_voxel_scatter_fused_algo_f32", ptr(ev), ptr(tabs[0]), ptr(tabs[1]), B, ptr(ch.er), ptr(tabs[2]), ptr(ch.ws), ptr(tabs[3]), FIX, 5, H, W,
         1.0, 1.0, None, 0, 0, 0, ptr(kws), ptr(raw), algo, stream_ptr())


k1 = {0: [], 3: []}
for algo in k1:
    timed(lambda: fused(algo), 3)
for rnd in range(ROUNDS):
    for algo in k1:
        k1[algo].append(timed(lambda: fused(algo), 20))
print(f"fused K1 alone (cuts + fast pass + repair pass, no view), 20 launches per round, {ROUNDS} alternating rounds")
print(f"fused K1 float32 cells (two y-tiles): {spread(k1[0])}")
print(f"fused K1 float64 cells (three y-tiles): {spread(k1[3])}")
print(f"fused K1 float64 / float32 cells: {min(k1[3]) / min(k1[0]):.3f} x (min over min)")
g64 = raw.clone()
fused(3)
torch.cuda.synchronize()
print(f"two float64-cell launches differ in {int((g64 != raw).sum())} of {raw.numel()} elements")
fused(0)
torch.cuda.synchronize()
print(f"float32-cell launch against float64: max |diff| {float((g64 - raw).abs().max()):.3e}")
p = GpuInputPipeline(pa, **kw)
print(f"algorithmic bytes, train chain: {p.algorithmic_bytes(np.full(B, FIX), fused=True) / 1e6:.0f} MB per batch")

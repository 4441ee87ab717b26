#!/usr/bin/env python3
"""evp_mvsec_flow_propagate beside what it replaces, one process, one box, 64-sample batches at MVSEC's 260 x 346:

  the kernel        direct, 2-hop and 4-hop batches from 512 resident float32 frames (369 MB: more than the Infinity Cache holds; every
                    sample of a batch walks frames of its own), next to its traffic floor -- 8 B gathered per hop and pixel + 8 B written
  the upload        the [64,2,260,346] float32 label batch from a pinned slot to the device, as the loader does without gt_flow
  the host's label  tests/mvsec_flow_truth.py's numpy restatement of gen_correspond_gt_flow per sample (2 and 4 hops), on this host's CPU:
                    the stand-in for the reference's own function (two cv2.remap calls per hop on a DataLoader worker)

Device events around N calls per round, five alternating rounds (every form warmed first; min / median / max over the rounds). Before
anything is timed the kernel's output is compared with the restatement on one sample of each form."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

B, H, W, N_FRAMES, ROUNDS, N = 64, 260, 346, 512, 5, 20


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def report(name, v, nbytes=None):
    med = sorted(v)[len(v) // 2]
    rate = "" if nbytes is None else f"  floor {nbytes / 1e6:.1f} MB -> {nbytes / med / 1e6:.2f} TB/s at the median"
    print(f"{name:<46s} {len(v)} rounds x {N}: min {min(v):8.1f}  median {med:8.1f}  max {max(v):8.1f} us{rate}", flush=True)


def main():
    import mvsec_flow_truth as truth
    from eventpretrain_amd import _lib
    from eventpretrain_amd.dataset.finetune_dense.mvsec_flow import mvsec_flow_propagate_batch
    from eventpretrain_amd.testing import det_uniform
    _lib.require_device()
    one = det_uniform("ab.mvsec.gt", (8, 2, H, W), -4.0, 4.0).numpy()
    one[:, :, 100:140, 50:120] = 0                                         # (MVSEC's frames have large empty regions)
    host = np.concatenate([np.roll(one, 3 * i, axis=-1) for i in range(N_FRAMES // 8)], 0)
    frames = torch.from_numpy(host).cuda()
    out = torch.zeros(B, 2, H, W, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    forms, tables = {}, {}
    for tag, n_hops in (("direct", 0), ("2 hops", 2), ("4 hops", 4)):
        rows = max(n_hops, 1)
        hf, hs = np.zeros((B, 8), np.int64), np.zeros((B, 8), np.float64)
        for b in range(B):
            hf[b, :rows] = (b * 7 + np.arange(rows)) % N_FRAMES                # consecutive frames, a start of its own per sample
            hs[b, :rows] = [0.37 + 0.001 * b] + [1.0] * (rows - 2) + ([0.61 - 0.001 * b] if rows > 1 else [])
        nh = np.full(B, n_hops, np.int32)
        tables[tag] = (hf, hs, nh)
        d = tuple(torch.from_numpy(a).cuda() for a in (hf, hs, nh))
        mvsec_flow_propagate_batch(frames, *d, out, status)
        want = truth.propagate(host, hf[5], hs[5], n_hops).astype(np.float32)
        print(f"{tag}: sample 5 equal to the restatement: {np.array_equal(out[5].cpu().numpy(), want)}, status {status.tolist()}", flush=True)
        floor = B * H * W * (8 * rows + 8)
        forms[f"evp_mvsec_flow_propagate, {tag}"] = ((lambda d=d: mvsec_flow_propagate_batch(frames, *d, out, status)), floor)
    pin = torch.zeros(B, 2, H, W).pin_memory()
    pin.copy_(torch.from_numpy(host[:2 * B].reshape(B, 2, 2, H, W)[:, 0]))
    dev = torch.zeros(B, 2, H, W, device="cuda")
    forms["H2D copy of the label batch (pinned slot)"] = ((lambda: dev.copy_(pin, non_blocking=True)), B * 2 * H * W * 4)
    for fn, _ in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, (fn, _) in forms.items():
            times[k].append(timed(fn, N))
    for k in forms:
        report(k, times[k], forms[k][1])
    # the host's label, per sample, on this machine's CPU (one thread, as a DataLoader worker)
    torch.set_num_threads(1)
    for tag in ("2 hops", "4 hops"):
        hf, hs, nh = tables[tag]
        truth.propagate(host, hf[0], hs[0], int(nh[0]))
        per = []
        for r in range(ROUNDS):
            t0 = time.perf_counter()
            for b in range(8):
                truth.propagate(host, hf[b], hs[b], int(nh[b]))
            per.append((time.perf_counter() - t0) / 8 * 1e3)
        print(f"numpy restatement, {tag}, per SAMPLE on the host   {ROUNDS} rounds x 8: min {min(per):.2f}  median {sorted(per)[ROUNDS // 2]:.2f}  "
              f"max {max(per):.2f} ms  (x {B} samples = {B * sorted(per)[ROUNDS // 2]:.0f} ms per batch on one worker)", flush=True)


if __name__ == "__main__":
    main()

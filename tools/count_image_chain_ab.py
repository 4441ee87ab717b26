#!/usr/bin/env python3
"""The event-count-image loader chain (args.num_bins 2 and 3) beside the 5-bin voxel chain, one process, one box: 64 clips on N-ImageNet's
480 x 640 sensor, rescaled to 224 x 224 (grid="input"), bilinear views, at the reference's fine-tuning window lengths (fix_events_num 3000
for training, val_fix_events_num 40000).

  count 2 / count 3   the self-driven captured chain in its merged-clip form: plan, draw, erase / add merge, evp_event_image_count,
                      evp_event_image_finish, bilinear view kernel, evp_event_image_normalize;
  voxel 5 merged      the same chain with num_bins = 5 and fused_voxel=False (erase / add merge, K1, bilinear view kernel);
  voxel 5 fused       the 5-bin chain's default form, for scale;
  torch 2 / torch 3   the same transforms as per-sample torch ops on the device (bincount on the linear index, mean / std threshold,
                      F.interpolate, amax), on the count chain's own merged clips and crop rows.

Device events around 24 replays per round, five alternating rounds. Then evp_event_image_count alone on the chain's merged clips against its
read floor: rows x 32 B at the streaming rate measured here with a 1 GiB device copy."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from eventpretrain_amd._lib import call, ptr, stream_ptr
from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
from eventpretrain_amd.testing import make_args, synthetic_events

B, S, SENSOR, ROUNDS = 64, 224, (480, 640), 5
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


def torch_chain(chain, nb):
    """Per-sample torch ops on the device, on the merged clips and crop rows of the chain's last replay (read back once, outside the timing)."""
    off = chain.d_tab[:5 * (B + 1)].view(5, B + 1)[4].tolist()
    rows = chain.crop_rows.tolist()
    sx, sy = chain.pipe.scale
    ev = chain.ev

    def run():
        outs = []
        for c in range(B):
            e = ev[off[c]:off[c + 1]]
            lin = (e[:, 0] * sx).long() + (e[:, 1] * sy).long() * S
            pos = torch.bincount(lin[e[:, 3] == 1], minlength=S * S).reshape(S, S)
            neg = torch.bincount(lin[e[:, 3] == 0], minlength=S * S).reshape(S, S)
            if nb == 2:
                img = torch.stack([pos, neg]).float()
            else:
                img = torch.stack([pos, torch.zeros_like(pos), neg]).float() / 255
                thr = img[0::2].mean() + 10 * img[0::2].std()
                hot = (img[0] > thr) | (img[2] > thr)
                img[0::2] = img[0::2] * (~hot)
            x0, y0, w, h, hf, tf = rows[c]
            v = F.interpolate(img[None, :, y0:y0 + h, x0:x0 + w], size=(S, S), mode="bilinear")[0]
            if hf:
                v = v.flip(2)
            if tf:
                v = v.flip(0)
            if nb == 2:
                v = (v / (v.amax([1, 2], True) + 1) - 0.5) * 2
            else:
                v[0::2] = v[0::2] * (1.0 / v[0::2].max())
            outs.append(v)
        return torch.stack(outs)
    return run


def main():
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(big)
    timed(lambda: dst.copy_(big), 2)
    rate = 2 * big.numel() * 4 / (min(timed(lambda: dst.copy_(big), 5) for _ in range(3)) * 1e-6)
    del big, dst
    say(f"streaming rate of a 1 GiB device copy (read + write): {rate / 1e12:.2f} TB/s")
    for fix in (3000, 40000):
        clip = synthetic_events(4242, fix + fix // 2, width=W, height=H)
        ev = torch.from_numpy(np.concatenate([clip] * B, 0)).cuda()
        off = np.arange(0, (B + 1) * clip.shape[0], clip.shape[0], dtype=np.int64)
        chains = {}
        for nb in (2, 3, 5):
            a = make_args(crop_min=0.8, input_size=S, fix_events_num=fix, num_bins=nb, device="cuda")
            chains[nb] = GpuInputPipeline(a, seed=1, resize_mode="bilinear", representation="voxel" if nb == 5 else "count").capture(
                ev, B, clip_offsets=off, fused_voxel=False)
        a5 = make_args(crop_min=0.8, input_size=S, fix_events_num=fix, num_bins=5, device="cuda")
        fused5 = GpuInputPipeline(a5, seed=1, resize_mode="bilinear").capture(ev, B, clip_offsets=off)
        assert not chains[2].fused and not chains[5].fused and fused5.fused
        for ch in chains.values():
            ch.run_next()
        torch.cuda.synchronize()
        forms = {"count 2 chain": chains[2].run_next, "count 3 chain": chains[3].run_next, "voxel 5 merged chain": chains[5].run_next,
                 "voxel 5 fused chain": fused5.run_next, "torch 2 per-sample ops": torch_chain(chains[2], 2),
                 "torch 3 per-sample ops": torch_chain(chains[3], 3)}
        for fn in forms.values():
            timed(fn, 3)
        res = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, fn in forms.items():
                res[k].append(timed(fn, 24 if "torch" not in k else 4))
        say(f"B = {B}, {H} x {W} -> {S} x {S}, bilinear, windows of {fix} rows; per batch, {ROUNDS} alternating rounds")
        for k, v in res.items():
            say(f"  {k}: {spread(v)}")
        # the count entry alone (clears + scatter) on the 2-channel chain's merged clips
        ch = chains[2]
        tabs = ch.d_tab[:5 * (B + 1)].view(5, B + 1)
        rows = int(tabs[4, -1].item())
        work = torch.empty(B * (3 * S * S + 1), dtype=torch.int32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        sx, sy = ch.pipe.scale

        def count():
            call("evp_event_image_count", ptr(ch.ev), int(ch.ev.shape[0]), ptr(tabs[4]), B, fix + ch.kmax, S, S, sx, sy, ptr(work),
                 ptr(work[B * 3 * S * S:]), ptr(st), stream_ptr())

        timed(count, 3)
        t = [timed(count, 24) for _ in range(ROUNDS)]
        floor = rows * 32 / rate * 1e6
        say(f"  evp_event_image_count alone ({rows} rows, clears of {B * 3 * S * S * 4 / 1e6:.1f} MB included): {spread(t)}")
        say(f"  its read floor, rows x 32 B at the measured rate: {floor:.1f} us -> {min(t) / floor:.1f} x the floor; rows outside: {int(st.item())}")
    if len(sys.argv) > 1:                                     # keep the report: python tools/count_image_chain_ab.py REPORT.txt
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The dense fine-tuning input's new kernels beside what they replace, one process, one box, 64-clip batches at the two dense shapes:

  DSEC   labels 440 x 640, events on the 480 x 640 org sensor, 200 000 rows per clip, rectified through a (480, 640, 2) map
  MVSEC  labels 260 x 346, 100 000 rows per clip on 280 x 360, the plain crop mask (map = NULL)

per batch: evp_semseg_label_augment and evp_flow_label_augment_f32 under drawn crop rows against the same transforms as plain torch ops on
the device (per sample, as the reference's functions: crop -> F.interpolate(nearest) -> flip [-> scale, signs; the valid mask]), and
evp_events_rectify_compact_f64; then, at the DSEC shape, the self-driven captured chain alone (grid="sensor", bilinear, the view the labels
ride with) and a whole GpuDenseLoader batch (pack, upload, rectify, chain, label kernel), wall clock over a pass.

Device events around N calls per round, five alternating rounds (measuring guide: warm every shape, alternate, report the spread). Each
kernel's bytes moved (computed from the shapes, below) over its median time is printed next to the time, to be read against
tools/bw_probe.py's figures for this box."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

B, S, ROUNDS, N = 64, 224, 5, 20


def torch_semseg_view(labels, rows, size):
    """semseg_label_augment of the reference, sample by sample, as torch ops on the labels' device: uint8 [B,1,H,W] -> int64 [B,1,Ho,Wo]."""
    out = []
    for b, (x0, y0, w, h, hflip, _) in enumerate(rows.tolist()):
        v = F.interpolate(labels[b:b + 1, :, y0:y0 + h, x0:x0 + w].float(), size=size, mode="nearest")
        out.append((torch.flip(v, dims=[3]) if hflip else v).long())
    return torch.cat(out, 0)


def torch_flow_view(flow, rows, size):
    """flow_label_augment + the dataset's valid mask under flow_label_valid_augment, sample by sample -> ([B,2,Ho,Wo], [B,1,Ho,Wo])."""
    valid = ((torch.norm(flow, p=2, dim=1, keepdim=True) > 0) & (flow[:, :1].abs() < 1000) & (flow[:, 1:].abs() < 1000)).float()
    fo, vo = [], []
    for b, (x0, y0, w, h, hflip, tflip) in enumerate(rows.tolist()):
        f = F.interpolate(flow[b:b + 1, :, y0:y0 + h, x0:x0 + w], size=size, mode="nearest")
        f = f * torch.tensor([size[1] / w, size[0] / h], device=flow.device).view(1, 2, 1, 1)
        v = F.interpolate(valid[b:b + 1, :, y0:y0 + h, x0:x0 + w], size=size, mode="nearest")
        if hflip:
            f, v = torch.flip(f, dims=[3]) * torch.tensor([-1.0, 1.0], device=flow.device).view(1, 2, 1, 1), torch.flip(v, dims=[3])
        if tflip:
            f = f * -1.0
        fo.append(f), vo.append(v)
    return torch.cat(fo, 0), torch.cat(vo, 0)


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
    rate = "" if nbytes is None else f"  {nbytes / 1e6:.1f} MB -> {nbytes / med / 1e6:.2f} TB/s at the median"
    print(f"{name:<44s} min {min(v):8.1f}  median {med:8.1f}  max {max(v):8.1f} us{rate}", flush=True)
    return med


def alternate(forms):
    """forms: {name: (fn, bytes | None)} -> medians; every form warmed, then ROUNDS rounds in which the forms take turns."""
    for fn, _ in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, (fn, _) in forms.items():
            times[k].append(timed(fn, N))
    return {k: report(k, times[k], forms[k][1]) for k in forms}


def shape_forms(tag, sensor, org, rows_per_clip, with_map):
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import rectify_compact_batch
    from eventpretrain_amd.testing import det_uniform, synthetic_events
    H, W = sensor
    rows = va.draw_evg_params_batch(1, 0, B, H, W, 0.8)
    d_rows = torch.from_numpy(rows).cuda()
    lab = (det_uniform(f"ab.label.{tag}", (B, 1, H, W), 0.0, 19.0)).to(torch.uint8).cuda()
    flow = det_uniform(f"ab.flow.{tag}", (B, 2, H, W), -30.0, 30.0).cuda()
    flow[:, :, ::3] = 0.0
    lab_out = torch.zeros(B, 1, H, W, dtype=torch.int64, device="cuda")
    f_out, v_out = torch.zeros(B, 2, H, W, device="cuda"), torch.zeros(B, 1, H, W, device="cuda")
    # equal outputs first: what is timed computes the same thing
    same = [torch.equal(va.semseg_label_augment_batch(lab, d_rows, sensor, out=lab_out), torch_semseg_view(lab, rows, sensor))]
    tf, tv = torch_flow_view(flow, rows, sensor)
    va.flow_label_augment_batch(flow, d_rows, sensor, out=f_out, valid_out=v_out)
    same += [torch.equal(f_out, tf), torch.equal(v_out, tv)]
    print(f"{tag}: kernels equal to the torch forms (label, flow, valid): {same}", flush=True)
    clip = synthetic_events(4242, rows_per_clip, width=org[1], height=org[0])
    ev = torch.from_numpy(np.concatenate([clip] * B, 0)).cuda()
    off = torch.arange(0, (B + 1) * rows_per_clip, rows_per_clip, dtype=torch.int64, device="cuda")
    rmap = None
    if with_map:
        yy, xx = np.meshgrid(np.arange(org[0], dtype=np.float64), np.arange(org[1], dtype=np.float64), indexing="ij")
        rmap = torch.from_numpy(np.stack([xx + 0.3 * np.sin(yy / 7.0), yy - 0.5 * (org[0] - H)], -1).astype(np.float32)).cuda()
    out = torch.zeros(B * rows_per_clip, 4, dtype=torch.float64, device="cuda")
    off_out, status = torch.zeros(B + 1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.zeros(B * (rows_per_clip // 1024 + 1) + 1, dtype=torch.int32, device="cuda")
    compact = lambda: rectify_compact_batch(ev, off, rows_per_clip, rows_per_clip, sensor, out, off_out, status, rectify_map=rmap, workspace=ws)
    compact()
    kept = int(off_out[-1])
    n = B * rows_per_clip
    px = B * H * W
    print(f"--- {tag}: labels {H} x {W}, {rows_per_clip} rows per clip on {org[0]} x {org[1]}, {kept / n:.3f} of the rows kept, status {status.tolist()}")
    status.zero_()
    return {
        f"{tag} evp_semseg_label_augment": (lambda: va.semseg_label_augment_batch(lab, d_rows, sensor, out=lab_out), px * 9),
        f"{tag} semseg label view, torch ops": (lambda: torch_semseg_view(lab, rows, sensor), None),
        f"{tag} evp_flow_label_augment_f32": (lambda: va.flow_label_augment_batch(flow, d_rows, sensor, out=f_out, valid_out=v_out), px * 20),
        f"{tag} flow label + valid view, torch ops": (lambda: torch_flow_view(flow, rows, sensor), None),
        # two passes over the rows (counts, scatter), the map cell of a row in each, the survivors written once
        f"{tag} evp_events_rectify_compact_f64": (compact, n * 64 + (n * 16 if with_map else 0) + kept * 32),
    }


def dsec_chain_and_loader():
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import GpuDenseLoader
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    from eventpretrain_amd.testing import det_uniform, make_args, synthetic_events
    sensor, org, fix = (440, 640), (480, 640), 200_000
    H, W = sensor
    a = make_args(crop_min=0.8, input_size=S, fix_events_num=fix, val_fix_events_num=fix, device="cuda")
    clip = synthetic_events(4242, fix, width=W, height=H)
    ev = torch.from_numpy(np.concatenate([clip] * B, 0)).cuda()
    chain = GpuInputPipeline(a, seed=1, resize_mode="bilinear", grid="sensor", sensor=sensor).capture(
        ev, B, clip_offsets=np.arange(0, (B + 1) * fix, fix, dtype=np.int64))
    alternate({"DSEC self-driven chain alone (bilinear view)": (chain.run_next, None)})
    del chain, ev
    yy, xx = np.meshgrid(np.arange(org[0], dtype=np.float64), np.arange(org[1], dtype=np.float64), indexing="ij")
    rmap = np.stack([xx + 0.3 * np.sin(yy / 7.0), yy - 20.0], -1).astype(np.float32)
    raw = synthetic_events(4243, fix + 5000, width=org[1], height=org[0])
    label = det_uniform("ab.loader.label", (H, W), 0.0, 19.0).numpy().astype(np.uint8)
    n_batches = 4
    samples = [(raw, label, f"s{i}") for i in range(B * n_batches)]
    loader = GpuDenseLoader(a, samples, B, n_batches, True, "semseg", sensor, seed=1, rectify_map=rmap, org_sensor=org)
    per = []
    for _ in range(3):                                    # the first pass warms; a pass is wall clock from the first pack to the last kernel
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in loader:
            pass
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / n_batches * 1e6)
    print(f"DSEC GpuDenseLoader batch, wall clock per batch over a pass of {n_batches} (pack + upload + rectify + chain + label): "
          f"{', '.join('%.0f' % v for v in per)} us (first pass warms)", flush=True)
    # the device half of the same batch: rectify + replay + label kernel on what the last upload left in the buffers
    from eventpretrain_amd.dataset.augmentation.view_augment import semseg_label_augment_batch
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import rectify_compact_batch

    def device_half():
        rectify_compact_batch(loader.ev, loader.d_off, loader.cap, loader.keep, sensor, loader.cev, loader.c_off, loader.status, rectify_map=loader.map,
                              workspace=loader._ws)
        loader.chain.run_next()
        semseg_label_augment_batch(loader._lab, loader.chain.crop_rows, sensor, out=loader.label)
    alternate({"DSEC loader batch, device half": (device_half, None)})


def main():
    from eventpretrain_amd import _lib
    _lib.require_device()
    alternate(shape_forms("DSEC", (440, 640), (480, 640), 200_000, True))
    alternate(shape_forms("MVSEC", (260, 346), (280, 360), 100_000, False))
    dsec_chain_and_loader()


if __name__ == "__main__":
    main()

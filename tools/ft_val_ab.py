#!/usr/bin/env python3
"""Time of an evaluation pass (ft_val) of the classification fine-tune: one measurement per process, so that two source trees --
this one and a checkout of the commit before the captured evaluation, whose ft_val is the eager loop with three read-backs per
batch -- or the two forms of this tree can be alternated by the caller.

    ft_val_ab.py [--tree DIR] [--size small|base] [--graph 0|1] [--iters 60] [--calls 3] [--warmup 1] [--tag NAME]

`--tree`: root of the source tree to import eventpretrain_amd from (default: the tree this file is in). `--graph 0` sets
args.graph_step = False (this tree's eager loop; the parent tree has nothing else). Times whole ft_val calls on a device-resident
synthetic loader (batch 64, 224 x 224, bf16, 101 classes), device-synchronised at the end of each call, after `--warmup` calls that
are not timed (they hold the capture), and prints one JSON line: {tag, size, graph, note, ms_per_batch: [per measured call], ...}.
The metrics kernel's own floor is one read of the logits (64 x 101 floats = 26 KB: a few nanoseconds at the HBM rate): it is
bound by launch latency, not by bandwidth."""
import argparse
import contextlib
import io
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--size", default="small", choices=["small", "base"])
    ap.add_argument("--graph", type=int, default=1, choices=[0, 1])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tag", default="")
    a_ = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a_.tree))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_val
    ops.set_compute_dtype(torch.bfloat16)
    a = make_args(phase="finetune_cls", model_size=a_.size, backbone_type="vit", num_classes=a_.classes, mask_ratio=0.0, device="cuda",
                  dataset_type="n-caltech101", clip_grad=None, smoothing=0.1, drop_path_rate=0.1, drop_rate=0.0)
    a.graph_step = bool(a_.graph)
    a.print_freq = 10 ** 9
    torch.manual_seed(0)
    fac = ft.finetune_cls_hub_model_small_patch16 if a_.size == "small" else ft.finetune_cls_hub_model_base_patch16
    m = fac(a).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(a_.batch, 5, 224, 224, device="cuda", generator=g) * 0.5
    y = torch.randint(0, a_.classes, (a_.batch,), device="cuda", generator=g)
    loader = [dict(events_voxel_grid=x, label=y, image_name=["i"] * a_.batch)] * a_.iters
    times = []
    for call in range(a_.warmup + a_.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            st = ft_val(a, m, loader, 0)
        torch.cuda.synchronize()
        if call >= a_.warmup:
            times.append(time.perf_counter() - t0)
    ex = getattr(m, "_evp_auto_eval", (None, None))[1]
    print(json.dumps(dict(tag=a_.tag, size=a_.size, graph=a_.graph, note=("eager loop" if ex is None else ex.note), stats=st,
                          ms_per_batch=[round(1e3 * t / a_.iters, 4) for t in times], call_s=[round(t, 3) for t in times])))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of a fine-tune epoch with gradient clipping (the reference's default recipe: --clip_grad 5, drop_path 0.1): one
measurement per process, so that two source trees -- this one and a copy of the commit before device-side clipping, which runs
the clipped recipe eagerly with a read-back per step -- or two settings can be alternated by the caller.

    ft_clip_ab.py [--tree DIR] [--size small|base] [--clip 5|none] [--skip] [--iters 60] [--epochs 3] [--warmup 1] [--tag NAME]

`--tree`: root of the source tree to import eventpretrain_amd from (default: the tree this file is in). Times
ft_train_one_epoch on a device-resident synthetic loader (batch 64, 224 x 224, bf16), device-synchronised per epoch, and prints
one JSON line: {tag, size, clip, note, ms_per_step: [per measured epoch], epoch_s: [...]}.
The clip's own floor is one read of the gradients: 4 B per parameter over the HBM rate (about 14 us for ViT-Small's 22 M
parameters, 55 us for ViT-Base's 86 M at 6.3 TB/s). `--skip` sets args.skip_nonfinite (skipping the step on non-finite gradients,
on the device): with --clip it is the clip's single pass, without it one read of the gradients of its own. The four arms of
profiles/ft_guard_ab.txt are: a copy of the commit before the guard (--tree), and this tree with --clip none, --clip none --skip and
--clip 5 --skip (and --clip 5 alone, the baseline of the last)."""
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
    ap.add_argument("--clip", default="5")
    ap.add_argument("--skip", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tag", default="")
    a_ = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a_.tree))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    clip = None if a_.clip.lower() == "none" else float(a_.clip)
    ops.set_compute_dtype(torch.bfloat16)
    a = make_args(phase="finetune_cls", model_size=a_.size, backbone_type="vit", num_classes=101, mask_ratio=0.0, device="cuda",
                  dataset_type="n-caltech101", clip_grad=clip, smoothing=0.1, drop_path_rate=0.1, drop_rate=0.0)
    a.epochs, a.warmup_epochs, a.lr, a.min_lr = 100, 5, 1e-3, 1e-6
    a.print_freq = a.log_freq = 10 ** 9
    if a_.skip:
        a.skip_nonfinite = True
    torch.manual_seed(0)
    fac = ft.finetune_cls_hub_model_small_patch16 if a_.size == "small" else ft.finetune_cls_hub_model_base_patch16
    m = fac(a).cuda()
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, 0.05, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(a_.batch, 5, 224, 224, device="cuda", generator=g) * 0.5
    y = torch.randint(0, 101, (a_.batch,), device="cuda", generator=g)
    loader = [dict(events_voxel_grid=x, label=y, image_name=["i"] * a_.batch)] * a_.iters
    scaler = NativeScalerWithGradNormCount()
    times = []
    for ep in range(a_.warmup + a_.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            st = ft_train_one_epoch(a, m, loader, opt, ep, scaler)
        torch.cuda.synchronize()
        if ep >= a_.warmup:
            times.append(time.perf_counter() - t0)
    ex = getattr(m, "_evp_auto_executor", (None, None))[1]
    print(json.dumps(dict(tag=a_.tag, size=a_.size, clip=clip, skip=a_.skip, skipped_steps=st.get("skipped_steps"), note=("eager loop" if ex is None else ex.note), loss=st["loss_cls"],
                          n_param=sum(p.numel() for p in m.parameters() if p.requires_grad),
                          ms_per_step=[round(1e3 * t / a_.iters, 4) for t in times], epoch_s=[round(t, 3) for t in times])))


if __name__ == "__main__":
    main()

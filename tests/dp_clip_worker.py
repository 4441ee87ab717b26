"""Worker of tests/test_gpu_grad_clip.py::test_two_rank_clipped_finetune_steps: one rank of a 2-rank data-parallel fine-tune run with
gradient clipping, tensors on the GPU, both ranks on the one card of the test box (gloo transport, as tests/dp_cuda_worker.py).
Three runs from the same start and data: eager with a clip that never engages (its norms pick the clip value), then eager and
captured with that value. Started by torch.distributed.run; rank 0 writes the result file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

LR, WD, SMOOTHING = 1e-3, 0.05, 0.1


def build():
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, make_args
    from eventpretrain_amd.utils import lr_decay as lrd
    ops.set_compute_dtype(torch.float32)
    a = make_args(phase="finetune_cls", model_size="small", backbone_type="vit", num_classes=10, mask_ratio=0.0, device="cuda",
                  dataset_type="n-caltech101", clip_grad=None, smoothing=SMOOTHING, drop_path_rate=0.0, drop_rate=0.0)
    m = ft.finetune_cls_hub_model_small_patch16(a)
    det_fill_module_(m)
    m = m.cuda().train()
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, WD, layer_decay=0.75), lr=LR, betas=(0.9, 0.999))
    return a, m, opt


def batch_of(rank, step):
    from eventpretrain_amd.testing import det_normalish
    x = det_normalish(f"dpclip.x.{rank}.{step}", (2, 5, 224, 224)) * 0.5
    y = torch.tensor([(3 * step + rank) % 10, (step + 7 * rank + 1) % 10])
    return x, y


def forward(m, x, y, noise=None):
    from eventpretrain_amd import ops
    return (ops.CrossEntropyFn.apply(m(x)[-2], y, SMOOTHING),)


def run(mode, clip, steps, rank, world):
    from eventpretrain_amd.engine import GraphedStep
    from eventpretrain_amd.parallel import BucketedGradReducer
    from helpers import checksums
    a, m, opt = build()
    red = BucketedGradReducer.for_module(m)
    x0, y0 = batch_of(rank, 0)
    ex = GraphedStep(m, opt, forward, [x0.cuda(), y0.cuda()], use_graph=(mode == "graph"), warmup=2, reducer=red, clip_grad=clip)
    losses, norms = [], []
    for s in range(steps):
        x, y = batch_of(rank, s)
        losses.append(float(ex.step(x.cuda(), y.cuda()).item()))
        norms.append([float(v) for v in ex.grad_norm.cpu()])
    torch.cuda.synchronize()
    sums = {k: float(checksums(p)[2]) for k, p in m.named_parameters()}
    mine = torch.tensor([sums[k] for k in sorted(sums)] + [v for n in norms for v in n], dtype=torch.float64)
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    res = dict(losses=losses, norms=norms, wsums=sums, scale={k: float(p.detach().abs().sum()) for k, p in m.named_parameters()},
               note=ex.note, parts=bool(ex.parts), ranks_equal=bool(torch.equal(both[0], both[1])), grad_scale=opt.grad_scale,
               max_grad_norm_after=opt.max_grad_norm)
    del ex, m, opt, red
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {"free": run("eager", 1e9, args.steps, rank, world)}
    srt = sorted(n[0] for n in res["free"]["norms"])
    pick = torch.tensor([0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2])], dtype=torch.float64)
    dist.broadcast(pick, src=0)
    res["clip"] = float(pick.item())
    for mode in ("eager", "graph"):
        res[mode] = run(mode, res["clip"], args.steps, rank, world)
    if rank == 0:
        json.dump(res, open(args.out, "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

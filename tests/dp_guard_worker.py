"""Worker of tests/test_gpu_grad_guard.py::test_two_rank_guarded_finetune_steps: one rank of a 2-rank data-parallel fine-tune run with
skip_nonfinite, tensors on the GPU, both ranks on the one card of the test box (gloo transport, as tests/dp_clip_worker.py). One
captured run; one +inf cell goes into RANK 1's batch of step POISON only -- the guard judges the all-reduced gradients, so both ranks
must skip that step. Started by torch.distributed.run; rank 0 writes the result file."""
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

POISON = 1


def batch_of(rank, step):
    import dp_clip_worker as w
    x, y = w.batch_of(rank, step)
    if rank == 1 and step == POISON:
        x = x.clone()
        x[1, 2, 100, 50] = float("inf")
    return x, y


def run(steps, rank, world):
    import dp_clip_worker as w
    from eventpretrain_amd.engine import GraphedStep
    from eventpretrain_amd.parallel import BucketedGradReducer
    from helpers import checksums
    a, m, opt = w.build()
    red = BucketedGradReducer.for_module(m)
    x0, y0 = batch_of(rank, 0)
    ex = GraphedStep(m, opt, w.forward, [x0.cuda(), y0.cuda()], use_graph=True, warmup=2, reducer=red, skip_nonfinite=True)
    params = dict(m.named_parameters())
    losses, guards, same, wsums = [], [], [], []
    for s in range(steps):
        x, y = batch_of(rank, s)
        before = {k: p.detach().clone() for k, p in params.items()}
        losses.append(float(ex.step(x.cuda(), y.cuda()).item()))
        torch.cuda.synchronize()
        guards.append([int(v) for v in ex.guard_state.cpu()])
        same.append(all(torch.equal(before[k], p.detach()) for k, p in params.items()))
        wsums.append([float(checksums(params[k])[2]) for k in sorted(params)])
    mine = torch.tensor([v for ws in wsums for v in ws] + [float(v) for g in guards for v in g], dtype=torch.float64)
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    return dict(losses=losses, guards=guards, unchanged=same, note=ex.note, parts=bool(ex.parts),
                ranks_equal=bool(torch.equal(both[0], both[1])), grad_scale=opt.grad_scale,
                skip_after=opt.skip_nonfinite, finite=bool(all(torch.isfinite(p).all() for p in params.values())),
                applied=int(max(float(st["step"]) for st in opt.state_dict()["state"].values())), skipped=opt.skipped_steps())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = run(args.steps, rank, world)
    every = [None] * world
    dist.all_gather_object(every, res)
    if rank == 0:
        json.dump(every, open(args.out, "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Classification fine-tuning loops with the reference's signatures and return dicts (reference
trainer/finetune_cls/ft_cls_trainer.py:15-108 `ft_train_one_epoch`, :110-192 `ft_val`): per-iteration LR schedule,
loss / accum_iter, optimizer step cadence with optional gradient clipping (the loop itself is trainer.epoch.run_epoch), top-1 / top-5
accuracy meters."""
import time

import torch

from ... import ops
from ...utils import misc
from ..epoch import auto_executor, run_epoch


def _forward(args, model, x):
    out = model(x)
    return out, out[-2]          # (..., pred, attn) for every backbone type


def _topk_accuracy(pred, label, topk=(1,)):
    """timm.utils.accuracy: percentage of samples whose label is among the k largest logits (a metric, not on the
    training path)."""
    maxk = min(max(topk), pred.shape[1])
    _, idx = pred.detach().float().topk(maxk, 1, True, True)
    hit = idx.eq(label.view(-1, 1))
    return [hit[:, :min(k, maxk)].any(1).float().sum() * (100.0 / pred.shape[0]) for k in topk]


def auto_ft_step_executor(args, model, optimizer, loss_scaler, batch_tensors):
    """The fine-tuning step (dense backbone -> token mean -> head -> cross entropy -> backward -> FusedAdamW) captured once as a HIP
    graph, as trainer.pretrain.pr_trainer.auto_step_executor does for the pre-training loops. The stochastic
    regularisers of the recipe replay correctly: the DropPath draws and the dropout keys come from torch's device generator, which
    advances under replay (ops.draw_block_drop / draw_drop_seed). `args.clip_grad` (the reference's default recipe: --clip_grad 5) is
    captured with the step: norm, coefficient and the scaled update stay on the device (evp_grad_clip_multi); a changed value
    re-captures. Returns None where trainer.epoch.auto_executor refuses: gradient accumulation, backward off, an optimizer that is
    not FusedAdamW, a CPU device, or `args.graph_step = False`."""
    x, y = batch_tensors
    clip = getattr(args, "clip_grad", None)
    clip = None if clip is None else float(clip)

    def build():
        from ...engine import GraphedStep
        smoothing = float(getattr(args, "smoothing", 0) or 0)
        fwd = lambda m, x_, y_, noise: (ops.CrossEntropyFn.apply(m(x_)[-2], y_, smoothing),)
        return GraphedStep(model, optimizer, fwd, [x.clone(), y.clone()], reducer=getattr(loss_scaler, "reducer", None), clip_grad=clip)
    return auto_executor(args, model, optimizer, "loss_cls", build, extra=(clip,))


def ft_train_one_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer=None, evrepsl_model=None):
    """One fine-tuning epoch (reference ft_cls_trainer.py:15-108), run by trainer.epoch.run_epoch. On the GPU the steps run as HIP-graph
    replays (auto_ft_step_executor), the losses stay on the device between log points and batch i + 1 is uploaded while step i runs;
    `args.graph_step = False` or `args.sync_every_step = True` give the eager / per-step-synchronised loop."""
    if evrepsl_model is not None or getattr(args, "use_evrepsl", False):
        raise NotImplementedError("EvRepSL preprocessing is out of scope (SURVEY.md 2)")

    def eager_step(tensors, names):
        x, label = tensors
        # nn.CrossEntropyLoss, or timm's LabelSmoothingCrossEntropy when args.smoothing > 0 (reference :63-66)
        return (ops.CrossEntropyFn.apply(_forward(args, model, x)[1], label, float(getattr(args, "smoothing", 0) or 0)),), None
    build = None if getattr(args, "sync_every_step", False) else (lambda t: auto_ft_step_executor(args, model, optimizer, loss_scaler, t))
    return run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, ("loss_cls",), eager_step,
                     build_executor=build, clip_grad=getattr(args, "clip_grad", None), meter_divided=True)


@torch.no_grad()
def ft_val(args, model, data_loader, epoch, dataset_name="origin", evrepsl_model=None):
    if evrepsl_model is not None or getattr(args, "use_evrepsl", False):
        raise NotImplementedError("EvRepSL preprocessing is out of scope (SURVEY.md 2)")
    model.eval()
    logger = misc.MetricLogger(delimiter="  ")
    infer_time = 0.0
    for events_voxel_grid, label, image_name in logger.log_every(args, data_loader, args.print_freq, "Test:"):
        events_voxel_grid = events_voxel_grid.to(args.device, non_blocking=True)
        label = label.to(args.device, non_blocking=True)
        t0 = time.time()
        _, pred = _forward(args, model, events_voxel_grid)
        infer_time += time.time() - t0
        loss_cls = ops.CrossEntropyFn.apply(pred, label)
        logger.update(loss_cls=loss_cls.item())
        if getattr(args, "dataset_type", "") != "n-cars":
            acc1, acc5 = _topk_accuracy(pred, label, topk=(1, 5))
            logger.update(acc1=acc1.item())
            logger.update(acc5=acc5.item())
        else:
            (acc1,) = _topk_accuracy(pred, label, topk=(1,))
            logger.update(acc1=acc1.item())
    logger.synchronize_between_processes()
    if "acc5" in logger.meters:
        print("* Acc@1 {:.3f} Acc@5 {:.3f} loss_cls {:.3f}".format(logger.acc1.global_avg, logger.acc5.global_avg, logger.loss_cls.global_avg))
    else:
        print("* Acc@1 {:.3f} loss_cls {:.3f}".format(logger.acc1.global_avg, logger.loss_cls.global_avg))
    print("average inference time (ms): %.2f" % (infer_time / max(len(data_loader), 1) * 1.e3))
    return {k: m.global_avg for k, m in logger.meters.items()}

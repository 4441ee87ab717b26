"""Semantic-segmentation fine-tuning loops with the reference's signatures and return dicts (reference
trainer/finetune_semseg/ft_semseg_trainer.py:14-177 `ft_semseg_train_one_epoch`, :180-271 `ft_semseg_val`). The loop itself is
trainer.epoch.run_epoch / val_loop_deferred. What differs from the reference: its two `resize` calls in front of the loss are gone --
the heads' low-resolution predictions go straight into SemsegLoss / ops.semseg_metrics, which interpolate per pixel in registers
 -- and the steps run as HIP-graph replays. A batch is (events_voxel_grid, semseg_label, seq_name)."""
import time

import torch

from ... import ops
from ...utils import misc
from ..epoch import DevicePrefetcher, auto_executor, run_epoch, val_loop_deferred
from ..finetune_cls.ft_cls_trainer import EVAL_TABLE_SLOTS, _use_captured_eval
from .semseg_loss import SemsegLoss, prediction_map
from .semseg_metric import semseg_compute_confusion, semseg_confusion_to_macc, semseg_confusion_to_miou


def _refuse_evrepsl(args, evrepsl_model):
    if evrepsl_model is not None or getattr(args, "use_evrepsl", False):
        raise NotImplementedError("EvRepSL preprocessing is out of scope (SURVEY.md 2)")


def _loss_total(args, criterion, model, x, label):
    """decode_loss_weight * (ce + dice of the decode head) + aux_loss_weight * (ce + dice of the auxiliary head) (reference :77-114)."""
    out = model(x)
    decode_ce, decode_dice = criterion(out[-2], label)
    aux_ce, aux_dice = criterion(out[-1], label)
    return args.decode_loss_weight * (decode_ce + decode_dice) + args.aux_loss_weight * (aux_ce + aux_dice)


def auto_semseg_step_executor(args, model, optimizer, loss_scaler, batch_tensors, criterion):
    """The segmentation step (backbone -> both heads -> SemsegLoss on each -> backward -> FusedAdamW) captured once as a HIP graph, as
    finetune_cls.ft_cls_trainer.auto_ft_step_executor does for classification; `args.clip_grad`, `args.skip_nonfinite` and the two loss
    weights are captured with the step and are part of the key. None where trainer.epoch.auto_executor refuses."""
    x, y = batch_tensors
    clip = getattr(args, "clip_grad", None)
    clip = None if clip is None else float(clip)
    skip = bool(getattr(args, "skip_nonfinite", False))

    def build():
        from ...engine import GraphedStep
        fwd = lambda m, x_, y_, noise: (_loss_total(args, criterion, m, x_, y_),)
        return GraphedStep(model, optimizer, fwd, [x.clone(), y.clone()], reducer=getattr(loss_scaler, "reducer", None), clip_grad=clip,
                           skip_nonfinite=skip)
    extra = (clip, skip, float(args.decode_loss_weight), float(args.aux_loss_weight), args.num_classes, args.ignore_label)
    return auto_executor(args, model, optimizer, "loss_total", build, extra=extra)


def ft_semseg_train_one_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer=None, evrepsl_model=None):
    """One fine-tuning epoch (reference ft_semseg_trainer.py:14-177) -> {lr, loss_total}. On the GPU the steps run as HIP-graph replays
    (auto_semseg_step_executor) and the losses stay on the device between log points; `args.graph_step = False` or
    `args.sync_every_step = True` give the eager / per-step-synchronised loop. As in the reference the meter receives the loss before
    it is divided by accum_iter. Labels outside [0, num_classes) that are not args.ignore_label raise at the end of the epoch (the
    kernels count them on the device and leave them out of every sum)."""
    _refuse_evrepsl(args, evrepsl_model)
    criterion = SemsegLoss(args, num_classes=args.num_classes, ignore_index=args.ignore_label)

    def eager_step(tensors, names):
        x, label = tensors
        return (_loss_total(args, criterion, model, x, label),), None
    build = None if getattr(args, "sync_every_step", False) else (lambda t: auto_semseg_step_executor(args, model, optimizer, loss_scaler, t, criterion))
    stats = run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, ("loss_total",), eager_step,
                      build_executor=build, clip_grad=getattr(args, "clip_grad", None), meter_divided=False)
    if str(args.device).startswith("cuda"):
        ops.semseg_check_labels(args.device)
    return stats


def auto_semseg_eval_executor(args, model, batch_tensors):
    """The captured evaluation forward (backbone -> decode head -> ops.semseg_metrics into a device table), kept on the model in
    `model._evp_auto_eval` as (key, executor) under the rules of finetune_cls.ft_cls_trainer.auto_eval_executor."""
    from ...engine import GraphedEval, MetricsTable
    slots = int(getattr(args, "eval_table_slots", None) or EVAL_TABLE_SLOTS)
    key = ("semseg", str(ops.get_compute_dtype()), slots, args.num_classes, args.ignore_label,
           tuple((tuple(t.shape), str(t.dtype)) for t in batch_tensors))
    cached = getattr(model, "_evp_auto_eval", None)
    if cached is not None and cached[0] == key and cached[1].current(model):
        cached[1].table.rewind()
        return cached[1]
    table = MetricsTable(batch_tensors[0].device, slots)

    def fwd(m, x_, y_):
        pm, B, h, w = prediction_map(m(x_)[-2])
        ops.semseg_metrics(pm, B, h, w, y_, args.ignore_label, table.rows, table.cursor)
    model._evp_auto_eval = (key, GraphedEval(model, fwd, [t.clone() for t in batch_tensors], table=table))
    return model._evp_auto_eval[1]


def _val_loop_eager(args, model, data_loader, logger, vis_hook):
    """The reference's loop as it stands, batch by batch with its read-backs: forward, confusion -> mIoU / mAcc, SemsegLoss on the
    decode prediction. (The reference also resizes an `aux_predict` here, from the DECODE prediction, and uses it for nothing but
    the visualiser: it is not computed.)"""
    criterion = SemsegLoss(args, num_classes=args.num_classes, ignore_index=args.ignore_label)
    infer_time = 0.0
    for events_voxel_grid, semseg_label, seq_name in logger.log_every(args, data_loader, args.print_freq, "Test:"):
        events_voxel_grid = events_voxel_grid.to(args.device, non_blocking=True)
        semseg_label = semseg_label.to(args.device, non_blocking=True)
        t0 = time.time()
        out = model(events_voxel_grid)
        infer_time += time.time() - t0
        decode_predict = out[-2]
        confusion = semseg_compute_confusion(args, decode_predict, semseg_label)
        ce, dice = criterion(decode_predict, semseg_label)
        if vis_hook is not None:
            vis_hook(args, events_voxel_grid, semseg_label, decode_predict, seq_name)
        logger.update(loss_total=(ce + dice).item())
        logger.update(miou=semseg_confusion_to_miou(confusion).item())
        logger.update(macc=semseg_confusion_to_macc(confusion).item())
    return infer_time


@torch.no_grad()
def ft_semseg_val(args, model, data_loader, epoch, evrepsl_model=None, vis_hook=None):
    """One evaluation pass (reference ft_semseg_trainer.py:180-271) -> {loss_total, miou, macc}, each the mean over batches of the
    per-batch value (loss_total = ce + dice of the decode head; mIoU / mAcc of the batch's own confusion table). On the GPU the forward
    and its metrics run as HIP-graph replays and the per-batch values stay in a device table between progress lines; `args.graph_step
    = False`, `args.sync_every_step = True`, per-step visualisation or a `vis_hook` give the eager loop."""
    _refuse_evrepsl(args, evrepsl_model)
    model.eval()
    logger = misc.MetricLogger(delimiter="  ")
    if vis_hook is None and _use_captured_eval(args, model):
        loader = data_loader
        if getattr(args, "prefetch_to_device", True) and not getattr(data_loader, "yields_device_batches", False):
            loader = DevicePrefetcher(data_loader, args.device)
        infer_time = val_loop_deferred(args, loader, logger, lambda t: auto_semseg_eval_executor(args, model, t), ("loss_total", "miou", "macc"))
    else:
        infer_time = _val_loop_eager(args, model, data_loader, logger, vis_hook)
    if str(args.device).startswith("cuda"):
        ops.semseg_check_labels(args.device)
    logger.synchronize_between_processes()
    print("* miou {:.3f} macc {:.3f} loss_total {:.3f}".format(logger.miou.global_avg, logger.macc.global_avg, logger.loss_total.global_avg))
    print("average inference time (ms): %.2f" % (infer_time / max(len(data_loader), 1) * 1.e3))
    return {k: m.global_avg for k, m in logger.meters.items()}

"""Classification fine-tuning loops with the reference's signatures and return dicts (reference
trainer/finetune_cls/ft_cls_trainer.py:15-108 `ft_train_one_epoch`, :110-192 `ft_val`): per-iteration LR schedule,
loss / accum_iter, optimizer step cadence with optional gradient clipping (the loop itself is trainer.epoch.run_epoch), top-1 / top-5
accuracy meters."""
import time

import torch

from ... import ops
from ...utils import misc
from ..epoch import DevicePrefetcher, auto_executor, run_epoch, val_loop_deferred


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
    re-captures. `args.skip_nonfinite` is captured likewise (evp_grad_guard_multi in that place). Returns None where trainer.epoch.auto_executor refuses: gradient accumulation, backward off, an optimizer that is
    not FusedAdamW, a CPU device, or `args.graph_step = False`."""
    x, y = batch_tensors
    clip = getattr(args, "clip_grad", None)
    clip = None if clip is None else float(clip)
    skip = bool(getattr(args, "skip_nonfinite", False))

    def build():
        from ...engine import GraphedStep
        smoothing = float(getattr(args, "smoothing", 0) or 0)
        fwd = lambda m, x_, y_, noise: (ops.CrossEntropyFn.apply(m(x_)[-2], y_, smoothing),)
        return GraphedStep(model, optimizer, fwd, [x.clone(), y.clone()], reducer=getattr(loss_scaler, "reducer", None), clip_grad=clip,
                           skip_nonfinite=skip)
    return auto_executor(args, model, optimizer, "loss_cls", build, extra=(clip, skip))


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


EVAL_TABLE_SLOTS = 4096      # slots of the device metrics table of a captured evaluation (args.eval_table_slots overrides)


def auto_eval_executor(args, model, batch_tensors):
    """The captured evaluation forward (backbone -> token mean -> head -> ops.cls_metrics into a device table) ft_val builds on its
    first batch and keeps on the model, in `model._evp_auto_eval` as (key, executor), as trainer.epoch.auto_executor keeps the
    training step: one engine.GraphedEval per (compute dtype, table slots, shapes and dtypes of the batch), re-used by every later
    ft_val on the model -- the ten validation sets of an N-ImageNet epoch replay one capture -- as long as executor.current(model)
    holds (asked here, once per ft_val call); weights that moved to other addresses build a new one."""
    from ...engine import GraphedEval, MetricsTable
    slots = int(getattr(args, "eval_table_slots", None) or EVAL_TABLE_SLOTS)
    key = (str(ops.get_compute_dtype()), slots, tuple((tuple(t.shape), str(t.dtype)) for t in batch_tensors))
    cached = getattr(model, "_evp_auto_eval", None)
    if cached is not None and cached[0] == key and cached[1].current(model):
        cached[1].table.rewind()
        return cached[1]
    table = MetricsTable(batch_tensors[0].device, slots)
    fwd = lambda m, x_, y_: ops.cls_metrics(m(x_)[-2], y_, table.rows, table.cursor)
    model._evp_auto_eval = (key, GraphedEval(model, fwd, [t.clone() for t in batch_tensors], table=table))
    return model._evp_auto_eval[1]


def _use_captured_eval(args, model):
    """ft_val's captured form stands in for its eager loop on a CUDA device unless the caller opted out (`args.graph_step = False`,
    `args.sync_every_step = True`), replaced `forward` on the instance, or asked for per-step visualisation."""
    if not str(args.device).startswith("cuda") or not getattr(args, "graph_step", True) or getattr(args, "sync_every_step", False):
        return False
    return "forward" not in vars(model) and not (getattr(args, "test_experiment", False) and getattr(args, "visualize", False))


def _val_loop_deferred(args, data_loader, logger, executor_for, with_acc5):
    """trainer.epoch.val_loop_deferred with this trainer's meters on the table's columns {loss, acc1, acc5}."""
    return val_loop_deferred(args, data_loader, logger, executor_for, ("loss_cls", "acc1", "acc5" if with_acc5 else None))


def _val_loop_eager(args, model, data_loader, logger, with_acc5):
    """The reference's loop as it stands: eager forward, cross entropy and top-k on the device, three read-backs per batch."""
    infer_time = 0.0
    for events_voxel_grid, label, image_name in logger.log_every(args, data_loader, args.print_freq, "Test:"):
        events_voxel_grid = events_voxel_grid.to(args.device, non_blocking=True)
        label = label.to(args.device, non_blocking=True)
        t0 = time.time()
        _, pred = _forward(args, model, events_voxel_grid)
        infer_time += time.time() - t0
        loss_cls = ops.CrossEntropyFn.apply(pred, label)
        logger.update(loss_cls=loss_cls.item())
        if with_acc5:
            acc1, acc5 = _topk_accuracy(pred, label, topk=(1, 5))
            logger.update(acc1=acc1.item())
            logger.update(acc5=acc5.item())
        else:
            (acc1,) = _topk_accuracy(pred, label, topk=(1,))
            logger.update(acc1=acc1.item())
    return infer_time


@torch.no_grad()
def ft_val(args, model, data_loader, epoch, dataset_name="origin", evrepsl_model=None):
    """One evaluation pass (reference ft_cls_trainer.py:110-192) -> {loss_cls, acc1, acc5} (no acc5 for n-cars), each the mean over
    batches of the per-batch value. On the GPU the forward and its metrics run as HIP-graph replays (auto_eval_executor), the
    per-batch values stay in a device table between progress lines (_val_loop_deferred) and batch i + 1 is uploaded while batch i
    runs; `args.graph_step = False` or `args.sync_every_step = True` give the eager loop with its three read-backs per batch, which
    is also what a CPU device runs. The reported "average inference time" is host time around the forward call in both forms: the
    reference does not synchronise there either, so it times the enqueue (in the captured form, of the replay with its metrics)."""
    if evrepsl_model is not None or getattr(args, "use_evrepsl", False):
        raise NotImplementedError("EvRepSL preprocessing is out of scope (SURVEY.md 2)")
    model.eval()
    logger = misc.MetricLogger(delimiter="  ")
    with_acc5 = getattr(args, "dataset_type", "") != "n-cars"
    if _use_captured_eval(args, model):
        loader = data_loader
        if getattr(args, "prefetch_to_device", True) and not getattr(data_loader, "yields_device_batches", False):
            loader = DevicePrefetcher(data_loader, args.device)
        infer_time = _val_loop_deferred(args, loader, logger, lambda t: auto_eval_executor(args, model, t), with_acc5)
    else:
        infer_time = _val_loop_eager(args, model, data_loader, logger, with_acc5)
    logger.synchronize_between_processes()
    if "acc5" in logger.meters:
        print("* Acc@1 {:.3f} Acc@5 {:.3f} loss_cls {:.3f}".format(logger.acc1.global_avg, logger.acc5.global_avg, logger.loss_cls.global_avg))
    else:
        print("* Acc@1 {:.3f} loss_cls {:.3f}".format(logger.acc1.global_avg, logger.loss_cls.global_avg))
    print("average inference time (ms): %.2f" % (infer_time / max(len(data_loader), 1) * 1.e3))
    return {k: m.global_avg for k, m in logger.meters.items()}

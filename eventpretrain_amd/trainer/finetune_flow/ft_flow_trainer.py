"""Optical-flow fine-tuning loops with the reference's signatures and return dicts (reference
trainer/finetune_flow/ft_flow_trainer.py:14-159 `ft_flow_train_one_epoch`, :162-271 `ft_flow_val`). The loop itself is
trainer.epoch.run_epoch / val_loop_deferred. What differs from the reference: its `resize_flow` calls in front of the loss are gone --
the heads' low-resolution predictions go straight into FlowLoss / ops.flow_metrics, which interpolate and scale per pixel in
registers -- and the steps run as HIP-graph replays. A batch is (events_voxel_grid, events_voxel_grid_org,
flow_label, flow_label_valid, seq_name); events_voxel_grid_org feeds the validation's events mask and nothing else."""
import time

import torch

from ...utils import misc
from ..epoch import DevicePrefetcher, auto_executor, run_epoch, val_loop_deferred
from ..finetune_cls.ft_cls_trainer import EVAL_TABLE_SLOTS, _use_captured_eval
from ..finetune_semseg.ft_semseg_trainer import _refuse_evrepsl
from ..finetune_semseg.semseg_loss import prediction_map
from .flow_loss import FlowLoss
from .flow_metric import flow_compute_metrics

TRAIN_KEYS = tuple(k for k in misc.FLOW_BATCH_KEYS if k != "events_voxel_grid_org")
VAL_METERS = ("decode_l1_loss", "decode_aee_sparse", "decode_outlier_sparse")


class _TrainBatches:
    """The loader's dict batches without events_voxel_grid_org: the training loop of the reference builds its sparse mask from it for
    the visualiser alone (:56-57), so it is neither copied to the device nor a static input of the captured step."""

    def __init__(self, loader):
        self.loader = loader
        self.yields_device_batches = getattr(loader, "yields_device_batches", False)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield {k: batch[k] for k in TRAIN_KEYS}


def _loss_total(args, criterion, model, x, label, valid):
    """decode_loss_weight * L1(decode head) + aux_loss_weight * L1(auxiliary head) (reference :48-53, :88)."""
    out = model(x)
    return args.decode_loss_weight * criterion(out[-2], label, valid) + args.aux_loss_weight * criterion(out[-1], label, valid)


def auto_flow_step_executor(args, model, optimizer, loss_scaler, batch_tensors, criterion):
    """The flow step (backbone -> both heads -> FlowLoss on each -> backward -> FusedAdamW) captured once as a HIP graph, as
    finetune_semseg.ft_semseg_trainer.auto_semseg_step_executor does for segmentation; `args.clip_grad`, `args.skip_nonfinite`, the two
    loss weights and `args.max_flow` are captured with the step and are part of the key. None where trainer.epoch.auto_executor refuses."""
    x, y, v = batch_tensors
    clip = getattr(args, "clip_grad", None)
    clip = None if clip is None else float(clip)
    skip = bool(getattr(args, "skip_nonfinite", False))

    def build():
        from ...engine import GraphedStep
        fwd = lambda m, x_, y_, v_, noise: (_loss_total(args, criterion, m, x_, y_, v_),)
        return GraphedStep(model, optimizer, fwd, [x.clone(), y.clone(), v.clone()], reducer=getattr(loss_scaler, "reducer", None),
                           clip_grad=clip, skip_nonfinite=skip)
    extra = (clip, skip, float(args.decode_loss_weight), float(args.aux_loss_weight), float(args.max_flow))
    return auto_executor(args, model, optimizer, "loss_total", build, extra=extra)


def ft_flow_train_one_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer=None, evrepsl_model=None):
    """One fine-tuning epoch (reference ft_flow_trainer.py:14-159) -> {lr, loss_total}. On the GPU the steps run as HIP-graph replays
    (auto_flow_step_executor) and the losses stay on the device between log points; `args.graph_step = False` or
    `args.sync_every_step = True` give the eager / per-step-synchronised loop. As in the reference the meter receives the loss before
    it is divided by accum_iter. A batch without a valid pixel has a NaN loss and a zero gradient (the reference's, too)."""
    _refuse_evrepsl(args, evrepsl_model)
    criterion = FlowLoss(args)

    def eager_step(tensors, names):
        x, label, valid = tensors
        return (_loss_total(args, criterion, model, x, label, valid),), None
    build = None if getattr(args, "sync_every_step", False) else (lambda t: auto_flow_step_executor(args, model, optimizer, loss_scaler, t, criterion))
    return run_epoch(args, model, _TrainBatches(data_loader), optimizer, epoch, loss_scaler, log_writer, ("loss_total",), eager_step,
                     build_executor=build, clip_grad=getattr(args, "clip_grad", None), meter_divided=False, batch_keys=TRAIN_KEYS)


def auto_flow_eval_executor(args, model, batch_tensors):
    """The captured evaluation forward (backbone -> decode head -> ops.flow_metrics into a device table), kept on the model in
    `model._evp_auto_eval` as (key, executor) under the rules of finetune_cls.ft_cls_trainer.auto_eval_executor."""
    from ... import ops
    from ...engine import GraphedEval, MetricsTable
    slots = int(getattr(args, "eval_table_slots", None) or EVAL_TABLE_SLOTS)
    key = ("flow", str(ops.get_compute_dtype()), slots, float(args.max_flow), tuple((tuple(t.shape), str(t.dtype)) for t in batch_tensors))
    cached = getattr(model, "_evp_auto_eval", None)
    if cached is not None and cached[0] == key and cached[1].current(model):
        cached[1].table.rewind()
        return cached[1]
    table = MetricsTable(batch_tensors[0].device, slots)

    def fwd(m, x_, org_, y_, v_):
        pm, B, h, w = prediction_map(m(x_)[-2])
        ops.flow_metrics(pm, B, h, w, y_, v_, args.max_flow, org_, table.rows, table.cursor)
    model._evp_auto_eval = (key, GraphedEval(model, fwd, [t.clone() for t in batch_tensors], table=table))
    return model._evp_auto_eval[1]


def _val_loop_eager(args, model, data_loader, logger, vis_hook):
    """The reference's loop as it stands, batch by batch with its read-backs: forward, then the three values of the decode prediction.
    (The reference also makes an `aux_predict` here, from the DECODE prediction, and uses it for nothing but the visualiser: it is
    not computed.)"""
    infer_time = 0.0
    for events_voxel_grid, events_voxel_grid_org, flow_label, flow_label_valid, seq_name in logger.log_every(args, data_loader, args.print_freq, "Test:"):
        events_voxel_grid = events_voxel_grid.to(args.device, non_blocking=True)
        events_voxel_grid_org = events_voxel_grid_org.to(args.device, non_blocking=True)
        flow_label = flow_label.to(args.device, non_blocking=True)
        flow_label_valid = flow_label_valid.to(args.device, non_blocking=True)
        t0 = time.time()
        out = model(events_voxel_grid)
        infer_time += time.time() - t0
        decode_predict = out[-2]
        l1, aee, outlier = flow_compute_metrics(args, decode_predict, flow_label, flow_label_valid, events_voxel_grid_org)
        if vis_hook is not None:
            vis_hook(args, events_voxel_grid, events_voxel_grid_org, flow_label, flow_label_valid, decode_predict, seq_name)
        logger.update(decode_l1_loss=l1.item())
        logger.update(decode_aee_sparse=aee.item())
        logger.update(decode_outlier_sparse=outlier.item())
    return infer_time


@torch.no_grad()
def ft_flow_val(args, model, data_loader, epoch, dataset_name, evrepsl_model=None, vis_hook=None):
    """One evaluation pass (reference ft_flow_trainer.py:162-271) -> {decode_l1_loss, decode_aee_sparse, decode_outlier_sparse}, each
    the mean over batches of the per-batch value of the decode head. On the GPU the forward and its metrics run as HIP-graph replays
    and the per-batch values stay in a device table between progress lines; `args.graph_step = False`, `args.sync_every_step = True`,
    per-step visualisation or a `vis_hook` give the eager loop. `dataset_name` goes to the reference's visualiser alone."""
    _refuse_evrepsl(args, evrepsl_model)
    model.eval()
    logger = misc.MetricLogger(delimiter="  ")
    if vis_hook is None and _use_captured_eval(args, model):
        loader = data_loader
        if getattr(args, "prefetch_to_device", True) and not getattr(data_loader, "yields_device_batches", False):
            loader = DevicePrefetcher(data_loader, args.device)
        infer_time = val_loop_deferred(args, loader, logger, lambda t: auto_flow_eval_executor(args, model, t), VAL_METERS)
    else:
        infer_time = _val_loop_eager(args, model, data_loader, logger, vis_hook)
    logger.synchronize_between_processes()
    print("* decode_aee_sparse {:.3f} decode_outlier_sparse {:.3f} decode_l1_loss {:.3f}".format(
        logger.decode_aee_sparse.global_avg, logger.decode_outlier_sparse.global_avg, logger.decode_l1_loss.global_avg))
    print("average inference time (ms): %.2f" % (infer_time / max(len(data_loader), 1) * 1.e3))
    return {k: m.global_avg for k, m in logger.meters.items()}

"""The one-epoch loop of the pre-training and fine-tuning trainers, written once (reference trainer/pretrain/pr_trainer.py:9-89 and
its siblings, trainer/finetune_cls/ft_cls_trainer.py:15-108): set-up, per-iteration LR schedule, the step -- one HIP-graph replay
through an engine.GraphedStep, or the eager forward + loss / accum_iter + scaler call -- the three ways of recording a loss, the
TensorBoard rows, the visualisation hook, the close. trainer.pretrain.pr_trainer and trainer.finetune_cls.ft_cls_trainer pass in
what differs between the phases: the loss names, the eager step, the executor builder. val_loop_deferred is the evaluation loop of the
fine-tuning trainers over a device metrics table."""
import time

import torch

from ..utils import misc
from ..utils.lr_sched import adjust_learning_rate


class DevicePrefetcher:
    """Batch i + 1's host -> device copies on a side stream while step i runs (the loop used to issue them in front of the replay on
    the step's own stream: 64 MB of voxel grids per ViT-Base batch = 1.3 ms of a 10.7 ms step even from pinned memory). Wraps any
    loader of dict batches; tensors already on the device pass through. The consumer's stream waits on the copy's event."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(self.device)

    def __len__(self):
        return len(self.loader)

    def _move(self, batch):
        if not isinstance(batch, dict):          # (the reference's loaders yield dicts; anything else passes through untouched)
            return batch, None
        moved, ev = {}, None
        with torch.cuda.stream(self.stream):
            for k, v in batch.items():
                if torch.is_tensor(v) and v.device != self.device:
                    moved[k] = v.to(self.device, non_blocking=True)
                else:
                    moved[k] = v
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return moved, ev

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._move(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ev = nxt
            try:
                nxt = self._move(next(it))      # queued behind the previous copy, ahead of the step the consumer is about to run
            except StopIteration:
                nxt = None
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
                for v in cur.values():
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(torch.cuda.current_stream(self.device))
            yield cur


class DeferredLosses:
    """Per-step losses kept ON THE DEVICE. The reference reads the loss back every step (`loss.item()`,
    pr_trainer.py:46,64) and all-reduces it for the log (`utils/misc.py:406-414`): with a replayed step that is three host syncs
    per iteration and the host can never queue step N+1 while step N runs. Here every step's loss is copied into a device array
    (one tiny copy behind the replay); the meters receive the values -- one update per step, in order, so `global_avg`, the
    smoothed window and the returned dict are what per-step updates give -- when something is about to be printed or logged and
    at the end of the epoch. `args.sync_every_step = True` restores the reference's per-step read-back."""

    def __init__(self, n_iter, device):
        self.buf = torch.zeros(max(int(n_iter), 1), dtype=torch.float32, device=device)
        self.done = 0          # steps already handed to the meters
        self.n = 0

    def push(self, loss):
        if self.n >= self.buf.numel():        # a loader that yields more batches than len() promised
            self.buf = torch.cat([self.buf, torch.zeros_like(self.buf)])
        self.buf[self.n].copy_(loss.detach().reshape(()), non_blocking=True)
        self.n += 1

    def flush(self, logger, name):
        """-> the newest loss value (a host float) or None when nothing was pending; ONE device read-back."""
        if self.done == self.n:
            return None
        vals = self.buf[self.done:self.n].tolist()
        self.done = self.n
        for v in vals:
            logger.update(**{name: v})
        return vals[-1]


def val_loop_deferred(args, data_loader, logger, executor_for, meter_names):
    """The evaluation loop with no host round-trip per batch: every batch is one executor.run (a HIP-graph replay; eager_with for a
    batch of another shape) that leaves its three values in the executor's device table (engine.MetricsTable); the table is read back
    and rewound when a progress line is due, when it is full and at the end of the loader, and every slot becomes one update per
    meter, in batch order -- global_avg, the smoothed window and the returned dict are what per-batch updates give, the reference's
    equal weight of a short last batch included. `meter_names`: the meters of the table's three columns, None for a column the
    caller does not meter. A batch is the executor's tensors in order -- (input, label), or (input, events, label, valid) for flow --
    then the names. -> host seconds spent queueing the forwards."""
    n_iter = len(data_loader)
    executor, pending, infer_time = None, 0, 0.0

    def flush():
        for row in executor.table.read(pending):
            for name, v in zip(meter_names, row):
                if name is not None:
                    logger.update(**{name: v})
        return 0

    for it, batch in enumerate(logger.log_every(args, data_loader, args.print_freq, "Test:")):
        tensors = [t.to(args.device, non_blocking=True) for t in batch[:-1]]
        if executor is None:
            executor = executor_for(tensors)
        t0 = time.time()
        if all(tuple(t.shape) == tuple(s.shape) for t, s in zip(tensors, executor.inputs)):
            executor.run(*tensors)
        else:
            executor.eager_with(*tensors)
        infer_time += time.time() - t0
        pending += 1
        if (it + 1) % args.print_freq == 0 or pending >= executor.table.capacity or it + 1 == n_iter:
            pending = flush()
    if pending:              # (a loader that yields more batches than len() promised)
        flush()
    return infer_time


def auto_executor(args, model, optimizer, loss_name, build, extra=()):
    """The step executor an epoch loop builds by itself on its first batch and keeps on the model, in `model._evp_auto_executor`
    as (key, executor): `build()` makes it, once per (optimizer, loss name, compute dtype, *extra) -- `extra` is what else is
    captured with the step (fine-tuning: clip_grad; skip_nonfinite when on); a change of any of these builds anew. The batch shape is not in the key:
    an executor captured at another shape is handed back and the loop steps it eagerly (eager_step_with). None where a captured
    step cannot stand in for the eager loop: `args.graph_step = False` (the opt-out), gradient accumulation, backward off, a
    device that is not CUDA, an optimizer that is not FusedAdamW, a forward replaced on the instance."""
    from .. import ops
    from ..optim import FusedAdamW
    if not getattr(args, "graph_step", True) or args.accum_iter != 1 or not args.backward:
        return None
    if not str(args.device).startswith("cuda") or not isinstance(optimizer, FusedAdamW) or "forward" in vars(model):
        return None
    key = (id(optimizer), loss_name, str(ops.get_compute_dtype()), *extra)
    cached = getattr(model, "_evp_auto_executor", None)
    if cached is None or cached[0] != key:
        cached = model._evp_auto_executor = (key, build())
    return cached[1]


def _executor_step(args, executor, tensors):
    """HIP-graph replay of forward + backward + optimizer step (eventpretrain_amd/engine.py); the lr the loop has just set
    reaches the graph through the optimizer's staged scalars."""
    if args.accum_iter != 1 or not args.backward:
        raise ValueError("step_executor runs one optimizer step per batch (accum_iter=1, backward=True)")
    if all(tuple(t.shape) == tuple(s.shape) for t, s in zip(tensors, executor.inputs)):
        return executor.step(*tensors)
    return executor.eager_step_with(*tensors)      # the short last batch of an epoch: one eager step that leaves the graph usable


def run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, loss_names, eager_step, build_executor=None,
              step_executor=None, clip_grad=None, meter_divided=False, vis_hook=None, vis_last_batch=True, batch_keys=None):
    """One training epoch -> {meter: global_avg}. A batch is the tuple misc.MetricLogger.log_every yields: tensors, then the sample names.

    batch_keys      the keys of the loader's dict batches that make up that tuple, where they are not the phase's own (flow: the
                    step takes no events_voxel_grid_org).
    loss_names      the meters / TensorBoard tags, in the order the eager step returns the losses.
    eager_step      (tensors, names) -> (losses, vis): the forward(s) of one batch; `vis` is what vis_hook takes between args and epoch.
                    The loop sums the losses, divides by accum_iter and hands the result to loss_scaler with `clip_grad`.
    build_executor  (tensors) -> an engine.GraphedStep or None, asked once, with the first batch; `step_executor` (the caller's own)
                    takes its place. Only a single-loss epoch can run through an executor.
    meter_divided   the fine-tuning order (reference ft_cls_trainer.py:66-77): the loss is divided inside `if args.backward` and the
                    meter gets it afterwards; pre-training (False) meters first and divides whether or not backward is on.
    vis_hook        called per step under test_experiment and visualize, and on the last batch when the epoch is a vis_train_freq'th
                    (`vis_last_batch`: the joint epoch has only ever drawn per step).
    `args.skip_nonfinite` (default False; FusedAdamW only): an optimizer step whose gradients hold an Inf or NaN is left out, on the
    device, as the reference's GradScaler.step does (utils/misc.py:290). The returned dict then gains `skipped_steps`, this epoch's
    count (one read-back, at the end). The metered loss of such a batch stays what it is: the guard protects the weights, not the log."""
    skip = bool(getattr(args, "skip_nonfinite", False))
    if not skip:
        return _run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, loss_names, eager_step, build_executor,
                          step_executor, clip_grad, meter_divided, vis_hook, vis_last_batch, batch_keys)
    if not hasattr(optimizer, "skip_nonfinite"):
        raise ValueError("args.skip_nonfinite needs a FusedAdamW (the verdict is reached on the device, inside the optimizer's launch)")
    if step_executor is not None and not getattr(step_executor, "skip_nonfinite", False):
        raise ValueError("args.skip_nonfinite is set but the given step_executor was built without skip_nonfinite=True")
    before = optimizer.skipped_seen          # the host's last reading: the end of the epoch before, or 0
    saved, optimizer.skip_nonfinite = optimizer.skip_nonfinite, True      # the eager steps of this epoch guard too
    try:
        stats = _run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, loss_names, eager_step, build_executor,
                           step_executor, clip_grad, meter_divided, vis_hook, vis_last_batch, batch_keys)
    finally:
        optimizer.skip_nonfinite = saved
    stats["skipped_steps"] = optimizer.skipped_steps() - before
    return stats


def _run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, loss_names, eager_step, build_executor,
               step_executor, clip_grad, meter_divided, vis_hook, vis_last_batch, batch_keys=None):
    model.train(True)
    logger = misc.MetricLogger(delimiter="  ")
    logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Epoch: [{}]".format(epoch + 1)
    optimizer.zero_grad()
    if log_writer is not None:
        print("log_dir: {}".format(log_writer.log_dir))
    n_iter = len(data_loader)
    on_gpu = str(args.device).startswith("cuda")
    defer = on_gpu and not getattr(args, "sync_every_step", False)      # with an executor: losses stay on the device between log points
    if step_executor is not None:
        build_executor = None
    if defer and getattr(args, "prefetch_to_device", True) and not getattr(data_loader, "yields_device_batches", False):
        # (a loader whose batches are already device tensors it will overwrite -- dataset.pretrain.gpu_event_loader -- must not be
        # asked for batch i + 1 before batch i has been consumed)
        data_loader = DevicePrefetcher(data_loader, args.device)
    deferred = last = None

    def meter(values):
        for name, v in zip(loss_names, values):
            logger.update(**{name: v.item()})

    def write(values, lr, it):
        x = int((it / n_iter + epoch) * 1000)        # "epoch_1000x" axis
        for name, v in zip(loss_names, values):
            log_writer.add_scalar(name, v, x)
        log_writer.add_scalar("lr", lr, x)

    for it, batch in enumerate(logger.log_every(args, data_loader, args.print_freq, header, keys=batch_keys)):
        if it % args.accum_iter == 0:
            adjust_learning_rate(optimizer, it / n_iter + epoch, args)
        tensors = [t.to(args.device, non_blocking=True) for t in batch[:-1]]
        if build_executor is not None:
            # the fast path is the default path: the loop captures its own step executor on the first batch
            step_executor, build_executor = build_executor(tensors), None
        lr = optimizer.param_groups[0]["lr"]
        log_now = (it + 1) % args.log_freq == 0
        step_now = (it + 1) % args.accum_iter == 0
        if step_executor is not None:
            written = (_executor_step(args, step_executor, tensors),)
            if defer:
                if deferred is None:
                    deferred = DeferredLosses(n_iter, tensors[0].device)
                deferred.push(written[0])
                logger.update(lr=lr)
                # the host reads the device only when a value is needed: a progress line is due, a log point is due (the reduction of
                # the logged value is collective: every rank is here at the same iterations), or the epoch ends
                if log_now or (it + 1) % args.print_freq == 0 or it + 1 == n_iter:
                    newest = deferred.flush(logger, loss_names[0])
                    if log_now:
                        reduced = misc.all_reduce_mean(newest)
                        if log_writer is not None:
                            write((reduced,), lr, it)
                continue
            meter(written)
        else:
            metered, vis = eager_step(tensors, batch[-1])
            if vis_hook is not None:
                last = vis
                if args.test_experiment and args.visualize:
                    vis_hook(args, *vis, epoch)
            if not meter_divided:
                meter(metered)      # read back before the backward is queued, as the reference does: the host waits for the forward here
            total = sum(metered[1:], metered[0])
            if args.backward or not meter_divided:
                total = total / args.accum_iter
            # a lone loss is written as it stands after the division (reference: `reconstruct_loss /= args.accum_iter`); the joint
            # epoch divides the sum and writes its two losses undivided
            written = (total,) if len(metered) == 1 else metered
            if args.backward:
                loss_scaler(total, optimizer, clip_grad=clip_grad, parameters=model.parameters(), update_grad=step_now)
                if step_now:
                    optimizer.zero_grad()
            if meter_divided:
                meter(written)
        # the rest of the reference's per-step record: synchronize, all-reduce the loss for the log
        if on_gpu:
            torch.cuda.synchronize()
        logger.update(lr=lr)
        reduced = [misc.all_reduce_mean(v.item()) for v in written]
        if log_writer is not None and log_now and step_now:
            write(reduced, lr, it)
    if deferred is not None:
        deferred.flush(logger, loss_names[0])
    if last is not None and vis_last_batch and args.visualize and (epoch + 1) % args.vis_train_freq == 0:
        vis_hook(args, *last, epoch)
    logger.synchronize_between_processes()
    print("Averaged stats:", logger)
    return {k: m.global_avg for k, m in logger.meters.items()}

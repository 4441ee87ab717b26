"""One-epoch loops of the pre-training stages with the reference's signatures and return dicts
(reference trainer/pretrain/pr_trainer.py:9-89,91-155): per-iteration LR schedule, loss / accum_iter, optimizer step
cadence, metric all-reduce -- the loop itself is trainer.epoch.run_epoch; here are each stage's forward and its step executor.
The matplotlib visualisation the reference calls from inside the loop is an optional `vis_hook` (default off)."""
import torch

from ..epoch import auto_executor, run_epoch


def auto_step_executor(args, model, optimizer, loss_scaler, batch_tensors, loss_name, vis_hook=None):
    """The step executor the epoch loops build by themselves on their first batch (and keep on the model): forward + backward +
    FusedAdamW captured once as a HIP graph and replayed per batch -- an eager step of this path is ~600 launches from Python and
    runs host-bound at 2.5-3x the device time. Returns None where the captured form cannot stand in for the
    eager loop: visualisation inside the loop, and what trainer.epoch.auto_executor refuses (gradient accumulation, backward off,
    an optimizer that is not FusedAdamW, a CPU device, a forward replaced on the instance, `args.graph_step = False`). A
    data-parallel run takes the executor's multi-GPU form with the scaler's reducer -- the contrastive stage with its key all-gather
    between two captured graphs, the Swin backbone with a collective per-step verdict on its window plan."""
    if vis_hook is not None and args.visualize:
        return None
    x, y = batch_tensors
    skip = bool(getattr(args, "skip_nonfinite", False))      # captured with the step (evp_grad_guard_multi in front of the update)

    def build():
        from ...engine import GraphedStep
        noise_shape = step_prepare = None
        if loss_name == "reconstruct_loss":
            fwd = lambda m, x_, y_, noise: m(x_, y_, is_rec=True, noise=noise)
            if getattr(args, "masking_strategy", "random") == "random":
                noise_shape = (x.shape[0], model.backbone.num_patches)
                if getattr(model, "backbone_type", "") == "swin":
                    # (data-parallel too: the ranks agree per step whether every pattern fits the captured shape, engine.GraphedStep._vote)
                    step_prepare = model.backbone.enable_static_plan(x.device)
        else:
            fwd = lambda m, x_, y_, noise: m(x_, y_)
        seed = int(torch.empty((), dtype=torch.int64).random_().item())      # follows torch.manual_seed like the eager draw would
        return GraphedStep(model, optimizer, fwd, [x.clone(), y.clone()], noise_shape=noise_shape,
                           generator=torch.Generator(device=x.device).manual_seed(seed), reducer=getattr(loss_scaler, "reducer", None),
                           step_prepare=step_prepare, host_generator=torch.Generator().manual_seed(seed), skip_nonfinite=skip)
    return auto_executor(args, model, optimizer, loss_name, build, extra=(skip,))


def _epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, loss_name, forward, vis_hook, step_executor=None, auto=True):
    def eager_step(tensors, names):
        outputs = forward(*tensors)
        return (outputs[0],), (*tensors, outputs, names)
    build = (lambda t: auto_step_executor(args, model, optimizer, loss_scaler, t, loss_name, vis_hook)) if auto else None
    return run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, (loss_name,), eager_step,
                     build_executor=build, step_executor=step_executor, vis_hook=vis_hook)


def pr_rec_one_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer=None, vis_hook=None,
                     step_executor=None):
    """Masked-modeling epoch: model(events_voxel_grid, sub_frame, is_rec=True). The forward / backward / optimizer calls of a
    batch run as one HIP-graph replay: the loop builds its executor on the first batch (auto_step_executor; opt out with
    args.graph_step = False) or takes the `step_executor` (an eventpretrain_amd.engine.GraphedStep on this model / optimizer)
    it is given."""
    return _epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, "reconstruct_loss",
                  lambda x, y: model(x, y, is_rec=True), vis_hook, step_executor)


def pr_con_one_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer=None, vis_hook=None,
                     step_executor=None):
    """Contrastive / transfer epoch: model(events_voxel_grid, clip_emb)."""
    return _epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, "contrastive_loss",
                  lambda x, y: model(x, y), vis_hook, step_executor)


def pr_con_n_one_epoch(args, model, preprocess, clip_model, data_loader, optimizer, epoch, loss_scaler, log_writer=None,
                       vis_hook=None):
    """Contrastive epoch with the CLIP image branch evaluated on the fly (reference trainer/pretrain/pr_trainer.py:158-223):
    batches carry the pre-processed RGB image instead of stored CLIP tokens, `clip_model.encode_image(image)` supplies the
    (B, 197, 512) token tensor. The CLIP encoder itself is the caller's frozen module (out of scope here: SURVEY.md 8c takes the
    CLIP branch as an input tensor); `preprocess` is accepted for signature compatibility and unused, as in the reference."""
    def forward(x, image):
        with torch.no_grad():
            clip_emb = clip_model.encode_image(image).to(args.device, non_blocking=True).float()
        return model(x, clip_emb)
    # (the CLIP encoder runs inside this loop's forward: no captured step here)
    return _epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, "contrastive_loss", forward, vis_hook, auto=False)


def pr_rec_and_con_one_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer=None, vis_hook=None):
    """Joint epoch (reference trainer/pretrain/pr_trainer.py:225-304): one masked-modeling forward and one contrastive
    forward per batch, the two losses summed before the single backward."""
    def eager_step(tensors, names):
        x, sub_frame, clip_emb = tensors
        rec = model(x, sub_frame, is_rec=True)
        con = model(x, clip_emb)
        return (rec[0], con[0]), (x, (sub_frame, clip_emb), (rec, con), names)
    return run_epoch(args, model, data_loader, optimizer, epoch, loss_scaler, log_writer, ("reconstruct_loss", "contrastive_loss"),
                     eager_step, vis_hook=vis_hook, vis_last_batch=False)

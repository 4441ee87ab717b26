"""The epoch loop (eventpretrain_amd/trainer/epoch.py) on the GPU: the default way of recording losses -- kept on the device, handed
to the meters when a progress line or a log point is due -- against the reference's per-step read-back (args.sync_every_step), both
through the step executor the loop builds on its first batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Writer:
    log_dir = "tb"

    def __init__(self):
        self.rows = []

    def add_scalar(self, name, value, x):
        self.rows.append((name, value, x))


def _epoch(batches, sync):
    from eventpretrain_amd.model.pretrain import pr_hub_model as hub
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, make_args
    from eventpretrain_amd.trainer.pretrain.pr_trainer import pr_rec_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    a = make_args(model_size="tiny", pr_phase="rec", patch_size=16, device="cuda", input_size=64, print_freq=2, log_freq=3)
    a.batch_size, a.epochs, a.warmup_epochs, a.lr, a.min_lr, a.sync_every_step = 2, 4, 1, 1e-3, 1e-6, sync
    m = hub.pretrain_hub_model_tiny_patch16_64(a, emb_frames_dim=512, queue_length=8, T=0.07)
    det_fill_module_(m)
    m = m.cuda().train()
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, a.weight_decay, layer_decay=1), lr=a.lr, betas=(0.9, 0.95))
    w = _Writer()
    torch.manual_seed(11)          # the executor's mask-noise stream is seeded from it
    stats = pr_rec_one_epoch(a, m, batches, opt, 0, NativeScalerWithGradNormCount(), log_writer=w)
    return stats, w.rows, m._evp_auto_executor[1]


def test_deferred_and_per_step_loss_records_agree_through_the_captured_step():
    """Five batches of the tiny hub (64 x 64, f32), the last of one sample, print_freq 2, log_freq 3: the deferred record flushes at
    iterations 2 (progress), 3 (log point), 4 (progress) and 5 (end), hands the buffer over between them, and the short batch takes
    the executor's eager step. The same steps run in both modes, so stats and writer rows agree within the bar captured against
    eager already has (rel 2e-5, test_gpu_round4.py::test_finetune_epoch_runs_captured_and_follows_the_eager_loop)."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.testing import det_normalish
    ops.set_compute_dtype(torch.float32)
    batches = [dict(events_voxel_grid=det_normalish(f"loop.voxels.{s}", (b, 5, 64, 64)) * 0.5, sub_frame=det_normalish(f"loop.sub_frame.{s}", (b, 1, 64, 64)),
                    image_name=[f"s{s}"] * b) for s, b in enumerate([2, 2, 2, 2, 1])]
    (stats, rows, ex), (stats_s, rows_s, ex_s) = _epoch(batches, False), _epoch(batches, True)
    for e in (ex, ex_s):
        # four replays, then the short batch's one step outside the graph: it alone counts as a fallback, so none came before it
        assert e.note == "hip-graph" and e.eager_fallbacks == 1, (e.note, e.eager_fallbacks)
    print("deferred", stats, rows, "\nper step", stats_s, rows_s)
    assert list(stats) == list(stats_s) == ["lr", "reconstruct_loss"]
    assert stats["lr"] == stats_s["lr"] and stats["reconstruct_loss"] == pytest.approx(stats_s["reconstruct_loss"], rel=2e-5)
    assert [(n, x) for n, _, x in rows] == [(n, x) for n, _, x in rows_s] == [("reconstruct_loss", 400), ("lr", 400)]
    assert [v for _, v, _ in rows] == pytest.approx([v for _, v, _ in rows_s], rel=2e-5)

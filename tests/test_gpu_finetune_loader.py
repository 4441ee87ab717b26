"""GpuFinetuneLoader (dataset/finetune_cls/gpu_event_loader.py) on the GPU: the training chain in bilinear mode against the float32
restatement of the view (equal) and the CPU oracle's grids (the K1 bound), the validation form against voxel_grid_batch on the
host-picked windows, the labels' lifetime across reused slots, and both forms under ft_train_one_epoch / ft_val."""
import math

import numpy as np
import pytest
import torch

from bilinear_truth import evg_bilinear

pytestmark = pytest.mark.gpu

SENSOR, S, B, FIX, VAL_FIX = (48, 64), 32, 4, 2000, 3000
K1_TOL = 1e-5                    # float32 LDS atomics in another order than the oracle's sequential sum


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    base = dict(phase="finetune_cls", crop_min=0.8, input_size=S, num_bins=5, fix_events_num=FIX, val_fix_events_num=VAL_FIX,
                img_sensor_w=SENSOR[1], img_sensor_h=SENSOR[0], device="cuda", resize_mode="bilinear")
    base.update(kw)
    return make_args(**base)


def _samples(n, tag=0):
    """n clips of 1500 .. 5000 rows (shorter than both windows, between them, longer than both), labels that are no simple count."""
    from eventpretrain_amd.testing import synthetic_events
    sizes = [1500, 5000, 2500, 3000, 2000, 4321, 3001, 1999]
    return [(synthetic_events(5000 + 31 * tag + i, sizes[i % len(sizes)] + (7 * i if i >= len(sizes) else 0), width=SENSOR[1], height=SENSOR[0]),
             (7 * i + 3 * tag) % 10, f"clip{tag}_{i}") for i in range(n)]


def _windows(samples, fix, seed, step, first_sample):
    """The loader's window rule on the host: word 0 of the counter stream keyed by (seed, step, first_sample + i)."""
    from eventpretrain_amd.dataset.augmentation.events_augment import philox_words
    w0 = philox_words(seed, step, first_sample + np.arange(len(samples)), 0, 1)[:, 0]
    out = []
    for (e, _, _), w in zip(samples, w0):
        n = e.shape[0]
        s0 = (int(w) * (n - fix)) >> 32 if n > fix else 0
        out.append(e[s0:s0 + min(n, fix)])
    return out


def test_train_chain_bilinear_against_restatement_and_oracle():
    """(a) three replays of the captured chain in bilinear mode: `out` EQUALS the restatement of the raw grids the chain kept
    (chain.raw) under the crop rows it drew; the raw grids are the CPU oracle's for the decisions read back, within the K1 bound."""
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    from oracle import augment_oracle as ao
    from oracle.voxel_oracle import voxel_grid
    H, W = SENSOR
    a = _args()
    samples = _samples(3 * B)
    loader = GpuFinetuneLoader(a, samples, batch_size=B, n_batches=3, is_train=True, seed=21, first_sample=8, step0=5)
    chain = loader.chain
    assert chain.fused and chain.self_driven and chain.raw is not None and loader.pipe.resize_mode == "bilinear"
    n_aug, flips, worst = 0, set(), 0.0
    for k, batch in enumerate(loader):
        assert list(batch) == ["events_voxel_grid", "label", "image_name"]
        torch.cuda.synchronize()
        out, raw = batch["events_voxel_grid"].cpu().numpy(), chain.raw.cpu().numpy()
        d = chain.d_tab.cpu().numpy()
        tabs = d[:5 * (B + 1)].reshape(5, B + 1)
        o4, pw = 5 * (B + 1), (B * 6 + 1) // 2
        prm = d[o4:o4 + pw].view(np.int32)[:B * 6].reshape(B, 6)
        er_all, ai_all, nz_all = chain.er.cpu().numpy(), chain.ai.cpu().numpy(), chain.nz.cpu().numpy().reshape(-1, 3)
        wins = _windows(samples[B * k:B * k + B], FIX, 21, 5 + k, 8)
        off = loader.d_off.cpu().numpy()
        for c in range(B):
            what = (k, c)
            assert off[c + 1] - off[c] == wins[c].shape[0] == min(samples[B * k + c][0].shape[0], FIX), what
            assert (tabs[0, c], tabs[1, c]) == (off[c], off[c + 1]), what         # the chain takes the uploaded window whole
            p = tuple(int(v) for v in prm[c])
            assert 0 <= p[0] and p[0] + p[2] <= S and 0 <= p[1] and p[1] + p[3] <= S and p[2] >= 1 and p[3] >= 1, what
            flips.add(p[4:])
            assert np.array_equal(out[c], evg_bilinear(raw[c], p, (S, S))), what
            er, ai, nz = er_all[tabs[2, c]:tabs[2, c + 1]], ai_all[tabs[3, c]:tabs[3, c + 1]], nz_all[tabs[3, c]:tabs[3, c + 1]]
            dec = None if int(0.01 * wins[c].shape[0]) == 0 else (er, ai, nz)
            n_aug += int(er.size + ai.size > 0)
            rows = ao.erase_add_apply(wins[c], dec, SENSOR)
            want = voxel_grid(ao.events_reshape(rows, W, H, S, S), 5, (S, S))
            err = float(np.abs(raw[c] - want).max())
            worst = max(worst, err)
            assert err <= K1_TOL, (what, err)
    print("raw grids vs oracle: max |err|", worst, "flip pairs seen", sorted(flips))
    assert k == 2 and loader.step == 8 and n_aug > 0 and len(flips) > 1


def _val_loader(samples):
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    return GpuFinetuneLoader(_args(), samples, batch_size=B, n_batches=2, is_train=False, seed=3, first_sample=2, step0=7)


def test_val_form_equals_k1_on_the_host_windows():
    """(b) validation: windows of min(n, val_fix_events_num) rows picked by the same word-0 rule, then ONE K1 call and no view kernel:
    the batch EQUALS voxel_grid_batch of the host-picked windows with the loader's float64 cells (algo 3: the sum does not depend on
    the order the LDS atomics arrive in). Against K1's default float32 cells, whose result moves by an ulp or two from launch to
    launch, both are within the K1 bound of the sequential sum, so within twice the bound of each other."""
    from eventpretrain_amd.dataset.dataset_utils.events_to_voxel_grid import voxel_grid_batch
    H, W = SENSOR
    samples = _samples(2 * B, tag=1)
    loader = _val_loader(samples)
    assert loader.chain is None and loader.ev.shape[0] == B * VAL_FIX
    n_batches = 0
    for k, batch in enumerate(loader):
        got = batch["events_voxel_grid"].clone()
        assert tuple(got.shape) == (B, 5, S, S)
        lens = np.diff(loader.d_off.cpu().numpy())
        wins = _windows(samples[B * k:B * k + B], VAL_FIX, 3, 7 + k, 2)
        assert lens.tolist() == [w.shape[0] for w in wins] == [min(s[0].shape[0], VAL_FIX) for s in samples[B * k:B * k + B]]
        assert np.array_equal(loader.ev[:int(lens.sum())].cpu().numpy(), np.concatenate(wins, 0)), k      # the uploaded rows ARE those windows
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        rows = torch.from_numpy(np.concatenate(wins, 0)).cuda()
        want = voxel_grid_batch(rows, off, 5, (S, S), scale=(S / W, S / H), algo=3)
        f32 = voxel_grid_batch(rows, off, 5, (S, S), scale=(S / W, S / H))
        err = float((got - f32).abs().max())
        print(f"val batch {k}: {int((got != want).sum())} of {got.numel()} elements differ from a second K1 launch with float64 cells; "
              f"{int((got != f32).sum())} from one with float32 cells, max |diff| {err:.3e}")
        assert torch.equal(got, want), k
        assert err <= 2 * K1_TOL, (k, err)
        assert float(got.abs().sum()) > 0
        n_batches += 1
    assert n_batches == 2 and loader.step == 9 and any(s[0].shape[0] > VAL_FIX for s in samples)


def test_val_passes_from_the_same_step0_are_bit_identical():
    """(b) two passes of a validation loader, and a second loader built with the same step0, give the same bits: the same windows, and
    grids binned with float64 cells. (With K1's default float32 cells ~80 of the 20 480 elements of a batch moved by up to 4.8e-7
    from one pass to the next on the MI355X: the LDS atomics arrive in another order on every launch.)"""
    samples = _samples(2 * B, tag=1)
    loader = _val_loader(samples)
    first = [b["events_voxel_grid"].clone() for b in loader]
    again = [b["events_voxel_grid"].clone() for b in loader]
    other = [b["events_voxel_grid"].clone() for b in _val_loader(samples)]
    assert len(first) == len(again) == len(other) == 2
    for k, (x, y, z) in enumerate(zip(first, again, other)):
        print(f"val batch {k}: second pass differs in {int((x != y).sum())} elements (max {float((x - y).abs().max()):.3e}), "
              f"a second loader in {int((x != z).sum())} (max {float((x - z).abs().max()):.3e}) of {x.numel()}")
    for x, y, z in zip(first, again, other):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("is_train", [True, False])
def test_labels_survive_slot_reuse(is_train):
    """(c) five batches through two label slots: a clone taken on the stream at each yield holds that batch's labels."""
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    samples = _samples(5 * B, tag=2)
    loader = GpuFinetuneLoader(_args(), samples, batch_size=B, n_batches=5, is_train=is_train, seed=1)
    assert loader.yields_device_batches and len(loader) == 5
    got, names = [], []
    for batch in loader:
        assert batch["label"].is_cuda and batch["label"].dtype == torch.int64
        got.append(batch["label"].clone())
        names += batch["image_name"]
    torch.cuda.synchronize()
    assert torch.cat(got).cpu().tolist() == [s[1] for s in samples]
    assert names == [s[2] for s in samples]
    assert len({g.data_ptr() for g in got}) == 5 and len(loader._lab) == 2


def test_finetune_epoch_and_validation_run_captured_on_the_loader():
    """(d) ft_train_one_epoch then ft_val over three-batch loaders (ViT-Small, B = 2, bf16: what tests/test_gpu_finetune.py runs
    captured): finite losses, the reference's keys, and both executors on the model are captured graphs."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch, ft_val
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    a = _args(input_size=224, model_size="small", backbone_type="vit", num_classes=10, mask_ratio=0.0, dataset_type="n-caltech101",
              clip_grad=None, smoothing=0, lr=1e-3, min_lr=1e-4, warmup_epochs=0, epochs=1)
    m = ft.finetune_cls_hub_model_small_patch16(a)
    det_fill_module_(m)
    m = m.cuda().train()
    train = GpuFinetuneLoader(a, _samples(6, tag=3), batch_size=2, n_batches=3, is_train=True, seed=4)
    val = GpuFinetuneLoader(a, _samples(6, tag=4), batch_size=2, n_batches=3, is_train=False, seed=4)
    ops.set_compute_dtype(torch.bfloat16)
    try:
        opt = FusedAdamW(lrd.param_groups_lrd(a, m, a.weight_decay, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
        stats = ft_train_one_epoch(a, m, train, opt, 0, NativeScalerWithGradNormCount())
        vstats = ft_val(a, m, val, 0)
    finally:
        ops.set_compute_dtype(torch.float32)
    print(stats, vstats)
    assert set(stats) == {"loss_cls", "lr"} and math.isfinite(stats["loss_cls"])
    assert set(vstats) == {"loss_cls", "acc1", "acc5"} and all(math.isfinite(v) for v in vstats.values())
    step = m._evp_auto_executor[1]
    assert step.graph is not None and step.note == "hip-graph", step.note
    ev = m._evp_auto_eval[1]
    assert ev.graph is not None and ev.replays == 3 and ev.eager_calls == 0
    assert train.step == 3

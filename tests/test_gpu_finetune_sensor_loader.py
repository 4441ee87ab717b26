"""GpuFinetuneLoader's sensor-resolution recipe and noisy validation on the GPU (sensor 45 x 60 -> 32 x 32, B = 4, windows of 2000 / 3000
rows): the training chain with grid="sensor" in both resize modes, clean validation as K1 (float64 cells) + a real resize, noisy
validation (--val_event_noise) in both grid modes -- the grids against the CPU oracle for the decisions read back (the K1 bound), the
views against the float32 restatements (equal), passes against each other (equal) -- and one ft_train_one_epoch + ft_val run on the
N-Caltech101 recipe finetune_recipe gives."""
import math

import numpy as np
import pytest
import torch

from bilinear_truth import evg_bilinear

pytestmark = pytest.mark.gpu

SENSOR, S, B, FIX, VAL_FIX = (45, 60), 32, 4, 2000, 3000
K1_TOL = 1e-5                    # float32 LDS atomics in another order than the oracle's sequential sum
FULL = (0, 0, SENSOR[1], SENSOR[0], 0, 0)        # view_resize alone


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    # (img_sensor_* stay at the namespace's 640 x 480: the loader must take the sensor from its keyword)
    base = dict(phase="finetune_cls", crop_min=0.8, input_size=S, num_bins=5, fix_events_num=FIX, val_fix_events_num=VAL_FIX,
                device="cuda", resize_mode="bilinear")
    base.update(kw)
    return make_args(**base)


def _samples(n, tag=0, sensor=SENSOR):
    from eventpretrain_amd.testing import synthetic_events
    sizes = [1500, 5000, 2500, 3000, 2000, 4321, 3001, 1999]
    return [(synthetic_events(7000 + 31 * tag + i, sizes[i % len(sizes)] + (7 * i if i >= len(sizes) else 0), width=sensor[1], height=sensor[0]),
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


def _restate(mode):
    from oracle.augment_oracle import evg_transform
    return evg_bilinear if mode == "bilinear" else evg_transform


def _plan(chain):
    """What the chain's last replay planned and drew, read back: (crop rows int32 [B,6], per-clip (erase, add index, noise) lists)."""
    d = chain.d_tab.cpu().numpy()
    tabs = d[:5 * (B + 1)].reshape(5, B + 1)
    o4, pw = 5 * (B + 1), (B * 6 + 1) // 2
    prm = d[o4:o4 + pw].view(np.int32)[:B * 6].reshape(B, 6).copy()
    er, ai, nz = chain.er.cpu().numpy(), chain.ai.cpu().numpy(), chain.nz.cpu().numpy().reshape(-1, 3)
    dec = [(er[tabs[2, c]:tabs[2, c + 1]].copy(), ai[tabs[3, c]:tabs[3, c + 1]].copy(), nz[tabs[3, c]:tabs[3, c + 1]].copy()) for c in range(B)]
    return prm, dec


def _fused_f64(chain, view_rows=None):
    """The fused K1 with float64 cells launched again on the tables of the chain's last replay: the raw grids, or (view_rows) the
    nearest view. An order-independent sum: the bits are those of any other launch on these inputs."""
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    pipe = chain.pipe
    tabs = chain.d_tab[:5 * (B + 1)].view(5, B + 1)
    out = torch.empty(B, 5, *((pipe.gh, pipe.gw) if view_rows is None else (S, S)), dtype=torch.float32, device="cuda")
    kws = torch.zeros_like(chain.kws)
    prm = None if view_rows is None else torch.from_numpy(np.ascontiguousarray(view_rows, dtype=np.int32)).cuda()
    call("evp_voxel_scatter_fused_algo_f32", ptr(chain.events), ptr(tabs[0]), ptr(tabs[1]), B, ptr(chain.er), ptr(tabs[2]), ptr(chain.ws), ptr(tabs[3]),
         chain.fix, 5, pipe.gh, pipe.gw, pipe.scale[0], pipe.scale[1], ptr(prm), S if prm is not None else 0, S if prm is not None else 0,
         1 if prm is not None else 0, ptr(kws), ptr(out), 3, stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _oracle_grid(window, dec, grid):
    """voxel_grid(erase_add_apply(window, decisions)) at the sensor's size, or after events_reshape at the input's."""
    from oracle import augment_oracle as ao
    from oracle.voxel_oracle import voxel_grid
    H, W = SENSOR
    rows = ao.erase_add_apply(window, dec, SENSOR)
    if grid == "sensor":
        return voxel_grid(rows, 5, SENSOR)
    return voxel_grid(ao.events_reshape(rows, W, H, S, S), 5, (S, S))


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_train_chain_on_the_sensor_grid(mode):
    """Three replays with grid="sensor": the plan's crop rows are draw_evg_params_batch's for a 45 x 60 grid; the raw grids (45 x 60,
    unscaled) are the oracle's for the decisions read back within the K1 bound; `out` EQUALS the restatement of the raw grids under
    those rows. Bilinear mode keeps its raw grids (chain.raw). Nearest mode flushes the float32 tile through the view and stores no raw
    grid, and a second float32 launch would differ by an ulp or two, so there the equality is held on the float64-cell form of the
    same kernel launched on the chain's own tables (raw and flushed), and the chain's `out` is held to it within twice the K1 bound."""
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    H, W = SENSOR
    samples = _samples(3 * B)
    loader = GpuFinetuneLoader(_args(resize_mode=mode), samples, batch_size=B, n_batches=3, is_train=True, seed=21, first_sample=8, step0=5,
                               grid="sensor", sensor=SENSOR)
    chain, fn = loader.chain, _restate(mode)
    assert chain.fused and chain.self_driven and loader.pipe.resize_mode == mode and (loader.pipe.gh, loader.pipe.gw) == SENSOR
    assert (chain.raw is not None and tuple(chain.raw.shape) == (B, 5, H, W)) if mode == "bilinear" else chain.raw is None
    n_aug, flips, worst, boxes = 0, set(), 0.0, set()
    for k, batch in enumerate(loader):
        torch.cuda.synchronize()
        out = batch["events_voxel_grid"].cpu().numpy()
        assert out.shape == (B, 5, S, S)
        prm, dec = _plan(chain)
        assert np.array_equal(prm, va.draw_evg_params_batch(21, 5 + k, B, H, W, 0.8, 8)), k
        raw = chain.raw.cpu().numpy() if mode == "bilinear" else _fused_f64(chain)
        view = out if mode == "bilinear" else _fused_f64(chain, prm)
        wins = _windows(samples[B * k:B * k + B], FIX, 21, 5 + k, 8)
        for c in range(B):
            what = (mode, k, c)
            p = tuple(int(v) for v in prm[c])
            assert 0 <= p[0] and p[0] + p[2] <= W and 0 <= p[1] and p[1] + p[3] <= H and p[2] >= 1 and p[3] >= 1, what
            flips.add(p[4:]), boxes.add(p[:4])
            assert np.array_equal(view[c], fn(raw[c], p, (S, S))), what
            assert float(np.abs(out[c] - view[c]).max()) <= 2 * K1_TOL, what
            n_aug += int(dec[c][0].size + dec[c][1].size > 0)
            err = float(np.abs(raw[c] - _oracle_grid(wins[c], dec[c], "sensor")).max())
            worst = max(worst, err)
            assert err <= K1_TOL, (what, err)
    print(f"{mode}: raw grids vs oracle max |err| {worst:.3e}, flip pairs {sorted(flips)}, {len(boxes)} boxes")
    assert k == 2 and loader.step == 8 and n_aug > 0 and len(flips) > 1
    assert any(b[2] > H for b in boxes)          # boxes wider than the grid is high: drawn on 60 x 45


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_prepared_and_inline_forms_on_the_sensor_grid(mode):
    """prepare / run_prepared and run with grid="sensor" (K1 on the merged clip, then the view kernel; no raw grid is handed out): the
    views against the restatement of the ORACLE's grids. A nearest view picks cells, a bilinear one is a convex combination of four
    cells followed by three float32 roundings, so the bound is the K1 bound plus 3 x 2^-24 x the largest cell. Then the same with
    view_augment=False and the validation window: view_resize alone."""
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    H, W = SENSOR
    fn = _restate(mode)
    clips = [s[0] for s in _samples(B, tag=5)]
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
    ev = torch.from_numpy(np.concatenate(clips, 0)).cuda()
    for kw, fix in ((dict(), FIX), (dict(view_augment=False, fix_events_num=VAL_FIX), VAL_FIX)):
        pipe = GpuInputPipeline(_args(), seed=5, resize_mode=mode, grid="sensor", sensor=SENSOR, **kw)
        pb = pipe.prepare(off, step=2, first_sample=1)
        assert np.array_equal(pb.params, va.draw_evg_params_batch(5, 2, B, H, W, 0.8, 1))
        assert pb.sizes.tolist() == [min(c.shape[0], fix) for c in clips]
        dec = pipe.device_decisions(pb, "cuda")
        out = pipe.run_prepared(ev, pb)[0].cpu().numpy()
        inline = pipe.run(ev, off, pb.windows, dec, pb.params)[0].cpu().numpy()
        assert out.shape == inline.shape == (B, 5, S, S)
        for c in range(B):
            w0, w1 = (int(v) for v in pb.windows[c])
            grid = _oracle_grid(clips[c][w0:w1], dec[c], "sensor")
            want = fn(grid, tuple(int(v) for v in pb.params[c]) if pipe.view_augment else FULL, (S, S))
            tol = K1_TOL + 3 * 2.0 ** -24 * float(np.abs(grid).max())
            for name, got in (("run_prepared", out), ("run", inline)):
                err = float(np.abs(got[c] - want).max())
                assert err <= tol, (mode, kw, name, c, err, tol)
        assert float(np.abs(out).sum()) > 0
    # the crop-box validation tests against the 45 x 60 grid: a 46 x 46 box fits its width and not its height
    drawn = pipe.draw(np.diff(off), 2, 1)
    bad = drawn[2].copy()
    bad[0] = (0, 0, 46, 46, 0, 0)
    pipe.draw = lambda *a, **k: (drawn[0], drawn[1], bad)
    with pytest.raises(ValueError, match="outside the grid"):
        pipe.prepare(off, step=2, first_sample=1)


def _val_loader(samples, mode="bilinear", grid="sensor", **kw):
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    return GpuFinetuneLoader(_args(resize_mode=mode, **kw), samples, batch_size=B, n_batches=2, is_train=False, seed=3, first_sample=2, step0=7,
                             grid=grid, sensor=SENSOR)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_clean_validation_is_k1_plus_a_real_resize(mode):
    """Clean validation with grid="sensor": the batch [B, 5, 32, 32] EQUALS the resize restatement (view_resize alone: the full box, no
    flips) of voxel_grid_batch(..., algo=3) at 45 x 60 on the host-picked windows, which is the oracle's grid within the K1 bound."""
    from eventpretrain_amd.dataset.dataset_utils.events_to_voxel_grid import voxel_grid_batch
    samples = _samples(2 * B, tag=1)
    loader, fn = _val_loader(samples, mode), _restate(mode)
    assert loader.chain is None and tuple(loader.raw.shape) == (B, 5) + SENSOR
    n_batches = 0
    for k, batch in enumerate(loader):
        got = batch["events_voxel_grid"].cpu().numpy()
        assert got.shape == (B, 5, S, S)
        wins = _windows(samples[B * k:B * k + B], VAL_FIX, 3, 7 + k, 2)
        lens = [w.shape[0] for w in wins]
        assert np.diff(loader.d_off.cpu().numpy()).tolist() == lens
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        raw = voxel_grid_batch(torch.from_numpy(np.concatenate(wins, 0)).cuda(), off, 5, SENSOR, algo=3).cpu().numpy()
        for c in range(B):
            assert np.array_equal(got[c], fn(raw[c], FULL, (S, S))), (mode, k, c)
            assert float(np.abs(raw[c] - _oracle_grid(wins[c], None, "sensor")).max()) <= K1_TOL, (mode, k, c)
        assert float(np.abs(got).sum()) > 0
        n_batches += 1
    assert n_batches == 2 and loader.step == 9


@pytest.mark.parametrize("grid,mode", [("input", "bilinear"), ("sensor", "bilinear"), ("sensor", "nearest")])
def test_noisy_validation_grids_views_and_repeatability(grid, mode):
    """--val_event_noise: windows of val_fix_events_num rows, erase / add drawn by the chain, no view augmentation, float64 cells. The
    grid is the oracle's voxel_grid(erase_add_apply(window, decisions read back)) within the K1 bound and the view is exact (the identity
    for grid="input"; the bilinear kernel on chain.raw; the nearest flush against a second float64 launch's raw grids). A second pass
    and a second loader with the same step0 give the same bits; the clean validation batches of the same samples differ."""
    samples = _samples(2 * B, tag=1)
    loader, fn = _val_loader(samples, mode, grid, val_event_noise=True), _restate(mode)
    chain = loader.chain
    assert chain is not None and chain.fused and chain.self_driven and chain.algo == 3 and chain.fix == VAL_FIX and chain.kmax == 30
    assert loader.ev.shape[0] == B * VAL_FIX and not loader.pipe.view_augment and loader.args.fix_events_num == FIX
    first, n_er, n_ad, worst = [], 0, 0, 0.0
    for k, batch in enumerate(loader):
        torch.cuda.synchronize()
        out = batch["events_voxel_grid"].clone()
        first.append(out)
        got = out.cpu().numpy()
        assert got.shape == (B, 5, S, S)
        _, dec = _plan(chain)
        if grid == "input":
            assert chain.raw is None and not chain.resize
            raw = got                                        # view_resize of an S x S grid to S x S: the grids ARE the batch
        else:
            raw = chain.raw.cpu().numpy() if mode == "bilinear" else _fused_f64(chain)
        wins = _windows(samples[B * k:B * k + B], VAL_FIX, 3, 7 + k, 2)
        assert np.diff(loader.d_off.cpu().numpy()).tolist() == [w.shape[0] for w in wins]
        for c in range(B):
            what = (grid, mode, k, c)
            er, ai, _ = dec[c]
            n = wins[c].shape[0]
            assert int(0.001 * n) <= er.size < int(0.01 * n) and int(0.001 * n) <= ai.size < int(0.01 * n), (what, er.size, ai.size)
            n_er, n_ad = n_er + er.size, n_ad + ai.size
            err = float(np.abs(raw[c] - _oracle_grid(wins[c], dec[c], grid)).max())
            worst = max(worst, err)
            assert err <= K1_TOL, (what, err)
            if grid == "sensor":
                assert np.array_equal(got[c], fn(raw[c], FULL, (S, S))), what
    print(f"noisy val {grid} / {mode}: grids vs oracle max |err| {worst:.3e}; {n_er} rows erased, {n_ad} added")
    assert len(first) == 2 and loader.step == 9 and n_er > 0 and n_ad > 0
    again = [b["events_voxel_grid"].clone() for b in loader]
    other = [b["events_voxel_grid"].clone() for b in _val_loader(samples, mode, grid, val_event_noise=True)]
    clean = [b["events_voxel_grid"].clone() for b in _val_loader(samples, mode, grid)]
    assert len(again) == len(other) == len(clean) == 2
    for x, y, z, w in zip(first, again, other, clean):
        assert torch.equal(x, y) and torch.equal(x, z)
        assert not torch.equal(x, w) and float((x - w).abs().max()) > 100 * K1_TOL


def test_finetune_epoch_and_noisy_validation_on_the_caltech_recipe():
    """ft_train_one_epoch then ft_val over three-batch loaders built from finetune_recipe(args) for n-caltech101 (180 x 240 -> 224,
    ViT-Small, B = 2, bf16) with val_event_noise: finite stats, and both executors on the model are captured graphs."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader, finetune_recipe
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch, ft_val
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    a = _args(input_size=224, model_size="small", backbone_type="vit", num_classes=10, mask_ratio=0.0, dataset_type="n-caltech101",
              cal_sensor_h=180, cal_sensor_w=240, val_event_noise=True, clip_grad=None, smoothing=0, lr=1e-3, min_lr=1e-4, warmup_epochs=0,
              epochs=1)
    recipe = finetune_recipe(a)
    assert recipe == dict(grid="sensor", sensor=(180, 240))
    m = ft.finetune_cls_hub_model_small_patch16(a)
    det_fill_module_(m)
    m = m.cuda().train()
    train = GpuFinetuneLoader(a, _samples(6, tag=3, sensor=(180, 240)), batch_size=2, n_batches=3, is_train=True, seed=4, **recipe)
    val = GpuFinetuneLoader(a, _samples(6, tag=4, sensor=(180, 240)), batch_size=2, n_batches=3, is_train=False, seed=4, **recipe)
    assert tuple(train.chain.raw.shape) == tuple(val.chain.raw.shape) == (2, 5, 180, 240) and val.chain.algo == 3 and train.chain.algo == 0
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
    assert train.step == 3 and val.step == 3

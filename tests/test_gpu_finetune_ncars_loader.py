"""GpuFinetuneLoader's N-Cars recipe on the GPU (grid="window": every clip's grid is its own window's extent; capacity 48 x 64 -> 32 x 32,
B = 4, windows of 300 / 4000 rows, three batches): evp_events_window_geometry alone against numpy and draw_evg_params_batch's per-clip
form; the training chain in both resize modes -- extents, crop rows, raw grids against the CPU oracle for the decisions read back (the K1
bound) with the padding exactly zero, views against the float32 restatements (equal); clean and noisy validation; the host check of the
pack; one ft_train_one_epoch + ft_val run on ncars_recipe.

The clips are built for the geometry kernel's failure modes: extents at the full capacity, 9 x 13 and 30 x 1; a window shorter than one wave
(40 rows); lengths that are no multiple of the workgroup (1024 lanes), one of them longer than it; the maximum row first in one window and last in another; clips longer than
the window whose x range grows with time (the window's extent is not the clip's); clips dense at their right and bottom edges, so that
added rows land past the clip's own bound -- a bound taken from the capacity would leave them in the padding."""
import math

import numpy as np
import pytest
import torch

from bilinear_truth import evg_bilinear

pytestmark = pytest.mark.gpu

CAP, S, B, FIX, VAL_FIX = (48, 64), 32, 4, 300, 4000
K1_TOL = 1e-5                    # float32 LDS atomics in another order than the oracle's sequential sum

# (The edge-dense clips stay below a thousand rows: K1_TOL is an ABSOLUTE bound, and a cell that sums thousands of +-1 terms sequentially in
# float32, as the oracle does, carries more rounding than that on its own -- float32 spacing is 7.6e-6 at 64.)
# (H, W, rows, kind): "edge" = dense at the right / bottom edge, "grow" = x range grows with time, "first" / "last" = where the one row
# that holds the maximum of both coordinates sits
CLIPS = [(48, 64, 1000, "edge"), (9, 13, 300, "first"), (30, 1, 40, "edge"), (40, 41, 5000, "grow"),
         (37, 52, 777, "last"), (48, 64, 299, "edge"), (9, 13, 700, "edge"), (30, 1, 333, "edge"),
         (20, 64, 257, "first"), (48, 3, 650, "edge"), (9, 13, 2000, "grow"), (33, 47, 512, "last")]


def _clip(i, H, W, n, kind):
    rng = np.random.default_rng(9100 + i)
    if kind == "edge":
        x = np.maximum(W - 1 - np.floor(rng.exponential(1.0, n)), 0)
        y = np.maximum(H - 1 - np.floor(rng.exponential(1.0, n)), 0)
    elif kind == "grow":
        x = np.floor(rng.uniform(0, 1, n) * W * (0.2 + 0.8 * np.arange(n) / (n - 1)))
        y = np.floor(rng.uniform(0, H, n))
    else:
        x = np.floor(rng.uniform(0, max(W - 1, 1), n))
        y = np.floor(rng.uniform(0, max(H - 1, 1), n))
        x[0 if kind == "first" else n - 1], y[0 if kind == "first" else n - 1] = W - 1, H - 1
    t = np.sort(rng.uniform(0.0, 0.05, n))
    p = (rng.uniform(0, 1, n) < 0.5).astype(np.float64)
    return np.stack([x, y, t, p], 1).astype(np.float64)


def _samples(tag=0):
    return [(_clip(i + 100 * tag, *CLIPS[i]), (3 * i + tag) % 2, f"car{tag}_{i}") for i in range(len(CLIPS))]


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    base = dict(phase="finetune_cls", crop_min=0.8, input_size=S, num_bins=5, fix_events_num=FIX, val_fix_events_num=VAL_FIX,
                device="cuda", resize_mode="bilinear", dataset_type="n-cars", num_classes=2)
    base.update(kw)
    return make_args(**base)


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


def _extents(wins):
    return np.asarray([[int(w[:, 1].max()) + 1, int(w[:, 0].max()) + 1] for w in wins], np.int32)


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
    """The fused K1 with float64 cells launched again on the tables of the chain's last replay (its added rows are in chain.ws): the raw
    grids at the capacity, or (view_rows) the nearest view. An order-independent sum: the bits are those of any other launch."""
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


def _oracle_grid(window, dec, hw):
    """The padded grid: voxel_grid at the CAPACITY of erase_add_apply(window, decisions) bounded by the clip's own (H_c, W_c)."""
    from oracle import augment_oracle as ao
    from oracle.voxel_oracle import voxel_grid
    return voxel_grid(ao.erase_add_apply(window, dec, hw), 5, CAP)


def _moved(window, dec, hw):
    """Added rows the per-clip bound moves (x + noise past W_c - 1 or y + noise past H_c - 1)."""
    xy = window[dec[1], :2] + dec[2][:, :2]
    return int(((xy[:, 0] > hw[1] - 1) | (xy[:, 1] > hw[0] - 1)).sum())


def _padding_is_zero(grid, hw):
    return not grid[:, hw[0]:].any() and not grid[:, :, hw[1]:].any()


def _geometry(ev, wb, we, n, draw, seed=0, step=0, first=0, step_first=None, cap=CAP):
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    hw = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("evp_events_window_geometry", ptr(ev), ptr(wb), ptr(we), n, cap[0], cap[1], draw, 0.8, seed, step, first, ptr(step_first), ptr(hw), ptr(rows),
         ptr(status), stream_ptr())
    torch.cuda.synchronize()
    return hw.cpu().numpy(), rows.cpu().numpy(), int(status.item())


def test_window_geometry_kernel_alone():
    """All twelve clips in one launch, train windows (300 rows, starts inside the clips) and whole clips: clip_hw is numpy's, the rows
    are draw_evg_params_batch's on those extents (scalars and the device (step, first sample) pair agree), without draw_crop the clips' full
    boxes, status 0. Then refused windows -- past the capacity in x, in y, negative, empty -- are counted and their extents clamped."""
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    samples = _samples()
    n = len(samples)
    clips = [s[0] for s in samples]
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
    ev = torch.from_numpy(np.concatenate(clips, 0)).cuda()
    for fix in (FIX, VAL_FIX):
        wins = _windows(samples, fix, 21, 5, 8)
        beg = np.asarray([off[i] + int(np.flatnonzero((clips[i][:, 2] == wins[i][0, 2]))[0]) for i in range(n)], np.int64)
        end = beg + np.asarray([w.shape[0] for w in wins], np.int64)
        assert all(np.array_equal(ev[b:e].cpu().numpy(), w) for b, e, w in zip(beg, end, wins))
        want = _extents(wins)
        assert (want[:, 0] <= CAP[0]).all() and (want[:, 1] <= CAP[1]).all() and (want == CAP).all(1).any() and [30, 1] in want.tolist()
        wb, we = torch.from_numpy(beg).cuda(), torch.from_numpy(end).cuda()
        hw, rows, status = _geometry(ev, wb, we, n, 1, seed=21, step=5, first=8)
        assert status == 0 and np.array_equal(hw, want), (fix, hw.tolist(), want.tolist())
        host = va.draw_evg_params_batch(21, 5, n, want[:, 0], want[:, 1], 0.8, 8)
        assert np.array_equal(rows, host), (fix, rows.tolist(), host.tolist())
        assert ((rows[:, 2] < want[:, 1]) & (rows[:, 3] < want[:, 0])).any() and len({tuple(r[4:]) for r in rows}) > 1
        pair = torch.tensor([5, 8], dtype=torch.int64, device="cuda")
        hw2, rows2, _ = _geometry(ev, wb, we, n, 1, seed=21, step=99, first=1234, step_first=pair)
        assert np.array_equal(hw2, want) and np.array_equal(rows2, host)
        hw3, rows3, status = _geometry(ev, wb, we, n, 0)
        assert status == 0 and np.array_equal(hw3, want)
        assert np.array_equal(rows3, np.stack([0 * want[:, 0], 0 * want[:, 0], want[:, 1], want[:, 0], 0 * want[:, 0], 0 * want[:, 0]], 1))
    # the grow clips: the train window's extent is not the (longer) validation window's
    tw = _extents(_windows(samples, FIX, 21, 5, 8))
    assert (tw[[3, 10], 1] < want[[3, 10], 1]).any()
    # refused: x past the capacity / y past it / a negative coordinate / an empty window; the good windows beside them are untouched
    bad = [c.copy() for c in clips[:5]]
    bad[0][17, 0] = 64.0
    bad[1][299, 1] = 1e12
    bad[2][3, 0] = -1.0
    boff = np.concatenate([[0], np.cumsum([c.shape[0] for c in bad])]).astype(np.int64)
    beg, end = boff[:-1].copy(), boff[1:].copy()
    end[3] = beg[3]
    hw, rows, status = _geometry(torch.from_numpy(np.concatenate(bad, 0)).cuda(), torch.from_numpy(beg).cuda(), torch.from_numpy(end).cuda(), 5, 1,
                                 seed=3, step=1)
    assert status == 4, status
    assert hw.tolist() == [[48, 64], [48, 13], [30, 1], [1, 1], [37, 52]], hw.tolist()
    assert (rows[:, 0] >= 0).all() and (rows[:, 1] >= 0).all() and (rows[:, 2] >= 1).all() and (rows[:, 3] >= 1).all()
    assert (rows[:, 0] + rows[:, 2] <= hw[:, 1]).all() and (rows[:, 1] + rows[:, 3] <= hw[:, 0]).all()


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_train_chain_on_the_window_grids(mode):
    """Three replays with grid="window": chain.ext is numpy's extent of the host-picked windows; the crop rows read back are
    draw_evg_params_batch's on those extents; the raw grids (at the capacity) are the oracle's for the decisions read back, added rows
    bounded by (H_c, W_c), within the K1 bound, and exactly zero outside H_c x W_c; `out` EQUALS the restatement of the raw grids under
    the rows (nearest mode: held on the float64-cell relaunch on the chain's tables, as test_gpu_finetune_sensor_loader.py does, and the
    chain's float32 `out` within twice the K1 bound of it)."""
    from eventpretrain_amd.dataset.augmentation import view_augment as va
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    samples = _samples()
    loader = GpuFinetuneLoader(_args(resize_mode=mode), samples, batch_size=B, n_batches=3, is_train=True, seed=21, first_sample=8, step0=5,
                               grid="window", sensor=CAP)
    chain, fn = loader.chain, _restate(mode)
    assert chain.fused and chain.self_driven and chain.window and (loader.pipe.gh, loader.pipe.gw) == CAP and loader.pipe.scale == (1.0, 1.0)
    assert (chain.raw is not None and tuple(chain.raw.shape) == (B, 5) + CAP) if mode == "bilinear" else chain.raw is None
    assert tuple(chain.ext.shape) == (B, 2) and chain.ext.dtype == torch.int32 and int(chain.geom_status.item()) == 0
    n_aug, flips, worst, boxes, moved, k = 0, set(), 0.0, 0, 0, -1
    for k, batch in enumerate(loader):
        torch.cuda.synchronize()
        out = batch["events_voxel_grid"].cpu().numpy()
        assert out.shape == (B, 5, S, S)
        prm, dec = _plan(chain)
        wins = _windows(samples[B * k:B * k + B], FIX, 21, 5 + k, 8)
        hw = _extents(wins)
        assert np.array_equal(chain.ext.cpu().numpy(), hw), (k, hw.tolist())
        assert np.array_equal(prm, va.draw_evg_params_batch(21, 5 + k, B, hw[:, 0], hw[:, 1], 0.8, 8)), k
        raw = chain.raw.cpu().numpy() if mode == "bilinear" else _fused_f64(chain)
        view = out if mode == "bilinear" else _fused_f64(chain, prm)
        for c in range(B):
            what = (mode, k, c)
            Hc, Wc = (int(v) for v in hw[c])
            p = tuple(int(v) for v in prm[c])
            assert 0 <= p[0] and p[0] + p[2] <= Wc and 0 <= p[1] and p[1] + p[3] <= Hc and p[2] >= 1 and p[3] >= 1, what
            flips.add(p[4:])
            boxes += int(p[:4] != (0, 0, Wc, Hc))
            assert _padding_is_zero(raw[c], (Hc, Wc)), what
            assert np.array_equal(view[c], fn(raw[c], p, (S, S))), what
            assert float(np.abs(out[c] - view[c]).max()) <= 2 * K1_TOL, what
            n_aug += int(dec[c][0].size + dec[c][1].size > 0)
            moved += _moved(wins[c], dec[c], (Hc, Wc))
            err = float(np.abs(raw[c] - _oracle_grid(wins[c], dec[c], (Hc, Wc))).max())
            worst = max(worst, err)
            assert err <= K1_TOL, (what, err)
    print(f"{mode}: raw grids vs oracle max |err| {worst:.3e}, flip pairs {sorted(flips)}, {boxes} accepted boxes, {moved} added rows moved")
    assert k == 2 and loader.step == 8 and n_aug > 0 and len(flips) > 1 and boxes >= 1
    assert moved > 0                             # the oracle's added rows include some that only the per-clip bound moves


def _val_loader(samples, mode="bilinear", **kw):
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader
    return GpuFinetuneLoader(_args(resize_mode=mode, **kw), samples, batch_size=B, n_batches=3, is_train=False, seed=3, first_sample=2, step0=7,
                             grid="window", sensor=CAP)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_clean_validation_under_the_clips_full_boxes(mode):
    """Clean validation: the batch EQUALS the resize restatement under (0, 0, W_c, H_c, 0, 0) of voxel_grid_batch(..., algo=3) at the
    capacity on the host-picked windows, which is the oracle's padded grid within the K1 bound; a second pass gives the same bits."""
    from eventpretrain_amd.dataset.dataset_utils.events_to_voxel_grid import voxel_grid_batch
    samples = _samples(tag=1)
    loader, fn = _val_loader(samples, mode), _restate(mode)
    assert loader.chain is None and tuple(loader.raw.shape) == (B, 5) + CAP
    first = []
    for k, batch in enumerate(loader):
        first.append(batch["events_voxel_grid"].clone())
        got = first[-1].cpu().numpy()
        assert got.shape == (B, 5, S, S)
        wins = _windows(samples[B * k:B * k + B], VAL_FIX, 3, 7 + k, 2)
        hw = _extents(wins)
        assert np.array_equal(loader.ext.cpu().numpy(), hw), (k, hw.tolist())
        lens = [w.shape[0] for w in wins]
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        raw = voxel_grid_batch(torch.from_numpy(np.concatenate(wins, 0)).cuda(), off, 5, CAP, algo=3).cpu().numpy()
        for c in range(B):
            Hc, Wc = (int(v) for v in hw[c])
            assert np.array_equal(got[c], fn(raw[c], (0, 0, Wc, Hc, 0, 0), (S, S))), (mode, k, c)
            assert _padding_is_zero(raw[c], (Hc, Wc)), (mode, k, c)
            assert float(np.abs(raw[c] - _oracle_grid(wins[c], None, (Hc, Wc))).max()) <= K1_TOL, (mode, k, c)
        assert float(np.abs(got).sum()) > 0
    assert len(first) == 3 and loader.step == 10 and int(loader.geom_status.item()) == 0
    again = [b["events_voxel_grid"].clone() for b in loader]
    assert len(again) == 3 and all(torch.equal(x, y) for x, y in zip(first, again))


def test_noisy_validation_repeats_bit_for_bit():
    """--val_event_noise with grid="window": the chain with windows of 4000 rows, no view augmentation (the geometry kernel writes the clips'
    full boxes), float64 cells. The grids are the oracle's for the decisions read back, bounded per clip; the view is exact; two passes and
    a second loader give the same bits, the clean pass differs."""
    samples = _samples(tag=1)
    loader, fn = _val_loader(samples, val_event_noise=True), evg_bilinear
    chain = loader.chain
    assert chain is not None and chain.window and chain.algo == 3 and chain.fix == VAL_FIX and not loader.pipe.view_augment
    first, moved = [], 0
    for k, batch in enumerate(loader):
        torch.cuda.synchronize()
        first.append(batch["events_voxel_grid"].clone())
        got = first[-1].cpu().numpy()
        prm, dec = _plan(chain)
        wins = _windows(samples[B * k:B * k + B], VAL_FIX, 3, 7 + k, 2)
        hw = _extents(wins)
        assert np.array_equal(chain.ext.cpu().numpy(), hw)
        assert np.array_equal(prm, np.stack([0 * hw[:, 0], 0 * hw[:, 0], hw[:, 1], hw[:, 0], 0 * hw[:, 0], 0 * hw[:, 0]], 1))
        raw = chain.raw.cpu().numpy()
        for c in range(B):
            Hc, Wc = (int(v) for v in hw[c])
            moved += _moved(wins[c], dec[c], (Hc, Wc))
            assert _padding_is_zero(raw[c], (Hc, Wc)), (k, c)
            assert float(np.abs(raw[c] - _oracle_grid(wins[c], dec[c], (Hc, Wc))).max()) <= K1_TOL, (k, c)
            assert np.array_equal(got[c], fn(raw[c], (0, 0, Wc, Hc, 0, 0), (S, S))), (k, c)
    assert len(first) == 3 and moved > 0
    again = [b["events_voxel_grid"].clone() for b in loader]
    other = [b["events_voxel_grid"].clone() for b in _val_loader(samples, val_event_noise=True)]
    clean = [b["events_voxel_grid"].clone() for b in _val_loader(samples)]
    assert len(again) == len(other) == len(clean) == 3
    for x, y, z, w in zip(first, again, other, clean):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert any(not torch.equal(x, w) for x, w in zip(first, clean))


@pytest.mark.parametrize("kind", ["past the capacity", "negative", "empty"])
def test_pack_refuses_a_bad_window_before_upload(kind):
    samples = _samples(tag=2)
    e = samples[2][0].copy()
    if kind == "past the capacity":
        e[5, 0] = 64.0
    elif kind == "negative":
        e[5, 1] = -1.0
    else:
        e = e[:0]
    samples[2] = (e, 0, "the_bad_clip")
    loader = _val_loader(samples)
    with pytest.raises(ValueError, match="the_bad_clip"):
        for _ in loader:
            pass
    torch.cuda.synchronize()
    assert not loader.d_off.cpu().numpy().any() and not loader.ev.any() and loader.step == 7      # nothing was uploaded


def test_finetune_epoch_and_validation_on_the_ncars_recipe():
    """ft_train_one_epoch then ft_val over three-batch loaders built from ncars_recipe(args) (capacity 100 x 120 -> 224, ViT-Small, two
    classes, B = 2, bf16): finite stats, no acc5 for n-cars, and both executors on the model are captured graphs."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader, ncars_recipe
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, synthetic_events
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch, ft_val
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    a = _args(input_size=224, model_size="small", backbone_type="vit", num_classes=2, mask_ratio=0.0, fix_events_num=3000,
              clip_grad=None, smoothing=0, lr=1e-3, min_lr=1e-4, warmup_epochs=0, epochs=1)
    recipe = ncars_recipe(a)
    assert recipe == dict(grid="window", sensor=(100, 120))
    clips = lambda tag: [(synthetic_events(8000 + 10 * tag + i, 2500 + 900 * i, width=60 + 12 * i, height=40 + 12 * i), i % 2, f"car{tag}_{i}")
                         for i in range(6)]
    m = ft.finetune_cls_hub_model_small_patch16(a)
    det_fill_module_(m)
    m = m.cuda().train()
    train = GpuFinetuneLoader(a, clips(3), batch_size=2, n_batches=3, is_train=True, seed=4, **recipe)
    val = GpuFinetuneLoader(a, clips(4), batch_size=2, n_batches=3, is_train=False, seed=4, **recipe)
    assert tuple(train.chain.raw.shape) == tuple(val.raw.shape) == (2, 5, 100, 120) and val.chain is None
    ops.set_compute_dtype(torch.bfloat16)
    try:
        opt = FusedAdamW(lrd.param_groups_lrd(a, m, a.weight_decay, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
        stats = ft_train_one_epoch(a, m, train, opt, 0, NativeScalerWithGradNormCount())
        vstats = ft_val(a, m, val, 0)
    finally:
        ops.set_compute_dtype(torch.float32)
    print(stats, vstats)
    assert set(stats) == {"loss_cls", "lr"} and math.isfinite(stats["loss_cls"])
    assert set(vstats) == {"loss_cls", "acc1"} and all(math.isfinite(v) for v in vstats.values())
    step = m._evp_auto_executor[1]
    assert step.graph is not None and step.note == "hip-graph", step.note
    ev = m._evp_auto_eval[1]
    assert ev.graph is not None and ev.replays == 3 and ev.eager_calls == 0
    assert train.step == 3 and val.step == 3
    assert int(train.geom_status.item()) == 0 and int(val.geom_status.item()) == 0

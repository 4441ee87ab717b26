"""Event-count images (args.num_bins 2 and 3) on the GPU: the three kernels of csrc/evimage.hip against the integer restatement
(tests/count_image_truth.py, pinned to the reference's outputs by tests/test_count_image_host.py) with exact equality; GpuFinetuneLoader's
training, clean-validation and noisy-validation passes for an "input" and a "sensor" recipe against the restatements applied to the
chain's OWN merged clips under its own crop rows, bit for bit; repeatability; and a captured ViT-Small fine-tune step on loader output."""
import numpy as np
import pytest
import torch

from bilinear_truth import evg_bilinear
from conftest import load_golden
from count_image_truth import normalize, raw_image

pytestmark = pytest.mark.gpu

SENSOR, S, B, FIX, VAL_FIX = (45, 60), 32, 4, 400, 600


def _batch(clips, nb, size, scale=None, **kw):
    from eventpretrain_amd.dataset.dataset_utils.events_to_image import event_image_batch
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
    ev = torch.from_numpy(np.concatenate(clips, 0).reshape(-1, 4)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = event_image_batch(ev, torch.from_numpy(off).cuda(), nb, size, scale=scale, status=status, **kw)
    return out.cpu().numpy(), int(status.item())


def _four_clips(hw, n=150):
    """polarities {0, 1}, polarities {-1, 1}, positives only, no rows at all -- on integer pixel coordinates of an hw grid."""
    from eventpretrain_amd.testing import synthetic_events
    H, W = hw
    a = synthetic_events(1, n, width=W, height=H)
    b = synthetic_events(2, n + 13, width=W, height=H, signed_polarity=True)
    c = synthetic_events(3, n - 20, width=W, height=H)
    c[:, 3] = 1.0
    return [a, b, c, np.zeros((0, 4))]


@pytest.mark.parametrize("nb", [2, 3])
def test_count_and_finish_equal_the_truth(nb):
    """Four clips in one call on a 7 x 9 grid (no multiple of any tile): a row with x >= W that still lands inside (it wraps into the
    next row), ONE row outside the grid (status == 1), a row of another polarity (ignored); then fractional coordinates under a rescale,
    and clips long enough for several workgroups each."""
    clips = _four_clips((7, 9))
    clips[0][5] = (9.0, 2.0, clips[0][5, 2], 1.0)              # x == W: cell (3, 0)
    clips[0][6] = (11.5, 0.0, clips[0][6, 2], 0.0)             # cell (1, 2)
    clips[1][7] = (3.0, 7.0, clips[1][7, 2], -1.0)             # y == H: outside
    clips[2][8, 3] = 0.5                                       # neither 1, 0 nor -1
    got, status = _batch(clips, nb, (7, 9))
    outside = 0
    for c, ev in enumerate(clips):
        want, bad = raw_image(ev, nb, (7, 9))
        outside += bad
        assert np.array_equal(got[c], want), (nb, c)
    assert status == outside == 1 and not got[3].any() and got[0][0, 3, 0] > 0
    # the negative plane follows the clip: p == 0 rows where it has some, p == -1 rows otherwise
    assert got[1][-1].sum() > 0 and got[2][-1].sum() == 0
    # fractional coordinates under the sensor -> input rescale (24 x 32 -> 16 x 16), the product taken in float64 before the truncation
    from eventpretrain_amd.testing import synthetic_events
    frac = [synthetic_events(10 + i, 200, width=32, height=24, signed_polarity=bool(i & 1)) for i in range(3)]
    for i, ev in enumerate(frac):
        ev[:, 0] = np.minimum(ev[:, 0] + 0.37 * (i + 1), 31.999)
        ev[:, 1] = np.minimum(ev[:, 1] + 0.61, 23.999)
    scale = (16 / 32, 16 / 24)
    got, status = _batch(frac, nb, (16, 16), scale=scale)
    assert status == 0
    for c, ev in enumerate(frac):
        assert np.array_equal(got[c], raw_image(ev, nb, (16, 16), scale)[0]), (nb, c)
    # several workgroups per clip (4 rows per thread, 256 threads), clips of unequal length, one of them empty in the middle
    big = [synthetic_events(20, 5000, width=60, height=45), np.zeros((0, 4)), synthetic_events(21, 2300, width=60, height=45, signed_polarity=True)]
    got, status = _batch(big, nb, (45, 60), max_rows_per_clip=5000)
    again, _ = _batch(big, nb, (45, 60))
    assert status == 0 and np.array_equal(got, again)
    for c, ev in enumerate(big):
        assert np.array_equal(got[c], raw_image(ev, nb, (45, 60))[0]), (nb, c)


def test_hot_pixel_is_removed_and_the_largest_count_below_the_threshold_is_kept():
    g = load_golden("ft_count_images")
    kept = int(g["hot_kept"])
    got, status = _batch([g["hot_pre"], _four_clips((24, 32))[1]], 3, (24, 32))
    assert status == 0 and np.array_equal(got[0], g["hot_raw"])
    assert got[0][0, 1, 2] == 0 and got[0][2, 1, 2] == 0 and got[0][0, 4, 6] == np.float32(kept) / np.float32(255)
    assert np.array_equal(got[1], raw_image(_four_clips((24, 32))[1], 3, (24, 32))[0])
    # the single-clip forms with the reference's signatures
    from eventpretrain_amd.dataset.dataset_utils.events_to_image import events_to_image_ecdp, events_to_image_mem, remove_hot_pixel_mem
    two = events_to_image_ecdp(None, g["hot_pre"], (24, 32)).cpu().numpy()
    assert np.array_equal(two, raw_image(g["hot_pre"], 2, (24, 32))[0])
    mem = events_to_image_mem(None, g["hot_pre"][:, [2, 0, 1, 3]], (24, 32), is_txyp=True)
    assert np.array_equal(mem.cpu().numpy()[0::2], two) and not mem[1].any()
    assert np.array_equal(remove_hot_pixel_mem(mem / 255).cpu().numpy(), g["hot_raw"])


@pytest.mark.parametrize("nb", [2, 3])
def test_normalize_equals_the_truth_and_counts_empty_views(nb):
    """The reference's own views (72 x 72, 16 x 16 and 32 x 32 from the fixture), 7 x 9 images (a plane that is no multiple of four) and an
    all-zero view, with and without the guard: torch's bits, NaN where the reference divides by zero, and the count of empty views."""
    from eventpretrain_amd.dataset.dataset_utils.events_to_image import event_image_normalize_
    g = load_golden("ft_count_images")
    names = [str(n) for n in g["names"] if f"_{nb}_" in str(n) or str(n) == f"small_{nb}"]
    by_size = {}
    for n in names:
        by_size.setdefault(g[n + "_view"].shape[-1], []).append(g[n + "_view"])
    by_size[9] = [raw_image(ev, nb, (7, 9))[0] for ev in _four_clips((7, 9))[:3]]
    assert len(by_size) == 4
    for guard in (False, True):
        for views in by_size.values():
            x = np.stack(views + [np.zeros_like(views[0])])
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            got = event_image_normalize_(torch.from_numpy(x).cuda(), guard=guard, status=status).cpu().numpy()
            for i in range(x.shape[0]):
                want, _ = normalize(x[i], guard=guard)
                assert np.array_equal(got[i], want, equal_nan=True), (nb, guard, x.shape, i)
            assert int(status.item()) == (1 if nb == 3 else 0)
            if nb == 3:
                assert (not got[-1].any()) if guard else (np.isnan(got[-1][0::2]).all() and not got[-1][1].any())
            else:
                assert (got[-1] == -1).all()
            assert np.isfinite(got[:-1]).all()


# ---------------------------------------------------------------------------------------------------------------- the loader
def _args(**kw):
    from eventpretrain_amd.testing import make_args
    base = dict(phase="finetune_cls", crop_min=0.8, input_size=S, fix_events_num=FIX, val_fix_events_num=VAL_FIX, device="cuda",
                resize_mode="bilinear")
    base.update(kw)
    return make_args(**base)


def _samples(n, tag=0, sensor=SENSOR):
    from eventpretrain_amd.testing import synthetic_events
    sizes = [300, 900, 500, 600, 400, 777, 601, 399]
    out = []
    for i in range(n):
        ev = synthetic_events(9000 + 31 * tag + i, sizes[i % len(sizes)], width=sensor[1], height=sensor[0], signed_polarity=bool(i % 3 == 1))
        ev[::7, 0], ev[::7, 1] = 11.0, 17.0           # a busy pixel: the hot-pixel filter and the common max have something to do
        out.append((ev, (7 * i + 3 * tag) % 10, f"clip{tag}_{i}"))
    return out


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


def _expect(clip, row, pipe, mode):
    """The restatements on one merged clip: count -> (view under `row`, where the chain runs a view stage) -> normalise."""
    from oracle.augment_oracle import evg_transform
    raw, outside = raw_image(clip, pipe.bins, (pipe.gh, pipe.gw), pipe.scale)
    assert outside == 0
    if pipe.resize:
        raw = (evg_bilinear if mode == "bilinear" else evg_transform)(raw, tuple(int(v) for v in row), (S, S), negate=False)
    return normalize(raw, guard=pipe.norm_guard)[0]


def _chain_clips(chain):
    """The chain's own merged clips of its last replay: rows of chain.ev under the offsets tabs[4]; and its crop rows."""
    off = chain.d_tab[:5 * (B + 1)].view(5, B + 1)[4].cpu().numpy()
    ev = chain.ev.cpu().numpy()
    return [ev[off[c]:off[c + 1]] for c in range(B)], chain.crop_rows.cpu().numpy()


def _loader(kind, nb, is_train, samples, mode="bilinear", **kw):
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader, finetune_recipe
    prefix = {"n-imagenet": "img", "n-caltech101": "cal", "ucf101_dvs": "ucf"}[kind]
    a = _args(dataset_type=kind, num_bins=nb, resize_mode=mode, **{prefix + "_sensor_h": SENSOR[0], prefix + "_sensor_w": SENSOR[1]}, **kw)
    return GpuFinetuneLoader(a, samples, batch_size=B, n_batches=2, is_train=is_train, seed=13, first_sample=4, step0=6, **finetune_recipe(a))


@pytest.mark.parametrize("kind,nb,mode", [("n-imagenet", 2, "bilinear"), ("n-imagenet", 3, "nearest"), ("n-caltech101", 2, "nearest"),
                                          ("ucf101_dvs", 3, "bilinear")])
def test_loader_passes_equal_the_restatements_on_the_chains_own_clips(kind, nb, mode):
    """One training pass, one clean validation pass and one noisy validation pass per recipe ("input": N-ImageNet; "sensor": N-Caltech101
    with 2 channels, UCF101-DVS with 3 and the guard), B = 4, windows of 400 / 600 rows. Every output equals, bit for bit, count ->
    view -> normalise restated on the chain's own merged clips (chain.ev, tabs[4]) under its own crop rows (training) or the full box
    (validation); clean validation is restated on the host-picked windows. Passes and replays repeat bit for bit."""
    samples = _samples(2 * B, tag=nb)
    full = (0, 0, SENSOR[1], SENSOR[0], 0, 0)
    # training
    train = _loader(kind, nb, True, samples, mode)
    chain, pipe = train.chain, train.pipe
    assert chain is not None and not chain.fused and chain.self_driven and chain.ev is not None and pipe.count and pipe.bins == nb
    assert (pipe.gh, pipe.gw) == ((S, S) if kind == "n-imagenet" else SENSOR)
    flips, n_batches = set(), 0
    for k, batch in enumerate(train):
        torch.cuda.synchronize()
        out = batch["events_voxel_grid"].cpu().numpy()
        assert out.shape == (B, nb, S, S)
        clips, rows = _chain_clips(chain)
        wins = _windows(samples[B * k:B * k + B], FIX, 13, 6 + k, 4)
        for c in range(B):
            assert abs(clips[c].shape[0] - wins[c].shape[0]) < 0.01 * FIX and clips[c].shape[0] > 0, (k, c)
            assert np.array_equal(out[c], _expect(clips[c], rows[c], pipe, mode)), (kind, nb, "train", k, c)
            flips.add(tuple(int(v) for v in rows[c][4:]))
        n_batches, last = n_batches + 1, out
    assert n_batches == 2 and train.step == 8 and len(flips) > 1 and train.empty_views == 0
    # two replays of the training chain at the same state
    chain.set_state(7, 4)
    one = chain.run_next()[0].clone()
    chain.set_state(7, 4)
    two = chain.run_next()[0].clone()
    assert torch.equal(one, two) and np.array_equal(one.cpu().numpy(), last)
    # clean validation: no chain, the host-picked windows, view_resize alone
    val = _loader(kind, nb, False, samples, mode)
    assert val.chain is None and val.count
    first = []
    for k, batch in enumerate(val):
        got = batch["events_voxel_grid"].clone()
        first.append(got)
        wins = _windows(samples[B * k:B * k + B], VAL_FIX, 13, 6 + k, 4)
        for c in range(B):
            assert np.array_equal(got[c].cpu().numpy(), _expect(wins[c], full, val._clean_pipe, mode)), (kind, nb, "val", k, c)
    again = [b["events_voxel_grid"].clone() for b in val]
    assert len(first) == len(again) == 2 and all(torch.equal(x, y) for x, y in zip(first, again)) and val.empty_views == 0
    # noisy validation: the captured chain on validation windows, erase / add drawn, no view augmentation
    noisy = _loader(kind, nb, False, samples, mode, val_event_noise=True)
    chain = noisy.chain
    assert chain is not None and not chain.fused and chain.fix == VAL_FIX and not noisy.pipe.view_augment
    runs = []
    for k, batch in enumerate(noisy):
        torch.cuda.synchronize()
        got = batch["events_voxel_grid"].clone()
        runs.append(got)
        clips, _ = _chain_clips(chain)
        for c in range(B):
            assert np.array_equal(got[c].cpu().numpy(), _expect(clips[c], full, noisy.pipe, mode)), (kind, nb, "noisy", k, c)
    rerun = [b["events_voxel_grid"].clone() for b in noisy]
    assert len(runs) == 2 and all(torch.equal(x, y) for x, y in zip(runs, rerun))
    assert any(not torch.equal(x, y) for x, y in zip(runs, first))          # the erase / add reached the images


def test_loader_reports_rows_outside_the_grid_and_empty_views():
    """A row with y == H leaves the sensor's grid: the pass still hands out its batches, then raises ValueError (the reference raises in
    bincount / reshape). Clips without a row of polarity 1 / 0 / -1 give all-zero views: counted, zero under UCF101-DVS's guard, NaN
    without one."""
    samples = _samples(B, tag=5)
    bad = [(e.copy(), lab, n) for e, lab, n in samples]
    bad[0][0][3, 1] = float(SENSOR[0])                  # (clip 0 is shorter than the window: every row of it is uploaded)
    val = _loader("n-caltech101", 3, False, bad)
    val.n_batches = 1
    n = 0
    with pytest.raises(ValueError, match="1 event row"):
        for _ in val:
            n += 1
    assert n == 1 and val.image_status.tolist() == [0, 0]
    for kind, finite in (("ucf101_dvs", True), ("n-caltech101", False)):
        empty = [(e.copy(), lab, n) for e, lab, n in samples]
        for i in (0, 2):
            empty[i][0][:, 3] = 2.0
        val = _loader(kind, 3, False, empty)
        val.n_batches = 1
        outs = [b["events_voxel_grid"].clone() for b in val]
        assert len(outs) == 1 and val.empty_views == 2
        for i in range(B):
            if i in (0, 2):
                assert (not outs[0][i].any()) if finite else (torch.isnan(outs[0][i][0::2]).all() and not outs[0][i][1].any())
            else:
                assert torch.isfinite(outs[0][i]).all() and outs[0][i].abs().sum() > 0


@pytest.mark.parametrize("nb", [2, 3])
def test_captured_vit_small_step_on_loader_output(nb):
    """FtClsHubModel (ViT-Small, 224 x 224, f32) with num_bins 2 and 3 on GpuFinetuneLoader batches (N-Caltech101's recipe at 45 x 60):
    ft_train_one_epoch's captured step gives finite losses that equal the eager loop's (args.graph_step = False) from the same start,
    compared as test_gpu_round4.py::test_finetune_epoch_runs_captured_and_follows_the_eager_loop compares them."""
    import math
    from eventpretrain_amd import ops
    from eventpretrain_amd.dataset.finetune_cls.gpu_event_loader import GpuFinetuneLoader, finetune_recipe
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, make_args
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    from helpers import checksums
    ops.set_compute_dtype(torch.float32)

    def args(**kw):
        a = make_args(phase="finetune_cls", model_size="small", backbone_type="vit", num_classes=10, mask_ratio=0.0, device="cuda",
                      dataset_type="n-caltech101", clip_grad=None, smoothing=0.1, drop_path_rate=0.0, drop_rate=0.0, num_bins=nb, input_size=224,
                      fix_events_num=FIX, val_fix_events_num=VAL_FIX, resize_mode="bilinear", cal_sensor_h=SENSOR[0], cal_sensor_w=SENSOR[1], **kw)
        a.epochs, a.warmup_epochs, a.lr, a.min_lr = 4, 1, 1e-3, 1e-6
        return a

    a = args()
    loader = GpuFinetuneLoader(a, _samples(2 * B, tag=7), batch_size=B, n_batches=2, is_train=True, seed=2, **finetune_recipe(a))
    batches = [dict(events_voxel_grid=b["events_voxel_grid"].clone(), label=b["label"].clone(), image_name=b["image_name"]) for b in loader]
    assert len(batches) == 2 and tuple(batches[0]["events_voxel_grid"].shape) == (B, nb, 224, 224)
    assert all(torch.isfinite(b["events_voxel_grid"]).all() for b in batches)
    res = {}
    for mode in ("eager", "graph"):
        a = args()
        a.graph_step = mode == "graph"
        m = ft.finetune_cls_hub_model_small_patch16(a)
        det_fill_module_(m)
        m = m.cuda()
        opt = FusedAdamW(lrd.param_groups_lrd(a, m, 0.05, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
        st = [ft_train_one_epoch(a, m, batches, opt, ep, NativeScalerWithGradNormCount())["loss_cls"] for ep in range(2)]
        if mode == "graph":
            assert m._evp_auto_executor[1].note == "hip-graph"
        else:
            assert not hasattr(m, "_evp_auto_executor")
        res[mode] = (st, {k: checksums(p)[2] for k, p in m.named_parameters()}, {k: p.detach().abs().sum().item() for k, p in m.named_parameters()})
    assert all(math.isfinite(v) for v in res["graph"][0]), res["graph"][0]
    assert res["graph"][0] == pytest.approx(res["eager"][0], rel=2e-5)
    worst = max(abs(res["graph"][1][k] - v) / max(res["eager"][2][k], 1e-6) for k, v in res["eager"][1].items())
    assert worst <= 5e-6, worst

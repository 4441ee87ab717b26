"""The shipped loader chain (GpuEventLoader -> CapturedChain, self-driven, fused K1) against the CPU oracle.

The device's counter streams can never equal the reference's np.random, but every random decision the chain takes can be read back from
its device buffers (window rows, erase / add rows, noise, crop rows) and handed to oracle/augment_oracle.py + oracle/voxel_oracle.py,
which tests/test_oracle_golden.py pins to fixtures the reference produced. So each chain output here is a check of the device's data path
against the reference's: erase_and_add_events -> events_reshape -> events_to_voxel_grid -> evg_augment (+ frame_augment), and each
decision is checked to lie inside the reference's support."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOX_TOL, FRAME_TOL = 2e-5, 1e-5          # float32 LDS atomics in another order; the frame target's bicubic


def _oracle():
    from oracle import augment_oracle as ao
    from oracle.voxel_oracle import voxel_grid
    return ao, voxel_grid


def _clip(seed, n, sensor, offset=0.0, equal=False):
    from eventpretrain_amd.testing import synthetic_events
    H, W = sensor
    e = synthetic_events(seed, n, width=W, height=H)
    if equal:
        e[:, 2] = 0.0125
    e[:, 2] += offset
    return e


def _dev(x, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _oracle_rows(window, dec, sensor):
    """erase_add_apply of the oracle; `dec` = (erase rows, add rows, noise) or None."""
    ao, _ = _oracle()
    return ao.erase_add_apply(window, dec, sensor)


def _oracle_added(window, ai, nz, sensor):
    """The added rows as the reference builds them (events_augment.py:40-49): copy + noise, x / y clipped to the sensor, then the
    stable time sort erase_add_apply applies (added rows keep draw order among equal stamps)."""
    H, W = sensor
    add = window[ai].copy()
    add[:, :3] += nz
    add[:, 0] = np.clip(add[:, 0], 0, W - 1)
    add[:, 1] = np.clip(add[:, 1], 0, H - 1)
    return add[np.argsort(add[:, 2], kind="stable")]


def _oracle_view(rows, sensor, S, bins, params):
    ao, voxel_grid = _oracle()
    H, W = sensor
    g = voxel_grid(ao.events_reshape(rows, W, H, S, S), bins, (S, S))
    return ao.evg_transform(g, tuple(int(v) for v in params), (S, S), negate=bins in (5, 6))


def _read_back(chain):
    """One batch's decisions from the chain's device buffers."""
    nc = chain.nc
    d = chain.d_tab.cpu().numpy()
    tabs = d[:5 * (nc + 1)].reshape(5, nc + 1)
    pw = (nc * 6 + 1) // 2
    o4 = 5 * (nc + 1)
    prm = d[o4:o4 + pw].view(np.int32)[:nc * 6].reshape(nc, 6).copy()
    fprm = d[o4 + pw:o4 + 2 * pw].view(np.int32)[:nc * 6].reshape(nc, 6).copy() if chain.frames is not None else None
    return (tabs.copy(), prm, fprm, chain.er.cpu().numpy(), chain.ai.cpu().numpy(), chain.nz.cpu().numpy().reshape(-1, 3),
            chain.ws.cpu().numpy())


def _check_support(n, fix, s0, s1, er, ai, what):
    if n <= fix:
        assert (s0, s1) == (0, n), (what, n, s0, s1)
    else:
        assert 0 <= s0 < n - fix and s1 == s0 + fix, (what, n, s0, s1)      # randint(0, n - fix): the last start is never drawn
    nw = s1 - s0
    lo, hi = int(0.001 * nw), int(0.01 * nw)
    if hi == 0:
        assert er.size == 0 and ai.size == 0, what
    else:
        assert lo <= er.size < hi and lo <= ai.size < hi, (what, nw, er.size, ai.size)
    assert np.all(np.diff(er) > 0) and (er.size == 0 or (er[0] >= 0 and er[-1] < nw)), (what, er)     # distinct, ascending, in range
    assert np.unique(ai).size == ai.size and (ai.size == 0 or (ai.min() >= 0 and ai.max() < nw)), (what, ai)


# sensor (H, W), S, bins, n_clips, fix, frames, clip lengths (a ragged batch; "eq" = every stamp equal, "off" = stamps + 1.7e9)
CASES = [
    ((480, 640), 224, 5, 16, 3000, True,
     [0, 99, 150, ("eq", 150), 500, 3000, 3001, 15000, ("off", 9000), 1234, 2999, 4500, 6000, 100, 7777, 3002]),
    ((260, 346), 112, 6, 7, 15000, False, [15001, 0, ("eq", 150), 99, 500, 15000, 75000]),
    ((260, 346), 224, 3, 16, 100_000, True,
     [500_000, 100_000, 100_001, 0, 99, 150, ("eq", 150), 500, ("off", 120_000), 40_000, 70_000, 100, 150_000, 12_345, 99_999, 3000]),
    ((480, 640), 112, 10, 7, 3000, False, [3001, 15000, ("off", 3000), 0, 500, 99, ("eq", 150)]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_self_driven_chain_against_the_oracle(case):
    """A1 + A2: capture the self-driven fused chain, run 2-3 batches, read every decision back and rebuild each clip's augmented view
    (and frame target) with the oracle; the decisions must lie in the reference's support, the added rows equal the oracle's bit for bit.
    Then three altered oracles (one erased row left in, the window one row later, the crop one pixel over) must all be told apart."""
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    from eventpretrain_amd.testing import det_normalish, make_args
    ao, voxel_grid = _oracle()
    sensor, S, bins, nc, fix, with_frames, lens = CASES[case]
    H, W = sensor
    clips = []
    for i, spec in enumerate(lens):
        kind, n = spec if isinstance(spec, tuple) else ("", spec)
        clips.append(_clip(900 + 37 * case + i, n, sensor, offset=1.7e9 if kind == "off" else 0.0, equal=kind == "eq"))
    assert len(clips) == nc
    sizes = np.array([c.shape[0] for c in clips], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ev = _dev(np.concatenate(clips, 0), torch.float64)
    frames = None
    if with_frames:
        frames = torch.stack([det_normalish(f"chain_oracle.frame.{case}.{i}", (1, H, W)) for i in range(nc)]).cuda().contiguous()
    a = make_args(crop_min=0.8, input_size=S, num_bins=bins, fix_events_num=fix, img_sensor_w=W, img_sensor_h=H, device="cuda")
    pipe = GpuInputPipeline(a, seed=1000 + case)
    chain = pipe.capture(ev, nc, frames=frames, clip_offsets=off)
    assert chain.fused and chain.self_driven
    chain.set_state(40 + case, 16 * case)
    controls = None
    n_aug = 0
    for batch in range(3 if case % 2 else 2):
        vox, tgt = chain.run_next()
        torch.cuda.synchronize()
        vox = vox.cpu().numpy()
        tgt = None if tgt is None else tgt.cpu().numpy()
        tabs, prm, fprm, er_all, ai_all, nz_all, ws_all = _read_back(chain)
        for c in range(nc):
            what = (case, batch, c)
            s0, s1 = int(tabs[0, c] - off[c]), int(tabs[1, c] - off[c])
            er = er_all[tabs[2, c]:tabs[2, c + 1]]
            ai = ai_all[tabs[3, c]:tabs[3, c + 1]]
            nz = nz_all[tabs[3, c]:tabs[3, c + 1]]
            _check_support(int(sizes[c]), fix, s0, s1, er, ai, what)
            window = clips[c][s0:s1]
            dec = None if int(0.01 * (s1 - s0)) == 0 else (er, ai, nz)
            n_aug += int(dec is not None and (er.size + ai.size) > 0)
            assert np.array_equal(ws_all[tabs[3, c]:tabs[3, c + 1]], _oracle_added(window, ai, nz, sensor)), what
            rows = _oracle_rows(window, dec, sensor)
            want = _oracle_view(rows, sensor, S, bins, prm[c])
            err = float(np.abs(vox[c] - want).max())
            assert err <= VOX_TOL, (what, err)
            if tgt is not None:
                ft = ao.frame_transform(frames[c].cpu().numpy(), tuple(int(v) for v in fprm[c]), (S, S))
                assert float(np.abs(tgt[c] - ft).max()) <= FRAME_TOL, what
                assert fprm[c, 5] == prm[c, 5], what
            # A2, on the first batch: the longest clip, which has room to shift its window and rows to erase
            if batch == 0 and c == int(np.argmax(sizes)):
                controls = (c, window, s0, s1, er, ai, nz, prm[c].copy(), vox[c].copy())
    assert n_aug > 0
    # A2: each altered oracle differs from the device output by more than the tolerance
    c, window, s0, s1, er, ai, nz, p, got = controls
    assert sizes[c] > s1 and er.size >= 2
    x0, y0, w, h = (int(v) for v in p[:4])
    xs = (window[er, 0] * (S / W)).astype(np.int64)
    ys = (window[er, 1] * (S / H)).astype(np.int64)
    inside = np.nonzero((xs >= x0) & (xs < x0 + w) & (ys >= y0) & (ys < y0 + h) & (er > 0) & (er < window.shape[0] - 1))[0]
    assert inside.size, "no erased row inside the crop box"
    keep_one = np.delete(er, inside[0])
    alt_erase = _oracle_view(_oracle_rows(window, (keep_one, ai, nz), sensor), sensor, S, bins, p)
    shifted = clips[c][s0 + 1:s1 + 1]
    alt_window = _oracle_view(_oracle_rows(shifted, (er, ai, nz), sensor), sensor, S, bins, p)
    p2 = p.copy()
    p2[0] = x0 + 1 if x0 + w < S else x0 - 1
    alt_crop = _oracle_view(_oracle_rows(window, (er, ai, nz), sensor), sensor, S, bins, p2)
    for name, alt in (("erased row kept", alt_erase), ("window shifted", alt_window), ("crop x0 moved", alt_crop)):
        d = float(np.abs(got - alt).max())
        assert d > VOX_TOL, (name, d)


def _fused_abi(windows, er_l, ai_l, nz_l, sensor, bins, HW, max_window=None, view=None):
    """evp_events_build_added_f64 + evp_voxel_scatter_fused_f32 on explicit decisions (no view: the raw grids [n, bins, H, W])."""
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    Hs, Ws = sensor
    H, W = HW
    nc = len(windows)
    sizes = np.array([w.shape[0] for w in windows], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cum = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    e_off, a_off = cum(er_l), cum(ai_l)
    ev = _dev(np.concatenate(windows, 0) if sizes.sum() else np.zeros((1, 4)), torch.float64)
    d_wb, d_we, d_eo, d_ao = _dev(off[:-1]), _dev(off[1:]), _dev(e_off), _dev(a_off)
    d_er = _dev(np.concatenate(er_l + [np.zeros(1, np.int64)]).astype(np.int64))
    d_ai = _dev(np.concatenate(ai_l + [np.zeros(1, np.int64)]).astype(np.int64))
    d_nz = _dev(np.concatenate([z.reshape(-1, 3) for z in nz_l] + [np.zeros((1, 3))]).reshape(-1), torch.float64)
    kmax = int(np.diff(a_off).max())
    ws = torch.zeros(int(a_off[-1]) + 1, 4, dtype=torch.float64, device="cuda")
    call("evp_events_build_added_f64", ptr(ev), ptr(d_wb), nc, ptr(d_ai), ptr(d_nz), ptr(d_ao), kmax, float(Ws), float(Hs), ptr(ws), stream_ptr())
    out = torch.full((nc, bins, H, W), 7.0, device="cuda")
    kws = torch.zeros(nc * (bins + 5), dtype=torch.int64, device="cuda")
    mw = int(max(sizes.max(), 1)) if max_window is None else int(max_window)
    call("evp_voxel_scatter_fused_f32", ptr(ev), ptr(d_wb), ptr(d_we), nc, ptr(d_er), ptr(d_eo), ptr(ws), ptr(d_ao), mw, bins, H, W,
         W / Ws, H / Hs, None, 0, 0, 0, ptr(kws), ptr(out), stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws.cpu().numpy(), a_off


def _oracle_grid(window, dec, sensor, bins, HW):
    ao, voxel_grid = _oracle()
    Hs, Ws = sensor
    rows = ao.erase_add_apply(window, dec, sensor)
    return voxel_grid(ao.events_reshape(rows, Ws, Hs, HW[1], HW[0]), bins, HW)


@pytest.mark.parametrize("bins", [1, 2, 3, 5, 6, 10])
def test_fused_voxel_abi_edges_against_the_oracle(bins):
    """A3: the fused K1 fed explicit decisions at its edges, against erase_add_apply -> voxel_grid: integer stamps on bin boundaries
    (t1 - t0 a multiple of bins - 1: the division must floor exactly as a / dT does), the first and last rows erased, every row erased
    with and without added rows, added rows clipped at x = 0 and x = sensor_w - 1, and a grid whose width is not a multiple of 4 (the
    scalar store path of the no-view form)."""
    sensor = (260, 346)
    rng = np.random.default_rng(100 + bins)
    m = max(bins - 1, 1)
    wins, ers, ais, nzs = [], [], [], []

    def add(win, er, ai, nz):
        wins.append(win), ers.append(np.asarray(er, np.int64)), ais.append(np.asarray(ai, np.int64)), nzs.append(np.asarray(nz, np.float64).reshape(-1, 3))

    # (0) integer stamps 0 .. 8 m, 24 rows each: t1 - t0 = 8 (bins - 1), so ts = t / 8 lands exactly on every plane boundary
    n = (8 * m + 1) * 24
    win = np.zeros((n, 4))
    win[:, 0] = rng.integers(0, 346, n)
    win[:, 1] = rng.integers(0, 260, n)
    win[:, 2] = np.repeat(np.arange(8 * m + 1), 24).astype(np.float64)
    win[:, 3] = rng.integers(0, 2, n)
    ai = rng.choice(np.arange(30, n - 30), 6, replace=False)
    nz = np.zeros((6, 3))
    nz[:, :2] = rng.normal(0, 1.5, (6, 2))
    add(win, np.sort(rng.choice(np.arange(30, n - 30), 7, replace=False)), ai, nz)       # (t noise 0: t0 / t1 stay integers)
    # (1) the first and the last three rows erased
    win = _clip(11, 3000, sensor)
    er = np.unique(np.concatenate([[0, 1, 2, 2997, 2998, 2999], rng.choice(3000, 20, replace=False)]))
    ai = rng.choice(3000, 15, replace=False)
    add(win, er, ai, rng.normal(0, 1, (15, 3)) * [1.5, 1.5, 0.001])
    # (2) every row erased, rows added: t0 / t1 come from the added rows alone
    win = _clip(12, 400, sensor)
    ai = rng.choice(400, 4, replace=False)
    add(win, np.arange(400), ai, rng.normal(0, 1, (4, 3)) * [1.5, 1.5, 0.001])
    # (3) every row erased, nothing added: the grid is zero
    add(_clip(13, 300, sensor), np.arange(300), [], np.zeros((0, 3)))
    # (4) added rows pushed past x = 0 / x = W - 1 (and y = 0 / y = H - 1): clipped to the sensor
    win = _clip(14, 2000, sensor)
    lo_x, hi_x = np.argsort(win[:, 0], kind="stable")[[0, -1]]
    lo_y, hi_y = np.argsort(win[:, 1], kind="stable")[[0, -1]]
    ai = np.array([lo_x, hi_x, lo_y, hi_y, 1000])
    nz = np.array([[-9.0, 0.5, 0.0], [9.0, -0.5, 0.0], [0.3, -9.0, 0.0004], [0.0, 9.0, -0.0004], [0.25, 0.75, 0.0]])
    add(win, np.sort(rng.choice(2000, 12, replace=False)), ai, nz)
    # (5) an empty window beside them
    add(np.zeros((0, 4)), [], [], np.zeros((0, 3)))
    for HW in ((30, 37), (112, 112)):
        got, ws, a_off = _fused_abi(wins, ers, ais, nzs, sensor, bins, HW)
        for c in range(len(wins)):
            dec = (ers[c], ais[c], nzs[c])
            assert np.array_equal(ws[a_off[c]:a_off[c + 1]], _oracle_added(wins[c], ais[c], nzs[c], sensor)), (bins, HW, c)
            want = _oracle_grid(wins[c], dec, sensor, bins, HW)
            err = float(np.abs(got[c] - want).max())
            assert err <= VOX_TOL, (bins, HW, c, err)
        assert float(np.abs(got[3]).max()) == 0.0 and float(np.abs(got[5]).max()) == 0.0
        assert float(np.abs(got[2]).sum()) > 0
    x_added = ws[a_off[4]:a_off[5], 0]
    assert x_added.min() == 0.0 and x_added.max() == 345.0
    # the boundary case is a real one: some rows have ts exactly on an integer k in (0, bins - 1)
    if bins > 2:
        t = wins[0][:, 2]
        ts = (bins - 1) * (t - t.min()) / (t.max() - t.min())
        assert np.any((ts == np.floor(ts)) & (ts > 0) & (ts < bins - 1))


def test_fused_voxel_window_longer_than_max_window():
    """A3, last case: a window longer than `max_window` (the erased-row bitmap covers only the first max_window rows). The rows behind
    the bitmap are looked up in the ascending erase list, so the grid still equals the oracle's."""
    sensor = (480, 640)
    rng = np.random.default_rng(77)
    wins, ers, ais, nzs = [], [], [], []
    for i, n in enumerate((5000, 1024, 2100)):
        win = _clip(40 + i, n, sensor)
        er = np.unique(np.concatenate([rng.choice(n, 40, replace=False), [n - 1, n - 2]]))
        ai = rng.choice(n, 20, replace=False)
        wins.append(win), ers.append(er.astype(np.int64)), ais.append(ai.astype(np.int64))
        nzs.append(rng.normal(0, 1, (20, 3)) * [1.5, 1.5, 0.001])
    assert any((e >= 1024).sum() > 10 for e in ers)
    got, _, _ = _fused_abi(wins, ers, ais, nzs, sensor, 5, (112, 112), max_window=1024)
    for c in range(len(wins)):
        want = _oracle_grid(wins[c], (ers[c], ais[c], nzs[c]), sensor, 5, (112, 112))
        err = float(np.abs(got[c] - want).max())
        assert err <= VOX_TOL, (c, err)


def test_draw_kernel_top_up_keeps_the_erase_list_sorted():
    """A4: when the np2 candidates of a list hold fewer than k distinct rows, evp_events_draw_erase_add tops the list up with the
    smallest rows not drawn. The erase list must stay ascending (the fused K1 takes its first / last kept rows from that order), and
    both lists distinct and in range; the fused K1 fed that list equals the oracle."""
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    from eventpretrain_amd.dataset.augmentation import events_augment as ea
    n, k, seed, step = 48, 44, 7, 3
    want = k + 64 + k // 8
    np2 = 64
    while np2 < want:
        np2 <<= 1
    cands = lambda s, purpose: ((ea.philox_words(seed, step, [s], purpose, np2)[0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    sample = next((s for s in range(4096) if np.unique(cands(s, 1)).size < k and np.unique(cands(s, 2)).size < k), None)
    assert sample is not None, "no (seed, step, sample) with fewer than k distinct candidates in both lists"
    wb, we = _dev(np.array([0])), _dev(np.array([n]))
    eo, ao_ = _dev(np.array([0, k])), _dev(np.array([0, k]))
    er_d = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    ai_d = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    nz_d = torch.zeros(k * 3, dtype=torch.float64, device="cuda")
    call("evp_events_draw_erase_add", ptr(wb), ptr(we), 1, ptr(eo), ptr(ao_), seed, step, sample, None, k, ptr(er_d), ptr(ai_d), ptr(nz_d), stream_ptr())
    torch.cuda.synchronize()
    er, ai, nz = er_d.cpu().numpy(), ai_d.cpu().numpy(), nz_d.cpu().numpy().reshape(-1, 3)
    assert er.min() >= 0 and er.max() < n and np.unique(er).size == k, er
    assert np.all(np.diff(er) > 0), f"erase list not ascending: {er.tolist()}"
    assert ai.min() >= 0 and ai.max() < n and np.unique(ai).size == k, ai
    for got, purpose in ((er, 1), (ai, 2)):
        c = np.unique(cands(sample, purpose))                    # every distinct candidate, then the smallest rows never drawn
        rest = np.setdiff1d(np.arange(n), c)[:k - c.size]
        assert np.array_equal(np.sort(got), np.sort(np.concatenate([c, rest]))), purpose
    win = _clip(5, n, (480, 640))
    got, _, _ = _fused_abi([win], [er], [ai], [nz], (480, 640), 5, (224, 224))
    want = _oracle_grid(win, (er, ai, nz), (480, 640), 5, (224, 224))
    assert float(np.abs(got[0] - want).max()) <= VOX_TOL


def test_gpu_event_loader_covers_whole_clips():
    """A5: clips of up to 6 x fix_events_num through GpuEventLoader. The reference picks the window start uniformly over the WHOLE clip
    (pr_n_imagenet_dataset.py:82-83), so batch b must equal the self-driven chain run on the uncut clips at the same (seed, step,
    first sample) -- and windows late in a long clip must be reachable."""
    from eventpretrain_amd.dataset.pretrain.gpu_event_loader import GpuEventLoader
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    from eventpretrain_amd.testing import det_normalish, make_args
    B, S, fix = 4, 112, 3000
    a = make_args(crop_min=0.8, input_size=S, fix_events_num=fix, img_sensor_w=640, img_sensor_h=480, device="cuda")
    sizes = [18_000, 2_000, 17_500, 3_001, 12_000, 500, 16_000, 3_000]
    samples = [(_clip(700 + i, n, (480, 640)), det_normalish(f"loader_whole.frame.{i}", (1, 480, 640)), f"c{i}") for i, n in enumerate(sizes)]
    loader = GpuEventLoader(a, samples, batch_size=B, n_batches=2, seed=13, first_sample=4, frame_shape=(1, 480, 640), step0=9)
    got = [(b["events_voxel_grid"].clone(), b["sub_frame"].clone()) for b in loader]
    assert len(got) == 2 and loader.step == 11
    pipe = GpuInputPipeline(a, seed=13)
    for k in range(2):
        clips = [samples[B * k + i][0] for i in range(B)]
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int64)
        ev = _dev(np.concatenate(clips, 0), torch.float64)
        fr = torch.stack([samples[B * k + i][1] for i in range(B)]).cuda().contiguous()
        ch = pipe.capture(ev, B, frames=fr, clip_offsets=off)
        ch.set_state(9 + k, 4)
        v, t = ch.run_next()
        torch.cuda.synchronize()
        starts = (ch.d_tab[:B].cpu().numpy() - off[:-1]).tolist()
        err = float((got[k][0] - v).abs().max())
        assert err <= VOX_TOL and torch.equal(got[k][1], t), (k, err, starts)
    # some window of the run starts past 2 x fix (rows the old packing never uploaded)
    from eventpretrain_amd.dataset.augmentation import events_augment as ea
    late = 0
    for k in range(2):
        w0 = ea.philox_words(13, 9 + k, 4 + np.arange(B), 0, 1)[:, 0].astype(np.int64)
        for i in range(B):
            n = sizes[B * k + i]
            late += int(n > fix and (int(w0[i]) * (n - fix)) >> 32 > fix)        # the window ends past row 2 x fix
    assert late > 0


def test_device_draw_distributions():
    """A6: evp_events_draw_erase_add for 2048 clips of 1000 rows, 9 rows per list: the per-row inclusion counts of both lists are uniform
    (chi-square; rows 0 and n - 1 both occur), the noise columns are N(0, 1.5), N(0, 1.5), N(0, 0.001) (mean, standard deviation, KS).
    Fixed seeds: deterministic; thresholds at p ~ 1e-6."""
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    nc, n, k = 2048, 1000, 9
    wb = _dev(np.arange(nc) * n)
    we = _dev(np.arange(nc) * n + n)
    offs = _dev(np.arange(nc + 1) * k)
    er_d = torch.zeros(nc * k, dtype=torch.int64, device="cuda")
    ai_d = torch.zeros(nc * k, dtype=torch.int64, device="cuda")
    nz_d = torch.zeros(nc * k * 3, dtype=torch.float64, device="cuda")
    call("evp_events_draw_erase_add", ptr(wb), ptr(we), nc, ptr(offs), ptr(offs), 20240601, 17, 0, None, k, ptr(er_d), ptr(ai_d), ptr(nz_d), stream_ptr())
    torch.cuda.synchronize()
    from helpers import chi2_isf, normal_cdf
    thr = chi2_isf(1e-6, n - 1)
    for name, lst in (("erase", er_d.cpu().numpy()), ("add", ai_d.cpu().numpy())):
        per = lst.reshape(nc, k)
        assert per.min() >= 0 and per.max() < n and all(np.unique(r).size == k for r in per), name
        cnt = np.bincount(lst, minlength=n)
        expect = nc * k / n
        chi = float(((cnt - expect) ** 2 / expect).sum())
        assert chi < thr, (name, chi, thr)
        assert cnt[0] > 0 and cnt[n - 1] > 0, name
    nz = nz_d.cpu().numpy().reshape(-1, 3)
    N = nz.shape[0]
    ks_thr = math.sqrt(-math.log(1e-6 / 2) / (2 * N))
    for col, sd in enumerate((1.5, 1.5, 0.001)):
        x = nz[:, col]
        assert abs(x.mean()) <= 5 * sd / math.sqrt(N), (col, x.mean())
        assert abs(x.std() / sd - 1) <= 5 / math.sqrt(2 * N), (col, x.std())
        xs = np.sort(x) / sd
        cdf = normal_cdf(xs)
        i = np.arange(1, N + 1)
        D = max(float((i / N - cdf).max()), float((cdf - (i - 1) / N).max()))
        assert D < ks_thr, (col, D, ks_thr)

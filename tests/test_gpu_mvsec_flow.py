"""evp_mvsec_flow_propagate and GpuDenseLoader(gt_flow=...) on the GPU: the kernel against tests/mvsec_flow_truth.py (which
tests/test_mvsec_flow_host.py holds to the reference-made fixture) bit for bit -- every fixture case, one launch mixing the direct branch
with 2, 3 and 6 hops and a second sequence's base index, the sensor's own 260 x 346, a hop table that names no frame (skipped and
counted, nothing read through it), two launches -- and the loader fed timestamps against the same loader fed host-made labels.

The fixture's cv2.remap was a stand-in stating OpenCV's nearest rule (half to even) from its source: everything but that rule is pinned."""
import numpy as np
import pytest
import torch

import mvsec_flow_truth as truth
from conftest import load_golden

pytestmark = pytest.mark.gpu

MAX_HOPS = truth.MAX_HOPS


def _table(rows, max_hops=MAX_HOPS):
    """rows: [(frames, scales, n_hops)] with absolute frame indices -> the three device tensors."""
    B = len(rows)
    hf, hs, nh = np.zeros((B, max_hops), np.int64), np.zeros((B, max_hops), np.float64), np.zeros(B, np.int32)
    for b, (f, s, n) in enumerate(rows):
        hf[b, :len(f)], hs[b, :len(s)], nh[b] = f, s, n
    return tuple(torch.from_numpy(a).cuda() for a in (hf, hs, nh))


def _launch(frames, rows, out=None, status=None, max_hops=MAX_HOPS):
    from eventpretrain_amd.dataset.finetune_dense.mvsec_flow import mvsec_flow_propagate_batch
    d = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    hf, hs, nh = _table(rows, max_hops)
    if out is None:
        out = torch.full((len(rows), 2) + tuple(d.shape[2:]), 7.0, dtype=torch.float32, device="cuda")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
    mvsec_flow_propagate_batch(d, hf, hs, nh, out, status)
    torch.cuda.synchronize()
    return out, status


def _same_bits(got, want):
    want = np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def cases():
    """name -> (frames, flow_ts, t1, t2, the restatement's label as float32), computed once."""
    out = {}
    for name in truth.CASES:
        frames, ts, t1, t2 = truth.case_inputs(name)
        out[name] = (frames, ts, t1, t2, truth.label_f32(frames, ts, t1, t2))
    return out


def test_fixture_cases_bit_for_bit(cases):
    golden = load_golden("mvsec_gt_flow")
    for name, (frames, ts, t1, t2, want) in cases.items():
        out, status = _launch(frames, [truth.hops(ts, t1, t2)])
        got = out[0].cpu().numpy()
        assert status.item() == 0 and _same_bits(got, want), name
        assert _same_bits(got, golden[f"{name}|label"].astype(np.float32)), name          # (the reference's own output)


@pytest.mark.parametrize("d", truth.DTYPES)
def test_one_launch_mixes_branches_hop_counts_and_sequences(cases, d):
    """B = 5: n_hops 0, 2, 3, 6 and 4, every sample in a sequence of its own at base 10 * b of the concatenated frames."""
    names = [f"{k}.{d}" for k in ("F1_direct", "F2", "F3", "F6", "F4")]
    frames = np.concatenate([cases[n][0] for n in names], 0)
    rows = []
    for b, n in enumerate(names):
        f, s, k = truth.hops(*cases[n][1:4])
        rows.append((f + truth.N_SEQ * b, s, k))
    assert [r[2] for r in rows] == [0, 2, 3, 6, 4] and rows[4][0][0] == 4 * truth.N_SEQ + 2
    out, status = _launch(frames, rows)
    assert status.item() == 0
    for b, n in enumerate(names):
        assert _same_bits(out[b].cpu().numpy(), cases[n][4]), n
    again, _ = _launch(frames, rows)
    assert torch.equal(out, again)                                                       # two launches, equal bits


def test_sensor_size():
    """260 x 346, B = 2: three hops (more than one workgroup per sample, a last workgroup that is not full) and the direct branch."""
    from eventpretrain_amd.testing import det_uniform
    H, W = 260, 346
    frames = det_uniform("mvsec.gt.sensor", (4, 2, H, W), -8.0, 8.0).numpy()
    frames[:, :, 100:130, 200:260] = 0
    frames[1, 0, 5:9, 7] = 0.5
    ts = np.array([10.0, 10.05, 10.1, 10.15, 10.2])
    rows = [truth.hops(ts, 10.02, 10.13), truth.hops(ts, 10.16, 10.19)]
    assert [r[2] for r in rows] == [3, 0]
    out, status = _launch(frames, rows)
    assert status.item() == 0
    for b, r in enumerate(rows):
        want = truth.propagate(frames, *r)
        assert _same_bits(out[b].cpu().numpy(), want), b
    assert float(out[0].abs().max()) > 8.0 and int((out[0] == 0).sum()) > 30 * 60


def test_a_table_that_names_no_frame_is_skipped_and_counted(cases):
    frames, ts, t1, t2, want = cases["F3.f32"]
    f, s, n = truth.hops(ts, t1, t2)
    bad = f.copy()
    bad[1] = truth.N_SEQ                                    # == n_frames: one past the last frame
    out, status = _launch(frames, [(f, s, n), (bad, s, n)])
    assert status.item() == 1
    assert _same_bits(out[0].cpu().numpy(), want) and bool((out[1] == 7.0).all())        # the sentinel _launch filled: untouched
    neg = f.copy()
    neg[0] = -1
    out, status = _launch(frames, [(neg, s, n), (f, s, MAX_HOPS + 1), (f[:1], s[:1], 0)], status=status)
    assert status.item() == 3                               # accumulated: a negative frame, n_hops above max_hops
    assert bool((out[:2] == 7.0).all()) and _same_bits(out[2].cpu().numpy(), frames[f[0]].astype(np.float64) * s[0])


def test_wrapper_refusals(cases):
    from eventpretrain_amd._lib import EvpError
    from eventpretrain_amd.dataset.finetune_dense.mvsec_flow import mvsec_flow_propagate_batch
    frames = torch.from_numpy(cases["F2.f32"][0]).cuda()
    hf, hs, nh = _table([truth.hops(*cases["F2.f32"][1:4])])
    out, status = torch.zeros((1, 2) + truth.SHAPE, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for args in ((frames.half(), hf, hs, nh, out, status), (frames, hf.int(), hs, nh, out, status), (frames, hf, hs.float(), nh, out, status),
                 (frames, hf, hs, nh, out[:, :, :-1].contiguous(), status), (frames, hf, hs[:, :-1].contiguous(), nh, out, status),
                 (frames.cpu(), hf, hs, nh, out, status)):
        with pytest.raises(EvpError):
            mvsec_flow_propagate_batch(*args)


# ------------------------------------------------------------------------------------------------------------------ the loader
SENSOR, S, B = (20, 30), 32, 2


def _gt_sequences(dtype=np.float32):
    from eventpretrain_amd.testing import det_uniform
    H, W = SENSOR
    gt = {}
    for k, (name, n) in enumerate((("indoor_a", 7), ("indoor_b", 9))):
        f = det_uniform(f"mvsec.gt.loader.{name}", (n, 2, H, W), -2.5, 2.5).numpy().astype(dtype)
        f[:, :, 4:8, 10:16] = 0
        gt[name] = (f, 100.0 * (k + 1) + 0.05 * np.arange(n, dtype=np.float64))
    return gt


def _loader_samples(gt):
    """Four samples = two batches: direct, 2 hops, 3 hops in the second sequence, one frame as two hops."""
    from eventpretrain_amd.testing import synthetic_events
    ta, tb = gt["indoor_a"][1], gt["indoor_b"][1]
    stamps = [("indoor_a", ta[1] + 0.01, ta[1] + 0.04), ("indoor_b", tb[2] + 0.02, tb[3] + 0.02), ("indoor_b", tb[4] + 0.01, tb[6] + 0.03),
              ("indoor_a", ta[3], ta[3] + 0.04)]
    ev = [synthetic_events(900 + i, 1500 + 200 * i, width=SENSOR[1], height=SENSOR[0]) for i in range(len(stamps))]
    with_stamps = [(ev[i], (t1, t2), name) for i, (name, t1, t2) in enumerate(stamps)]
    with_labels = [(ev[i], truth.label_f32(gt[name][0], gt[name][1], t1, t2), name) for i, (name, t1, t2) in enumerate(stamps)]
    assert [truth.hops(gt[name][1], t1, t2)[2] for name, t1, t2 in stamps] == [0, 2, 3, 2]
    return with_stamps, with_labels


def _loader(samples, is_train, **kw):
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import GpuDenseLoader
    from eventpretrain_amd.testing import make_args
    a = make_args(phase="finetune_flow", crop_min=0.8, input_size=S, num_bins=5, fix_events_num=2000, val_fix_events_num=2000, device="cuda")
    return GpuDenseLoader(a, samples, B, 2, is_train, "flow", SENSOR, seed=11, first_sample=4, step0=3, max_events=4000, **kw)


def _pass(loader):
    seen = []
    for batch in loader:
        seen.append((batch["flow_label"].clone(), batch["flow_label_valid"].clone(), batch["events_voxel_grid"].clone(), list(batch["seq_name"])))
    torch.cuda.synchronize()
    return seen


@pytest.mark.parametrize("is_train", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_loader_from_timestamps_equals_loader_from_host_labels(is_train, dtype):
    gt = _gt_sequences(dtype)
    with_stamps, with_labels = _loader_samples(gt)
    mine = _loader(with_stamps, is_train, gt_flow=gt)
    assert mine.gt_frames.shape[0] == 16 and mine.gt_base == {"indoor_a": 0, "indoor_b": 7} and not hasattr(mine, "_pin_lab")
    got, want = _pass(mine), _pass(_loader(with_labels, is_train))
    assert len(got) == len(want) == 2
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) and g[3] == w[3], (is_train, k)
        # (training bins with float32 atomics, whose order is free: only validation's grids repeat bit for bit)
        assert is_train or torch.equal(g[2], w[2]), k
        assert 0.0 < float(g[1].mean()) < 1.0 and float(g[0].abs().max()) > 0.5                 # labels with valid and masked pixels
    if not is_train:
        again = _pass(mine)                                                                       # a second pass repeats bit for bit
        assert len(again) == 2 and all(torch.equal(x[i], y[i]) for x, y in zip(got, again) for i in range(3))
    assert mine.gt_status.item() == 0


def test_loader_refusals():
    gt = _gt_sequences()
    with_stamps, with_labels = _loader_samples(gt)
    with pytest.raises(ValueError, match=r"frames must be float32 or float64 \[F,2,20,30\]"):
        _loader(with_stamps, True, gt_flow={"indoor_a": (gt["indoor_a"][0][:, :, :-1], gt["indoor_a"][1])})
    with pytest.raises(ValueError, match="flow_ts must be float64"):
        _loader(with_stamps, True, gt_flow={"indoor_a": (gt["indoor_a"][0], gt["indoor_a"][1][:-1])})
    with pytest.raises(ValueError, match="one dtype for all"):
        _loader(with_stamps, True, gt_flow={"indoor_a": gt["indoor_a"], "indoor_b": (gt["indoor_b"][0].astype(np.float64), gt["indoor_b"][1])})
    with pytest.raises(ValueError, match="sequence 'indoor_b', gt_flow holds"):
        _pass(_loader(with_stamps, False, gt_flow={"indoor_a": gt["indoor_a"]}))
    late = [(with_stamps[0][0], (100.06, 100.31), "indoor_a")] + with_stamps[1:]               # (the sequence's last frame is at 100.3)
    with pytest.raises(ValueError, match="'indoor_a' ends at 100.31, at or after the sequence's last flow frame"):
        _pass(_loader(late, False, gt_flow=gt))
    with pytest.raises(ValueError, match="more than max_hops = 2"):
        _pass(_loader(with_stamps, False, gt_flow=gt, max_hops=2))
    with pytest.raises(ValueError, match="carries \\(image1_ts, image2_ts\\)"):
        _pass(_loader(with_labels, False, gt_flow=gt))
    # without gt_flow nothing changes: a pair of timestamps is no label
    with pytest.raises(ValueError, match="label must be float32"):
        _pass(_loader(with_stamps, False))

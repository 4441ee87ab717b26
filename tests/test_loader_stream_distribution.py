"""The device decision stream's distributions against the reference's (CPU).

The device plan and draw kernels are bit-equal to their numpy forms (philox_words, draw_erase_add_counts, draw_evg_params_batch: see
tests/test_gpu_round4.py), so checking those forms checks the device. What is checked here is that they draw what the reference draws
(get_random_index: randint(0, n - fix); erase_and_add_events: randint(int(0.001 n), int(0.01 n)); evg_augment's crop box and flip coins,
oracle/augment_oracle.draw_evg_params on a legacy RandomState). Fixed seeds; thresholds at p ~ 1e-6."""
import math

import numpy as np

from helpers import chi2_isf

from eventpretrain_amd.dataset.augmentation import events_augment as ea
from eventpretrain_amd.dataset.augmentation import view_augment as va
from oracle import augment_oracle as ao

P = 1e-6


def _chi2_uniform(values, lo, hi):
    cnt = np.bincount(values - lo, minlength=hi - lo)
    assert cnt.size == hi - lo, "a value outside [lo, hi)"
    e = values.size / (hi - lo)
    return float(((cnt - e) ** 2 / e).sum()), cnt


def _chi2_two_sample(a, b, min_count=10):
    """Two-sample chi-square on integer samples; rare values are pooled into one bin. -> (statistic, degrees of freedom)."""
    vals = np.union1d(a, b)
    ca = np.array([(a == v).sum() for v in vals], np.float64)
    cb = np.array([(b == v).sum() for v in vals], np.float64)
    small = (ca + cb) < min_count
    if small.any():
        ca = np.append(ca[~small], ca[small].sum())
        cb = np.append(cb[~small], cb[small].sum())
        keep = (ca + cb) > 0
        ca, cb = ca[keep], cb[keep]
    k1, k2 = math.sqrt(cb.sum() / ca.sum()), math.sqrt(ca.sum() / cb.sum())
    return float(((k1 * ca - k2 * cb) ** 2 / (ca + cb)).sum()), ca.size - 1


def _window_starts(seed, step, n, fix, count):
    """s0 as the plan (evp_events_plan_batch / GpuInputPipeline.draw) computes it: (w0 * (n - fix)) >> 32."""
    w0 = ea.philox_words(seed, step, np.arange(count), 0, 1)[:, 0].astype(np.uint64)
    return ((w0 * np.uint64(n - fix)) >> np.uint64(32)).astype(np.int64)


def test_window_start_is_uniform_over_the_room():
    fix = 3000
    for room, count in ((3, 20_000), (50, 100_000), (997, 200_000)):
        s0 = _window_starts(5, 11, fix + room, fix, count)
        assert s0.min() >= 0 and s0.max() < room, room                     # randint(0, n - fix): n - fix itself never
        chi, cnt = _chi2_uniform(s0, 0, room)
        assert chi < chi2_isf(P, room - 1), (room, chi)
        if room == 3:
            assert (cnt > 0).all()
    # the pipeline's host plan draws the same starts
    from eventpretrain_amd.dataset.pretrain.gpu_input_pipeline import GpuInputPipeline
    from eventpretrain_amd.testing import make_args
    pipe = GpuInputPipeline(make_args(fix_events_num=fix, input_size=32), seed=5)
    win = pipe.draw(np.full(4096, fix + 50), step=11)[0]
    assert np.array_equal(win[:, 0], _window_starts(5, 11, fix + 50, fix, 4096)) and np.array_equal(win[:, 1] - win[:, 0], np.full(4096, fix))
    assert np.array_equal(pipe.draw(np.array([fix, 17, 0]), step=11)[0], [[0, fix], [0, 17], [0, 0]])


def test_erase_and_add_counts_are_uniform_on_the_reference_range():
    for n in (150, 999, 1000, 15_000, 100_000):
        count = 200_000
        lo, hi = int(0.001 * n), int(0.01 * n)
        e, a = ea.draw_erase_add_counts(21, 4, np.full(count, n))
        for name, v in (("erase", e), ("add", a)):
            assert v.min() == lo and v.max() == hi - 1, (n, name, v.min(), v.max())      # both ends occur, hi never
            if hi - lo > 1:
                chi, _ = _chi2_uniform(v, lo, hi)
                assert chi < chi2_isf(P, hi - lo - 1), (n, name, chi)
        if hi - lo > 1:
            assert abs(np.corrcoef(e, a)[0, 1]) < 5 / math.sqrt(count), n      # two independent words of the stream
    e, a = ea.draw_erase_add_counts(21, 4, np.array([0, 50, 99]))
    assert not e.any() and not a.any()                                     # int(0.01 n) == 0: the reference leaves the clip alone


def _reference_params(seed, count, H, W):
    rs = np.random.RandomState(seed)
    return np.array([ao.draw_evg_params(rs, H, W, 0.8) for _ in range(count)], np.int64)


def _stream_params(seed, count, H, W):
    return va.draw_evg_params_batch(seed, 3, count, H, W, 0.8).astype(np.int64)


def test_crop_box_support_on_a_small_view():
    H, W = 10, 12
    ref = _reference_params(1, 30_000, H, W)
    ours = _stream_params(1, 300_000, H, W)
    for p in (ref, ours):
        full = (p[:, 2] == W) & (p[:, 3] == H)
        assert ((p[:, 2] < W) & (p[:, 3] < H) | full).all()
        assert (p[:, 0] >= 0).all() and (p[:, 1] >= 0).all()
        assert (p[~full, 0] < W - p[~full, 2]).all() and (p[~full, 1] < H - p[~full, 3]).all()
        assert (p[full, 0] == 0).all() and (p[full, 1] == 0).all()
    key = lambda p: p[:, 2] * 1000 + p[:, 3]
    sr, so = np.unique(key(ref)), np.unique(key(ours), return_counts=True)
    assert set(sr) <= set(so[0]), sorted(set(sr) - set(so[0]))
    frequent = set(so[0][so[1] / ours.shape[0] > 3e-4])               # expected >= 9 times in the reference's 30 000: missing it is ~1e-4
    assert frequent <= set(sr), sorted(frequent - set(sr))
    # every start the reference can draw for a box, the stream draws too (x0 in [0, W - w), y0 in [0, H - h))
    rx = set(map(tuple, ref[:, [0, 2]]))
    ox = set(map(tuple, ours[:, [0, 2]]))
    assert rx <= ox, sorted(rx - ox)


def test_crop_box_and_flips_follow_the_reference_distribution():
    S = 224
    ref = _reference_params(2, 20_000, S, S)
    ours = _stream_params(2, 100_000, S, S)
    for col, name in ((2, "w"), (3, "h")):
        chi, dof = _chi2_two_sample(ref[:, col], ours[:, col])
        assert chi < chi2_isf(P, dof), (name, chi, dof)
    for col, size, name in ((0, 2, "x0"), (1, 3, "y0")):
        rel = lambda p: np.where(p[:, size] < S, np.floor(10 * p[:, col] / np.maximum(S - p[:, size], 1)), -1).astype(np.int64)
        chi, dof = _chi2_two_sample(rel(ref), rel(ours))
        assert chi < chi2_isf(P, dof), (name, chi, dof)
    for col in (4, 5):
        for p in (ref, ours):
            assert abs(p[:, col].mean() - 0.5) < 5 * 0.5 / math.sqrt(p.shape[0]), (col, p[:, col].mean())

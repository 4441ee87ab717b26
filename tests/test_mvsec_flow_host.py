"""MVSEC's flow label on the host: tests/mvsec_flow_truth.py (the hop schedule + the per-pixel rule evp_mvsec_flow_propagate implements)
against tests/golden/mvsec_gt_flow.npz, which the reference's own gen_correspond_gt_flow made (tools/gen_mvsec_flow_golden.py) -- bit
for bit, at 13 x 17, F in {1 direct, 1 two-hop, 2, 2 at the edge t2 == ts[left + 1], 3, 4, 6}, float32 and float64 frames; the package's
mvsec_flow_hops against the frames and scales the reference's prop_flow was called with; its ValueErrors; and five named mutations of the
rule, each of which must fail the fixture (so the fixture tells them apart).

The fixture was made with a stand-in for cv2.remap that states OpenCV's nearest rule (cvRound, half to even) as read from its source: it
pins everything but that rule."""
import numpy as np
import pytest

import mvsec_flow_truth as truth
from conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    g = load_golden("mvsec_gt_flow")
    assert [str(c) for c in g["cases"]] == truth.CASES
    return g


@pytest.fixture(scope="module")
def inputs():
    return {name: truth.case_inputs(name) for name in truth.CASES}


def _propagated(golden):
    return [n for n in truth.CASES if int(golden[f"{n}|n_hops"]) > 0]


def test_restatement_equals_the_reference_bit_for_bit(golden, inputs):
    seen = set()
    for name in truth.CASES:
        frames, ts, t1, t2 = inputs[name]
        want = golden[f"{name}|label"]
        got = truth.label(frames, ts, t1, t2)
        assert got.dtype == want.dtype and got.shape == want.shape == (2,) + truth.SHAPE, name
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, float(np.abs(got.astype(np.float64) - want).max()))
        n = int(golden[f"{name}|n_hops"])
        assert want.dtype == (np.float32 if n else frames.dtype), name          # the direct branch keeps the frames' dtype
        seen.add((int(np.diff(golden[f"{name}|slice"])[0]), n))
    # (frames sliced, hops): one frame direct and as two hops, two frames direct (the edge) and propagated, 3, 4, 6
    assert seen == {(1, 0), (1, 2), (2, 0), (2, 2), (3, 3), (4, 4), (6, 6)}


def test_cases_hold_what_they_are_meant_to(golden, inputs):
    """Each propagated case: a zero in one plane only (both ways), pixels leaving on the first hop and (3 hops and more) on a later one,
    a first or last scale of exactly 1 somewhere, ties of both parities wherever the first scale is exact."""
    ones = 0
    for name in _propagated(golden):
        frames, ts, t1, t2 = inputs[name]
        stats = {}
        truth.label(frames, ts, t1, t2, stats=stats)
        n = int(golden[f"{name}|n_hops"])
        assert stats["zero_x_only"] > 0 and stats["zero_y_only"] > 0 and stats["left_first"] > 0, (name, stats)
        assert n < 3 or stats["left_later"] > 0, (name, stats)
        if truth.case_times(name.split(".")[0])[3] is not None:
            assert stats["tie_even"] > 0 and stats["tie_odd"] > 0, (name, stats)
        scales = golden[f"{name}|hop_scales"]
        ones += int(scales[0] == 1.0 or scales[-1] == 1.0)
    assert ones >= 4
    # the edge: t2 == ts[left + 1] is counted by searchsorted('right'), two frames are sliced, and the branch test still says direct
    _, ts, t1, t2 = inputs["F2_edge_direct.f32"]
    left, right = truth.flow_slice(ts, t1, t2)
    assert right - left == 2 and t2 == ts[left + 1] and int(golden["F2_edge_direct.f32|n_hops"]) == 0


def test_hops_equal_what_the_reference_was_called_with(golden, inputs):
    from eventpretrain_amd.dataset.finetune_dense.mvsec_flow import MAX_HOPS, mvsec_flow_hops
    assert MAX_HOPS == truth.MAX_HOPS == 8
    for name in truth.CASES:
        _, ts, t1, t2 = inputs[name]
        want_f, want_s, want_n = golden[f"{name}|hop_frames"], golden[f"{name}|hop_scales"], int(golden[f"{name}|n_hops"])
        for who, (frames, scales, n) in (("truth", truth.hops(ts, t1, t2)), ("package", mvsec_flow_hops(ts, t1, t2, name=name))):
            rows = max(n, 1)
            assert n == want_n and frames.dtype == np.int64 and scales.dtype == np.float64, (who, name)
            assert np.array_equal(frames[:rows], want_f) and np.array_equal(scales[:rows].view(np.int64), want_s.view(np.int64)), (who, name)
        assert frames.shape == scales.shape == (MAX_HOPS,) and not frames[rows:].any() and not scales[rows:].any()


def test_schedule_refusals(inputs):
    from eventpretrain_amd.dataset.finetune_dense.mvsec_flow import mvsec_flow_hops
    _, ts, t1, t2 = inputs["F6.f32"]
    assert mvsec_flow_hops(ts, t1, t2, 6)[2] == 6
    with pytest.raises(ValueError, match="'day1_17' spans 6 flow frames = 6 hops, more than max_hops = 5"):
        mvsec_flow_hops(ts, t1, t2, 5, name="day1_17")
    with pytest.raises(ValueError, match="more than max_hops = 1"):           # the one-frame form takes two hops
        mvsec_flow_hops(ts, ts[3], ts[3] + 0.01, 1)
    with pytest.raises(ValueError, match="'s' starts at .* before the sequence's first flow frame"):
        mvsec_flow_hops(ts, ts[0] - 0.001, ts[1], name="s")
    for end in (ts[-1], ts[-1] + 1.0):                                          # right == len(ts): the reference's third assert
        with pytest.raises(ValueError, match="at or after the sequence's last flow frame"):
            mvsec_flow_hops(ts, ts[-3], end)
    with pytest.raises(ValueError, match="before it starts"):
        mvsec_flow_hops(ts, ts[4] + 0.01, ts[3])
    with pytest.raises(ValueError, match="float64"):
        mvsec_flow_hops(ts.astype(np.float32), t1, t2)
    assert mvsec_flow_hops(ts, ts[0], ts[-1] - 0.001, 16)[2] == len(ts) - 1      # the whole sequence, first frame on: fine


@pytest.mark.parametrize("variant", truth.MUTATIONS)
def test_each_mutation_fails_the_fixture(golden, inputs, variant):
    """half_away: round half away from zero; x_first: x updated before y's plane is sampled; shared_mask: one flag for both components;
    f32_product: flow * float32(scale) and a float32 sum; fma: x + a * s rounded once (exact rational arithmetic)."""
    order = sorted(_propagated(golden), key=lambda n: not n.startswith("F3"))      # (F3 holds the planted double-rounding case: first)
    failed = []
    for name in order:
        frames, ts, t1, t2 = inputs[name]
        if not np.array_equal(truth.label(frames, ts, t1, t2, variant=variant), golden[f"{name}|label"]):
            failed.append(name)
            if variant == "fma":
                break                                                            # (exact arithmetic per pixel: one case is enough)
    print(variant, "fails", failed)
    assert failed, f"the fixture does not tell {variant!r} from the rule"

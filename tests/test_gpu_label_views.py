"""evp_semseg_label_augment and evp_flow_label_augment_f32 on the GPU against tests/dense_input_truth.py (which equals the reference's
functions, tests/test_dense_input_host.py): EQUAL, at B = 3 with a row of its own per sample -- the full box, an accepted box of the
fixture, a hand-made box touching the bottom-right corner -- for 11 x 14 -> 11 x 14, 5 x 300 -> 5 x 300 (two 256-wide x blocks) and
26 x 35 -> 13 x 50 (a real size change in both directions), both values of both flips, labels holding 255, flows holding exact zeros,
+-1000, 999.99994 and 1e-6 next to a zero component; crop rows as a host array and as a device tensor; the host-side box check."""
import numpy as np
import pytest
import torch

import dense_input_truth as truth
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASES = [(0, (11, 14), (11, 14)), (1, (5, 300), (5, 300)), (3, (26, 35), (13, 50))]      # (fixture shape index, in, out)
B = 3


def _rows(i, hw, hflip, tflip):
    H, W = hw
    fx = load_golden("dense_label_views")[f"rows_{i}"]
    accepted = next(r for r in fx if tuple(r[:4]) != (0, 0, W, H))
    bw, bh = max(W // 2, 1), max(H - 2, 1)
    return np.asarray([(0, 0, W, H, hflip, tflip), tuple(accepted), (W - bw, H - bh, bw, bh, 1 - hflip, 1 - tflip)], np.int32)


def _inputs(hw):
    H, W = hw
    lab = np.stack([np.roll(truth.label_input(H, W), 3 * b, axis=-1) for b in range(B)])
    flow = np.stack([np.roll(truth.flow_input(H, W), 3 * b, axis=-1) for b in range(B)])
    assert lab.max() == 255 and (flow == 0).any() and (np.abs(flow) == 1000).any() and (flow == truth.F32_BELOW_1000).any()
    assert ((np.abs(flow[:, 0]) == np.float32(1e-6)) & (flow[:, 1] == 0)).any()
    return lab, flow


@pytest.mark.parametrize("i,hw,out_hw", CASES)
@pytest.mark.parametrize("on_device", [False, True])
def test_label_views_equal_the_truth(i, hw, out_hw, on_device):
    from eventpretrain_amd.dataset.augmentation.view_augment import flow_label_augment_batch, semseg_label_augment_batch
    lab, flow = _inputs(hw)
    d_lab, d_flow = torch.from_numpy(lab).cuda(), torch.from_numpy(flow).cuda()
    seen_valid = set()
    for hflip in (0, 1):
        for tflip in (0, 1):
            rows = _rows(i, hw, hflip, tflip)
            prm = torch.from_numpy(rows).cuda() if on_device else rows
            got_lab = semseg_label_augment_batch(d_lab, prm, out_hw)
            got_flow, got_valid = flow_label_augment_batch(d_flow, prm, out_hw)
            assert got_lab.dtype == torch.int64 and tuple(got_lab.shape) == (B, 1) + out_hw
            assert got_flow.dtype == got_valid.dtype == torch.float32 and tuple(got_flow.shape) == (B, 2) + out_hw and tuple(got_valid.shape) == (B, 1) + out_hw
            got_lab, got_flow, got_valid = got_lab.cpu().numpy(), got_flow.cpu().numpy(), got_valid.cpu().numpy()
            for b in range(B):
                what = (hw, out_hw, tuple(rows[b]))
                assert np.array_equal(got_lab[b], truth.semseg_label_view(lab[b], rows[b], out_hw)), what
                want_flow, want_valid = truth.flow_label_view(flow[b], rows[b], out_hw)
                assert np.array_equal(got_flow[b], want_flow), what
                assert np.array_equal(got_valid[b], want_valid), what
                seen_valid.update(np.unique(got_valid[b]).tolist())
            if hw == out_hw:                  # the full box at equal size: the label only widens, the flow keeps its values up to the flips' signs
                assert np.array_equal(got_lab[0], lab[0][..., ::-1] if hflip else lab[0])
                assert np.array_equal(np.abs(got_flow[0]), np.abs(flow[0][..., ::-1] if hflip else flow[0]))
    assert seen_valid == {0.0, 1.0}


def test_outputs_may_be_given_and_are_checked():
    from eventpretrain_amd.dataset.augmentation.view_augment import flow_label_augment_batch, semseg_label_augment_batch
    hw = (11, 14)
    lab, flow = _inputs(hw)
    d_lab, d_flow = torch.from_numpy(lab).cuda(), torch.from_numpy(flow).cuda()
    rows = _rows(0, hw, 1, 0)
    out = torch.full((B, 1) + hw, -7, dtype=torch.int64, device="cuda")
    assert semseg_label_augment_batch(d_lab, rows, hw, out=out) is out and int(out.min()) >= 0
    f, v = torch.zeros(B, 2, *hw, device="cuda"), torch.full((B, 1) + hw, 5.0, device="cuda")
    assert flow_label_augment_batch(d_flow, rows, hw, out=f, valid_out=v)[1] is v and float(v.max()) == 1.0
    with pytest.raises(ValueError, match="out must be"):
        semseg_label_augment_batch(d_lab, rows, hw, out=out.int())
    with pytest.raises(ValueError, match="out must be"):
        flow_label_augment_batch(d_flow, rows, hw, valid_out=torch.zeros(B, 2, *hw, device="cuda"))


def test_host_side_box_check_raises():
    from eventpretrain_amd.dataset.augmentation.view_augment import flow_label_augment_batch, semseg_label_augment_batch
    hw = (11, 14)
    lab, flow = _inputs(hw)
    d_lab, d_flow = torch.from_numpy(lab).cuda(), torch.from_numpy(flow).cuda()
    for bad in ((0, 0, 15, 11, 0, 0), (1, 0, 14, 11, 0, 0), (0, 2, 14, 10, 0, 0), (-1, 0, 4, 4, 0, 0), (0, 0, 0, 4, 0, 0)):
        rows = _rows(0, hw, 0, 0)
        rows[1] = bad
        with pytest.raises(ValueError, match="semseg_label_augment_batch: crop box outside the view"):
            semseg_label_augment_batch(d_lab, rows, hw)
        with pytest.raises(ValueError, match="flow_label_augment_batch: crop box outside the view"):
            flow_label_augment_batch(d_flow, rows, hw)
    with pytest.raises(ValueError, match="params must be int32"):
        semseg_label_augment_batch(d_lab, torch.zeros(B, 6, dtype=torch.int64, device="cuda"), hw)

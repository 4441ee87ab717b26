"""Host checks of the optical-flow objective's truth (tests/flow_truth.py): the float64 restatement equals what the reference's own
resize_flow / FlowLoss / flow_compute_aee_outlier recorded (tests/golden/ft_flow_objective.npz, tools/gen_flow_golden.py); every named
mutant of the restatement fails the comparator the GPU test uses; the input conditions of the GPU cases hold; the plain metric
functions equal the fixture; the new entry points are declared, exported and bound and refuse bad arguments without a device."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import pytest
import torch

import flow_truth as ft
from conftest import ROOT, jload, load_golden


@pytest.fixture(scope="module")
def fixture():
    return load_golden("ft_flow_objective")


def _truth(name, **kw):
    s = ft.CASES[name]
    inputs = ft.case_inputs(name, **{k: kw.pop(k) for k in ("all_invalid", "no_events") if k in kw})
    return ft.truth(inputs[0], s["B"], s["h"], s["w"], *inputs[1:], s["max_flow"], **kw)


@pytest.fixture(scope="module")
def truths():
    return {name: _truth(name) for name in ft.CASES}


def _close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return bool(((a - b).abs() <= tol * b.abs().max()).all())


def test_fixture_lists_the_cases(fixture):
    assert jload(fixture["cases"]) == list(ft.CASES)


@pytest.mark.parametrize("name", list(ft.CASES))
def test_restatement_equals_the_reference(name, fixture, truths):
    t = truths[name]
    f = {k: torch.from_numpy(fixture[f"{name}|{k}"]) for k in ("l1", "grad_l1", "aee", "outlier", "n_sparse")}
    assert _close(t["l1"], f["l1"], 1e-12) and _close(t["aee"], f["aee"], 1e-12)
    assert int(f["n_sparse"]) == t["n_sparse"] > 0
    # the reference's outlier share goes through .float(): a count over a count, then times 100, in float32
    assert _close(t["outlier"], f["outlier"], ft.REL_PERCENT)
    assert round(float(f["outlier"]) / 100.0 * t["n_sparse"]) == t["n_outlier"]
    # the upstream weights scale the one recorded gradient
    for g, grad in t["grad"].items():
        assert _close(grad, g * f["grad_l1"], 1e-12)


def test_truth_passes_its_own_comparator_in_float64_and_float32(truths):
    for name in ft.CASES:
        assert ft.compare(ft.as_got(truths[name]), truths[name]) == []
        assert ft.compare(ft.as_got(_truth(name, dtype=torch.float32)), truths[name]) == [], name


@pytest.mark.parametrize("mut", ft.MUTANTS)
def test_mutants_fail_the_comparator(mut, truths):
    """Each mutant in at least one case, and there in the quantity it spoils. The two scale mutants cannot show in `ident`, whose
    factors are 1."""
    want = dict(scale_swapped="l1", no_scale="l1", valid_nonzero_in_loss="l1", no_max_flow="l1", mean_over_pixels="l1",
                max_flow_in_metrics="aee", valid_ge_half_in_metrics="aee", outlier_or="outlier", events_mask_ignored="aee")[mut]
    caught = {name: ft.compare(ft.as_got(_truth(name, mut=mut)), truths[name]) for name in ft.CASES}
    assert any(caught.values()), mut
    assert any(b.startswith(want) for bad in caught.values() for b in bad), (mut, caught)
    if mut in ("scale_swapped", "no_scale"):
        assert caught["ident"] == [] and caught["slice"] and caught["odd"]
    if want == "l1":      # the loss mutants move the gradient too
        assert any(b.startswith("grad") for b in caught["slice"])
    if mut == "outlier_or":
        assert all(b.startswith("outlier") for b in caught["slice"])


def test_input_conditions_of_the_gpu_cases(truths):
    for name, s in ft.CASES.items():
        flow_map, target, valid, org = ft.case_inputs(name)
        t = truths[name]
        B, h, w, H, W = (s[k] for k in ("B", "h", "w", "H", "W"))
        assert tuple(flow_map.shape) == (B * h * w, 2) and s["ld"] == (2 if name == "ident" else 8)
        assert tuple(target.shape) == (B, 2, H, W) and tuple(valid.shape) == (B, 1, H, W) and tuple(org.shape) == (B, s["E"], H, W)
        assert all(x.dtype == torch.float32 for x in (flow_map, target, valid, org))
        # no component next to its prediction (one flipped sign breaks the gradient bound): share 0
        p, t64 = ft.resize_flow(flow_map.double(), B, h, w, H, W), target.double()
        assert int(((p - t64).abs() <= ft.TIE * torch.maximum(p.abs(), t64.abs())).sum()) == 0, name
        # no magnitude next to max_flow, a visible share above it
        mag = t64.pow(2).sum(1).sqrt()
        assert int(((mag - s["max_flow"]).abs() <= ft.NEAR_MAX_FLOW * s["max_flow"]).sum()) == 0, name
        assert 0.1 < (mag >= s["max_flow"]).double().mean().item() < 0.5, name
        assert set(valid.unique().tolist()) <= set(ft.VALID_LEVELS)
        if H * W > 100:
            assert set(valid.unique().tolist()) == set(ft.VALID_LEVELS)
        # about half of the pixels carry no event; the others carry values of at least 1e-3
        empty = (org == 0).all(1)
        assert 0.3 < empty.double().mean().item() < 0.7, name
        assert bool(((org != 0).all(1) | empty).all()) and org[org != 0].abs().min().item() >= 1e-3
        assert t["n_valid"] > 0 and t["n_sparse"] > 0 and t["n_unsure"] <= ft.MAX_UNSURE * t["n_sparse"], (name, t["n_unsure"])
        assert t["n_outlier_sure"] <= t["n_outlier"] <= t["n_outlier_sure"] + t["n_unsure"]
        # both outlier conditions are live: epe straddles 3.0 and epe / mag 0.05 over the sparse pixels of the larger cases
        if H * W > 100:
            sm = ft.sparse_mask(target, valid, org, s["max_flow"])
            epe, m = (p - t64).pow(2).sum(1).sqrt()[sm], mag[sm]
            for cond in (epe > 3.0, epe / m > 0.05):
                assert 0.1 < cond.double().mean().item() < 0.9, name
    s = ft.CASES["slice"]
    assert s["W"] * s["h"] != s["H"] * s["w"]                                      # x and y factors differ
    s = ft.CASES["odd"]
    assert float(torch.tensor(s["W"] / s["w"])) != s["W"] / s["w"]                 # 45 / 7 is not a float32
    _, _, valid, _ = ft.case_inputs("odd")
    assert bool((valid[1] == 0).all()) and bool((valid[0] >= 0.5).any())
    # downsampling leaves cells without a pixel: their gradient is exactly zero in the truth
    g = truths["down"]["grad"][1.0]
    assert int((g.abs().sum(1) == 0).sum()) > 0 and int((g.abs().sum(1) != 0).sum()) > 0


def test_degenerate_batches_in_the_truth():
    """No valid pixel: a NaN loss whose gradient is exactly zero (autograd scatters nothing), while the sparse mask -- valid NON-ZERO --
    still has pixels. No event: NaN aee and outlier."""
    t = _truth("slice", all_invalid=True)
    assert t["l1"] != t["l1"] and t["n_valid"] == 0 and t["n_sparse"] > 0 and float(t["aee"]) == float(t["aee"])
    assert all(bool((g == 0).all()) for g in t["grad"].values())
    t = _truth("slice", no_events=True, need_grad=False)
    assert t["n_sparse"] == 0 and t["aee"] != t["aee"] and t["outlier"] != t["outlier"] and float(t["l1"]) == float(t["l1"])
    assert ft.compare(dict(l1=t["l1"], aee=float("nan"), outlier=float("nan")), t) == []
    assert len(ft.compare(dict(l1=t["l1"], aee=0.0, outlier=0.0), t)) == 2


@pytest.mark.parametrize("name", list(ft.CASES))
def test_plain_metric_functions_equal_the_fixture(name, fixture):
    """trainer/finetune_flow/flow_metric.py on the CPU, on predictions already resized (the restatement's resize_flow in float64)."""
    from eventpretrain_amd.trainer.finetune_flow import flow_metric as fm
    s = ft.CASES[name]
    flow_map, target, valid, org = ft.case_inputs(name)
    p = ft.resize_flow(flow_map.double(), s["B"], s["h"], s["w"], s["H"], s["W"])
    mask = torch.logical_and(valid.squeeze(1), torch.linalg.norm(org, ord=2, dim=1) > 0)
    aee, outlier = fm.flow_compute_aee_outlier(p, target.double(), mask=mask)
    assert _close(aee, fixture[f"{name}|aee"], 1e-12) and outlier.dtype == torch.float32
    assert float(outlier) == float(fixture[f"{name}|outlier"])
    epe, mag = fm.flow_compute_epe(p, target.double(), mask=mask), fm.flow_compute_mag(target.double(), mask=mask)
    assert epe.shape == mag.shape == (int(fixture[f"{name}|n_sparse"]),)
    assert torch.equal(fm.flow_compute_aee(epe), aee) and torch.equal(fm.flow_compute_outlier(epe, mag), outlier)
    assert tuple(fm.flow_compute_mag(target).shape) == (s["B"], s["H"], s["W"])
    # a zero magnitude gives inf, which counts
    assert float(fm.flow_compute_outlier(torch.tensor([4.0, 4.0, 1.0]), torch.tensor([0.0, 100.0, 0.0]))) == pytest.approx(100.0 / 3.0)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_flow_entries_are_declared_exported_and_bound():
    from eventpretrain_amd import _lib
    txt = open(os.path.join(ROOT, "include", "evtpretrain.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("evp_flow_nblk", 1), ("evp_flow_objective_fwd", 14), ("evp_flow_objective_bwd", 15), ("evp_flow_metrics", 17)):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt) and hasattr(lib, name)
        assert name in _lib.exported_symbols() and len(_lib.SIGNATURES[name]) == nargs
    for macro, value in (("WS_ROW", _lib.FLOW_WS_ROW), ("SAVED", _lib.FLOW_SAVED)):
        assert int(re.search(r"#define EVP_FLOW_%s (\d+)" % macro, txt).group(1)) == value
    _lib.load()
    assert _lib.call("evp_flow_nblk", 1) == 1 and _lib.call("evp_flow_nblk", 257) == 2 and _lib.call("evp_flow_nblk", 1 << 30) == 1024
    assert "flow.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


def test_flow_argument_validation_without_gpu():
    """Arguments are checked in front of any launch: bad ones come back as a status with a message, on a machine with no device."""
    from eventpretrain_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused

    def fwd(ld=8, B=2, h=14, w=14, H=40, W=56, m=p, tgt=p, val=p, out=p):
        return lib.evp_flow_objective_fwd(m, ld, B, h, w, H, W, tgt, val, 40.0, out, p, p, None)
    assert fwd(ld=1) == -2 and b"leading dimension" in lib.evp_last_error()
    assert fwd(h=0) == -2 and fwd(W=-3) == -2 and fwd(B=1 << 20, H=1 << 10, W=1 << 10) == -2 and fwd(B=1 << 20, h=1 << 6, w=1 << 6) == -2
    assert fwd(m=None) == -1 and fwd(tgt=None) == -1 and fwd(val=None) == -1 and fwd(out=None) == -1

    def bwd(ld=8, ldg=8, g=p, grad=p):
        return lib.evp_flow_objective_bwd(p, ld, 2, 14, 14, 40, 56, p, p, 40.0, p, g, grad, ldg, None)
    assert bwd(ldg=1) == -2 and bwd(ld=0) == -2 and bwd(g=None) == -1 and bwd(grad=None) == -1

    def met(E=3, cap=4, org=p, cur=p, ld=8):
        return lib.evp_flow_metrics(p, ld, 2, 14, 14, 40, 56, p, p, 40.0, org, E, cur, p, cap, p, None)
    assert met(E=0) == -2 and b"channels" in lib.evp_last_error()
    assert met(cap=0) == -2 and met(ld=1) == -2 and met(org=None) == -1 and met(cur=None) == -1


def test_python_api_refuses_what_it_cannot_do():
    from eventpretrain_amd import _lib, ops
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_flow import ft_flow_trainer as ftt
    from eventpretrain_amd.trainer.finetune_flow.flow_loss import FlowLoss
    from eventpretrain_amd.trainer.finetune_flow.flow_metric import flow_compute_metrics
    a = make_args(phase="finetune_flow", max_flow=40.0, sample_mode="bilinear")
    with pytest.raises(NotImplementedError):
        FlowLoss(make_args(sample_mode="nearest", max_flow=40.0))
    with pytest.raises(NotImplementedError):
        flow_compute_metrics(make_args(sample_mode="nearest", max_flow=40.0), torch.zeros(2, 2, 3, 3), None, None, None)
    with pytest.raises(_lib.EvpError, match="no CPU path"):
        FlowLoss(a)(torch.zeros(2, 2, 14, 14), torch.zeros(2, 2, 40, 56), torch.zeros(2, 1, 40, 56))
    with pytest.raises(ValueError):
        FlowLoss(a)(torch.zeros(2, 3, 14, 14), torch.zeros(2, 2, 40, 56), torch.zeros(2, 1, 40, 56))
    with pytest.raises(_lib.EvpError, match="no CPU path"):
        ops.flow_metrics(torch.zeros(18, 2), 2, 3, 3, torch.zeros(2, 2, 3, 3), torch.zeros(2, 1, 3, 3), 40.0, torch.zeros(2, 1, 3, 3),
                         torch.zeros(4, 3), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        ftt.ft_flow_train_one_epoch(a, None, [], None, 0, None, evrepsl_model=object())
    with pytest.raises(NotImplementedError):
        ftt.ft_flow_val(a, None, [], 0, "mvsec", evrepsl_model=object())
    assert ftt.VAL_METERS == ("decode_l1_loss", "decode_aee_sparse", "decode_outlier_sparse")


def _batches(n):
    return [dict(events_voxel_grid=torch.full((2, 1), float(i)), events_voxel_grid_org=torch.full((2, 1, 2, 2), 100.0 + i),
                 flow_label=torch.zeros(2, 2, 2, 2), flow_label_valid=torch.ones(2, 1, 2, 2), seq_name=["s"] * 2) for i in range(n)]


def test_training_batches_leave_the_event_grid_behind():
    """The training step takes (events_voxel_grid, flow_label, flow_label_valid): events_voxel_grid_org is dropped in front of the
    prefetcher and the loop; the validation loop gets all four tensors in the reference's order."""
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_flow import ft_flow_trainer as ftt
    from eventpretrain_amd.utils import misc
    a = make_args(phase="finetune_flow", device="cpu")
    wrapped = ftt._TrainBatches(_batches(2))
    assert len(wrapped) == 2 and all(list(b) == list(ftt.TRAIN_KEYS) for b in wrapped)
    assert ftt.TRAIN_KEYS == ("events_voxel_grid", "flow_label", "flow_label_valid", "seq_name")
    with redirect_stdout(io.StringIO()):
        train = list(misc.MetricLogger().log_every(a, wrapped, 10, "", keys=ftt.TRAIN_KEYS))
        val = list(misc.MetricLogger().log_every(a, _batches(2), 10, ""))
    assert [len(b) for b in train] == [4, 4] and tuple(train[1][1].shape) == (2, 2, 2, 2) and train[0][-1] == ["s"] * 2
    assert [len(b) for b in val] == [5, 5] and float(val[1][1].flatten()[0]) == 101.0


def test_shared_deferred_loop_takes_four_tensors():
    """trainer.epoch.val_loop_deferred with a flow batch: the executor is built from, and run with, the four tensors in order; one
    update per meter per batch."""
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer import epoch
    from eventpretrain_amd.utils import misc

    class Table:
        capacity = 2

        def __init__(self):
            self.rows, self.reads = [], []

        def read(self, n):
            self.reads.append(n)
            vals, self.rows = self.rows[:n], self.rows[n:]
            return vals

    class Exec:
        def __init__(self, first):
            self.table, self.inputs = Table(), first

        def run(self, x, org, y, v):
            self.table.rows.append([float(x.flatten()[0]), float(org.flatten()[0]), float(v.sum())])
        eager_with = run
    a = make_args(phase="finetune_flow", device="cpu")
    made = []
    lg = misc.MetricLogger(delimiter="  ")
    with redirect_stdout(io.StringIO()):
        epoch.val_loop_deferred(a, _batches(3), lg, lambda t: made.append(Exec(t)) or made[-1], ("decode_l1_loss", "decode_aee_sparse", "decode_outlier_sparse"))
    assert len(made) == 1 and len(made[0].inputs) == 4 and made[0].table.reads == [2, 1]
    assert list(lg.meters) == ["decode_l1_loss", "decode_aee_sparse", "decode_outlier_sparse"]
    assert lg.meters["decode_l1_loss"].global_avg == pytest.approx(1.0) and lg.meters["decode_aee_sparse"].global_avg == pytest.approx(101.0)
    assert lg.meters["decode_outlier_sparse"].global_avg == pytest.approx(8.0) and lg.meters["decode_outlier_sparse"].count == 3

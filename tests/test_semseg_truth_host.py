"""Host checks of the segmentation objective's truth (tests/semseg_truth.py): the float64 restatement equals what the reference's own
SemsegLoss / resize / semseg_compute_confusion recorded (tests/golden/ft_semseg_objective.npz, tools/gen_semseg_golden.py); every
named mutant of the restatement fails the comparator the GPU test uses; the input conditions of the GPU cases hold; the new entry
points are declared, exported and bound and refuse bad arguments without a device."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import pytest
import torch

import semseg_truth as st
from conftest import ROOT, jload, load_golden


@pytest.fixture(scope="module")
def fixture():
    return load_golden("ft_semseg_objective")


@pytest.fixture(scope="module")
def truths():
    out = {}
    for name, s in st.CASES.items():
        logits, label = st.case_inputs(name)
        out[name] = st.truth(logits, s["B"], s["h"], s["w"], label)
    return out


def _close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return bool(((a - b).abs() <= tol * b.abs().max().clamp(min=1.0)).all())


def test_fixture_lists_the_cases(fixture):
    assert jload(fixture["cases"]) == list(st.CASES)


@pytest.mark.parametrize("name", list(st.CASES))
def test_restatement_equals_the_reference(name, fixture, truths):
    s, t = st.CASES[name], truths[name]
    logits, label = st.case_inputs(name)
    x = logits.double().requires_grad_(True)
    ce, dice = st.objective(x, s["B"], s["h"], s["w"], label)
    (g_ce,) = torch.autograd.grad(ce, x, retain_graph=True)
    (g_dice,) = torch.autograd.grad(dice, x)
    f = {k: torch.from_numpy(fixture[f"{name}|{k}"]) for k in ("ce", "dice", "grad_ce", "grad_dice", "confusion", "miou", "macc")}
    assert _close(dice.detach(), f["dice"], 1e-10) and _close(g_dice, f["grad_dice"], 1e-10)
    assert torch.equal(t["confusion"], f["confusion"])
    assert _close(t["miou"], f["miou"], 1e-10) and _close(t["macc"], f["macc"], 1e-10)
    # the reference casts to float32 in front of nn.CrossEntropyLoss
    assert _close(ce.detach(), f["ce"], 1e-6) and _close(g_ce, f["grad_ce"], 1e-6)
    # the upstream pairs are linear combinations of the two recorded gradients
    for (a, b), g in t["grad"].items():
        assert _close(g, a * f["grad_ce"] + b * f["grad_dice"], 1e-6)


def test_truth_passes_its_own_comparator_in_float64_and_float32(truths):
    for name, s in st.CASES.items():
        logits, label = st.case_inputs(name)
        assert st.compare(st.as_got(truths[name]), truths[name]) == []
        t32 = st.truth(logits, s["B"], s["h"], s["w"], label, dtype=torch.float32)
        assert st.compare(dict(ce=t32["ce"], dice=t32["dice"], grad=t32["grad"]), truths[name]) == [], name


@pytest.mark.parametrize("mut", st.MUTANTS)
def test_mutants_fail_the_comparator(mut, truths):
    """Each on the first case (two samples, ignored pixels, an asymmetric confusion table); dice_per_sample also needs B > 1."""
    s = st.CASES["slice"]
    logits, label = st.case_inputs("slice")
    m = st.truth(logits, s["B"], s["h"], s["w"], label, mut=mut)
    bad = st.compare(st.as_got(m), truths["slice"])
    assert bad, mut
    want = dict(dice_per_sample="dice", ignored_as_class0="dice", ce_mean_all="ce", confusion_transposed="confusion", weights_swapped="grad")[mut]
    assert any(b.startswith(want) for b in bad), (mut, bad)
    if mut == "weights_swapped":       # equal weights hide the swap: only the pair (0.3, 1.7) shows it
        assert all("(0.3, 1.7)" in b for b in bad if b.startswith("grad")), bad


def test_input_conditions_of_the_gpu_cases(truths):
    for name, s in st.CASES.items():
        logits, label = st.case_inputs(name)
        t = truths[name]
        assert tuple(logits.shape) == (s["B"] * s["h"] * s["w"], s["C"]) and s["ld"] >= s["C"] and s["ld"] % 8 == 0
        assert 2 <= s["C"] <= 32
        ignored = (label == st.IGNORE).float().mean().item()
        assert 0.1 < ignored < 0.6, (name, ignored)          # about 20 %, more where a row or a sample is ignored on top
        assert t["n_valid"] > 0 and t["n_unsure"] <= st.MAX_UNSURE * t["n_valid"], (name, t["n_unsure"], t["n_valid"])
        assert int(t["confusion"].sum()) == t["n_valid"]
    _, label = st.case_inputs("slice")
    assert bool((label[0, 0, 5] == st.IGNORE).all()) and not bool((label == 7).any()) and bool((label == 3).any())
    _, label = st.case_inputs("odd")
    assert bool((label[1] == st.IGNORE).all()) and bool((label[0] != st.IGNORE).any())
    _, label = st.case_inputs("slice", all_ignored=True)
    assert bool((label == st.IGNORE).all())
    # the three kernel forms (8, 16, 32 class slots) and both backward block sizes are reached
    assert {8 if s["C"] <= 8 else 16 if s["C"] <= 16 else 32 for s in st.CASES.values()} == {8, 16, 32}
    # downsampling leaves cells without a pixel: their gradient is exactly zero in the truth
    g = truths["down"]["grad"][(1.0, 1.0)]
    assert int((g.abs().sum(1) == 0).sum()) > 0


def test_all_ignored_truth_is_nan_ce_and_zero_dice():
    s = st.CASES["slice"]
    logits, label = st.case_inputs("slice", all_ignored=True)
    t = st.truth(logits, s["B"], s["h"], s["w"], label, need_grad=False)
    assert t["ce"] != t["ce"] and float(t["dice"]) == 0.0 and t["n_valid"] == 0


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_semseg_entries_are_declared_exported_and_bound():
    from eventpretrain_amd import _lib
    txt = open(os.path.join(ROOT, "include", "evtpretrain.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("evp_semseg_nblk", 1), ("evp_semseg_objective_fwd", 16), ("evp_semseg_objective_bwd", 17), ("evp_semseg_metrics", 20)):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt) and hasattr(lib, name)
        assert name in _lib.exported_symbols() and len(_lib.SIGNATURES[name]) == nargs
    for macro, value in (("MAX_CLASSES", _lib.SEMSEG_MAX_CLASSES), ("WS_ROW", _lib.SEMSEG_WS_ROW), ("SAVED", _lib.SEMSEG_SAVED)):
        assert int(re.search(r"#define EVP_SEMSEG_%s (\d+)" % macro, txt).group(1)) == value
    _lib.load()
    assert _lib.call("evp_semseg_nblk", 1) == 1 and _lib.call("evp_semseg_nblk", 257) == 2 and _lib.call("evp_semseg_nblk", 1 << 30) == 1024


def test_semseg_argument_validation_without_gpu():
    """Arguments are checked in front of any launch: bad ones come back as a status with a message, on a machine with no device."""
    from eventpretrain_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused

    def fwd(C=11, ld=16, B=2, h=14, w=14, H=40, W=56, m=p, out=p):
        return lib.evp_semseg_objective_fwd(m, ld, B, h, w, H, W, C, p, 255, 1, out, p, None, p, None)
    assert fwd(C=1) == -2 and b"classes" in lib.evp_last_error()
    assert fwd(C=33) == -2 and fwd(ld=8) == -2 and fwd(h=0) == -2 and fwd(B=1 << 20, H=1 << 10, W=1 << 10) == -2
    assert fwd(m=None) == -1 and fwd(out=None) == -1
    assert lib.evp_semseg_objective_bwd(p, 16, 2, 14, 14, 40, 56, 11, p, 255, 1, p, p, p, p, 8, None) == -2      # ldg < C
    assert lib.evp_semseg_objective_bwd(p, 16, 2, 14, 14, 40, 56, 11, p, 255, 1, p, None, p, p, 16, None) == -1
    assert lib.evp_semseg_metrics(p, 16, 2, 14, 14, 40, 56, 11, p, 255, 1, p, p, 0, None, None, None, p, p, None) == -2      # no slot
    assert lib.evp_semseg_metrics(p, 16, 2, 14, 14, 40, 56, 40, p, 255, 1, p, p, 4, None, None, None, p, p, None) == -2
    assert lib.evp_semseg_metrics(p, 16, 2, 14, 14, 40, 56, 11, p, 255, 1, None, p, 4, None, None, None, p, p, None) == -1


def test_python_api_refuses_what_it_cannot_do():
    from eventpretrain_amd import _lib, ops
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_semseg import ft_semseg_trainer as ft
    from eventpretrain_amd.trainer.finetune_semseg.semseg_loss import SemsegLoss, prediction_map
    from eventpretrain_amd.trainer.finetune_semseg.semseg_metric import semseg_confusion_to_macc, semseg_confusion_to_miou
    a = make_args(phase="finetune_semseg", num_classes=11, ignore_label=255, sample_mode="bilinear")
    with pytest.raises(NotImplementedError):
        SemsegLoss(make_args(sample_mode="nearest"), num_classes=11, ignore_index=255)
    with pytest.raises(_lib.EvpError, match="no CPU path"):
        SemsegLoss(a, 11, 255)(torch.zeros(2, 11, 14, 14), torch.zeros(2, 1, 40, 56, dtype=torch.int64))
    with pytest.raises(ValueError):
        SemsegLoss(a, 11, 255)(torch.zeros(2, 6, 14, 14), torch.zeros(2, 1, 40, 56, dtype=torch.int64))
    with pytest.raises(_lib.EvpError, match="no CPU path"):
        ops.semseg_metrics(torch.zeros(18, 2), 2, 3, 3, torch.zeros(2, 1, 3, 3, dtype=torch.int64), 255, torch.zeros(4, 3), torch.zeros(1, dtype=torch.int64))
    for evr in (dict(evrepsl_model=object()),):
        with pytest.raises(NotImplementedError):
            ft.ft_semseg_train_one_epoch(a, None, [], None, 0, None, **evr)
        with pytest.raises(NotImplementedError):
            ft.ft_semseg_val(a, None, [], 0, **evr)
    # a head's prediction -- the permuted view of a padded token-major map -- is consumed where it lies
    buf = torch.arange(2 * 3 * 4 * 16, dtype=torch.float32).view(24, 16)
    pred = buf[:, :11].view(2, 3, 4, 11).permute(0, 3, 1, 2)
    m, B, h, w = prediction_map(pred)
    assert (B, h, w) == (2, 3, 4) and m.data_ptr() == buf.data_ptr() and m.stride() == (16, 1) and tuple(m.shape) == (24, 11)
    m2, *_ = prediction_map(torch.zeros(2, 11, 3, 4))
    assert m2.is_contiguous() and tuple(m2.shape) == (24, 11)
    # the conversions against the truth's, absent classes included
    conf = torch.tensor([[5, 1, 0], [2, 3, 0], [0, 0, 0]])
    miou, macc = st.miou_macc(conf)
    assert float(semseg_confusion_to_miou(conf)) == pytest.approx(float(miou), rel=1e-12)
    assert float(semseg_confusion_to_macc(conf)) == pytest.approx(float(macc), rel=1e-12)
    assert float(macc) == pytest.approx((500 / 6 + 300 / 5 + 0) / 3, rel=1e-12)


def test_shared_deferred_loop_takes_meter_names():
    """trainer.epoch.val_loop_deferred with the segmentation meters: one update per meter per batch, in order; a None column is skipped."""
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

        def run(self, x, y):
            self.table.rows.append([float(x.flatten()[0]), 10.0, 20.0])
        eager_with = run
    a = make_args(phase="finetune_semseg", device="cpu")
    loader = [dict(events_voxel_grid=torch.full((2, 1), float(i)), semseg_label=torch.zeros(2, 1, 2, 2, dtype=torch.int64), seq_name=["s"] * 2) for i in range(3)]
    made = []
    for names in (("loss_total", "miou", "macc"), ("loss_total", None, "macc")):
        lg = misc.MetricLogger(delimiter="  ")
        with redirect_stdout(io.StringIO()):
            epoch.val_loop_deferred(a, loader, lg, lambda t: made.append(Exec(t)) or made[-1], names)
        assert made[-1].table.reads == [2, 1]
        assert set(lg.meters) == {n for n in names if n} and lg.meters["loss_total"].global_avg == pytest.approx(1.0) and lg.meters["macc"].count == 3

"""The segmentation objective on the GPU (csrc/semseg.hip, ops.SemsegObjectiveFn / semseg_metrics, trainer/finetune_semseg) against the
float64 truth of tests/semseg_truth.py, whose comparator and bounds are used as they are: ce and dice within 1e-4 relative, the map
gradient within 1e-4 of the truth's largest magnitude under three upstream pairs, exactly-zero pad columns, the argmax map equal to
torch.argmax over ops.resize_map bit for bit, the confusion table up to the unsure pixels, the table slot, determinism under repeat and
HIP-graph replay, and the two trainer loops captured against eager.

Measured on an MI355X (worst case over the five shapes): see DESIGN.md 5 (K27)."""
import pytest
import torch

import semseg_truth as st

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _abi():
    from eventpretrain_amd import _lib
    return _lib.call, _lib.stream_ptr


def _dev_case(name, all_ignored=False):
    """-> (shape dict, the [R, ld] buffer whose first C columns hold the logits and whose pad holds NaN, that column slice, labels)."""
    s = st.CASES[name]
    logits, label = st.case_inputs(name, all_ignored)
    buf = torch.full((logits.shape[0], s["ld"]), NAN, device="cuda")
    buf[:, :s["C"]] = logits.cuda()
    return s, buf, buf[:, :s["C"]], label.cuda()


def _geom(s, buf, lab, ignore=st.IGNORE):
    return (buf.data_ptr(), s["ld"], s["B"], s["h"], s["w"], s["H"], s["W"], s["C"], lab.data_ptr(), 0 if ignore is None else ignore, int(ignore is not None))


def _fwd(s, buf, lab, ignore=st.IGNORE):
    from eventpretrain_amd import _lib
    call, sp = _abi()
    out, saved = torch.full((2,), NAN, device="cuda"), torch.full((_lib.SEMSEG_SAVED,), NAN, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(call("evp_semseg_nblk", lab.numel()) * _lib.SEMSEG_WS_ROW, dtype=torch.int32, device="cuda")
    call("evp_semseg_objective_fwd", *_geom(s, buf, lab, ignore), out.data_ptr(), saved.data_ptr(), status.data_ptr(), ws.data_ptr(), sp())
    return out, saved, status


def _bwd(s, buf, lab, saved, g_ce, g_dice, ignore=st.IGNORE):
    call, sp = _abi()
    grad = torch.full((buf.shape[0], s["ld"]), NAN, device="cuda")
    a, b = torch.tensor([g_ce], device="cuda"), torch.tensor([g_dice], device="cuda")
    call("evp_semseg_objective_bwd", *_geom(s, buf, lab, ignore), saved.data_ptr(), a.data_ptr(), b.data_ptr(), grad.data_ptr(), s["ld"], sp())
    return grad


def _metrics(s, m, lab, capacity=4, ignore=st.IGNORE, want_argmax=True):
    from eventpretrain_amd import ops
    table = torch.full((capacity, 3), -1.0, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    conf = torch.full((s["C"], s["C"]), -1, dtype=torch.int64, device="cuda")
    am = torch.full((s["B"], s["H"], s["W"]), 255, dtype=torch.uint8, device="cuda") if want_argmax else None
    ops.semseg_metrics(m, s["B"], s["h"], s["w"], lab, ignore, table, cursor, confusion=conf, argmax=am)
    return table, cursor, conf, am


@pytest.fixture(scope="module")
def truths():
    out = {}
    for name, s in st.CASES.items():
        logits, label = st.case_inputs(name)
        out[name] = st.truth(logits, s["B"], s["h"], s["w"], label)
    return out


@pytest.mark.parametrize("name", list(st.CASES))
def test_objective_against_float64_truth(name, truths):
    from eventpretrain_amd import ops
    s, buf, m, lab = _dev_case(name)
    t = truths[name]
    out, saved, status = _fwd(s, buf, lab)
    grads = {k: _bwd(s, buf, lab, saved, *k) for k in st.UPSTREAM}
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got = dict(ce=out[0].item(), dice=out[1].item(), grad={k: g[:, :s["C"]] for k, g in grads.items()})
    rel = {k: abs(got[k] - float(t[k])) / abs(float(t[k])) / st.REL_LOSS for k in ("ce", "dice")}
    gr = {k: (g[:, :s["C"]].double().cpu() - t["grad"][k]).abs().max().item() / (st.REL_GRAD * t["grad"][k].abs().max().item()) for k, g in grads.items()}
    print(f"{name}: share of the bound -- ce {rel['ce']:.4f} dice {rel['dice']:.4f} grad " + " ".join(f"{k}: {v:.4f}" for k, v in gr.items()))
    assert st.compare(got, t) == []
    for k, g in grads.items():
        assert bool((g[:, s["C"]:] == 0).all()), f"pad columns of the gradient under {k}"
    if name == "down":      # cells no output pixel names: an exact zero, as in the truth
        empty = t["grad"][(1.0, 1.0)].abs().sum(1) == 0
        assert int(empty.sum()) > 0 and bool((grads[(1.0, 1.0)].cpu()[empty] == 0).all())
    # the autograd route over the column slice: the same launches, the same bits; its gradient keeps the map's leading dimension
    leaf = m.detach().requires_grad_(True)
    ce, dice = ops.SemsegObjectiveFn.apply(leaf, s["B"], s["h"], s["w"], lab, st.IGNORE)
    assert ce.dim() == 0 and dice.dim() == 0 and torch.equal(torch.stack([ce, dice]).detach(), out)
    for (a, b), g in grads.items():
        (ga,) = torch.autograd.grad(a * ce + b * dice, leaf, retain_graph=True)
        assert tuple(ga.shape) == tuple(m.shape) and ga.stride(0) == s["ld"] and torch.equal(ga, g[:, :s["C"]])


def test_every_label_ignored_gives_nan_ce_and_the_truth_dice():
    s, buf, m, lab = _dev_case("slice", all_ignored=True)
    logits, label = st.case_inputs("slice", all_ignored=True)
    t = st.truth(logits, s["B"], s["h"], s["w"], label, need_grad=False)
    out, saved, status = _fwd(s, buf, lab)
    assert out[0].item() != out[0].item() and int(status.item()) == 0
    assert st.compare(dict(ce=out[0].item(), dice=out[1].item()), t) == [] and out[1].item() == 0.0


def test_ignore_none_and_labels_out_of_range():
    """ignore_label = None: nothing is ignored (labels made valid first). A valid label >= C is an input error: counted in the status
    word, kept out of every sum -- the results are those of the same labels with these pixels ignored -- and raised by the check."""
    from eventpretrain_amd import _lib, ops
    s, buf, m, lab = _dev_case("odd")
    logits, label = st.case_inputs("odd")
    full = label.clone()
    full[full == st.IGNORE] = 2
    t = st.truth(logits, s["B"], s["h"], s["w"], full, ignore=None, upstream=((1.0, 1.0),))
    out, saved, status = _fwd(s, buf, full.cuda(), ignore=None)
    g = _bwd(s, buf, full.cuda(), saved, 1.0, 1.0, ignore=None)
    assert st.compare(dict(ce=out[0].item(), dice=out[1].item(), grad={(1.0, 1.0): g[:, :s["C"]]}), t) == [] and int(status.item()) == 0
    bad = label.clone()
    bad[0, 0, :2, :] = s["C"]                       # 90 pixels of sample 0
    bad[2, 0, 7, 3] = -1
    n_bad = int(((bad == s["C"]) | (bad == -1)).sum())
    as_ignored = bad.clone()
    as_ignored[(bad == s["C"]) | (bad == -1)] = st.IGNORE
    t = st.truth(logits, s["B"], s["h"], s["w"], as_ignored, upstream=((1.0, 1.0),))
    out, saved, status = _fwd(s, buf, bad.cuda())
    g = _bwd(s, buf, bad.cuda(), saved, 1.0, 1.0)
    assert int(status.item()) == n_bad
    assert st.compare(dict(ce=out[0].item(), dice=out[1].item(), grad={(1.0, 1.0): g[:, :s["C"]]}), t) == []
    ops.semseg_check_labels("cuda")                  # clean so far
    table, cursor, conf, _ = _metrics(s, m, bad.cuda())
    assert st.compare(dict(ce=t["ce"], dice=t["dice"], confusion=conf), t) == []
    with pytest.raises(_lib.EvpError, match=f"{n_bad} pixels"):
        ops.semseg_check_labels("cuda")
    ops.semseg_check_labels("cuda")                  # the count starts again
    with pytest.raises(_lib.EvpError, match="classes"):
        ops.SemsegObjectiveFn.apply(torch.zeros(9, 33, device="cuda"), 1, 3, 3, torch.zeros(1, 1, 3, 3, dtype=torch.int64, device="cuda"), 255)
    with pytest.raises(_lib.EvpError, match="classes"):
        ops.SemsegObjectiveFn.apply(torch.zeros(9, 1, device="cuda"), 1, 3, 3, torch.zeros(1, 1, 3, 3, dtype=torch.int64, device="cuda"), 255)


@pytest.mark.parametrize("name", list(st.CASES))
def test_metrics_argmax_confusion_and_slot(name, truths):
    from eventpretrain_amd import ops
    s, buf, m, lab = _dev_case(name)
    t = truths[name]
    table, cursor, conf, am = _metrics(s, m, lab)
    out, _, _ = _fwd(s, buf, lab)
    resized = ops.resize_map(m, s["B"], s["h"], s["w"], s["H"], s["W"])
    assert torch.equal(am, resized.argmax(1).view(s["B"], s["H"], s["W"]).to(torch.uint8))
    assert st.compare(dict(ce=t["ce"], dice=t["dice"], confusion=conf), t) == []
    print(f"{name}: {t['n_unsure']} unsure of {t['n_valid']} valid pixels; confusion differs from the truth's in "
          f"{int((conf.cpu() != t['confusion']).sum())} cells")
    # without the argmax map the same table
    _, _, conf2, _ = _metrics(s, m, lab, want_argmax=False)
    assert torch.equal(conf, conf2)
    assert int(cursor.item()) == 1 and bool((table[1:] == -1).all())
    miou, macc = st.miou_macc(conf.cpu())
    slot = table[0].double().cpu()
    assert slot[1].item() == pytest.approx(float(miou), rel=1e-6) and slot[2].item() == pytest.approx(float(macc), rel=1e-6)
    assert slot[0].item() == pytest.approx(out[0].item() + out[1].item(), rel=1e-6)


def test_metrics_cursor_and_full_table():
    from eventpretrain_amd import ops
    s, buf, m, lab = _dev_case("ident")
    table = torch.full((2, 3), -1.0, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    for k in (1, 2):
        ops.semseg_metrics(m, s["B"], s["h"], s["w"], lab, st.IGNORE, table, cursor)
        assert int(cursor.item()) == k
    assert torch.equal(table[0], table[1]) and bool((table != -1).all())
    keep = table.clone()
    table[1, 0] = 7.0
    keep[1, 0] = 7.0
    ops.semseg_metrics(m, s["B"], s["h"], s["w"], lab, st.IGNORE, table, cursor)          # full: left alone
    assert int(cursor.item()) == 2 and torch.equal(table, keep)


def test_logits_already_at_label_size():
    """The reference's call form: the logits resized first (ops.resize_map), then the objective with (h, w) == (H, W). The interpolated
    logits are the resized map's bit for bit and the pixel pass is the same, so the losses are EQUAL; the gradient, now in the
    full-size logits, against the truth."""
    from eventpretrain_amd import ops
    s, buf, m, lab = _dev_case("slice")
    out, _, _ = _fwd(s, buf, lab)
    full = ops.resize_map(m, s["B"], s["h"], s["w"], s["H"], s["W"]).detach().contiguous().requires_grad_(True)
    ce, dice = ops.SemsegObjectiveFn.apply(full, s["B"], s["H"], s["W"], lab, st.IGNORE)
    assert torch.equal(torch.stack([ce, dice]).detach(), out)
    (g,) = torch.autograd.grad(0.3 * ce + 1.7 * dice, full)
    t = st.truth(full.detach().cpu(), s["B"], s["H"], s["W"], lab.cpu(), upstream=((0.3, 1.7),))
    assert st.compare(dict(ce=ce.item(), dice=dice.item(), grad={(0.3, 1.7): g}), t) == []


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from eventpretrain_amd import ops
    s, buf, m, lab = _dev_case("slice")
    gw = torch.tensor([0.3, 1.7], device="cuda")

    def run():
        leaf = m.detach().requires_grad_(True)
        ce, dice = ops.SemsegObjectiveFn.apply(leaf, s["B"], s["h"], s["w"], lab, st.IGNORE)
        (g,) = torch.autograd.grad(gw[0] * ce + gw[1] * dice, leaf)
        table, cursor, conf, am = _metrics(s, m, lab)
        return [ce.detach(), dice.detach(), g.detach(), table, conf, am]
    first, second = run(), run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        held = run()
    for _ in range(2):
        for h in held[2:]:         # (ce and dice are views of one buffer; the slot's loss stands in for them)
            h.zero_() if h.dtype != torch.float32 else h.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, held):
            assert torch.equal(a, b)


def test_python_api_on_a_heads_prediction():
    """SemsegLoss and semseg_compute_confusion take (B, C, h, w): the permuted view of the padded map is read where it lies and gives
    the bits of the C-ABI call; a contiguous NCHW tensor gives them too (gathered into a map first)."""
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_semseg.semseg_loss import SemsegLoss
    from eventpretrain_amd.trainer.finetune_semseg.semseg_metric import semseg_compute_confusion, semseg_confusion_to_macc, semseg_confusion_to_miou
    s, buf, m, lab = _dev_case("slice")
    a = make_args(phase="finetune_semseg", num_classes=s["C"], ignore_label=st.IGNORE, sample_mode="bilinear", device="cuda")
    out, saved, _ = _fwd(s, buf, lab)
    g = _bwd(s, buf, lab, saved, 1.0, 1.0)
    pred = m.view(s["B"], s["h"], s["w"], s["C"]).permute(0, 3, 1, 2).detach().requires_grad_(True)
    crit = SemsegLoss(a, num_classes=s["C"], ignore_index=st.IGNORE)
    ce, dice = crit(pred, lab)
    assert torch.equal(torch.stack([ce, dice]).detach(), out)
    (ce + dice).backward()
    assert torch.equal(pred.grad.permute(0, 2, 3, 1).reshape(-1, s["C"]), g[:, :s["C"]])
    ce2, dice2 = crit(pred.detach().contiguous(), lab)
    assert torch.equal(torch.stack([ce2, dice2]), out)
    _, _, conf, _ = _metrics(s, m, lab)
    conf2 = semseg_compute_confusion(a, pred.detach(), lab)
    assert conf2.dtype == torch.int64 and torch.equal(conf, conf2)
    miou, macc = st.miou_macc(conf.cpu())
    assert semseg_confusion_to_miou(conf2).item() == pytest.approx(float(miou), rel=1e-12)
    assert semseg_confusion_to_macc(conf2).item() == pytest.approx(float(macc), rel=1e-12)


# ------------------------------------------------------------------------------------------------------------- the trainer
def _trainer_args(graph):
    from eventpretrain_amd.testing import make_args
    a = make_args(phase="finetune_semseg", model_size="small", backbone_type="vit", num_classes=11, mask_ratio=0.0, sample_mode="bilinear",
                  device="cuda", drop_rate=0.0, drop_path_rate=0.0, clip_grad=None, ignore_label=st.IGNORE, decode_loss_weight=1.0,
                  aux_loss_weight=0.4)
    a.epochs, a.warmup_epochs, a.lr, a.min_lr, a.graph_step = 4, 1, 1e-3, 1e-6, graph
    return a


def _hub(a):
    """ViT-Small hub with closed-form weights; the heads' Dropout2d off (its draws differ between a capture and an eager run)."""
    from eventpretrain_amd.model.finetune_dense.ft_dense_hub_model import FtDenseHubModel
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_
    from eventpretrain_amd.utils import lr_decay as lrd
    m = FtDenseHubModel(a)
    for h in (m.decode_head, m.auxiliary_head):
        h.dropout = None
    det_fill_module_(m)
    m = m.cuda()
    return m, FusedAdamW(lrd.param_groups_lrd(a, m, 0.05, layer_decay=1), lr=a.lr, betas=(0.9, 0.999))


def _loader():
    from eventpretrain_amd.testing import det_normalish, det_uniform
    batches = []
    for i in range(3):
        lab = (det_uniform(f"semseg.train.label.{i}", (2, 1, 40, 56), 0.0, 1.0) * 11).floor().clamp(0, 10).long()
        lab[det_uniform(f"semseg.train.ignore.{i}", (2, 1, 40, 56), 0.0, 1.0) < 0.2] = st.IGNORE
        batches.append(dict(events_voxel_grid=det_normalish(f"semseg.train.x.{i}", (2, 5, 224, 224)) * 0.5, semseg_label=lab, seq_name=["s"] * 2))
    return batches


def test_trainer_captured_against_eager_and_truth():
    """ViT-Small hub, B = 2, labels 40 x 56, three batches: the captured epoch and the eager one (args.graph_step = False) return
    bit-equal meters and leave bit-equal weights and buffers; the first batch's loss_total equals the truth on the model's own logits
    within 1e-4; ft_semseg_val captured equals its eager loop within 1e-6 per meter.

    The compute dtype is bf16 (the objective itself is float32 either way: the heads hand out float32 logits). That is the mode in
    which a step of this code base has one set of bits (test_gpu_dense_heads.py::test_captured_dense_step_replays_bit_equal_to_eager):
    weight gradients go through the grouped launch, which takes no split-K. In float32 mode the backbone's per-layer weight-gradient
    GEMMs split K and add their partial sums with float atomics, so two EAGER epochs already differ from each other: measured on an
    MI355X with this test's inputs, after one step all 246 tensors and the loss are bit-equal between eager / eager, captured /
    captured and eager / captured (Adam's first update is lr * sign(g) up to eps: it hides last-bit differences of g), after three
    steps 229 of 246 tensors differ between two eager runs (largest |diff| 2.3e-4, backbone.patch_embed.proj.weight), 228 between two
    captured runs and 228 between eager and captured, the third loss by one ulp. Bit equality of captured against eager can only
    be asked where eager equals eager."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.trainer.finetune_semseg.ft_semseg_trainer import ft_semseg_train_one_epoch, ft_semseg_val
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    ops.set_compute_dtype(torch.bfloat16)
    loader = _loader()
    res, models = {}, {}
    for mode in ("eager", "graph"):
        a = _trainer_args(mode == "graph")
        m, opt = _hub(a)
        stats = ft_semseg_train_one_epoch(a, m, loader, opt, 0, NativeScalerWithGradNormCount())
        assert list(stats) == ["lr", "loss_total"]
        if mode == "graph":
            assert m._evp_auto_executor[1].note == "hip-graph"
        else:
            assert not hasattr(m, "_evp_auto_executor")
        res[mode], models[mode] = stats, (a, m)
    print("train:", res)
    assert res["graph"] == res["eager"]
    for (k, p), (_, q) in zip(models["graph"][1].state_dict().items(), models["eager"][1].state_dict().items()):
        assert torch.equal(p, q), k
    # the first batch's loss_total against the truth on the model's own logits (a third model from the same start)
    a = _trainer_args(False)
    m, opt = _hub(a)
    m.train()
    with torch.no_grad():
        out = m(loader[0]["events_voxel_grid"].cuda())
    want = 0.0
    for pred, wgt in ((out[-2], a.decode_loss_weight), (out[-1], a.aux_loss_weight)):
        B, C, h, w = pred.shape
        t = st.truth(pred.permute(0, 2, 3, 1).reshape(-1, C).cpu(), B, h, w, loader[0]["semseg_label"], need_grad=False)
        want += wgt * (float(t["ce"]) + float(t["dice"]))
    first = ft_semseg_train_one_epoch(a, m, loader[:1], opt, 0, NativeScalerWithGradNormCount())["loss_total"]
    print(f"first batch: loss_total {first!r}, truth {want!r}, rel {abs(first - want) / want:.2e}")
    assert abs(first - want) <= 1e-4 * abs(want)
    # evaluation: the captured loop against the eager one, on the trained model
    a, m = models["graph"]
    val = {}
    for graph in (True, False):
        a.graph_step = graph
        val[graph] = ft_semseg_val(a, m, loader, 0)
        assert list(val[graph]) == ["loss_total", "miou", "macc"]
    assert m._evp_auto_eval[1].note == "hip-graph" and m._evp_auto_eval[1].replays == 3
    print("val:", val)
    for k in val[True]:
        assert val[True][k] == pytest.approx(val[False][k], rel=1e-6), k

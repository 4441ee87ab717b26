"""The optical-flow objective on the GPU (csrc/flow.hip, ops.FlowObjectiveFn / flow_metrics, trainer/finetune_flow) against the float64
truth of tests/flow_truth.py, whose comparator and bounds are used as they are: l1 and aee within 1e-4 relative, the map gradient
within 1e-4 of the truth's largest magnitude under three upstream weights, exactly-zero pad columns and unnamed cells, the outlier
count between the sure count and the sure count plus the unsure pixels, the table slot, determinism under repeat and HIP-graph
replay, and the two trainer loops captured against eager.

Measured on an MI355X (worst case over the five shapes): see DESIGN.md 5 (K28)."""
import pytest
import torch

import flow_truth as ft

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _abi():
    from eventpretrain_amd import _lib
    return _lib.call, _lib.stream_ptr


def _dev_case(name, **kw):
    """-> (shape dict, the [R, ld] buffer whose first 2 columns hold the map and whose pad holds NaN, that column slice, target, valid, org)."""
    s = ft.CASES[name]
    flow_map, target, valid, org = ft.case_inputs(name, **kw)
    buf = torch.full((flow_map.shape[0], s["ld"]), NAN, device="cuda")
    buf[:, :2] = flow_map.cuda()
    return s, buf, buf[:, :2], target.cuda(), valid.cuda(), org.cuda()


def _geom(s, buf, tgt, val, max_flow=None):
    return (buf.data_ptr(), s["ld"], s["B"], s["h"], s["w"], s["H"], s["W"], tgt.data_ptr(), val.data_ptr(), s["max_flow"] if max_flow is None else max_flow)


def _ws(n):
    from eventpretrain_amd import _lib
    return torch.empty(_lib.call("evp_flow_nblk", n) * _lib.FLOW_WS_ROW, dtype=torch.int32, device="cuda")


def _fwd(s, buf, tgt, val, max_flow=None):
    from eventpretrain_amd import _lib
    call, sp = _abi()
    out, saved = torch.full((1,), NAN, device="cuda"), torch.full((_lib.FLOW_SAVED,), NAN, device="cuda")
    ws = _ws(val.numel())
    call("evp_flow_objective_fwd", *_geom(s, buf, tgt, val, max_flow), out.data_ptr(), saved.data_ptr(), ws.data_ptr(), sp())
    return out, saved


def _bwd(s, buf, tgt, val, saved, g, max_flow=None):
    call, sp = _abi()
    grad = torch.full((buf.shape[0], s["ld"]), NAN, device="cuda")
    gl = torch.tensor([g], device="cuda")
    call("evp_flow_objective_bwd", *_geom(s, buf, tgt, val, max_flow), saved.data_ptr(), gl.data_ptr(), grad.data_ptr(), s["ld"], sp())
    return grad


def _metrics(s, m, tgt, val, org, capacity=4, max_flow=None):
    from eventpretrain_amd import ops
    table = torch.full((capacity, 3), -1.0, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.flow_metrics(m, s["B"], s["h"], s["w"], tgt, val, s["max_flow"] if max_flow is None else max_flow, org, table, cursor)
    return table, cursor


def _truth(name, **kw):
    s = ft.CASES[name]
    inputs = ft.case_inputs(name, **{k: kw.pop(k) for k in ("all_invalid", "no_events") if k in kw})
    return ft.truth(inputs[0], s["B"], s["h"], s["w"], *inputs[1:], s["max_flow"], **kw)


@pytest.fixture(scope="module")
def truths():
    return {name: _truth(name) for name in ft.CASES}


@pytest.mark.parametrize("name", list(ft.CASES))
def test_objective_against_float64_truth(name, truths):
    from eventpretrain_amd import ops
    s, buf, m, tgt, val, org = _dev_case(name)
    t = truths[name]
    out, saved = _fwd(s, buf, tgt, val)
    grads = {g: _bwd(s, buf, tgt, val, saved, g) for g in ft.UPSTREAM}
    torch.cuda.synchronize()
    got = dict(l1=out[0].item(), grad={g: x[:, :2] for g, x in grads.items()})
    rel = abs(got["l1"] - float(t["l1"])) / abs(float(t["l1"])) / ft.REL_LOSS
    gr = {g: (x[:, :2].double().cpu() - t["grad"][g]).abs().max().item() / (ft.REL_GRAD * t["grad"][g].abs().max().item()) for g, x in grads.items()}
    print(f"{name}: share of the bound -- l1 {rel:.4f} grad " + " ".join(f"{g}: {v:.4f}" for g, v in gr.items()))
    assert saved[0].item() == t["n_valid"]
    assert ft.compare(got, t) == []
    for g, x in grads.items():
        assert bool((x[:, 2:] == 0).all()), f"pad columns of the gradient under {g}"
    if name == "down":      # cells no output pixel names: an exact zero, as in the truth
        empty = t["grad"][1.0].abs().sum(1) == 0
        assert int(empty.sum()) > 0 and bool((grads[1.0].cpu()[empty] == 0).all())
    # the autograd route over the column slice: the same launches, the same bits; its gradient keeps the map's leading dimension
    leaf = m.detach().requires_grad_(True)
    loss = ops.FlowObjectiveFn.apply(leaf, s["B"], s["h"], s["w"], tgt, val, s["max_flow"])
    assert loss.dim() == 0 and torch.equal(loss.detach(), out[0])
    for g, x in grads.items():
        (ga,) = torch.autograd.grad(g * loss, leaf, retain_graph=True)
        assert tuple(ga.shape) == tuple(m.shape) and ga.stride(0) == s["ld"] and torch.equal(ga, x[:, :2])


def test_tied_components_add_nothing():
    """`ident` (identity taps, factors 1: a pixel's prediction IS its map cell), every pixel valid, some targets bit-equal to the map:
    those components add nothing to the loss and nothing to the gradient (sign(0) = 0)."""
    s, buf, m, tgt, val, org = _dev_case("ident")
    flow_map, target, valid, _ = ft.case_inputs("ident")
    target, valid = target.clone(), torch.ones_like(valid)
    tied = [(0, 0), (4, 0), (4, 1), (7, 1)]                       # (pixel, component)
    for px, c in tied:
        target[0, c, px // 3, px % 3] = flow_map[px, c]
    big = 1e9
    t = ft.truth(flow_map, 1, 3, 3, target, valid, torch.zeros(1, 1, 3, 3), big, upstream=(1.7,))
    assert t["n_valid"] == 9 and all(float(t["grad"][1.7][px, c]) == 0.0 for px, c in tied)
    out, saved = _fwd(s, buf, target.cuda(), valid.cuda(), big)
    grad = _bwd(s, buf, target.cuda(), valid.cuda(), saved, 1.7, big)
    assert ft.compare(dict(l1=out[0].item(), grad={1.7: grad[:, :2]}), t) == []
    d = (flow_map.double() - target[0].permute(1, 2, 0).reshape(9, 2).double()).abs()
    assert all(float(d[px, c]) == 0.0 for px, c in tied)
    assert out[0].item() == pytest.approx(float(d.sum()) / 18.0, rel=1e-6)
    for px, c in tied:
        assert grad[px, c].item() == 0.0
    others = [(px, c) for px in range(9) for c in range(2) if (px, c) not in tied]
    assert all(abs(grad[px, c].item()) == pytest.approx(1.7 / 18.0, rel=1e-6) for px, c in others)


def test_degenerate_batches():
    """Every pixel below 0.5: a NaN loss and an all-zero gradient (never 0 * inf), while the sparse mask -- valid NON-ZERO -- still has
    pixels. No event anywhere: NaN aee and outlier in the slot next to a finite l1."""
    s, buf, m, tgt, val, org = _dev_case("slice", all_invalid=True)
    t = _truth("slice", all_invalid=True)
    out, saved = _fwd(s, buf, tgt, val)
    assert out[0].item() != out[0].item() and saved[0].item() == 0.0
    for g in ft.UPSTREAM:
        assert bool((_bwd(s, buf, tgt, val, saved, g) == 0).all())
    table, cursor = _metrics(s, m, tgt, val, org)
    slot = table[0].tolist()
    assert slot[0] != slot[0] and int(cursor.item()) == 1
    assert ft.compare(dict(l1=slot[0], aee=slot[1], outlier=slot[2]), t) == [] and t["n_sparse"] > 0
    s, buf, m, tgt, val, org = _dev_case("slice", no_events=True)
    out, _ = _fwd(s, buf, tgt, val)
    table, cursor = _metrics(s, m, tgt, val, org)
    slot = table[0].tolist()
    assert torch.equal(table[0, 0], out[0]) and slot[0] == slot[0] and slot[1] != slot[1] and slot[2] != slot[2] and int(cursor.item()) == 1


@pytest.mark.parametrize("name", list(ft.CASES))
def test_metrics_and_slot(name, truths):
    s, buf, m, tgt, val, org = _dev_case(name)
    t = truths[name]
    table, cursor = _metrics(s, m, tgt, val, org)
    out, _ = _fwd(s, buf, tgt, val)
    assert torch.equal(table[0, 0], out[0])                      # l1: the objective's bits
    l1, aee, outlier = table[0].tolist()
    count = outlier / 100.0 * t["n_sparse"]
    print(f"{name}: share of the bound -- aee {abs(aee - float(t['aee'])) / float(t['aee']) / ft.REL_LOSS:.4f}; outlier count {count:.3f}, "
          f"truth {t['n_outlier']} ({t['n_outlier_sure']} sure + {t['n_unsure']} unsure of {t['n_sparse']} sparse pixels)")
    assert ft.compare(dict(l1=l1, aee=aee, outlier=outlier), t) == []
    assert int(cursor.item()) == 1 and bool((table[1:] == -1).all())


def test_metrics_cursor_and_full_table():
    from eventpretrain_amd import ops
    s, buf, m, tgt, val, org = _dev_case("ident")
    table = torch.full((2, 3), -1.0, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    args = (m, s["B"], s["h"], s["w"], tgt, val, s["max_flow"], org, table, cursor)
    for k in (1, 2):
        ops.flow_metrics(*args)
        assert int(cursor.item()) == k
    assert torch.equal(table[0], table[1]) and bool((table != -1).all())
    keep = table.clone()
    table[1, 0] = 7.0
    keep[1, 0] = 7.0
    ops.flow_metrics(*args)                                       # full: left alone
    assert int(cursor.item()) == 2 and torch.equal(table, keep)
    cursor.fill_(-1)
    ops.flow_metrics(*args)                                       # a corrupt cursor: left alone, too
    assert int(cursor.item()) == -1 and torch.equal(table, keep)


def test_prediction_already_at_label_size():
    """The reference's call form: the prediction resized first (ops.resize_map), scaled in torch by the float32 factors, then the
    objective with (h, w) == (H, W), whose own factors are 1. The interpolated values are the resized map's bit for bit and the pixel
    pass is the same, so the loss is EQUAL to the low-resolution call's; it and the gradient, now in the full-size prediction, also
    against the plain FlowLoss of that tensor in float64."""
    from eventpretrain_amd import ops
    s, buf, m, tgt, val, org = _dev_case("slice")
    B, h, w, H, W = (s[k] for k in ("B", "h", "w", "H", "W"))
    out, _ = _fwd(s, buf, tgt, val)
    factors = torch.tensor([W / w, H / h], device="cuda")
    full = (ops.resize_map(m, B, h, w, H, W).detach() * factors).contiguous().requires_grad_(True)
    loss = ops.FlowObjectiveFn.apply(full, B, H, W, tgt, val, s["max_flow"])
    assert torch.equal(loss.detach(), out[0])
    (g,) = torch.autograd.grad(1.7 * loss, full)
    p = full.detach().double().cpu().view(B, H, W, 2).permute(0, 3, 1, 2).requires_grad_(True)
    t64, mask = tgt.double().cpu(), ft.loss_mask(tgt.double().cpu(), val.cpu(), s["max_flow"]).repeat(1, 2, 1, 1)
    plain = (p[mask] - t64[mask]).abs().mean()
    (gp,) = torch.autograd.grad(1.7 * plain, p)
    want = dict(l1=plain.detach(), grad={1.7: gp.permute(0, 2, 3, 1).reshape(-1, 2)})
    assert ft.compare(dict(l1=loss.item(), grad={1.7: g}), want) == []


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from eventpretrain_amd import ops
    s, buf, m, tgt, val, org = _dev_case("slice")
    gw = torch.tensor(1.7, device="cuda")

    def run():
        leaf = m.detach().requires_grad_(True)
        loss = ops.FlowObjectiveFn.apply(leaf, s["B"], s["h"], s["w"], tgt, val, s["max_flow"])
        (g,) = torch.autograd.grad(gw * loss, leaf)
        table, _ = _metrics(s, m, tgt, val, org)
        return [loss.detach().view(1), g.detach(), table]
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
        for x in held:
            x.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, held):
            assert torch.equal(a, b)


def test_python_api_on_a_heads_prediction():
    """FlowLoss and flow_compute_metrics take (B, 2, h, w): the permuted view of the padded map is read where it lies and gives the
    bits of the C-ABI call; a contiguous NCHW tensor gives them too (gathered into a map first); a `valid` of another dtype is
    converted; an event grid of another size is refused."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.testing import make_args
    from eventpretrain_amd.trainer.finetune_flow.flow_loss import FlowLoss
    from eventpretrain_amd.trainer.finetune_flow.flow_metric import flow_compute_metrics
    s, buf, m, tgt, val, org = _dev_case("slice")
    a = make_args(phase="finetune_flow", max_flow=s["max_flow"], sample_mode="bilinear", device="cuda")
    out, saved = _fwd(s, buf, tgt, val)
    g = _bwd(s, buf, tgt, val, saved, 1.0)
    pred = m.view(s["B"], s["h"], s["w"], 2).permute(0, 3, 1, 2).detach().requires_grad_(True)
    crit = FlowLoss(a)
    loss = crit(pred, tgt, val)
    assert loss.dim() == 0 and torch.equal(loss.detach(), out[0])
    loss.backward()
    assert torch.equal(pred.grad.permute(0, 2, 3, 1).reshape(-1, 2), g[:, :2])
    assert torch.equal(crit(pred.detach().contiguous(), tgt, val), out[0])
    assert torch.equal(crit(pred.detach(), tgt, val.double()), out[0])
    table, _ = _metrics(s, m, tgt, val, org)
    l1, aee, outlier = flow_compute_metrics(a, pred.detach(), tgt, val, org)
    assert torch.equal(torch.stack([l1, aee, outlier]), table[0])
    with pytest.raises(ValueError, match="label's size"):
        flow_compute_metrics(a, pred.detach(), tgt, val, org[:, :, :-1])
    with pytest.raises(ValueError):
        ops.flow_metrics(m, s["B"], s["h"], s["w"], tgt, val, s["max_flow"], org[:1], table, torch.zeros(1, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------------------------------------- the trainer
MAX_FLOW = 8.0


def _trainer_args(graph):
    from eventpretrain_amd.testing import make_args
    a = make_args(phase="finetune_flow", model_size="small", backbone_type="vit", num_classes=11, mask_ratio=0.0, sample_mode="bilinear",
                  device="cuda", drop_rate=0.0, drop_path_rate=0.0, clip_grad=None, max_flow=MAX_FLOW, decode_loss_weight=1.0,
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
        level = (det_uniform(f"flow.train.valid.{i}", (2, 1, 40, 56), 0.0, 1.0) * 4).floor().clamp(0, 3).long()
        org = det_normalish(f"flow.train.org.{i}", (2, 5, 40, 56)) * (det_uniform(f"flow.train.events.{i}", (2, 1, 40, 56), 0.0, 1.0) >= 0.5)
        batches.append(dict(events_voxel_grid=det_normalish(f"flow.train.x.{i}", (2, 5, 224, 224)) * 0.5, events_voxel_grid_org=org,
                            flow_label=det_normalish(f"flow.train.label.{i}", (2, 2, 40, 56)) * 4.0,
                            flow_label_valid=torch.tensor(ft.VALID_LEVELS)[level], seq_name=["s"] * 2))
    return batches


def test_trainer_captured_against_eager_and_truth():
    """ViT-Small hub, B = 2, labels 40 x 56, three batches: the captured epoch and the eager one (args.graph_step = False) return
    equal meters and leave bit-equal weights and buffers; the first batch's loss_total equals the truth on the model's own predictions
    within 1e-4; ft_flow_val captured equals its eager loop within 1e-6 per meter. The compute dtype is bf16, the mode in which a
    step of this code base has one set of bits (test_gpu_semseg_objective.py says why); the objective itself is float32 either way."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.trainer.finetune_flow.ft_flow_trainer import ft_flow_train_one_epoch, ft_flow_val
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    ops.set_compute_dtype(torch.bfloat16)
    loader = _loader()
    res, models = {}, {}
    for mode in ("eager", "graph"):
        a = _trainer_args(mode == "graph")
        m, opt = _hub(a)
        stats = ft_flow_train_one_epoch(a, m, loader, opt, 0, NativeScalerWithGradNormCount())
        assert list(stats) == ["lr", "loss_total"]
        if mode == "graph":
            assert m._evp_auto_executor[1].note == "hip-graph" and len(m._evp_auto_executor[1].inputs) == 3      # no events_voxel_grid_org
        else:
            assert not hasattr(m, "_evp_auto_executor")
        res[mode], models[mode] = stats, (a, m)
    print("train:", res)
    assert res["graph"] == res["eager"]
    for (k, p), (_, q) in zip(models["graph"][1].state_dict().items(), models["eager"][1].state_dict().items()):
        assert torch.equal(p, q), k
    # the first batch's loss_total against the truth on the model's own predictions (a third model from the same start)
    a = _trainer_args(False)
    m, opt = _hub(a)
    m.train()
    with torch.no_grad():
        out = m(loader[0]["events_voxel_grid"].cuda())
    want = 0.0
    b0 = loader[0]
    for pred, wgt in ((out[-2], a.decode_loss_weight), (out[-1], a.aux_loss_weight)):
        B, C, h, w = pred.shape
        assert C == 2
        t = ft.truth(pred.permute(0, 2, 3, 1).reshape(-1, 2).cpu(), B, h, w, b0["flow_label"], b0["flow_label_valid"], b0["events_voxel_grid_org"],
                     MAX_FLOW, need_grad=False)
        assert 0 < t["n_valid"] < B * 40 * 56 // 2
        want += wgt * float(t["l1"])
    first = ft_flow_train_one_epoch(a, m, loader[:1], opt, 0, NativeScalerWithGradNormCount())["loss_total"]
    print(f"first batch: loss_total {first!r}, truth {want!r}, rel {abs(first - want) / want:.2e}")
    assert abs(first - want) <= 1e-4 * abs(want)
    # evaluation: the captured loop against the eager one, on the trained model
    a, m = models["graph"]
    val = {}
    for graph in (True, False):
        a.graph_step = graph
        val[graph] = ft_flow_val(a, m, loader, 0, "mvsec")
        assert list(val[graph]) == ["decode_l1_loss", "decode_aee_sparse", "decode_outlier_sparse"]
    assert m._evp_auto_eval[1].note == "hip-graph" and m._evp_auto_eval[1].replays == 3
    print("val:", val)
    for k in val[True]:
        assert val[True][k] == pytest.approx(val[False][k], rel=1e-6), k

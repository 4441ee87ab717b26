"""Captured evaluation on the GPU: evp_cls_metrics through the C-ABI against a float64 cross entropy and CPU torch.topk, its
tie / NaN / bad-label rules against the rule restated here, the device cursor, and ft_val's captured form (engine.GraphedEval +
the device metrics table) against the eager loop it stands in for -- same dict, one capture, weights that change in between.

The float64 reference is restated in this file. Accuracies are compared with float equality: the kernel and the eager meters
both compute float32(hits) * float32(100 / R). The loss bound, 1e-5 relative to the float64 value, is the one
test_label_smoothing_and_grad_clipping holds the training cross-entropy kernel to."""
import io
import math
import types
from contextlib import redirect_stdout

import pytest
import torch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ references
def _pct(hits, R):
    """float32(hits) * float32(100 / R): what `hit.float().sum() * (100.0 / R)` evaluates to."""
    return (torch.tensor(float(hits), dtype=torch.float32) * (100.0 / R)).item()


def _ref_topk(logits, labels):
    """{loss (float64), acc1, acc5} of tie-free f32 logits [R, n]: float64 cross entropy, hits from CPU torch.topk."""
    R, n = logits.shape
    loss = (torch.logsumexp(logits.double(), 1) - logits.double().gather(1, labels.view(-1, 1)).squeeze(1)).mean().item()
    maxk = min(5, n)
    idx = logits.topk(maxk, 1, True, True).indices
    hit = idx.eq(labels.view(-1, 1))
    return loss, _pct(hit[:, :1].any(1).sum().item(), R), _pct(hit[:, :maxk].any(1).sum().item(), R)


def _before(a, j, x, lab):
    """Column j (value a) precedes the label's column: larger first, NaN above every number, equal values lower index first."""
    an, xn = math.isnan(a), math.isnan(x)
    if an or xn:
        return an and (not xn or j < lab)
    return a > x or (a == x and j < lab)


def _ref_rule(logits, labels):
    """The rule of include/evtpretrain.h spelt out row by row, ties, NaN and out-of-range labels included."""
    R, n = logits.shape
    h1 = h5 = 0
    loss = 0.0
    for r in range(R):
        row, lab = logits[r].tolist(), int(labels[r])
        if not 0 <= lab < n:
            loss = float("nan")
            continue
        rank = sum(1 for j in range(n) if j != lab and _before(row[j], j, row[lab], lab))
        h1 += rank < 1
        h5 += rank < min(5, n)
        loss += (torch.logsumexp(logits[r].double(), 0) - logits[r, lab].double()).item()
    return loss / R, _pct(h1, R), _pct(h5, R)


def _run_kernel(logits, labels, ld=None, table=None, cursor=None, capacity=None, pad=float("nan")):
    """One evp_cls_metrics call through the C-ABI on logits [R, n] stored with leading dimension ld (the padding holds NaN: a kernel
    that read it as a class would say so) -> (table, cursor) on the device."""
    from eventpretrain_amd import _lib
    R, n = logits.shape
    ld = n if ld is None else ld
    buf = torch.full((R, ld), pad, dtype=torch.float32)
    buf[:, :n] = logits
    buf = buf.cuda()
    lab = labels.cuda()
    table = torch.full((4, 3), -7.0, device="cuda") if table is None else table
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda") if cursor is None else cursor
    ws = torch.empty(_lib.CLS_METRICS_WS, device="cuda") if R > _lib.CLS_METRICS_SINGLE_ROWS else None
    _lib.call("evp_cls_metrics", buf.data_ptr(), lab.data_ptr(), R, n, ld, cursor.data_ptr(), table.data_ptr(),
              table.shape[0] if capacity is None else capacity, _lib.ptr(ws), _lib.stream_ptr())
    torch.cuda.synchronize()
    return table, cursor


def _tie_free_logits(R, n, seed):
    """randn * 2 from a seeded CPU generator with the values of every row pairwise distinct: rows that hold a collision (among 1000
    float32 normals one row in a few hundred does) are taken from the next seed's draw, until none is left."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, n, generator=g) * 2
    while True:
        tied = (x.sort(1).values.diff(dim=1) == 0).any(1)
        if not bool(tied.any()):
            return x, g
        seed += 1
        x[tied] = (torch.randn(R, n, generator=torch.Generator().manual_seed(seed)) * 2)[tied]


# ------------------------------------------------------------------------------------------------ 1. kernel against float64
@pytest.mark.parametrize("n_cls", [2, 5, 10, 101, 1000, 1030])
def test_cls_metrics_against_float64_and_topk(n_cls):
    """R in {1, 6, 65, 1030} (one wave, a few, more rows than one pass of the single workgroup's 16 waves, and the two-launch form
    above 1024 rows) x ld = n_cls and ld padded to the next multiple of 8 (the float4 path; 1000 takes it unpadded too). Labels: uniform
    with column 0 and column n_cls - 1 forced in, and a second set that puts row r's label at rank r % 8 so that both accuracies
    sit between 0 and 100."""
    for R in (1, 6, 65, 1030):
        x, g = _tie_free_logits(R, n_cls, 100 * n_cls + R)
        assert bool((x.sort(1).values.diff(dim=1) != 0).all())          # pairwise distinct per row: the hit counts are exact
        uniform = torch.randint(0, n_cls, (R,), generator=g)
        uniform[0] = n_cls - 1
        if R > 1:
            uniform[1] = 0
        order = x.argsort(1, descending=True)
        ranked = order[torch.arange(R), torch.arange(R) % min(8, n_cls)]
        for labels in (uniform, ranked):
            loss, acc1, acc5 = _ref_topk(x, labels)
            for ld in (n_cls, (n_cls + 7) // 8 * 8):
                table, cursor = _run_kernel(x, labels, ld)
                got = table[0].tolist()
                print(f"R={R} n_cls={n_cls} ld={ld}: loss {got[0]!r} (f64 {loss!r}, rel {abs(got[0] - loss) / abs(loss):.2e}) acc1 {got[1]!r}/{acc1!r} acc5 {got[2]!r}/{acc5!r}")
                assert cursor.item() == 1 and bool((table[1:] == -7.0).all()), (R, n_cls, ld)
                assert got[1] == acc1 and got[2] == acc5, (R, n_cls, ld, got, acc1, acc5)
                assert abs(got[0] - loss) <= 1e-5 * abs(loss), (R, n_cls, ld, got[0], loss)
        if R >= 6 and n_cls >= 10:
            assert 0.0 < _ref_topk(x, ranked)[1] < _ref_topk(x, ranked)[2] < 100.0


# ------------------------------------------------------------------------------------------------ 2. ties, NaN, bad labels
def _check_rule(rows, labels, want=None, ld=None):
    x, lab = torch.tensor(rows, dtype=torch.float32), torch.tensor(labels, dtype=torch.int64)
    loss, acc1, acc5 = _ref_rule(x, lab)
    for ld_ in ((x.shape[1], (x.shape[1] + 7) // 8 * 8) if ld is None else (ld,)):
        got = _run_kernel(x, lab, ld_)[0][0].tolist()
        assert got[1] == acc1 and got[2] == acc5, (got, acc1, acc5)
        if math.isnan(loss):
            assert math.isnan(got[0]), got
        else:
            assert abs(got[0] - loss) <= 1e-5 * abs(loss), (got[0], loss)
        if want is not None:
            assert got[1] == _pct(want[0], x.shape[0]) and got[2] == _pct(want[1], x.shape[0]), (got, want)
    return loss


def test_cls_metrics_ties_nan_and_bad_labels():
    nan = float("nan")
    # the label's value duplicated: only a LOWER index precedes it
    #   row 0: duplicate at a lower and at a higher index, nothing larger: rank 1 -> top-1 miss, top-5 hit
    #   row 1: four larger values and a duplicate at a HIGHER index only: rank 4 -> top-5 hit (5 if the duplicate counted)
    #   row 2: a duplicate at a higher index only, nothing larger: rank 0 -> top-1 hit
    ties = [[1.0, 5.0, 2.0, 5.0, 0.0, 5.0, 3.0],
            [9.0, 8.0, 2.0, 7.0, 6.0, 2.0, 1.0],
            [4.0, 0.0, 1.0, 4.0, 2.0, 3.0, -1.0]]
    assert not math.isnan(_check_rule(ties, [3, 2, 0], want=(1, 3)))
    # four larger and a duplicate at a LOWER index: rank 5 -> miss for both
    _check_rule([[9.0, 8.0, 2.0, 7.0, 6.0, 2.0, 1.0]], [5], want=(0, 0))
    # a NaN at a non-label column outranks the label (otherwise the row's maximum) and the loss is NaN; neighbours keep their hits
    assert math.isnan(_check_rule([[1.0, nan, 3.0, 0.0, 2.0, -1.0, 0.5], [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0]],
                                  [2, 6, 0], want=(2, 3)))
    # the label's own logit is NaN: it is the largest; another NaN at a lower index precedes it, one at a higher index does not
    assert math.isnan(_check_rule([[1.0, 2.0, nan, 0.0, 3.0, 4.0, 5.0]], [2], want=(1, 1)))
    assert math.isnan(_check_rule([[nan, 2.0, nan, 0.0, 3.0, 4.0, 5.0]], [2], want=(0, 1)))
    assert math.isnan(_check_rule([[1.0, 2.0, nan, 0.0, nan, 4.0, 5.0]], [2], want=(1, 1)))
    # labels -1 and n_cls: nothing out of range is read, a miss for both k, loss NaN, the neighbouring rows' hits unaffected
    good = [[0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0], [1.0, 7.0, 2.0, 3.0, 4.0, 5.0, 6.0]]
    for bad in (-1, 7, 1 << 40, -(1 << 40)):
        assert math.isnan(_check_rule(good, [6, bad, 1], want=(2, 2)))
        assert math.isnan(_check_rule(good, [bad, 0, 1], want=(2, 2)))
    assert not math.isnan(_check_rule(good, [6, 0, 1], want=(3, 3)))
    # two classes: acc5 is the top-2 rate
    _check_rule([[0.0, 1.0], [0.0, 1.0], [2.0, 1.0]], [0, 1, 0], want=(2, 3))
    # a long row (more than the 1024 columns a wave holds), ascending: the label's value duplicated in an earlier chunk
    long_row = torch.linspace(-3, 3, 1100).tolist()
    _check_rule([long_row], [1099], want=(1, 1), ld=1100)
    long_row[10] = long_row[1095]          # four larger values (1096..1099) and the duplicate at a lower index: rank 5
    _check_rule([long_row], [1095], want=(0, 0), ld=1100)
    _check_rule([long_row], [1096], want=(0, 1), ld=1104)
    long_row[1097] = nan                   # a NaN in a later chunk than the label's
    assert math.isnan(_check_rule([long_row], [20], want=(0, 0), ld=1100))


# ------------------------------------------------------------------------------------------------ 3. cursor
def test_cls_metrics_cursor_and_determinism():
    batches = []
    for i, (R, n) in enumerate(((6, 10), (65, 101), (1030, 37))):
        x, g = _tie_free_logits(R, n, 7 + i)
        batches.append((x, torch.randint(0, n, (R,), generator=g)))

    def fill(capacity=None, rows=4, start=0):
        table = torch.full((rows, 3), -7.0, device="cuda")
        cursor = torch.full((1,), start, dtype=torch.int64, device="cuda")
        for x, lab in batches:
            _run_kernel(x, lab, table=table, cursor=cursor, capacity=capacity)
        return table.cpu(), cursor.item()

    table, cur = fill()
    assert cur == 3 and bool((table[3] == -7.0).all())
    for i, (x, lab) in enumerate(batches):
        loss, acc1, acc5 = _ref_topk(x, lab)
        assert table[i, 1].item() == acc1 and table[i, 2].item() == acc5 and abs(table[i, 0].item() - loss) <= 1e-5 * abs(loss), i
    again, cur2 = fill()
    assert cur2 == 3 and torch.equal(table.view(torch.int32), again.view(torch.int32))       # bit-identical
    # capacity 2 inside a 4-row table: the third call leaves table and cursor untouched
    small, cur = fill(capacity=2)
    assert cur == 2 and torch.equal(small[:2].view(torch.int32), table[:2].view(torch.int32)) and bool((small[2:] == -7.0).all())
    # a cursor preset to -1 (and one far out of range) writes nothing
    for start in (-1, 1 << 40):
        untouched, cur = fill(start=start)
        assert cur == start and bool((untouched == -7.0).all())


def test_ops_cls_metrics_reads_a_padded_head_output_in_place():
    """ops.cls_metrics on the column slice LinearFn returns for a 10-class head (leading dimension 16) and on a contiguous copy:
    the same bits, one slot each."""
    from eventpretrain_amd import ops
    x, g = _tie_free_logits(6, 10, 3)
    labels = torch.randint(0, 10, (6,), generator=g)
    padded = torch.full((6, 16), float("nan"))
    padded[:, :10] = x
    pred = padded.cuda()[:, :10]
    assert pred.stride(0) == 16
    table, cursor = torch.zeros(4, 3, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.cls_metrics(pred, labels.cuda(), table, cursor)
    ops.cls_metrics(pred.contiguous(), labels.cuda(), table, cursor)
    ops.cls_metrics(pred[:1], labels.cuda()[:1], table, cursor)
    assert cursor.item() == 3 and torch.equal(table[0], table[1])
    loss, acc1, acc5 = _ref_topk(x, labels)
    assert table[0, 1].item() == acc1 and table[0, 2].item() == acc5 and abs(table[0, 0].item() - loss) <= 1e-5 * abs(loss)
    assert table[2, 1].item() == _ref_topk(x[:1], labels[:1])[1]


# ------------------------------------------------------------------------------------------------ 4-6. ft_val
_HUBS = {}


def _hub(bt="vit", num_classes=10, dataset_type="n-caltech101", fresh=False):
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.testing import det_fill_module_, make_args
    a = make_args(phase="finetune_cls", model_size="small" if bt == "vit" else "tiny", backbone_type=bt, num_classes=num_classes,
                  mask_ratio=0.0, device="cuda", dataset_type=dataset_type, clip_grad=None, smoothing=0)
    key = (bt, num_classes)
    if fresh or key not in _HUBS:
        m = (ft.finetune_cls_hub_model_small_patch16 if bt == "vit" else ft.finetune_cls_hub_model_swin_tiny_window7)(a)
        det_fill_module_(m)
        m = m.cuda()
        if fresh:
            return a, m
        _HUBS[key] = m
    return a, _HUBS[key]


def _val_loader(model, num_classes, sizes=(4, 4, 4, 3)):
    """Batches of det_normalish voxels with distinct tags; labels from one eager pass so that hits and misses both occur: the
    model's own top class for even samples, the class after it for odd ones."""
    from eventpretrain_amd.testing import det_normalish
    loader = []
    model.eval()
    with torch.no_grad():
        for i, b in enumerate(sizes):
            x = det_normalish(f"eval.voxels.{i}", (b, 5, 224, 224)) * 0.5
            top = model(x.cuda())[-2].argmax(1).cpu()
            label = (top + (torch.arange(b) % 2)) % num_classes
            loader.append(dict(events_voxel_grid=x, label=label, image_name=["s"] * b))
    return loader


def _val(a, m, loader, **over):
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_val
    with redirect_stdout(io.StringIO()):
        return ft_val(types.SimpleNamespace(**dict(vars(a), **over)), m, loader, 0)


def _same(got, want, keys=("loss_cls", "acc1", "acc5")):
    assert set(got) == set(want) == set(keys), (got, want)
    for k in keys:
        if k == "loss_cls":
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (got, want)
        else:
            assert got[k] == want[k], (got, want)


@pytest.fixture
def bf16():
    from eventpretrain_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.float32)


def test_captured_ft_val_equals_the_eager_loop(bf16):
    a, m = _hub()
    loader = _val_loader(m, 10)
    eager = _val(a, m, loader, graph_step=False)
    assert getattr(m, "_evp_auto_eval", None) is None                # the opt-out builds nothing
    captured = _val(a, m, loader)
    print("eager", eager, "captured", captured)
    _same(captured, eager)
    assert 0.0 < captured["acc1"] < 100.0
    ex = m._evp_auto_eval[1]
    assert ex.note == "hip-graph" and (ex.captures, ex.replays, ex.eager_calls) == (1, 3, 1), (ex.note, ex.captures, ex.replays, ex.eager_calls)
    again = _val(a, m, loader)                                       # a second evaluation re-uses the capture
    assert again == captured and m._evp_auto_eval[1] is ex and (ex.captures, ex.replays, ex.eager_calls) == (1, 6, 2)
    # a table smaller than the loader (its own executor: the slots are part of the key): flushed when full, nothing lost
    small = _val(a, m, loader, eval_table_slots=2)
    assert small == captured and m._evp_auto_eval[1] is not ex and m._evp_auto_eval[1].table.capacity == 2
    # a progress line every other batch reads the table back mid-loop
    assert _val(a, m, loader, print_freq=2) == captured


def test_captured_ft_val_n_cars_has_no_acc5(bf16):
    a, m = _hub(num_classes=2, dataset_type="n-cars")
    loader = _val_loader(m, 2, sizes=(4, 4, 3))
    eager = _val(a, m, loader, graph_step=False)
    captured = _val(a, m, loader)
    _same(captured, eager, keys=("loss_cls", "acc1"))
    assert m._evp_auto_eval[1].note == "hip-graph"


def test_captured_ft_val_swin_tiny(bf16):
    a, m = _hub("swin")
    loader = _val_loader(m, 10, sizes=(4, 4, 3))
    eager = _val(a, m, loader, graph_step=False)
    captured = _val(a, m, loader)
    _same(captured, eager)
    ex = m._evp_auto_eval[1]
    assert ex.note == "hip-graph" and (ex.captures, ex.replays, ex.eager_calls) == (1, 2, 1)


def test_weights_that_change_between_evaluations(bf16):
    """FusedAdamW graph replays between two evaluations need nothing (same parameter and shadow buffers); load_state_dict leaves
    the bf16 shadows stale and .current() re-casts them in place; shadows re-allocated by an eager pass build a new executor."""
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_uniform
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    a, m = _hub(fresh=True)
    loader = _val_loader(m, 10, sizes=(4, 4, 3))
    first = _val(a, m, loader)
    ex = m._evp_auto_eval[1]
    a.lr, a.min_lr, a.warmup_epochs, a.epochs = 5e-3, 1e-4, 0, 4
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, a.weight_decay, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
    with redirect_stdout(io.StringIO()):
        ft_train_one_epoch(a, m, loader[:2], opt, 0, NativeScalerWithGradNormCount())      # two captured steps
    assert m._evp_auto_executor[1].note.startswith("hip-graph")
    second = _val(a, m, loader)
    assert m._evp_auto_eval[1] is ex and ex.captures == 1
    _same(second, _val(a, m, loader, graph_step=False))
    assert abs(second["loss_cls"] - first["loss_cls"]) > 1e-3 * abs(first["loss_cls"]), (first, second)

    def reload(scale):
        sd = {k: (v * scale + det_uniform("reload." + k, v.shape).to(v.device) * 0.01 if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
    reload(0.9)                                   # versions move, the shadows are stale: the captured form first
    third = _val(a, m, loader)
    assert m._evp_auto_eval[1] is ex and ex.captures == 1
    _same(third, _val(a, m, loader, graph_step=False))
    assert abs(third["loss_cls"] - second["loss_cls"]) > 1e-3 * abs(second["loss_cls"]), (second, third)
    reload(1.1)                                   # the eager loop first: ops.lp_weight allocates new shadows
    eager = _val(a, m, loader, graph_step=False)
    fourth = _val(a, m, loader)
    assert m._evp_auto_eval[1] is not ex and m._evp_auto_eval[1].note == "hip-graph"
    _same(fourth, eager)

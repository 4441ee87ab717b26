"""CPU-side checks of the captured evaluation path: evp_cls_metrics is declared, exported and bound and validates its arguments on
the host before any launch; the flush-and-rewind bookkeeping of ft_val's deferred loop, driven with a stub executor whose `run`
appends known triples to a CPU table; a CPU device takes the eager loop."""
import ctypes
import io
import os
import re
import types
from contextlib import redirect_stdout

import pytest
import torch

from conftest import ROOT


def test_cls_metrics_is_declared_exported_and_bound():
    from eventpretrain_amd import _lib
    txt = open(os.path.join(ROOT, "include", "evtpretrain.h")).read()
    assert re.search(r"\bint\s+evp_cls_metrics\s*\(", txt)
    assert "ft_cls_trainer.py:152-164" in txt and "EVP_ABI_VERSION 5" in txt
    for name, value in (("SINGLE_ROWS", _lib.CLS_METRICS_SINGLE_ROWS), ("WS", _lib.CLS_METRICS_WS)):
        assert int(re.search(r"#define EVP_CLS_METRICS_%s (\d+)" % name, txt).group(1)) == value
    _lib.build_library()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "evp_cls_metrics")
    assert "evp_cls_metrics" in _lib.exported_symbols() and len(_lib.SIGNATURES["evp_cls_metrics"]) == 10
    assert "metrics.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


def test_cls_metrics_argument_validation_without_gpu():
    """EVP_EINVAL (-1) for null pointers, EVP_ESHAPE (-2) for shapes; nothing is launched (no device here). The pointers are never
    dereferenced on the host, so any non-null value serves."""
    from eventpretrain_amd import _lib
    lib = _lib.load()
    p = 4096
    ok = dict(logits=p, labels=p, R=4, n_cls=10, ld=16, cursor=p, table=p, capacity=8, ws=None)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.evp_cls_metrics(a["logits"], a["labels"], a["R"], a["n_cls"], a["ld"], a["cursor"], a["table"], a["capacity"], a["ws"], None)

    for name in ("logits", "labels", "cursor", "table"):
        assert rc(**{name: None}) == -1, name
        assert b"null" in lib.evp_last_error()
    assert rc(R=0) == -2 and rc(R=-3) == -2
    assert rc(n_cls=0) == -2
    assert rc(ld=9) == -2                      # ld < n_cls
    assert b"bad shape" in lib.evp_last_error()
    assert rc(capacity=0) == -2
    assert b"slot" in lib.evp_last_error()
    assert rc(R=_lib.CLS_METRICS_SINGLE_ROWS + 1) == -1      # the two-launch form needs its workspace
    assert b"workspace" in lib.evp_last_error()


def test_ops_cls_metrics_refuses_cpu_tensors():
    from eventpretrain_amd import ops
    from eventpretrain_amd._lib import EvpError
    with pytest.raises(EvpError):
        ops.cls_metrics(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ ft_val bookkeeping
class _CpuTable:
    """engine.MetricsTable's surface on the CPU, with a count of the read-backs."""

    def __init__(self, capacity):
        self.capacity, self.rows, self.cursor, self.reads = capacity, torch.zeros(capacity, 3), 0, []

    def rewind(self):
        self.cursor = 0

    def read(self, n):
        assert n == self.cursor, (n, self.cursor)          # the host's count of queued batches is the device cursor
        self.reads.append(n)
        vals = self.rows[:n].tolist()
        self.rewind()
        return vals


class _StubExecutor:
    """`run` / `eager_with` write the triple the test planned for the batch (identified by its first voxel) into the next slot, as
    the kernel does: a full table is left alone."""

    def __init__(self, capacity, triples, first):
        self.table, self.triples, self.inputs = _CpuTable(capacity), triples, [t.clone() for t in first]
        self.runs = self.eagers = 0

    def _push(self, x):
        if self.table.cursor < self.table.capacity:
            self.table.rows[self.table.cursor] = torch.tensor(self.triples[int(x.flatten()[0])])
            self.table.cursor += 1

    def run(self, x, y):
        assert tuple(x.shape) == tuple(self.inputs[0].shape)
        self.runs += 1
        self._push(x)

    def eager_with(self, x, y):
        assert tuple(x.shape) != tuple(self.inputs[0].shape)
        self.eagers += 1
        self._push(x)


def _loader(n_full, short=True):
    sizes = [4] * n_full + ([3] if short else [])
    return [dict(events_voxel_grid=torch.full((b, 1, 2, 2), float(i)), label=torch.zeros(b, dtype=torch.int64), image_name=["s"] * b)
            for i, b in enumerate(sizes)]


def _triples(n):
    return [[0.5 + 0.25 * i, float((37 * i) % 101), float(100 - i)] for i in range(n)]


class _RecordingLogger:
    def __new__(cls):
        from eventpretrain_amd.utils import misc
        lg = misc.MetricLogger(delimiter="  ")
        lg.calls = []
        inner = lg.update

        def update(**kw):
            lg.calls.extend(kw.items())
            inner(**kw)
        lg.update = update
        return lg


def _args(**kw):
    from eventpretrain_amd.testing import make_args
    return make_args(**dict(dict(phase="finetune_cls", device="cpu", dataset_type="n-caltech101"), **kw))


@pytest.mark.parametrize("capacity,print_freq,reads", [(4096, 1000, [6]), (2, 1000, [2, 2, 2]), (4096, 4, [4, 2]), (3, 2, [2, 2, 2]), (5, 1000, [5, 1])])
def test_deferred_loop_flushes_in_order_and_loses_nothing(capacity, print_freq, reads):
    from eventpretrain_amd.trainer.finetune_cls import ft_cls_trainer as ft
    loader, tri = _loader(5), _triples(6)
    made = []

    def executor_for(tensors):
        made.append(_StubExecutor(capacity, tri, tensors))
        return made[-1]
    lg = _RecordingLogger()
    with redirect_stdout(io.StringIO()):
        ft._val_loop_deferred(_args(print_freq=print_freq), loader, lg, executor_for, True)
    (ex,) = made
    assert ex.runs == 5 and ex.eagers == 1 and ex.table.reads == reads
    want = [kv for t in tri for kv in (("loss_cls", t[0]), ("acc1", t[1]), ("acc5", t[2]))]
    assert lg.calls == want                                         # one update per meter per batch, in batch order
    # the returned averages are what per-batch updates give: every batch weighs the same, the short last one included
    for j, k in enumerate(("loss_cls", "acc1", "acc5")):
        assert lg.meters[k].count == 6 and lg.meters[k].global_avg == pytest.approx(sum(t[j] for t in tri) / 6, rel=1e-12)


def test_deferred_loop_n_cars_has_no_acc5():
    from eventpretrain_amd.trainer.finetune_cls import ft_cls_trainer as ft
    loader, tri = _loader(3, short=False), _triples(3)
    lg = _RecordingLogger()
    with redirect_stdout(io.StringIO()):
        ft._val_loop_deferred(_args(dataset_type="n-cars"), loader, lg, lambda t: _StubExecutor(2, tri, t), False)
    assert set(lg.meters) == {"loss_cls", "acc1"} and [k for k, _ in lg.calls] == ["loss_cls", "acc1"] * 3


def test_ft_val_on_cpu_takes_the_eager_loop(monkeypatch):
    """device = "cpu": the present loop, batch by batch (model and loss stubbed: the kernels have no CPU form), and its dict equals
    what the deferred loop returns for the same per-batch values."""
    from eventpretrain_amd.trainer.finetune_cls import ft_cls_trainer as ft
    loader = _loader(2)
    logits = torch.tensor([[0.0, 3.0, 1.0, 2.0, -1.0, 0.5, -0.25]])      # label 0 ranks 5th: top-5 hit, top-1 miss

    class Model(torch.nn.Module):
        def forward(self, x):
            return None, None, None, logits.expand(x.shape[0], -1) + x.flatten(1)[:, :1], None

    class Loss:
        calls = 0

        @staticmethod
        def apply(pred, label):
            Loss.calls += 1
            return torch.nn.functional.cross_entropy(pred, label)
    monkeypatch.setattr(ft.ops, "CrossEntropyFn", Loss)
    monkeypatch.setattr(ft, "auto_eval_executor", lambda *a: pytest.fail("a CPU device must not build an executor"))
    a = _args()
    assert not ft._use_captured_eval(a, Model())
    with redirect_stdout(io.StringIO()) as out:
        stats = ft.ft_val(a, Model(), loader, 0)
    assert Loss.calls == 3 and set(stats) == {"loss_cls", "acc1", "acc5"}
    assert stats["acc1"] == 0.0 and stats["acc5"] == 100.0
    assert stats["loss_cls"] == pytest.approx(torch.nn.functional.cross_entropy(logits, torch.zeros(1, dtype=torch.int64)).item(), rel=1e-6)
    assert "* Acc@1 0.000 Acc@5 100.000" in out.getvalue() and "average inference time (ms)" in out.getvalue()


def test_the_opt_outs_keep_the_eager_loop():
    from eventpretrain_amd.trainer.finetune_cls import ft_cls_trainer as ft
    m = torch.nn.Linear(2, 2)
    on = lambda **kw: ft._use_captured_eval(types.SimpleNamespace(**dict(dict(device="cuda", graph_step=True), **kw)), m)
    assert on() and on(device="cuda:1")
    assert not on(graph_step=False) and not on(sync_every_step=True) and not on(device="cpu")
    assert not on(test_experiment=True, visualize=True) and on(test_experiment=True, visualize=False)
    m.forward = lambda x: x
    assert not on()

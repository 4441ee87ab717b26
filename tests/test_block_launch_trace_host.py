"""ViTBlockFn, ConvBlockFn and SwinBlockFn on the host, no GPU: the sequence of kernel entries, their scalar arguments, operand
shapes / dtypes / identities and the deferred-queue entries of a forward + backward + flush (tests/launch_trace.py) against
tests/golden/block_launch_trace.json, which was recorded from ops.py as it was before the blocks' MLP half and Linear backward moved
into shared helpers (`python tests/launch_trace.py --root <that tree> --write` reproduces it byte for byte).

* One test per case; a mismatch prints a unified diff of the two traces.
* Mutation: a wrapped ops._wgrad_bias that loses `dy_colsum`, and a wrapped ops._branch_grad that forces side=False, each change the
  trace of the named cases -- the trace sees the two things a rewrite of the blocks' backward could silently drop."""
import json

import pytest

from eventpretrain_amd import ops

import launch_trace as lt


@pytest.fixture(scope="module")
def golden():
    return lt.load_golden()


def _got(name):
    return json.loads(json.dumps(lt.run_case(ops, name)))       # as the golden file holds it: tuples are lists


def test_golden_file_holds_exactly_the_case_table(golden):
    assert list(golden) == list(lt.CASES)


@pytest.mark.parametrize("name", list(lt.CASES))
def test_block_launch_trace_equals_golden(name, golden):
    got = _got(name)
    assert got == golden[name], "\n" + lt.diff(golden[name], got, name)


def test_trace_restores_what_it_replaced():
    before = {k: getattr(ops, k) for k in ("call", "ptr", "stream_ptr", "_chk", "gemm", "_compute_dtype", "_use_grad_side",
                                           "_use_fused_attention", "_use_window_mfma")}
    flush, enabled = ops._deferred.flush, ops._deferred.enabled
    _got("vit_bf16_stacked_side_off_deferred_off")
    _got("swin_bf16_window_lds")
    assert before == {k: getattr(ops, k) for k in before}
    assert ops._deferred.flush == flush and ops._deferred.enabled == enabled and not ops._deferred.w and not ops._deferred.b


# the single bf16 block hands its own norm2 backward's column sums to the proj / conv2 bias; the stacked pair also the lower fc2's
COLSUM_CASES = ["vit_bf16_rd_none", "vit_bf16_stacked_side_on_deferred_on", "conv_bf16_rd_none_no_map", "swin_bf16_rd_none_groups1"]


@pytest.mark.parametrize("name", COLSUM_CASES)
def test_mutation_dropped_dy_colsum_changes_the_trace(name, golden, monkeypatch):
    real = ops._wgrad_bias

    def mutant(*a, **kw):
        kw.pop("dy_colsum", None)
        return real(*a[:11], **kw)               # (a 12th positional argument would be dy_colsum)
    monkeypatch.setattr(ops, "_wgrad_bias", mutant)
    assert _got(name) != golden[name]


@pytest.mark.parametrize("name", COLSUM_CASES)
def test_mutation_forced_side_false_changes_the_trace(name, golden, monkeypatch):
    real = ops._branch_grad

    def mutant(g, rd, which, rps, mk, T, side, lp=None):
        return real(g, rd, which, rps, mk, T, False, lp)
    monkeypatch.setattr(ops, "_branch_grad", mutant)
    assert _got(name) != golden[name]

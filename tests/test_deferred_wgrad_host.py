"""The deferred bf16 weight / bias gradient planner (wgrad_plan.layout bound by ops._DeferredGrads.build_plan) on the host, no GPU: its grouped launch
tables are run by a float64 interpreter of the four entries' ABI (tests/deferred_plan.py).

* Sweep: the per-layer problem lists of every benchmarked model (taken from the instantiated modules), batches 1-256, every
  n_chunks in 1-4 and the XCD order on and off -- contracts and coverage only (each output tile and each K row exactly once,
  each bias exactly once, first contribution writes, later ones accumulate, concurrent steps write disjoint gradients).
* Numeric: reduced shapes that reach each path, against dY^T X and sum_rows(dY) in float64.
* Mutation: one table item or K-slice removed from a copy of the tables is caught, numerically by a wide margin."""
import numpy as np
import pytest
import torch

from eventpretrain_amd import _lib, ops, wgrad_plan

import deferred_plan as dp

CONFIGS = ["vit_base_rec", "vit_base_con", "vit_base_adj", "convvit_base_rec", "swin_tiny_rec", "swin_base_rec",
           "convvit_small_rec", "vit_small_rec", "vit_tiny_rec"]
# ConvViT stage 2 (28 x 28 tokens) at these batches left a 32-row last K-slice in the G4 table before the planner folded it
SHORT_TAIL_BATCHES = (50, 58, 138, 158, 186, 194, 246)


@pytest.fixture
def switches(monkeypatch):
    def set_(g4=True, xcd=True):
        monkeypatch.setattr(ops, "_use_wgrad_g4", g4)
        monkeypatch.setattr(ops, "_wgrad_xcd_order", xcd)
    set_()
    return set_


def _sweep_one(config, B, n_chunks):
    m, phase = dp.bench_model(config)
    d = ops._DeferredGrads()
    params = dp.model_queue(m, phase, B, d)
    try:
        dp.interpret_plan(d, n_chunks, numeric=False)
    except dp.PlanError as e:
        raise AssertionError(f"{config} B={B} n_chunks={n_chunks} xcd={ops._wgrad_xcd_order}: {e}") from None
    finally:
        for p_ in params:
            p_.grad = None


@pytest.mark.slow
@pytest.mark.parametrize("config", CONFIGS)
def test_plan_sweep_contracts_and_coverage(config, switches):
    """Every batch 1-256 once (n_chunks and XCD order cycling with the batch, so every combination is met many times), and
    the batches that produced short G4 tails under all eight combinations."""
    for B in range(1, 257):
        switches(xcd=(B // 4) % 2 == 0)
        _sweep_one(config, B, 1 + B % 4)
    for B in SHORT_TAIL_BATCHES + (64,):
        for xcd in (True, False):
            switches(xcd=xcd)
            for n_chunks in (1, 2, 3, 4):
                _sweep_one(config, B, n_chunks)


def test_convvit_stage2_slices_meet_the_g4_contract(switches):
    """The issue's case: 1536 x 384 (ConvViT-Base stage-2 fc1) at rows = 50 * 784 = 39200 planned [9792] * 4 + [32]; every
    slice must now be a multiple of 32 and >= 96 rows and the slices must partition the rows."""
    for rows in (50 * 784, 58 * 784, 64 * 784, 42 * 3136):
        d = ops._DeferredGrads()
        p = torch.nn.Parameter(torch.zeros(1536, 384))
        d.wgrad(p, dp.FakeOperand(rows, 1536), dp.FakeOperand(rows, 384), 1536, 384, rows, None)
        steps = d.build_plan(1)
        ks = [int(k) for s in steps for k in s.pt.numpy().view(dp.PDT)["K"]]
        assert len(ks) > 1 and sum(ks) == rows and all(k % 32 == 0 and k >= 96 for k in ks), (rows, ks)
        assert all(s.entry == dp.G4 for s in steps)


def test_g4_contract_is_checked_on_the_host():
    ops._check_g4_problem(256, 256, 96)
    for M, N, K in [(256, 256, 32), (256, 256, 64), (256, 256, 112), (255, 256, 96), (256, 248, 96), (256, 260, 96)]:
        with pytest.raises(_lib.EvpError):
            ops._check_g4_problem(M, N, K)


def test_route_is_decided_once_and_consistent():
    """Routing of one problem needs no tensors: a fused bias implies the 256 tile and one slice, every G4 slice meets the
    contract, and the slices partition the rows."""
    for n_out, k_in in [(1536, 384), (256, 256), (768, 768), (128, 64), (264, 1032), (256, 136)]:
        for rows in list(range(1, 400)) + [b * 784 for b in range(1, 257)] + [b * 3136 for b in (8, 42, 64, 256)]:
            for g4 in (True, False):
                r = wgrad_plan.route(n_out, k_in, rows, True, g4)
                assert r.bias == ("fused" if r.tile == 256 and len(r.slices) == 1 else "listed")
                assert r.tile == (256 if g4 and rows % 32 == 0 and rows >= 96 and min(n_out, k_in) >= 256 else 128)
                assert [k0 for k0, _ in r.slices] == [sum(k for _, k in r.slices[:i]) for i in range(len(r.slices))]
                assert sum(k for _, k in r.slices) == rows
                assert r.tile == 128 or all(k % 32 == 0 and k >= 96 for _, k in r.slices), (n_out, k_in, rows, r)
                assert wgrad_plan.route(n_out, k_in, rows, False, g4) == r._replace(bias="none")


# ------------------------------------------------------------------------------------------------------ numeric cases
def _ints(shape, gen, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=gen).to(torch.bfloat16)


def _queue_case(case, gen):
    """A _DeferredGrads holding the queue of one reduced-shape case. Integer data: every partial sum is exact in float64 (and
    in f32 on the device)."""
    d = ops._DeferredGrads()
    entries = []

    def lin(n_out, k_in, rows, fused=False, listed=False, pre=False, dy=None, x=None, p=None, b=None):
        dy = _ints((rows, n_out), gen) if dy is None else dy
        x = _ints((rows, k_in), gen) if x is None else x
        p = torch.nn.Parameter(torch.zeros(n_out, k_in)) if p is None else p
        if (fused or listed) and b is None:
            b = torch.nn.Parameter(torch.zeros(n_out))
        if pre:
            p.grad = torch.full((n_out, k_in), 7.0)
            if b is not None:
                b.grad = torch.full((n_out,), -5.0)
        d.wgrad(p, dy, x, n_out, k_in, rows, b if fused else None)
        if listed:
            d.colsum(b, dy)
        entries.append((p, b, dy, x))
        return p, b

    if case == "t128_and_g4":
        lin(256, 512, 1024)                 # G4
        lin(136, 264, 200)                  # 128x128, ragged M / N, K tail
        lin(512, 256, 96)                   # G4 at the minimum K
        lin(264, 1032, 128)                 # G4, ragged M / N
        lin(1024, 64, 512)                  # 128: narrow N
    elif case == "fused_bias":
        lin(512, 256, 320, fused=True)      # G4: bias from the A fragments
        lin(256, 136, 160, fused=True)      # not G4 (N < 256): bias goes to the column-sum list
        lin(264, 264, 100, fused=True)      # not G4 (K % 32): column-sum list
    elif case == "g4_sliced_bias":
        lin(256, 256, 32768 + 512, fused=True)       # 1 output tile, K >= 32768: K-slices, bias moves to the column sums
    elif case == "t128_sliced_odd_tail":
        lin(128, 64, 32768 + 8 * 64 + 37)            # 128x128, sliced, rows not a multiple of 64 (or 32)
    elif case == "convvit_stage2_tail":
        lin(1536, 384, 50 * 784)                     # the old 32-row tail
    elif case == "two_rounds":
        p, b = lin(512, 256, 256, fused=True)
        lin(512, 256, 160, fused=True, p=p, b=b)     # second contribution (rec+con): round 1, not G4 (K % 32)
        q, _ = lin(264, 256, 192)
        lin(264, 256, 192, p=q)
        lin(264, 256, 33000, p=q)                    # third contribution: K % 32 != 0 -> 128x128 tiles, K-sliced
    elif case == "accumulate_existing":
        lin(512, 256, 256, fused=True, pre=True)
        lin(136, 264, 200, pre=True)
        lin(256, 256, 32768 + 256, fused=True, pre=True)
        lin(256, 128, 96, listed=True, pre=True)
    else:
        raise AssertionError(case)
    for p, b, dy, x in entries[:1]:
        part = torch.randint(-4, 5, (9, 520), generator=gen).float()       # LayerNorm-style partial rows (f32, N % 128 != 0)
        g = torch.nn.Parameter(torch.zeros(520))
        d.colsum(g, part)
    return d


NUMERIC_CASES = ["t128_and_g4", "fused_bias", "g4_sliced_bias", "t128_sliced_odd_tail", "convvit_stage2_tail", "two_rounds",
                 "accumulate_existing"]


def truth(w, b):
    """float64 gradient of every parameter of a queue: pre-existing .grad + sum of its contributions."""
    ref = {}

    def add(p_, v):
        if id(p_) not in ref:
            ref[id(p_)] = (p_, (p_.grad.double() if p_.grad is not None else torch.zeros(p_.shape, dtype=torch.float64, device=p_.device)))
        ref[id(p_)] = (p_, ref[id(p_)][1] + v.reshape(p_.shape))
    for (p_, dy, x, n_out, k_in, rows, bias) in w:
        add(p_, dy.double().t() @ x.double())
        if bias is not None:
            add(bias, dy.double().sum(0))
    for p_, x2d in b:
        add(p_, x2d.double().sum(0))
    return ref


@pytest.mark.parametrize("case", NUMERIC_CASES)
@pytest.mark.parametrize("n_chunks,xcd,g4", [(1, True, True), (4, True, True), (2, False, True), (1, True, False)])
def test_plan_numeric_matches_float64(case, n_chunks, xcd, g4, switches):
    switches(g4=g4, xcd=xcd)
    gen = torch.Generator().manual_seed(NUMERIC_CASES.index(case))
    d = _queue_case(case, gen)
    ref = truth(d.w, d.b)
    it, steps = dp.interpret_plan(d, n_chunks)
    if case == "convvit_stage2_tail" and g4:
        assert any(s.entry == dp.G4 and len(s.post) for s in steps)
    for p_, r in ref.values():
        assert torch.equal(it.grad(p_), r), (case, tuple(p_.shape))


# ------------------------------------------------------------------------------------------------------ mutations
def _drop_item(entry_sel, which):
    def mut(steps):
        st = next(s for s in steps if s.entry == entry_sel)
        items = st.it.numpy().view(np.int32).reshape(-1, 4)
        live = np.nonzero(items[:, 0] >= 0)[0]
        items[live[which]] = (-1, 0, 0, 0)
    return mut


def _drop_slice(steps):
    """Cut the last K-slice problem out of a sliced G4 launch (its workspace slice is then never written)."""
    st = next(s for s in steps if s.entry == dp.G4 and s.post)
    items = st.it.numpy().view(np.int32).reshape(-1, 4)
    probs = st.pt.numpy().view(dp.PDT)
    last = int(np.argmin(probs["K"]))
    items[items[:, 0] == last] = (-1, 0, 0, 0)


def _shorten_slice(steps):
    """Give the last K-slice 64 rows fewer (a slice lost at the end of the rows; every tile still present)."""
    st = next(s for s in steps if s.entry == dp.G4 and s.post)
    probs = st.pt.numpy().view(dp.PDT)
    probs["K"][int(np.argmin(probs["K"]))] -= 64


def _double_item(steps):
    st = next(s for s in steps if s.entry == dp.G4)
    items = st.it.numpy().view(np.int32).reshape(-1, 4)
    live = np.nonzero(items[:, 0] >= 0)[0]
    items[live[1]] = items[live[0]]


@pytest.mark.parametrize("mutation", ["g4_item", "t128_item", "colsum_item", "drop_slice", "shorten_slice", "double_item"])
def test_mutated_tables_are_caught(mutation, switches):
    """A copy of the tables with one item / K-slice removed fails the interpreter's checks; with the checks bypassed it misses
    the float64 truth by far more than the GPU gates of tests/test_gpu_deferred_wgrad.py allow (1e-4 of a 128x128 block's
    norm, 2e-5 of the whole gradient's)."""
    gen = torch.Generator().manual_seed(5)
    d = _queue_case("convvit_stage2_tail" if mutation in ("drop_slice", "shorten_slice") else "t128_and_g4", gen)
    ref = truth(d.w, d.b)
    mut = {"g4_item": _drop_item(dp.G4, 3), "t128_item": _drop_item(dp.T128, 2), "colsum_item": _drop_item(dp.COLSUM, 0),
           "drop_slice": _drop_slice, "shorten_slice": _shorten_slice, "double_item": _double_item}[mutation]
    w, b, fresh = dp.snapshot_queue(d)
    steps = d.build_plan(1)
    mut(steps)
    with pytest.raises(dp.PlanError):
        dp.Interpreter(w, b, fresh).run(steps)
    # the same tables run without the coverage / partition checks: the numbers are far off
    loose = dp.Interpreter(w, b, fresh)
    loose._final_checks = lambda: None
    loose._count = lambda items, count, what: [c.__iadd__(1) for c in count]
    try:
        loose.run(steps)
    except dp.PlanError:
        return           # a slice whose workspace is never written cannot even be reduced
    worst = 0.0
    for p_, r in ref.values():
        g = loose.grad(p_)
        bad = ~torch.isfinite(g)
        err = float("inf") if bad.any() else ((g - r).norm() / r.norm()).item()
        worst = max(worst, err)
    assert worst > 1e-3, (mutation, worst)

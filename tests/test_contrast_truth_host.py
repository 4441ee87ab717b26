"""The float64 gates of the contrastive stage (tests/contrast_truth.py) on the host, no GPU: the float32 restatement of every kernel in
the kernel's own order passes every gate at the shapes the GPU tests run, each single mutation of it fails at least one, and the
conditions the part-2 comparator puts on the INPUTS (non-zero yardstick error, the cap on left-out sub-blocks) hold for every case."""
import pytest
import torch
import torch.nn.functional as F

import contrast_truth as ct


def _part1_fails(mutant=None, kinds=("bn", "nce", "ce", "enq")):
    """Every part-1 gate the mutant can touch, at the small shapes (the grid-stride shapes add nothing a mutant could hide behind)."""
    fails = []
    if "bn" in kinds:
        for io in ("f32", "bf16"):
            for key in ct.bn_cases(io):
                if (key[0], key[1]) in ct.BN_GRID_STRIDE:
                    continue
                c = ct.bn_case(*key)
                fails += ct.check_bn(c, ct.bn_restated(c, mutant)).fails
    if "nce" in kinds:
        for shape in ct.NCE_SHAPES:
            c = ct.nce_case(*shape)
            fails += ct.check_nce(c, ct.nce_restated(c["pos"], c["neg"], c["K"], mutant=mutant)).fails
    if "ce" in kinds:
        for shape in ct.CE_SHAPES:
            for s in (0.0, 0.1):
                c = ct.ce_case(*shape, s)
                fails += ct.check_ce(c, ct.ce_restated(c["logits"], c["labels"], c["n_cls"], s, mutant=mutant)).fails
    if "enq" in kinds:
        for shape in ct.ENQ_SHAPES[:3]:
            c = ct.enq_case(*shape)
            for start in ct.enq_starts(c["B"], c["K"]):
                q, p = ct.enqueue_restated(c["queue"], c["keys"], start, mutant)
                fails += ct.check_enqueue(c, start, q, p).fails
    return fails


@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_batchnorm_restatement_passes_every_gate(io):
    """Slab-wise Welford + Chan in float32 / double as the kernels order it, at every shape and flag combination of the GPU test.
    Worst error over its bound here: f32 0.55, bf16 I/O 0.99 (y: 2^-8 is bf16's unit roundoff, so a correct round-to-nearest store
    reaches the bound to within its f32 term)."""
    worst = 0.0
    for key in ct.bn_cases(io):
        c = ct.bn_case(*key)
        rep = ct.check_bn(c, ct.bn_restated(c))
        assert not rep.fails, rep.fails
        worst = max(worst, max(w for _, _, w in rep.rows))
    print(f"\nbatchnorm restatement {io}: worst error / bound {worst:.3f}")


def test_batchnorm_offset_case_separates_welford_from_sum_of_squares():
    """Columns of mean 30 and unit variance: u * kappa = 6e-8 * 30 ~ 2e-6 on the variance for Welford, u * kappa^2 ~ 5e-5 for
    E[x^2] - E[x]^2. The restatement and torch's own float32 batch_norm pass the 1e-5 class at offset 30; the sum-of-squares form does
    not. Measured here (error / bound): restatement y 0.028, invstd 0.010; torch-CPU float32 y 0.10, invstd 0.007; sum of squares
    invstd 6.5."""
    R, C = ct.BN_OFFSET_SHAPE
    c = ct.bn_case(R, C, 0, True, True, "f32", ct.BN_OFFSET)
    rep = ct.check_bn(c, ct.bn_restated(c))
    assert not rep.fails, rep.fails
    x = c["x"]
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    y = F.batch_norm(x, rm, rv, c["gamma"], c["beta"], training=True, momentum=ct.MOMENTUM, eps=ct.EPS)
    tr = ct.Report("torch f32")
    tr.f32_class("y", y, c["T"]["y"])
    tr.f32_class("running_mean", rm, c["T"]["running_mean"])
    tr.f32_class("running_var", rv, c["T"]["running_var"])
    tr.f32_class("invstd", 1.0 / torch.sqrt(x.var(0, unbiased=False) + ct.EPS), c["T"]["invstd"])
    assert not tr.fails, tr.fails
    ss = ct.Report("sum of squares")
    var = (x * x).mean(0) - x.mean(0) ** 2
    ss.f32_class("invstd", 1.0 / torch.sqrt(var + ct.EPS), c["T"]["invstd"])
    print("\n" + rep.text() + "\n" + tr.text() + "\n" + ss.text())
    assert ss.fails


def test_row_loss_enqueue_and_mean_restatements_pass_every_gate():
    """l2norm / rowdot / scale_rows, InfoNCE, cross entropy (smoothing 0 and 0.1), the enqueue (tiled and element-wise, every start
    position, the guard) and the token mean at the GPU test's shapes. The truth of the row normalisation is written out; it equals
    autograd of F.normalize on the rows that are not all zero."""
    for shape in ct.SCALE_SHAPES:
        c = ct.row_case(*shape)
        rep = ct.check_rows(c, ct.rows_restated(c))
        assert not rep.fails, rep.fails
        xr = c["x"].double().clone().requires_grad_(True)
        F.normalize(xr, dim=-1).backward(c["dy"].double())
        keep = torch.arange(c["R"]) != (c["zero_row"] if c["zero_row"] is not None else -1)
        assert torch.allclose(xr.grad[keep], c["T"]["dx"][keep], rtol=1e-12, atol=1e-14)
    assert not _part1_fails(None, kinds=("nce", "ce")), _part1_fails(None, kinds=("nce", "ce"))
    for shape in ct.ENQ_SHAPES:
        c = ct.enq_case(*shape)
        for start in ct.enq_starts(c["B"], c["K"]):
            q, p = ct.enqueue_restated(c["queue"], c["keys"], start)
            assert not ct.check_enqueue(c, start, q, p).fails
        for bad in (c["K"] - c["B"] + 1, -1):
            assert torch.equal(ct.enqueue_restated(c["queue"], c["keys"], bad)[0], c["queue"])
    for shape in ct.MEAN_SHAPES:
        c = ct.mean_case(*shape)
        assert not ct.check_mean(c, ct.token_mean_restated(c["x"], c["g"])).fails


@pytest.mark.parametrize("name,mode,T_", ct.stage_runs())
def test_stage_references_and_restatement(name, mode, T_):
    """Part 2 on the host: the yardstick differs from truth in every tensor, the float32 oracle sits at the f32 class, truth keeps
    within MAX_EXCLUDED for every family (compare() asserts it), truth + once and twice the yardstick's noise passes the bf16 gates,
    and the float32 restatement of the module tail passes the f32 gates (and so the bf16 ones).
    Measured here: the f32 oracle 6e-10 to 9e-7 per tensor (the loss alone below 4e-8), the restatement at most 1.2 x it for every
    tensor but the loss (up to 56 x the oracle's draw, under the 1e-5 floor). The yardstick at T = 0.07 and, measured for the first
    time, at T = 1.0, which differ in the loss alone: loss 7e-6 to 2.5e-3 / 1.4e-6 to 2.4e-4 (pooled per loss form: queue 3.3e-4 /
    3.9e-5, in-batch 1.2e-3 / 1.1e-4), h 1.3e-2, d clip_emb 1.3e-2 to 1.6e-2, d emb_h 0.10 to 0.12, parameter gradients 1.4e-2 (the
    last head's) to 0.14, running means 3.5e-4 to 3.1e-3, running variances 1.1e-4 to 2.7e-4."""
    ref = ct.stage_reference(name, mode, T_)
    gated = [t for t in ref.tensors if t not in ("queue", "ptr")]
    for t in gated:
        assert torch.isfinite(ref.T[t]).all() and ref.T[t].norm() > 0, t
        assert ref.e_ref(t) > 0, t
        assert ref.e_f32(t) <= ct.F32_TOL, (t, ref.e_f32(t))
    def span(pick, e):
        v = [e(t) for t in gated if pick(t)]
        return f"{min(v):.1e}..{max(v):.1e}"
    groups = (("loss", lambda t: t == "loss"), ("h", lambda t: t == "act:h"), ("d clip_emb", lambda t: t == "act:d_clip_emb"),
              ("d emb_h", lambda t: t == "act:d_emb_h"), ("grads", lambda t: t.startswith("grad:")),
              ("running means", lambda t: t.endswith("running_mean")), ("running variances", lambda t: t.endswith("running_var")))
    print(f"\n{name} {mode} T={T_} yardstick: " + "  ".join(f"{g} {span(p, ref.e_ref)}" for g, p in groups) +
          f"  | f32 oracle, all tensors: {span(lambda t: True, ref.e_f32)}  | pooled loss yardstick {ct.loss_yardstick(mode, T_):.1e}")
    Y = ct.stage_yardstick(name, mode, T_)
    assert 0 < ct.loss_yardstick(mode, T_) < 1e-2
    for k in (1.0, 2.0):
        fails, worst, _ = ct.gate_bf16(name, mode, T_, {t: ref.T[t] + k * (Y[t] - ref.T[t]) for t in gated})
        assert not fails and worst[0] <= k + 1e-9, (fails, worst)
    got, keys = ct.stage_restated(name, mode, T_)
    fails, worst, table = ct.check_stage_f32(name, mode, T_, got, keys)
    print(f"restatement: worst e / e_F {worst[0]:.2f} at {worst[1]}\n{table}")
    assert not fails, fails
    fails, worst, _ = ct.check_stage_bf16(name, mode, T_, got, keys)
    assert not fails, fails


PART1_OF = {
    "last_slab_dropped": ("bn",), "empty_lane_counts_one": ("bn",), "biased_running_var": ("bn",), "momentum_on_wrong_term": ("bn",),
    "relu_mask_from_y_pre": ("bn",), "no_1_over_R_in_dx": ("bn",), "dgamma_dbeta_swapped": ("bn",), "eps_outside_sqrt": ("bn",),
    "no_positive_in_denominator": ("nce",), "one_over_T_once": ("nce",), "padding_in_softmax": ("nce", "ce"), "smoothing_over_ld": ("ce",),
    "enqueue_without_reversal": ("enq",), "pointer_without_modulo": ("enq",), "backward_reads_queue_after_enqueue": (),
}


@pytest.mark.parametrize("mutant", list(ct.MUTANTS))
def test_every_mutation_fails_a_gate(mutant):
    """One mutation of the restatement at a time: a part-1 gate of the kernel it sits in fails, and the part-2 f32 gates of the module
    tail (queue mode at T = 0.07, K = 40) fail too wherever the mutated operation is part of the tail."""
    assert sorted(PART1_OF) == sorted(ct.MUTANTS)
    fails = _part1_fails(mutant, kinds=PART1_OF[mutant])
    assert fails or not PART1_OF[mutant], f"{mutant}: no part-1 gate failed"
    in_tail = mutant not in ("smoothing_over_ld", "padding_in_softmax", "empty_lane_counts_one", "eps_outside_sqrt")
    #   smoothing is no part of the tail; at K = 40 there are no padding columns; 135 rows leave no row lane empty; at the heads' unit
    #   variances 1 / (sqrt(var) + eps) is 5e-6 from 1 / sqrt(var + eps), inside the f32 class (part 1 has columns of variance 0.0025)
    got, keys = ct.stage_restated("k40", "queue", 0.07, mutant)
    stage_fails = ct.check_stage_f32("k40", "queue", 0.07, got, keys)[0]
    print(f"\n{mutant}: {len(fails)} part-1 gates, {len(stage_fails)} part-2 gates failed")
    assert stage_fails or not in_tail, f"{mutant}: no part-2 gate failed"
    assert fails or stage_fails

"""The float64-truth gate of the bf16 Swin, ConvViT and fine-tuning steps (tests/backbone_truth.py) on the host, no GPU: the oracle
additions it rests on are pinned, its references are sane for every case the GPU tests run, and the comparator is neither vacuous nor
blind -- it accepts the yardstick's own noise, also doubled, rejects each of a list of confined defects laid over that noise, and rejects
the oracle itself run with a wrong algorithm."""
import pytest
import torch

import backbone_truth as kt
import block_truth as bt
from oracle import model_oracle as mo


def _noisy(ref, k=1.0):
    """Truth plus k times the yardstick's own error: what a correct bf16 implementation looks like to the comparator."""
    return {t: ref.T[t] + k * (ref.Y[t] - ref.T[t]) for t in ref.tensors}


def _check(name, got):
    return kt.compare_all(name, got)[0]


def _f64_state(name):
    c = kt.make_case(name)
    return c, {k: v.detach().double() if v.is_floating_point() else v.detach() for k, v in c["module"].state_dict().items()}


def test_convvit_dense_equals_the_masked_oracle_at_ratio_0():
    """mo.convvit_dense has no reference fixture of its own: it is pinned to the reference-validated mo.convvit_masked, which at mask
    ratio 0, increasing noise (ids_keep = the identity) and without fusion computes the same emb_h; float64, <= 1e-12 relative. The
    taps agree as well."""
    c, sd = _f64_state("convvit_masked")
    x = c["x"].double()
    noise = torch.arange(16.0).repeat(x.shape[0], 1)
    l1, l2, lh, mask, ids_restore = mo.convvit_masked(sd, x, noise, heads=kt.CONVVIT["heads"], mask_ratio=0.0, fusion=False, pre="")
    assert mask.sum() == 0 and torch.equal(ids_restore, torch.arange(16).repeat(x.shape[0], 1))
    d1, d2, emb_h, attn = mo.convvit_dense(sd, x, heads=kt.CONVVIT["heads"], pre="")
    assert emb_h.dtype == torch.float64 and bt.rel_err(emb_h, lh) <= 1e-12
    assert bt.rel_err(d1, l1) <= 1e-12 and bt.rel_err(d2, l2) <= 1e-12
    assert attn.shape == (x.shape[0], kt.CONVVIT["heads"], 16, 16) and torch.allclose(attn.sum(-1), torch.ones(()).double(), atol=1e-12)


def test_ft_cls_step_takes_convvit_and_smoothing():
    """ft_cls_step on the ConvViT branch is convvit_dense + token mean + head + label_smoothing_ce; smoothing 0 is plain cross-entropy."""
    c, sd = _f64_state("convvit_ft")
    x, label = c["x"].double(), c["label"]
    cfg = dict(backbone="convvit", heads=kt.CONVVIT["heads"])
    loss, pred, emb_h, attn, taps = mo.ft_cls_step(sd, x, label, cfg, smoothing=0.1, want_taps=True)
    _, _, want_h, _ = mo.convvit_dense(sd, x, heads=kt.CONVVIT["heads"])
    assert torch.equal(emb_h, want_h) and len(taps) == 2
    want = torch.nn.functional.linear(want_h.mean(1), sd["classify_head.weight"], sd["classify_head.bias"])
    assert torch.equal(pred, want)
    assert loss.item() == pytest.approx(torch.nn.functional.cross_entropy(want, label, label_smoothing=0.1).item(), rel=1e-12)
    loss0 = mo.ft_cls_step(sd, x, label, cfg)[0]
    assert loss0.item() == pytest.approx(torch.nn.functional.cross_entropy(want, label).item(), rel=1e-12)


def test_swin_masked_oracle_runs_in_float64():
    """The masked Swin forward used to allocate its dense fusion grids in the default dtype and stop on float64 inputs."""
    ref = kt.reference("swin_masked")
    assert all(ref.T[t].dtype == torch.float64 for t in ref.tensors)
    assert bt.rel_err(ref.F["act:emb_lh"], ref.T["act:emb_lh"]) > 1e-9       # truth is not an up-cast f32 run


def test_yardstick_layer_norm_keeps_forward_and_dx_and_sums_its_parameter_gradients_in_f32():
    """backbone_truth._LayerNormF32ParamGrads on a bf16 stream of 6272 rows whose gradients all point the same way (what the dense
    Swin stage 1 hands its first norm): output and dx bit-equal to torch's F.layer_norm, dgamma and dbeta within a few bf16 ulps of the
    rows' noise from the float64 sums of the SAME bf16 gradient -- independent of the thread count, which torch's own CPU kernel is not."""
    g = torch.Generator().manual_seed(7)
    M, D = 6272, 32
    x = torch.randn(M, D, generator=g).bfloat16()
    w, b = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1
    dy = (3e-4 * (1.0 + 0.3 * torch.randn(M, D, generator=g))).bfloat16()
    outs = []
    for fn in (lambda x_, w_, b_: torch.nn.functional.layer_norm(x_, (D,), w_, b_, 1e-6), lambda x_, w_, b_: kt._yardstick_layer_norm(x_, w_, b_, 1e-6)):
        x_, w_, b_ = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = fn(x_, w_, b_)
        y.backward(dy)
        outs.append((y.detach(), x_.grad, w_.grad, b_.grad))
    (y0, dx0, _, _), (y1, dx1, dg1, db1) = outs
    assert y1.dtype == torch.bfloat16 and torch.equal(y0, y1) and torch.equal(dx0, dx1)
    xhat = torch.nn.functional.layer_norm(x.double(), (D,), None, None, 1e-6)
    assert bt.rel_err(db1, dy.double().sum(0)) <= 1e-6 and bt.rel_err(dg1, (dy.double() * xhat).sum(0)) <= 1e-5
    assert dg1.dtype == db1.dtype == torch.float32


@pytest.mark.parametrize("name", kt.CASES)
def test_references_are_sane(name):
    """The f32 oracle within 1e-5 relative of the float64 run (truth is truth); every trainable parameter has a gradient of non-zero
    truth norm; e_ref >= 1e-3 for every tensor (a condition on the INPUTS: there is a scale to measure with, no gate is vacuous); the
    three runs masked the same tokens and walked the same coordinates; truth itself keeps within the cap on left-out sub-blocks
    (compare() asserts the share for every family)."""
    ref = kt.reference(name)
    c = kt.make_case(name)
    want = {"grad:" + k for k, p in c["module"].named_parameters() if p.requires_grad}
    assert want == {t for t in ref.tensors if t.startswith("grad:")} and len(want) >= 98
    assert ("attn" in ref.tensors) == (name != "convvit_masked")
    assert sum(t.startswith("act:l") for t in ref.tensors) == (4 if c["backbone"] == "swin" else 2)          # the stage taps
    for t in ref.tensors:
        assert torch.isfinite(ref.T[t]).all() and ref.T[t].norm() > 0, t
        assert 1e-3 <= ref.e_ref(t) <= 0.1, (t, ref.e_ref(t))          # 0.1: three times it stays below what a factor 1 / 0.7 moves
        assert bt.rel_err(ref.F[t], ref.T[t]) <= 1e-5, (t, bt.rel_err(ref.F[t], ref.T[t]))
    assert ref.exact == (["_mask", "_ids_restore"] + ([f"_coords{i}" for i in range(1, 5)] if name == "swin_masked" else [])
                         if c["kind"] == "masked" else [])
    for k in ref.exact:
        assert torch.equal(ref.T[k], ref.Y[k]) and torch.equal(ref.T[k], ref.F[k]), k
    assert _check(name, {t: ref.T[t] for t in ref.tensors}) == []
    if name == "swin_masked":       # the token counts the case is there for
        assert [ref.T[f"act:l{i}"].shape[1] for i in range(1, 5)] == [1536, 384, 96, 24]
    if name == "swin_ft":
        assert [ref.T[f"act:l{i}"].shape[1] for i in range(1, 5)] == [3136, 784, 196, 49]


@pytest.mark.parametrize("name", kt.CASES)
def test_comparator_accepts_the_yardsticks_noise_and_twice_it(name):
    ref = kt.reference(name)
    assert _check(name, _noisy(ref)) == []
    fails, worst, _ = kt.compare_all(name, _noisy(ref, 2.0))
    assert fails == []
    assert 1.9 < worst[0] <= 2.0 + 1e-9, worst


def _last(ref, suffix):
    return [t for t in ref.tensors if t.endswith(suffix)][-1]


def _defects(name):
    """-> [(label, tensor that must be flagged, function changing the dict of tensors in place)]."""
    ref = kt.reference(name)
    c = kt.make_case(name)
    out = []

    def two_d(t):
        return t.view(-1, t.shape[-1])

    def flat(t):
        return t.view(t.shape[0], -1)

    o = "act:emb_lh" if c["kind"] == "masked" else "act:emb_h"
    out.append((f"{o}: one 16 x 64 block zeroed", o, lambda g: two_d(g[o])[16:32, 0:64].zero_()))
    out.append((f"{o}: one 16-row strip doubled", o, lambda g: two_d(g[o])[0:16].mul_(2.0)))
    fc1 = _last(ref, "mlp.fc1.weight")
    out.append(("fc1 weight gradient: one 128 x 128 block dropped", fc1, lambda g: flat(g[fc1])[128:256, 0:128].zero_()))
    qw, qb = _last(ref, "attn.qkv.weight"), _last(ref, "attn.qkv.bias")
    D = ref.T[qb].shape[0] // 3
    dh = D // kt.heads_of(name)(qw)
    assert dh == (64 if c["backbone"] == "vit" else 32)

    def swap(g):
        k = g[qw][D:2 * D].clone()
        g[qw][D:2 * D] = g[qw][2 * D:]
        g[qw][2 * D:] = k
    out.append(("qkv weight gradient: k and v thirds swapped", qw, swap))
    out.append(("qkv bias gradient: one head's slice negated", qb, lambda g: g[qb][2 * D + dh:2 * D + 2 * dh].neg_()))
    for t in ref.tensors:
        if t.startswith("grad:") and t.endswith(".weight") and ref.T[t].dim() == 1:         # the LayerNorms
            b = t[:-len("weight")] + "bias"
            out.append((f"{t}: replaced by the norm-bias gradient", t, lambda g, t=t, b=b: g[t].copy_(g[b])))
    if c["backbone"] == "swin":
        rw = [t for t in ref.tensors if t.endswith("downsample.reduction.weight")][0]

        def swap_neighbours(g):
            a, b, c_, d = g[rw].chunk(4, dim=1)
            g[rw] = torch.cat([a, c_, b, d], dim=1)
        out.append(("patch merging: neighbour column blocks 1 and 2 of the reduction weight gradient swapped", rw, swap_neighbours))
        tab = _last(ref, "relative_position_bias_table")
        out.append(("relative-position table gradient: one head's column zeroed", tab, lambda g: g[tab][:, 1].zero_()))
    if c["kind"] == "masked":
        dec = [t for t in ref.tensors if t.endswith("stage1_output_decode.weight")][0]
        out.append(("stage1_output_decode weight gradient: one kernel position zeroed", dec, lambda g: g[dec][:, :, 1, 2].zero_()))
    else:
        hw = "grad:classify_head.weight"
        out.append(("classify_head weight gradient: the ragged tail rows 96-100 zeroed", hw, lambda g: g[hw][96:].zero_()))
        n_tok = ref.T["act:emb_h"].shape[1]
        out.append(("pred scaled by N / (N - 1)", "pred", lambda g: g["pred"].mul_(n_tok / (n_tok - 1.0))))
    return out


def _missed(name, defects):
    """The defects, each laid over truth + the yardstick's noise (which the test above shows accepted), that the comparator does NOT
    flag in the tensor they sit in. -> [(label, e_ref of the tensor)]"""
    ref = kt.reference(name)
    missed = []
    for label, tensor, apply in defects:
        got = {t: v.clone() for t, v in _noisy(ref).items()}
        apply(got)
        fails = _check(name, {tensor: got[tensor]})
        assert all(f.startswith(tensor + "/") for f in fails), (label, fails)
        if not fails:
            missed.append((label, ref.e_ref(tensor)))
    return missed


@pytest.mark.parametrize("name", kt.CASES)
def test_comparator_rejects_confined_defects(name):
    """A zeroed tile, a doubled strip, a dropped gradient tile, swapped thirds, a negated head slice, every norm weight gradient
    replaced by its bias gradient, and the defects of the glue: swapped neighbour blocks of patch merging, a zeroed kernel position of a
    fusion conv, a zeroed head of a relative-position table, the zeroed ragged tail of the head, a token mean over N - 1."""
    defects = _defects(name)
    assert len(defects) >= 15
    assert _missed(name, defects) == []


@pytest.mark.parametrize("name", kt.CASES)
def test_comparator_rejects_a_missing_scale_in_every_tensor(name):
    """Every tensor on its own scaled by 1 / 0.7 (a missing keep_prob): visible wherever FACTOR * e_ref < 0.43, i.e. e_ref < 0.14 --
    the largest yardstick error of any tensor of any case is 0.02."""
    ref = kt.reference(name)
    assert _missed(name, [(f"{t}: scaled by 1 / 0.7", t, lambda g, t=t: g[t].div_(0.7)) for t in ref.tensors]) == []


@pytest.mark.parametrize("kind", kt.MUTANTS)
def test_comparator_rejects_a_wrong_algorithm(kind):
    """The float32 oracle of swin_masked with one mutation -- every tensor computed to 1e-6, from the wrong algorithm -- is rejected,
    and the tensors the mutation sits in are among the flagged: the blocks that lost their shift, the fusion convs, the merging layers."""
    ref = kt.reference("swin_masked")
    got = kt.mutant_run(kind)
    for k in ref.exact:
        assert torch.equal(got[k], ref.T[k]), k          # the defect is in the arithmetic, not in the masking
    fails = _check("swin_masked", {t: got[t] for t in ref.tensors})
    flagged = {f.split("/")[0] for f in fails}
    where = {"no_shift": "grad:swin_block.0.blocks.1.attn.relative_position_bias_table",
             "fusion_ids_of_sample_0": "grad:stage1_output_decode.weight",
             "merge_row_major": "grad:swin_block.0.downsample.reduction.weight"}[kind]
    assert where in flagged, (kind, sorted(flagged)[:10])
    assert "act:emb_lh" in flagged
    print(f"{kind}: {len(flagged)} of {len(ref.tensors)} tensors flagged")

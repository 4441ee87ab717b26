"""The float64-truth gate of the attention cores (tests/attention_truth.py) on the host, no GPU: the references are sane for every
case the GPU tests run, the gates accept the yardstick Y and the f32 run F, and they reject each of nine single defects of the torch
restatement (attention_truth.MUTANTS) at the smallest case where the defect applies, laid over the yardstick's own noise."""
import pytest
import torch

import attention_truth as at
import block_truth as bt

ALL = at.FUSED_VIT + at.HEAD_MAP_CASES + at.PEAKED + at.WIN_EDGE + at.WIN_WALK_CASES + at.UNFUSED
ALL = list(dict.fromkeys(ALL))


@pytest.mark.parametrize("name", ALL)
def test_references_are_sane_and_gates_accept_yardstick_and_f32(name):
    """F within 1e-5 of T on every tensor (truth is truth), Y at bf16 distance (1e-3 .. 1e-2 class; 1e-5 .. 1e-3 on lse; up to 6e-2
    on the peaked rows), no family over the exclusion cap (compare() asserts it), and F, Y and T + 2 (Y - T) all pass."""
    ref = at.reference(name)
    c = at.make_case(name)
    assert set(ref.tensors) == {"core:out", "core:lse", "core:dqkv", "core:dq", "core:dk", "core:dv", "core:attn" if c["kind"] == "vit" else "core:dtable"}
    for t in ref.tensors:
        assert torch.isfinite(ref.T[t]).all() and ref.T[t].norm() > 0, t
        assert bt.rel_err(ref.F[t], ref.T[t]) <= 1e-5, (t, bt.rel_err(ref.F[t], ref.T[t]))
        lo, hi = (1e-6, 2e-3) if t == "core:lse" else (1e-3, 6e-2 if c["amp"] > 1 else 1.2e-2)
        assert lo <= ref.e_ref(t) <= hi, (t, ref.e_ref(t))
    if c["kind"] == "win":
        assert (ref.T["core:dtable"].abs().sum(0) > 0).all()            # no empty head column
    for got in (ref.F, ref.Y):
        assert at.gate(name, got)[0] == []
    if name not in at.WIN_WALK_CASES:           # (those have a thousand blocks per family; two passes of the comparator are enough)
        fails, worst, _ = at.gate(name, {t: ref.T[t] + 2.0 * (ref.Y[t] - ref.T[t]) for t in ref.tensors})
        assert fails == [] and 1.9 < worst[0] <= 2.0 + 1e-9, (fails, worst)


@pytest.mark.parametrize("name", [at.vit_name(2, 2, 17, 64), at.win_name(3, 2, 2, 17)])
def test_core_is_the_oracles_formulation(name):
    """attention_truth.core against oracle/model_oracle.py::attention / ::window_attention in float64, the qkv Linear given a random
    weight and the proj Linear the identity: same out and, for the ViT form, the same probabilities."""
    from oracle import model_oracle as mo
    c = at.make_case(name)
    Bt, N, h, dh = c["Bt"], c["N"], c["heads"], c["dh"]
    C = h * dh
    g = torch.Generator().manual_seed(5)
    x = torch.randn(Bt, N, C, generator=g, dtype=torch.float64)
    sd = {"qkv.weight": torch.randn(3 * C, C, generator=g, dtype=torch.float64) * C ** -0.5, "qkv.bias": torch.randn(3 * C, generator=g, dtype=torch.float64),
          "proj.weight": torch.eye(C, dtype=torch.float64), "proj.bias": torch.zeros(C, dtype=torch.float64)}
    qkv = torch.nn.functional.linear(x, sd["qkv.weight"], sd["qkv.bias"]).reshape(Bt, N, 3, h, dh)
    if c["kind"] == "vit":
        o_ref, p_ref = mo.attention(sd, "", x, h)
        o, p, _ = at.core(c, qkv)
    else:
        sd["relative_position_bias_table"] = c["table"].double()
        mask = torch.where(c["blocked"], -100.0, 0.0).double()
        o_ref, p_ref = mo.window_attention(sd, "", x, mask, c["rel"], h)
        o, p, _ = at.core(c, qkv, sd["relative_position_bias_table"])
    assert torch.allclose(o, o_ref, rtol=1e-12, atol=1e-13) and torch.allclose(p, p_ref, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", [at.vit_name(2, 2, 17, 32), at.vit_name(2, 2, 65, 64), at.win_name(3, 2, 2, 17), at.win_name(16, 16, 3, 24)])
def test_restatement_by_hand_is_truth(name):
    """attention_truth.manual without a defect -- the form the mutants are cut from -- against autograd in float64."""
    ref, m = at.reference(name), at.manual(name)
    assert sorted(m) == sorted(ref.tensors)
    for t in ref.tensors:
        assert bt.rel_err(m[t], ref.T[t]) <= 1e-12, (t, bt.rel_err(m[t], ref.T[t]))


def test_n1_has_no_scale_and_walk_table_matches_formula():
    """N = 1: the yardstick equals truth on out (P = 1) and dq = dk = 0, so compare() refuses it -- the GPU test asserts identities
    there. The (per, nchunk) columns of the batch-walk table are those of the launcher's formula."""
    for name in (at.vit_name(2, 2, 1, 32), at.win_name(3, 2, 2, 1)):
        ref = at.reference(name)
        assert ref.e_ref("core:out") == 0 and ref.T["core:dq"].abs().max() == 0 and ref.T["core:dk"].abs().max() == 0
        with pytest.raises(AssertionError):
            bt.compare("core:out", ref.Y["core:out"], ref.T["core:out"], ref.Y["core:out"])
    for nG, heads, B, N, per, nchunk in at.WIN_WALK:
        assert at.win_chunks(B * nG, nG, heads) == (nchunk, per)
    assert at.win_chunks(6, 3, 2) == (2, 1)                # the edge cases: one item per workgroup
    import launch_trace
    for Bg, nG, heads in [(6, 3, 2), (48, 16, 16), (66, 22, 24), (24, 8, 32), (80, 16, 16), (64 * 64, 64, 3), (1, 1, 24), (6, 2, 2)]:
        assert launch_trace._win_nchunk(Bg, nG, heads) == at.win_chunks(Bg, nG, heads)[0]      # the trace's stub answers the same


def test_exclusion_cap_is_asserted():
    """More than MAX_EXCLUDED of a family's blocks empty in TRUTH is a fault of the inputs: compare() refuses to measure."""
    name = at.vit_name(2, 2, 17, 32)
    ref = at.reference(name)
    T = ref.T["core:out"].clone()
    T[0, 0] = 0                                             # one (batch, head) of four
    with pytest.raises(AssertionError, match="empty"):
        bt.compare("core:out", T, T, ref.Y["core:out"])


V15, V17, V129, W16 = at.vit_name(2, 2, 15, 32), at.vit_name(2, 2, 17, 32), at.vit_name(2, 2, 129, 32), at.win_name(3, 2, 2, 16)
REJECT = [      # mutant, case, the tensors that have to be flagged, a gate that has to be among the failures (or None)
    ("a_pad_keys_unmasked", V15, ("core:out",), None),
    ("a_pad_keys_unmasked", V129, ("core:out",), None),
    ("a_pad_keys_unmasked", at.win_name(3, 2, 2, 17), ("core:out",), None),
    ("b_last_key_tile_dropped", V17, ("core:out",), "strip16"),
    ("b_last_key_tile_dropped", V129, ("core:out",), "strip16"),
    ("c_head_pair_exchanged", V15, ("core:out",), None),
    ("d_dk_dv_exchanged", V15, ("core:dk", "core:dv"), None),
    ("e_dq_unscaled", V15, ("core:dq",), "scale"),
    ("f_lse_base2", V15, ("core:lse",), None),
    ("g_bias_transposed_in_dkdv", W16, ("core:dk", "core:dv"), None),
    ("h_dtable_last_item_missing", W16, ("core:dtable",), None),
    ("i_dq_stale_item", W16, ("core:dq",), "head"),
]


@pytest.mark.parametrize("mutant,name,flagged,gate", REJECT)
def test_gates_reject_mutants(mutant, name, flagged, gate):
    """Each defect of the restatement, laid over truth + the yardstick's noise (accepted above), is flagged in the tensors it sits in;
    the last key tile dropped for the one-row strip at N = 129 -- one key in 129, one row in 129 -- by the strip family."""
    ref = at.reference(name)
    got = {t: v + (ref.Y[t] - ref.T[t]) for t, v in at.manual(name, mutant).items()}
    fails = at.gate(name, got)[0]
    for t in flagged:
        mine = [f for f in fails if f.startswith(t + "/")]
        assert mine, (mutant, t, fails)
        assert gate is None or any(f.startswith(f"{t}/{gate}:") for f in mine), (mutant, gate, mine)
    if mutant == "b_last_key_tile_dropped" and name == V129:
        assert not any(f.startswith("core:out/whole") for f in fails), fails       # the whole-tensor gate cannot see it

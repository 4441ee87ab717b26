"""The gates of tests/pretrain_truth.py on the host, no GPU: the float64 truths agree with what the tree already trusts (the oracle's
patchify, rec_loss, masking_from_noise and density_noise, torch.optim.AdamW on float64 parameters), the float32 restatement of every
kernel in the kernel's own order stays at or below a quarter of every gate at every case of the GPU test, every single mutation of
it is rejected by the case its comment names, and the case lists reach the edges they claim."""
import pathlib
import re

import pytest
import torch
import torch.nn.functional as F

import pretrain_truth as pt
from oracle import model_oracle as mo

CSRC = pathlib.Path(__file__).resolve().parent.parent / "eventpretrain_amd" / "csrc"


def _headroom(rep):
    assert not rep.fails, rep.fails
    worst = max((w for _, _, w in rep.rows), default=0.0)
    assert worst <= pt.HEADROOM, (rep.what, [(n, g, w) for n, g, w in rep.rows if w > pt.HEADROOM])
    return worst


def _source_int(name, pattern):
    m = re.search(pattern, (CSRC / name).read_text())
    assert m, (name, pattern)
    return int(m.group(1))


# ---------------------------------------------------------------------------------------------------------------- truths
def test_truths_agree_with_the_oracle():
    """frame2emb and the loss against mo.patchify / mo.rec_loss for C = 1, 2, 3, 5 (float64, to 1e-12), density noise against
    mo.density_noise, the masks against mo.masking_from_noise, the patch gather against F.unfold."""
    for key in pt.rec_cases():
        c = pt.rec_case(*key)
        assert torch.equal(pt.frame2emb(c["target"], c["p"]), mo.patchify(c["target"], c["p"]))
        pr = c["pred"].double().clone().requires_grad_(True)
        m = c["mask"].double() if c["mask"] is not None else None
        loss = mo.rec_loss(pr, c["target"].double(), m, c["p"], bool(c["norm_pix"]), 0.5 if m is not None else 0)
        loss.backward()
        assert torch.allclose(loss.detach(), c["T"]["loss"], rtol=1e-12, atol=0)
        assert torch.allclose(pr.grad, c["T"]["dpred"], rtol=1e-12, atol=1e-300)
    for shape in pt.DENS_SHAPES:
        for sign, name in ((1, "density"), (-1, "anti-density")):
            c = pt.density_case(*shape, sign)
            assert torch.allclose(mo.density_noise(c["x"].double(), c["p"], name), c["T"], rtol=1e-12, atol=1e-15)
    for c in pt.mask_cases():
        B, L, keep = c["B"], c["L"], c["len_keep"]
        ratio = 1.0 - keep / L
        if int(L * (1 - ratio)) == keep:
            ids_keep, mask, restore = mo.masking_from_noise(c["noise"], ratio)
            assert torch.equal(ids_keep, c["T"]["ids_keep"]) and torch.equal(mask, c["T"]["mask"]) and torch.equal(restore, c["T"]["ids_restore"])
    for key in pt.PATCHIFY_CASES:
        c = pt.patchify_case(*key)
        cols = F.unfold(c["x"], c["p"], stride=c["p"]).transpose(1, 2)
        if c["ids"] is not None:
            cols = torch.gather(cols, 1, c["ids"].unsqueeze(-1).expand(-1, -1, cols.shape[-1]))
        assert torch.equal(cols.reshape(c["T"].shape), c["T"])


@pytest.mark.parametrize("recipe", [False, True])
def test_adamw_truth_is_torch_adamw_in_float64(recipe):
    """The written-out truth equals torch.optim.AdamW on float64 parameters, moments included, at every step of the case -- the resumed
    step through load_state_dict with step = 100000 -- with the hyper-parameters at their float32 values."""
    c = pt.adam_case(recipe)
    ps = [torch.nn.Parameter(p.double().clone()) for p in c["p0"]]
    groups = [dict(params=[p for i, p in enumerate(ps) if c["group_of"][i] == gi], weight_decay=pt.f32(g["weight_decay"]), lr=pt.f32(g["lr"]))
              for gi, g in enumerate(c["groups"])]
    opt = torch.optim.AdamW(groups, betas=(pt.f32(pt.ADAM_BETAS[0]), pt.f32(pt.ADAM_BETAS[1])), eps=pt.f32(pt.ADAM_EPS), foreach=False)
    done = 0
    for k, ((step, lrs), gk) in enumerate(zip(c["steps"], c["grads"])):
        if step != done + 1:
            sd = opt.state_dict()
            for st in sd["state"].values():
                st["step"] = torch.tensor(float(step - 1))
            opt.load_state_dict(sd)
        done = step
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = pt.f32(lrs[gi])
        for p, g in zip(ps, gk):
            p.grad = g.double() * c["grad_scale"]
        opt.step()
        for i, p in enumerate(ps):
            Tp, Tm, Tv = c["T"][k][i]
            st = opt.state[p]
            assert torch.allclose(p.detach(), Tp, rtol=1e-13, atol=1e-15), (k, i)
            assert torch.allclose(st["exp_avg"], Tm, rtol=1e-12, atol=1e-15), (k, i)           # torch forms it as a lerp: absolute near 0
            assert torch.allclose(st["exp_avg_sq"], Tv, rtol=1e-12, atol=1e-300), (k, i)


# ---------------------------------------------------------------------------------------------------------------- restatements
def test_rec_loss_restatement_keeps_a_quarter_of_every_gate():
    """Every case of the GPU test. Measured here, worst error over the bound: see the printed figure (loss, per-row losses, dpred)."""
    worst = 0.0
    for key in pt.rec_cases():
        c = pt.rec_case(*key)
        worst = max(worst, _headroom(pt.check_rec(c, pt.rec_restated(c))))
    print(f"\nrec loss restatement: worst error / bound {worst:.3f}")


def test_token_restatements_keep_a_quarter_of_every_gate():
    """Unshuffle forward / backward (both versions of every shape), the row gather, density noise, the masks, the element-wise entries and
    the cast."""
    worst = 0.0
    for shape in pt.UNSH_SHAPES:
        for kind in ("random", "int"):
            c = pt.unsh_case(*shape, kind)
            worst = max(worst, _headroom(pt.check_unsh(c, pt.unsh_restated(c))))
            if c["n_keep"] == c["L"]:
                assert bool((pt.unsh_restated(c)["dmask_token"] == 0).all())
    for key in pt.GATHER_CASES:
        for kind in ("random", "int"):
            c = pt.gather_case(*key, kind)
            assert torch.equal(c["restated"], c["T"].float())
    for shape in pt.DENS_SHAPES:
        for sign in (1, -1):
            for kind in ("random", "int"):
                c = pt.density_case(*shape, sign, kind)
                worst = max(worst, _headroom(pt.check_density(c, pt.density_restated(c))))
    for c in pt.mask_cases():
        assert not pt.check_mask(c, pt.mask_restated(c)).fails
    for n in pt.EW_SIZES:
        for kind in ("random", "int"):
            c = pt.ew_case(n, kind)
            worst = max(worst, _headroom(pt.check_ew(c, c["restated"])))
    for n in pt.CAST_SIZES:
        c = pt.cast_case(n)
        rep = pt.Report("cast")
        pt.bits_equal(rep, "bf16", pt.cast_restated(c["x"]), c["T"])
        assert not rep.fails
    print(f"\ntoken restatements: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("recipe", [False, True])
def test_adamw_restatement_keeps_a_quarter_of_every_gate(recipe):
    """adamw_kernel's operation order in float32 against the float64 truth after every step. Measured here, worst error over the bound
    (V_RTOL = 2e-6 for exp_avg_sq): printed; exp_avg_sq's worst relative error is printed too and has to stay under V_RTOL / 4."""
    c = pt.adam_case(recipe)
    got = pt.adam_restated(c)
    worst, vrel = {}, 0.0
    for k in range(len(c["steps"])):
        rep = pt.check_adam(c, k, got[k])
        _headroom(rep)
        for n, w in pt.worst_by_kind(rep).items():
            worst[n] = max(worst.get(n, 0.0), w)
        for i, (_, _, v, _) in enumerate(got[k]):
            Tv = c["T"][k][i][2]
            vrel = max(vrel, float(((v.double() - Tv).abs() / Tv).max()))
    print(f"\nadamw restatement (recipe {recipe}): " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()) + f"  | exp_avg_sq relative {vrel:.2e}")
    assert vrel <= pt.V_RTOL / 4


# ---------------------------------------------------------------------------------------------------------------- mutants
def _mutant_fails(name):
    area, _, key = pt.MUTANTS[name]
    if area == "rec":
        c = pt.rec_case(*key)
        return pt.check_rec(c, pt.rec_restated(c, name)).fails
    if area == "unsh":
        c = pt.unsh_case(*key)
        return pt.check_unsh(c, pt.unsh_restated(c, name)).fails
    if area == "adam":
        c = pt.adam_case()
        return pt.check_adam(c, key, pt.adam_restated(c, name)[key]).fails
    if area == "cast":
        c = pt.cast_case(key)
        rep = pt.Report("cast")
        pt.bits_equal(rep, "bf16", pt.cast_restated(c["x"], name), c["T"])
        return rep.fails
    if area == "density":
        c = pt.density_case(*key)
        return pt.check_density(c, pt.density_restated(c, name)).fails
    raise AssertionError(area)


@pytest.mark.parametrize("mutant", list(pt.MUTANTS))
def test_every_mutation_is_rejected_by_its_named_case(mutant):
    fails = _mutant_fails(mutant)
    print(f"\n{mutant}: {len(fails)} gates failed: {fails[:3]}")
    assert fails, f"{mutant} ({pt.MUTANTS[mutant][1]}): no gate failed in {pt.MUTANTS[mutant][2]}"


def test_named_cases_are_cases_of_the_gpu_test():
    rec, unsh = set(pt.rec_cases()), {s + (k,) for s in pt.UNSH_SHAPES for k in ("random", "int")}
    for name, (area, _, key) in pt.MUTANTS.items():
        if area == "rec":
            assert key in rec, name
        elif area == "unsh":
            assert key in unsh, name
        elif area == "cast":
            assert key in pt.CAST_SIZES, name
        elif area == "density":
            assert key[:5] in pt.DENS_SHAPES, name


# ---------------------------------------------------------------------------------------------------------------- edges
def test_case_lists_reach_the_edges_they_claim():
    """From the constants of the kernels' sources: a change of UM_ROWS, CHUNK or a grid cap breaks this test, not the coverage."""
    from eventpretrain_amd import optim
    assert _source_int("tokens.hip", r"constexpr int UM_ROWS = (\d+);") == pt.UM_ROWS
    assert _source_int("tokens.hip", r"__shared__ float sh\[(\d+)\]\[65\];") == pt.FOLD_GROUPS
    assert _source_int("tokens.hip", r"const int d = blockIdx\.x \* (\d+) \+ threadIdx\.x;") == pt.UM_COLS
    assert _source_int("tokens.hip", r"if \(g > (\d+)\) g = \1;") * 256 == pt.EW_GRID_ITEMS
    assert _source_int("loss.hip", r"if \(grid > (\d+)\) grid = \1;") * 4 == pt.REC_PASS_ROWS
    assert _source_int("loss.hip", r"rec_loss_reduce, dim3\(1\), dim3\((\d+)\)") == pt.REC_REDUCE_THREADS
    assert optim.CHUNK == pt.CHUNK and pt.CHUNK % 4 == 0

    rows = [B * (H // p) * (W // p) for B, C, H, W, p in pt.REC_SHAPES]
    P = [p * p * C for B, C, H, W, p in pt.REC_SHAPES]
    assert min(rows) == 1 and max(rows) > pt.REC_PASS_ROWS and max(rows) > pt.REC_REDUCE_THREADS
    assert 2 in P and any(q < 64 for q in P) and max(P) > 1024
    assert any(q % 64 != 0 for q in P) and any(C > 1 and p > 1 for B, C, H, W, p in pt.REC_SHAPES)
    assert any(H // p != W // p for B, C, H, W, p in pt.REC_SHAPES)
    c = pt.rec_case(*pt.MUTANTS["rows_past_one_pass_not_written"][2])
    assert int(c["mask"].reshape(-1).nonzero()[0]) >= pt.REC_PASS_ROWS            # the single masked row sits in the second pass

    slabs = [pt.unsh_slabs(B, L) for B, L, k, D in pt.UNSH_SHAPES]
    assert {1, pt.FOLD_GROUPS, pt.FOLD_GROUPS + 1, 2 * pt.FOLD_GROUPS + 1} <= set(slabs)
    assert any(B * L == pt.UM_ROWS for B, L, k, D in pt.UNSH_SHAPES)
    last_of_one = [(B, L, k, D) for B, L, k, D in pt.UNSH_SHAPES if B * L % pt.UM_ROWS == 1 and B * L > 1]
    assert len(last_of_one) >= 2
    for s in last_of_one:
        c = pt.unsh_case(*s)
        assert int(c["ids"][-1, -1]) >= c["n_keep"]                                # the lone row carries a term of the sum
    D = [d for _, _, _, d in pt.UNSH_SHAPES]
    assert any(d > pt.UM_COLS for d in D) and any(d % 64 for d in D) and any(d // 4 > 256 for d in D) and 4 in D
    assert any(k == L for B, L, k, D_ in pt.UNSH_SHAPES) and any(k == 1 and L > 1 for B, L, k, D_ in pt.UNSH_SHAPES)
    assert {d // 4 for _, _, _, d, _ in pt.GATHER_CASES} >= {1, 65, 257} and {w for *_, w in pt.GATHER_CASES} == {True, False}
    assert max(C * p * p for _, C, _, _, p, _, _ in pt.PATCHIFY_CASES) > 256 * 4
    assert {p * p for *_, p in pt.DENS_SHAPES} >= {16, 1024}

    n = pt.ADAM_NUMEL
    assert {1, 3, 4, 5, pt.CHUNK - 1, pt.CHUNK, pt.CHUNK + 1, pt.CHUNK + 3, 2 * pt.CHUNK + 2} == set(n)
    assert any(x > pt.CHUNK and x % 4 for x in n)                                  # a tail in the last chunk of a multi-chunk tensor
    assert all(n[i] % 4 for i in pt.ADAM_SHADOWS) and any(n[i] > pt.CHUNK for i in pt.ADAM_SHADOWS)       # the bf16 shadow on a tail
    assert set(pt.ADAM_GROUP_OF) == {0, 1} and n[pt.ADAM_TINY] % 4 and n[pt.ADAM_TINY] > 4
    assert max(pt.EW_SIZES) // 4 > pt.EW_GRID_ITEMS and max(pt.EW_SIZES) % 4 and {1, 2, 3, 4, 5} <= set(pt.EW_SIZES)
    assert max(pt.CAST_SIZES) // 4 > pt.EW_GRID_ITEMS
    for m in pt.CAST_SIZES:
        x = pt.cast_case(m)["x"]
        assert m % 4 and not torch.isfinite(x[-1]) or x[-1] in (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8)     # a special in the scalar tail
    big = pt.cast_case(max(pt.CAST_SIZES))["x"][:8]
    assert torch.isnan(big).any() and torch.isinf(big).sum() == 2 and (big == 0).any() and torch.signbit(big[big == 0]).all()
    assert pt.cast_case(5)["T"].float()[-1] == 1.0 + 2.0 ** -6 and pt.cast_case(3)["T"].float()[-1] == 1.0
    assert torch.isinf(torch.tensor(3.4e38).bfloat16()) and torch.isfinite(torch.tensor(3.4e38))

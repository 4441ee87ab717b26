"""tests/conv_stage_truth.py proved on the CPU: (a) the case list reaches both sides of every band_ok clause and the row-walker
tails, (b) every planted fault falls outside the per-element bounds, (c) the truth passes its own bounds when evaluated in float32,
and the torch index arithmetic of the patch gather / scatter against plain loops."""
import pytest
import torch

import conv_stage_truth as ct

CASE_NAMES = list(ct.CASES)


# ---- (a) clause coverage --------------------------------------------------------------------------------------------------------
def test_case_list_is_the_one_the_kernels_need():
    assert [v[:5] for v in ct.CASES.values()] == [(1, 4, 8, 32, 0), (3, 4, 9, 64, 1), (1, 8, 64, 64, 4), (1, 4, 65, 64, 0),
                                                   (3, 5, 7, 68, 1), (2, 12, 20, 96, 4), (5, 4, 8, 128, 2), (2, 8, 12, 64, 4)]
    assert [k for k, v in ct.CASES.items() if v[5]] == ["frac"]


@pytest.mark.parametrize("dtype", ct.DTYPES)
def test_both_sides_of_every_band_clause(dtype):
    shapes = [v[1:4] for v in ct.CASES.values()]
    cb = ct.CB[dtype]
    # a case that fails ONLY through the clause in question, where the list allows it, and one that passes it inside a band launch
    clauses = {
        "H % 4": lambda H, W, C: H % 4 == 0,
        "W >= 8": lambda H, W, C: W >= 8,
        "W <= 64": lambda H, W, C: W <= 64,
        "C % CB": lambda H, W, C: C % cb == 0,
    }
    for name, ok in clauses.items():
        assert any(not ok(*s) for s in shapes), (dtype, name, "no case on the failing side")
        assert any(ok(*s) and ct.band_ok(*s, dtype) for s in shapes), (dtype, name, "no band case on the passing side")
    assert any(not ct.band_ok(H, W, C, dtype) and H % 4 == 0 and 8 <= W and C % cb == 0 for H, W, C in shapes), "W > 64 alone"
    # on the limits themselves
    assert any(W == 64 and ct.band_ok(H, W, C, dtype) for H, W, C in shapes) and any(W == 65 for H, W, C in shapes)
    assert any(W == 8 and ct.band_ok(H, W, C, dtype) for H, W, C in shapes) and any(W == 7 for H, W, C in shapes)
    assert any(W % 2 == 1 and ct.band_ok(H, W, C, dtype) for H, W, C in shapes), "odd W inside the band"
    # one shape where the two dtypes take different forms
    assert any(ct.band_ok(H, W, C, "f32") != ct.band_ok(H, W, C, "bf16") for H, W, C in shapes)
    assert ct.form("c96", "f32", 1) == "band" and ct.form("c96", "bf16", 1) == "rows" and ct.form("c96", "f32", 0) == "rows"
    assert ct.form("w65", dtype, 1) == "rows" and ct.form("w64", dtype, 1) == "band"


def test_row_walker_tails_and_mask_forms_are_reached():
    rows = {k: v[0] * v[1] for k, v in ct.CASES.items()}
    assert any(r % ct.FWD_ROWS for r in rows.values()), "no forward block cut by r < nrows"
    assert any(r % 2 for r in rows.values()), "no wave with a single live row"
    assert any(r % ct.DW_ROWS % 4 for r in rows.values()), "no weight-gradient wave with a partial set of rows"
    assert any(r > ct.DW_ROWS and r % ct.DW_ROWS and ct.band_ok(*ct.CASES[k][1:4], "f32") for k, r in rows.items()), "short last band slab"
    assert any(v[3] % 128 and v[3] > 64 for v in ct.CASES.values()), "no lane cut in the middle of a wave"
    assert any(v[3] > 64 and ct.band_ok(*v[1:4], "bf16") for v in ct.CASES.values()), "no band launch with two channel blocks"
    scales = {v[4] for v in ct.CASES.values()}
    assert {0, 1, 2, 4} <= scales
    for k, (B, H, W, C, s, frac) in ct.CASES.items():
        if s:
            assert H % s == 0 and W % s == 0
            assert H // s != W // s, (k, "a square mask grid hides gw / gh mix-ups")
            m = ct.inputs(k, "f32")["mask"]
            assert set(m.unique().tolist()) == ({0.0, 0.25, 1.0} if frac else {0.0, 1.0}), k
    assert (3, 5) == (ct.CASES["c96"][1] // 4, ct.CASES["c96"][2] // 4)
    assert max(ct.nslab(k) for k in ct.CASES) >= 2


# ---- (b) the bounds bite --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", list(ct.FAULTS))
@pytest.mark.parametrize("case", CASE_NAMES)
def test_planted_fault_falls_outside_the_bounds(case, fault):
    tensors, needs_mask = ct.FAULTS[fault]
    if needs_mask and not ct.CASES[case][4]:
        assert ct.inputs(case, "f32")["mask"] is None        # without a mask this fault changes nothing: nothing to show
        return
    for dtype in ct.DTYPES:
        ref, _ = ct.truth(case, dtype)
        bad = ct.evaluate(case, dtype, fault=fault)
        for kernel_form in ("band", "rows"):                 # "band" carries the widest bound a case can have
            bd = ct.bounds(case, dtype, kernel_form)
            for k in tensors:
                r = ct.worst_ratio(bad[k], ref[k], bd[k])
                assert r > 1.0, (case, fault, dtype, kernel_form, k, r)


# ---- (c) the truth passes itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASE_NAMES)
def test_float32_evaluation_passes_the_bounds(case):
    for dtype in ct.DTYPES:
        ref, _ = ct.truth(case, dtype)
        got = ct.evaluate(case, dtype, dt=torch.float32)
        if dtype == "bf16":
            got = {k: (v.bfloat16().float() if k in ("y", "dx") else v) for k, v in got.items()}
        bd = ct.bounds(case, dtype, "rows")                  # the plain bound
        for k in ("y", "dx", "dw", "db"):
            r = ct.worst_ratio(got[k], ref[k], bd[k])
            assert r <= 1.0, (case, dtype, k, r)
            assert got[k].shape == ref[k].shape
    # the float64 truth is its own fixed point, and a bound of 0 demands equality
    ref, _ = ct.truth(case, "f32")
    assert ct.worst_ratio(ref["y"], ref["y"], torch.zeros_like(ref["y"])) == 0.0
    off = ref["y"].clone()
    off[-1, -1, -1, -1] += 1e-12
    assert ct.worst_ratio(off, ref["y"], torch.zeros_like(ref["y"])) == float("inf")
    nan = ref["y"].clone()
    nan[0, 0, 0, 0] = float("nan")
    assert ct.worst_ratio(nan, ref["y"], ct.bounds(case, "f32", "rows")["y"]) == float("inf")


def test_fractional_keep_term_is_what_separates_the_forms():
    """In bf16 the band form of the fractional case rounds keep * x to bf16: restated on the CPU, that result needs the extra
    2^-8 term (it is outside the plain bound somewhere) and is inside the widened one."""
    import torch.nn.functional as F
    B, H, W, C, s, _ = ct.CASES["frac"]
    t = ct.inputs("frac", "bf16")
    keep = ct.keep_map(t["mask"], B, H, W, s, torch.float32)
    staged = (t["x"].permute(0, 3, 1, 2) * keep).bfloat16().double()
    y = F.conv2d(staged, t["w"].double().view(C, 1, 5, 5), t["b"].double(), padding=2, groups=C).permute(0, 2, 3, 1)
    ref, _ = ct.truth("frac", "bf16")
    y = y.bfloat16().float()
    assert ct.worst_ratio(y, ref["y"], ct.bounds("frac", "bf16", "rows")["y"]) > 1.0
    assert ct.worst_ratio(y, ref["y"], ct.bounds("frac", "bf16", "band")["y"]) <= 1.0


# ---- patch gather / scatter ------------------------------------------------------------------------------------------------------
def test_patch_index_arithmetic_against_loops():
    B, H, W, C, p = 2, 4, 6, 4, 2
    gw, L = W // p, (H // p) * (W // p)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, C, generator=g)
    ids = torch.tensor([[4, 0, 3], [1, 5, 2]])
    for keep in (ids, None):
        idx = keep if keep is not None else torch.arange(L).expand(B, L)
        n_keep = idx.shape[1]
        cols = torch.zeros(B * n_keep, C * p * p)
        for b in range(B):
            for j in range(n_keep):
                gy, gx = divmod(int(idx[b, j]), gw)
                for c in range(C):
                    for py in range(p):
                        for px in range(p):
                            cols[b * n_keep + j, c * p * p + py * p + px] = x[b, gy * p + py, gx * p + px, c]
        assert torch.equal(ct.patchify_ref(x, keep, p), cols)
        back = ct.unpatchify_ref(cols, keep, B, H, W, C, p)
        kept = torch.zeros(B, H // p, gw, dtype=torch.bool).view(B, L)
        kept.scatter_(1, idx, True)
        full = kept.view(B, H // p, 1, gw, 1, 1).expand(B, H // p, p, gw, p, C).reshape(B, H, W, C)
        assert torch.equal(back[full], x[full]) and torch.count_nonzero(back[~full]) == 0
        base = torch.randn(B, H, W, C, generator=g)
        assert torch.equal(ct.unpatchify_ref(cols, keep, B, H, W, C, p, base=base), base + back)

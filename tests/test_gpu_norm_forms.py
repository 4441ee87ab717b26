"""The forms in csrc/norm.hip share their arithmetic (row statistics, the affine line, the backward's per-chunk step and output line,
the partial-row flush; one column-sum body). Pinned here, bit for bit, on operands where the forms must agree:

  - evp_embed_post_fwd with beta = 40, |gamma| <= 1 and no position table == evp_layernorm_fwd: at z >= 30 erff(z / sqrt 2) is exactly
    1, so GELU(z) = 0.5 * z * 2 = z (the test checks min z >= 30);
  - evp_embed_post_bwd on the same operands == evp_layernorm_bwd without gres / x2 / x3: dGELU(z) = 1 + z * 0 there, both kernels see
    the same dy, both run ln_grid(M) blocks, and the two-row schedule adds rows into dgamma / dbeta in the one-row form's order;
  - evp_layernorm_bwd_cs == evp_layernorm_bwd in dx, dx_lp and the first two partial rows of every block;
  - evp_colsum_grouped == evp_colsum == the exact sums, on integer-valued data where no order of the atomics can change a bit.

Shapes and launchers come from tools/norm_digest.py: D 96 (one chunk per lane, ragged) and 772 (four, ragged: the two-row schedule),
M 5 (one block, three idle waves) and 2053 (the 512-block cap: five waves with a live second row, the others a dead one)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(M, D) for D in (96, 772) for M in (5, 2053)]


def test_shapes_are_the_tools():
    from tools.norm_digest import FORMS_D, FORMS_M
    assert SHAPES == [(M, D) for D in FORMS_D for M in FORMS_M]


@functools.lru_cache(maxsize=None)
def _gelu_free(M, D):
    """(embed operands with beta = 40 and |gamma| <= 1, the same as LayerNorm operands with dy = the embed's upstream gradient, both
    forwards): computed once per shape, read by the forward and the backward test."""
    from tools.norm_digest import embed_fwd, embed_operands, ln_fwd
    p = embed_operands(M, D, seed=500 + D)
    gen = torch.Generator().manual_seed(600 + D)
    p["gamma"] = (torch.rand(D, generator=gen) * 2 - 1).cuda()
    p["beta"] = torch.full((D,), 40.0, device="cuda")
    q = dict(M=M, D=D, x=p["y"], dy=p["g"], gamma=p["gamma"], beta=p["beta"])
    return p, q, embed_fwd(p), ln_fwd(q, False, torch.float32)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), what


@pytest.mark.parametrize("M,D", SHAPES)
def test_embed_post_fwd_is_layernorm_fwd_where_gelu_is_the_identity(M, D):
    _, _, e, f = _gelu_free(M, D)
    zmin = float(f["y"].min())
    print(f"M={M} D={D}: min z = {zmin:.3f}")
    assert zmin >= 30.0
    _same(e["out"], f["y"], "out")
    _same(e["mean"], f["mean"], "mean")
    _same(e["rstd"], f["rstd"], "rstd")


@pytest.mark.parametrize("M,D", SHAPES)
def test_embed_post_bwd_is_layernorm_bwd_where_gelu_is_the_identity(M, D):
    from tools.norm_digest import embed_bwd, ln_bwd
    p, q, e, f = _gelu_free(M, D)
    eb = embed_bwd(p, (e["mean"], e["rstd"]), torch.float32, affine=True)
    lb = ln_bwd(q, (f["mean"], f["rstd"]), cs=False, outs="dx", affine=True)
    _same(eb["dy"], lb["dx"], "dy / dx")
    _same(eb["ws"], lb["ws"], "partial rows")
    _same(eb["dgamma"], lb["dgamma"], "dgamma")
    _same(eb["dbeta"], lb["dbeta"], "dbeta")


@pytest.mark.parametrize("M,D", SHAPES)
def test_layernorm_bwd_cs_is_layernorm_bwd_plus_a_third_partial_row(M, D):
    from tools.norm_digest import ln_bwd, ln_fwd, ln_operands
    p = ln_operands(M, D, seed=700 + D)
    f = ln_fwd(p, True, torch.float32)
    for dyd in (torch.float32, torch.bfloat16):
        a = ln_bwd(p, (f["mean"], f["rstd"]), True, dyd, x23=True, gres=True, outs="both")
        b = ln_bwd(p, (f["mean"], f["rstd"]), False, dyd, x23=True, gres=True, outs="both", affine=False)
        _same(a["dx"], b["dx"], "dx")
        _same(a["dx_lp"], b["dx_lp"], "dx_lp")
        _same(a["ws"][:, :2].contiguous(), b["ws"], "partial rows 0 and 1")


def test_colsum_grouped_is_colsum_is_the_exact_sum():
    from tools.norm_digest import FILL, colsum, colsum_grouped, colsum_operands
    problems = colsum_operands()
    assert {x.dtype for x, _ in problems} == {torch.float32, torch.bfloat16} and len({N for _, N in problems}) == 2
    for pair in (problems[0:2], problems[2:4], problems[1:3]):          # each pair: both dtypes in one launch
        for (x, N), g in zip(pair, colsum_grouped(pair)):
            c = colsum(x, N)
            want = x[:, :N].double().sum(0)
            assert float(want.abs().max()) < 2 ** 24
            assert torch.equal(c[:N].double(), want) and torch.equal(g[:N].double(), want), (tuple(x.shape), N, x.dtype)
            _same(c, g, "colsum == grouped")
            assert bool((c[N:] == FILL).all()) and bool((g[N:] == FILL).all()), "wrote behind N"

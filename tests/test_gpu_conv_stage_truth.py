"""The ConvViT stage kernels of csrc/conv.hip at every edge of their launch forms, per element (tests/conv_stage_truth.py holds the
float64 truth, the derived bounds and the cases; test_conv_stage_truth_host.py proves them on the CPU).

Depthwise 5x5: each case runs in f32 and bf16, with the band switch on and off, over NaN-prefilled outputs and workspace; every
element of y, dx, dw and db is compared with its own bound. MEASURED below records the worst error / bound ratio seen per case and
dtype (the larger of the two switch settings), printed by the test -- a record, not a bound.

Patch gather / scatter: pure copies, compared for equality against index arithmetic in torch, including the accumulate form, the
zeroing of dropped patches, a launch past one grid of threads and the refusals."""
import pytest
import torch

import conv_stage_truth as ct

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}

# case: {dtype: worst error / bound ratio measured on an MI355X for (y, dx, dw, db)}, the larger of the two switch settings.
# bf16 y / dx sit just under 1 by construction: the bound's 2^-8 |ref| term IS the half-ulp of a bf16 rounding, reached whenever a
# result falls next to a tie; the f32 figures show the headroom of the chain itself. frac / bf16 / dw: 0.154 under the band bound
# with its 2^-8 staging term, 0.011 for the row walkers under the plain one.
MEASURED = {
    "band_min": {"f32": (0.066, 0.048, 0.039, 0.020), "bf16": (0.980, 0.963, 0.020, 0.000)},
    "odd_w": {"f32": (0.055, 0.066, 0.035, 0.021), "bf16": (0.988, 0.989, 0.016, 0.000)},
    "w64": {"f32": (0.070, 0.091, 0.006, 0.002), "bf16": (0.986, 0.983, 0.003, 0.000)},
    "w65": {"f32": (0.087, 0.064, 0.012, 0.005), "bf16": (0.994, 0.976, 0.005, 0.000)},
    "ragged": {"f32": (0.060, 0.049, 0.034, 0.015), "bf16": (0.989, 0.979, 0.022, 0.000)},
    "c96": {"f32": (0.079, 0.065, 0.010, 0.005), "bf16": (0.994, 0.987, 0.005, 0.000)},
    "slabs": {"f32": (0.074, 0.071, 0.036, 0.010), "bf16": (0.986, 0.985, 0.031, 0.001)},
    "frac": {"f32": (0.063, 0.062, 0.022, 0.010), "bf16": (0.984, 0.984, 0.154, 0.000)},
}
assert set(MEASURED) == set(ct.CASES)


def _run_dwconv(case, dtype, band):
    """-> {y, dx, dw, db} on the CPU as float32 / the I/O dtype widened, from one forward and one backward call."""
    from eventpretrain_amd._lib import call, dt, ptr, stream_ptr
    B, H, W, C, scale, _ = ct.CASES[case]
    t = ct.inputs(case, dtype)
    td = TORCH_DTYPE[dtype]
    xd, dyd, wd, bd = t["x"].to(td).cuda(), t["dy"].to(td).cuda(), t["w"].cuda().contiguous(), t["b"].cuda()
    md = None if t["mask"] is None else t["mask"].cuda()
    nan = float("nan")
    call("evp_dwconv_set_band", band)
    y = torch.full((B, H, W, C), nan, dtype=td, device="cuda")
    call("evp_dwconv5x5_fwd", ptr(xd), dt(xd), ptr(md), int(scale), ptr(wd), ptr(bd), B, H, W, C, ptr(y), stream_ptr())
    ns = call("evp_dwconv5x5_bwd_nslab", B, H, W)
    assert ns == ct.nslab(case)
    ws = torch.full((ns * 26 * C,), nan, device="cuda")
    dx = torch.full((B, H, W, C), nan, dtype=td, device="cuda")
    dw = torch.full((C, 25), nan, device="cuda")
    db = torch.full((C,), nan, device="cuda")
    call("evp_dwconv5x5_bwd", ptr(dyd), ptr(xd), dt(xd), ptr(md), int(scale), ptr(wd), B, H, W, C, ptr(dx), ptr(dw), ptr(db), ptr(ws),
         stream_ptr())
    torch.cuda.synchronize()
    assert torch.isfinite(ws).all(), (case, dtype, band, "workspace not fully written")
    return dict(y=y.float().cpu(), dx=dx.float().cpu(), dw=dw.cpu(), db=db.cpu())


@pytest.mark.parametrize("dtype", ct.DTYPES)
@pytest.mark.parametrize("case", list(ct.CASES))
def test_dwconv5x5_every_form_edge_per_element(case, dtype):
    from eventpretrain_amd._lib import call
    ref, _ = ct.truth(case, dtype)
    ratios, got = {}, {}
    try:
        for band in (1, 0):
            got[band] = _run_dwconv(case, dtype, band)
    finally:
        call("evp_dwconv_set_band", 1)
    for band in (1, 0):
        kernel_form = ct.form(case, dtype, band)
        bd = ct.bounds(case, dtype, kernel_form)
        for k in ("y", "dx", "dw", "db"):
            assert got[band][k].shape == ref[k].shape and torch.isfinite(got[band][k]).all(), (case, dtype, band, k)
            ratios[band, k] = ct.worst_ratio(got[band][k], ref[k], bd[k])
        print(f"dwconv {case} {dtype} switch={band} ({kernel_form}): " + "  ".join(f"{k} {ratios[band, k]:.3f}" for k in ("y", "dx", "dw", "db")))
    for (band, k), r in ratios.items():
        assert r <= 1.0, (case, dtype, band, k, r)
    if ct.form(case, dtype, 1) == "rows":                       # the switch changed nothing: the same kernels, the same bits
        for k in ("y", "dx", "dw", "db"):
            assert torch.equal(got[1][k], got[0][k]), (case, dtype, k)


# ---- patch gather / scatter ------------------------------------------------------------------------------------------------------
def _patchify(x, ids, p, n_keep, out_dtype):
    from eventpretrain_amd._lib import EVP_BF16, EVP_F32, call, ptr, stream_ptr
    B, H, W, C = x.shape
    cols = torch.full((B * n_keep, C * p * p), float("nan"), dtype=out_dtype, device="cuda")
    call("evp_patchify_nhwc", ptr(x), ptr(ids), B, H, W, C, p, n_keep, ptr(cols), EVP_F32 if out_dtype == torch.float32 else EVP_BF16,
         stream_ptr())
    torch.cuda.synchronize()
    return cols.cpu()


def _unpatchify(dcols, ids, shape, p, n_keep, accumulate, dx):
    from eventpretrain_amd._lib import call, dt, ptr, stream_ptr
    B, H, W, C = shape
    call("evp_unpatchify_nhwc", ptr(dcols), dt(dcols), ptr(ids), B, H, W, C, p, n_keep, accumulate, ptr(dx), stream_ptr())
    torch.cuda.synchronize()
    return dx.cpu()


def _same(a, b):
    """bitwise equality (NaN-safe, sign-of-zero-safe)"""
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


PATCH_GEOMETRIES = {
    # name: (B, H, W, C, patch, ids_keep or None)
    "kept3": (2, 4, 6, 4, 2, [[4, 0, 3], [1, 5, 2]]),          # n_keep = 3 of L = 6, unsorted
    "all": (2, 4, 6, 4, 2, None),                              # ids_keep = NULL, n_keep = L
    # rows * C against one grid of 8192 * 256 = 2,097,152 threads: 2 x 64 x 64 / 4 x 520 = 1,064,960 stays inside it, so the
    # same geometry runs at B = 4 as well (2,129,920: the first 32,768 threads take a second, grid-strided element)
    "wide": (2, 64, 64, 520, 2, None),
    "past_one_grid": (4, 64, 64, 520, 2, None),
}


@pytest.mark.parametrize("geometry", list(PATCH_GEOMETRIES))
def test_patchify_and_unpatchify_are_exact_copies(geometry):
    B, H, W, C, p, ids = PATCH_GEOMETRIES[geometry]
    L = (H // p) * (W // p)
    ids_c = None if ids is None else torch.tensor(ids)
    n_keep = L if ids is None else ids_c.shape[1]
    if geometry == "past_one_grid":
        assert B * n_keep * C > 8192 * 256
    g = torch.Generator().manual_seed(B + C)
    x = torch.randn(B, H, W, C, generator=g)
    ids_d = None if ids is None else ids_c.cuda()
    want = ct.patchify_ref(x, ids_c, p)
    cols = _patchify(x.cuda(), ids_d, p, n_keep, torch.float32)
    assert _same(cols, want)
    cols_lp = _patchify(x.cuda(), ids_d, p, n_keep, torch.bfloat16)
    assert _same(cols_lp, want.bfloat16())
    for dcols in (torch.randn(want.shape, generator=g), torch.randn(want.shape, generator=g).bfloat16()):
        # accumulate = 0 over NaN: kept patches written, dropped patches exactly 0
        dx = _unpatchify(dcols.cuda(), ids_d, (B, H, W, C), p, n_keep, 0, torch.full((B, H, W, C), float("nan"), device="cuda"))
        assert _same(dx, ct.unpatchify_ref(dcols, ids_c, B, H, W, C, p))
        if ids is not None:
            assert torch.count_nonzero(dx) == B * n_keep * C * p * p < dx.numel()
        # accumulate = 1 onto a known dx: the float32 sum, dropped patches untouched
        base = torch.randn(B, H, W, C, generator=g)
        dx = _unpatchify(dcols.cuda(), ids_d, (B, H, W, C), p, n_keep, 1, base.clone().cuda())
        assert _same(dx, ct.unpatchify_ref(dcols, ids_c, B, H, W, C, p, base=base))


def test_patch_refusals():
    from eventpretrain_amd._lib import EVP_F32, EvpError, call, ptr, stream_ptr
    B, H, W, C, p = 2, 4, 6, 4, 2
    L = 6
    x = torch.zeros(B, H, W, C, device="cuda")
    ids = torch.zeros(B, L + 1, dtype=torch.int64, device="cuda")
    cols = torch.full((B * (L + 1), C * p * p), float("nan"), device="cuda")
    dx = torch.full((B, H + 1, W, C), float("nan"), device="cuda")
    bad = {"n_keep > L": (H, L + 1, ids), "H % patch != 0": (H + 1, L, None), "ids_keep NULL with n_keep < L": (H, 3, None)}
    for what, (h, n_keep, idp) in bad.items():
        with pytest.raises(EvpError):
            call("evp_patchify_nhwc", ptr(x), ptr(idp), B, h, W, C, p, n_keep, ptr(cols), EVP_F32, stream_ptr())
        with pytest.raises(EvpError):
            call("evp_unpatchify_nhwc", ptr(cols), EVP_F32, ptr(idp), B, h, W, C, p, n_keep, 0, ptr(dx), stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(cols).all() and torch.isnan(dx).all()    # a refused call launches nothing

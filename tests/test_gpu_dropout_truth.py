"""csrc/dropout.hip on the GPU against its host restatement (tests/dropout_truth.py), bit for bit -- no tolerance anywhere.

evp_dropout_fwd: the Philox4x32-10 stream (known-answer vectors: test_dropout_truth_host.py), both key words, a counter that carries
into its second word inside a launch, the n % 4 tail, f32 and bf16 I/O, the device seed scalar, the stream property that
BlockDrop.next_offset relies on, and a launch larger than one pass of the largest grid. evp_dropout_apply: a given mask and scale,
past one grid too. evp_rows_scale_f32: the per-sample factor with the draw on the float32 keep / drop boundary, every pointer
combination, and the sum with the residual as one of the two float32 results a compiler may produce (fused or not). Refusals."""
import numpy as np
import pytest
import torch

import dropout_truth as dtr

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want32, what):
    """got: result tensor on the CPU; want32: numpy float32 of the exact float32 result (rounded to bf16 by torch for bf16 I/O)."""
    want = torch.from_numpy(np.ascontiguousarray(want32)).to(got.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), int(bad.nonzero()[0, 0]))


def _x(n, dtype, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + n % 1000)).to(dtype)


def _fwd(x, p, seed, offset, seed_dev=None):
    """One evp_dropout_fwd launch over NaN- / 7-prefilled outputs -> (out on the CPU, mask uint8 numpy)."""
    from eventpretrain_amd._lib import call, dt, ptr, stream_ptr
    xd = x.cuda()
    out = torch.full_like(xd, float("nan"))
    mask = torch.full((x.numel(),), 7, dtype=torch.uint8, device="cuda")
    call("evp_dropout_fwd", ptr(xd), dt(xd), ptr(out), ptr(mask), x.numel(), float(p), int(seed), ptr(seed_dev), int(offset), stream_ptr())
    torch.cuda.synchronize()
    return out.cpu(), mask.cpu().numpy()


def _check_fwd(x, p, seed, offset, out, mask, what, first_elem=0):
    want_mask = dtr.keep_mask(x.numel(), p, seed, offset, first_elem)
    assert np.array_equal(mask, want_mask), (what, "mask", int((mask != want_mask).sum()))
    _same_bits(out, dtr.dropout_out(x.float().numpy(), want_mask, dtr.inv_keep(p)), what)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_dropout_fwd_stream_tail_and_arithmetic(dtype, p):
    """n in {1, 3, 5, 1023}: every n % 4 tail; a seed with both key words set; a non-zero offset."""
    for n in (1, 3, 5, 1023):
        x = _x(n, dtype)
        out, mask = _fwd(x, p, dtr.BIG_SEED, 11)
        _check_fwd(x, p, dtr.BIG_SEED, 11, out, mask, (n, p))
        if p == 0.0:
            assert mask.all() and torch.equal(_bits(out), _bits(x))
        elif n == 1023:
            assert 0 < mask.sum() < n and (x[torch.from_numpy(mask == 0)] < 0).any()        # the +0 of a dropped negative is looked at


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_dropout_fwd_counter_carries_into_second_word(dtype):
    x = _x(16, dtype)
    off = 2 ** 32 - 2
    out, mask = _fwd(x, 0.5, dtr.BIG_SEED, off)
    _check_fwd(x, 0.5, dtr.BIG_SEED, off, out, mask, "carry")
    # a counter cut to 32 bits would replay the groups of offsets 0 and 1 here
    assert not np.array_equal(mask[8:], dtr.keep_mask(8, 0.5, dtr.BIG_SEED, 0))


@pytest.mark.parametrize("s,d", [(0x00000001FFFFFFF0, 0x20), (0xFFFFFFFFFFFFFFF0, 0x25), (dtr.BIG_SEED, 0)])
def test_dropout_fwd_device_seed_is_added_mod_2_64(s, d):
    """(seed s, device scalar d) draws what (s + d mod 2^64, no device scalar) draws: a carry between the key words, a wrap."""
    x = _x(37, torch.float32)
    sd = torch.tensor([d], dtype=torch.int64, device="cuda")
    out_a, mask_a = _fwd(x, 0.5, s, 3, seed_dev=sd)
    out_b, mask_b = _fwd(x, 0.5, (s + d) % 2 ** 64, 3)
    assert np.array_equal(mask_a, mask_b) and torch.equal(_bits(out_a), _bits(out_b))
    _check_fwd(x, 0.5, (s + d) % 2 ** 64, 3, out_a, mask_a, "seed_dev")
    if d:
        assert not np.array_equal(mask_a, dtr.keep_mask(37, 0.5, s, 3))


def test_dropout_fwd_stream_property_and_block_drop_offsets():
    """mask(offset o, n)[4k:] == mask(offset o + k, n - 4k); and two consecutive ops.dropout_fwd uses of one BlockDrop draw
    consecutive slices of one stream, in units of 4 elements, numel % 4 != 0 included."""
    from eventpretrain_amd import ops
    o, n, k = 7, 23, 2
    x = _x(n, torch.float32)
    _, whole = _fwd(x, 0.5, dtr.BIG_SEED, o)
    _, rest = _fwd(x[4 * k:], 0.5, dtr.BIG_SEED, o + k)
    assert np.array_equal(whole[4 * k:], rest)
    rd = ops.BlockDrop(drop=0.5, seed=dtr.BIG_SEED)
    at = 0
    for numel in (5, 1, 8, 1023):
        xs = _x(numel, torch.bfloat16, seed=1)
        out, mk = ops.dropout_fwd(xs.cuda(), rd, "proj")
        torch.cuda.synchronize()
        _check_fwd(xs, 0.5, dtr.BIG_SEED, at, out.cpu(), mk.cpu().numpy(), ("BlockDrop", numel))
        at += (numel + 3) // 4


def test_dropout_fwd_past_one_grid():
    """n4 = 16384 * 256 + 301 groups: the first 301 threads take a second, grid-strided group (bf16, with an n % 4 == 3 tail)."""
    n = 4 * (dtr.GRID_GROUPS + 300) + 3
    p, seed, off = 0.1, dtr.BIG_SEED, 2 ** 32 - 1000
    x = _x(n, torch.bfloat16)
    out, mask = _fwd(x, p, seed, off)
    want = dtr.keep_mask(n, p, seed, off)
    head, tail = 4096, 4 * 300 + 3
    for sl in (slice(0, head), slice(n - tail, n)):
        assert np.array_equal(mask[sl], want[sl])
        _same_bits(out[sl], dtr.dropout_out(x[sl].float().numpy(), want[sl], dtr.inv_keep(p)), sl)
    assert int(mask.sum()) == int(want.sum())
    assert np.array_equal(mask, want)                          # and in fact every flag
    assert not torch.isnan(out.float()).any()


@pytest.mark.parametrize("n", [5, dtr.GRID_GROUPS + 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_dropout_apply_given_mask(dtype, n):
    from eventpretrain_amd._lib import call, dt, ptr, stream_ptr
    x = _x(n, dtype, seed=2)
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(n % 97)) < 0.6).to(torch.uint8)
    scale = np.float32(1.0) / np.float32(0.7)
    xd, md = x.cuda(), mask.cuda()
    out = torch.full_like(xd, float("nan"))
    call("evp_dropout_apply", ptr(xd), dt(xd), ptr(md), ptr(out), n, float(scale), stream_ptr())
    torch.cuda.synchronize()
    _same_bits(out.cpu(), dtr.dropout_out(x.float().numpy(), mask.numpy(), scale), ("apply", n))


# ---- evp_rows_scale_f32 ----------------------------------------------------------------------------------------------------------
def _rows_scale(x, u, kp, rps, res, want_out, want_lp):
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    M, D = x.shape
    xd = x.cuda()
    ud = None if u is None else torch.from_numpy(u).cuda()
    rd = None if res is None else res.cuda()
    out = torch.full((M, D), float("nan"), device="cuda") if want_out else None
    lp = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device="cuda") if want_lp else None
    call("evp_rows_scale_f32", ptr(xd), ptr(ud), float(kp), ptr(rd), M, D, rps, ptr(out), ptr(lp), stream_ptr())
    torch.cuda.synchronize()
    return None if out is None else out.cpu(), None if lp is None else lp.cpu()


def _check_rows_scale(x, u, kp, rps, res, out, lp, what):
    xn = x.numpy()
    rn = None if res is None else res.numpy()
    prod, _, unfused = dtr.rows_scale_truth(xn, u, kp, rps, None if rn is None else rn)
    if lp is not None:
        _same_bits(lp, prod, (what, "lp"))                      # bf16 of s_b * x, never of the sum
    if out is None:
        return
    if res is None:
        _same_bits(out, prod, (what, "out"))
        return
    o = out.numpy()
    off = o.view(np.int32) != unfused.view(np.int32)           # not the unfused sum: then it must be the fused one
    if off.any():
        s = np.broadcast_to(np.repeat(dtr.rows_factor(u, kp, (x.shape[0] + rps - 1) // rps), rps)[:x.shape[0], None], xn.shape)
        fused = dtr.fma_f32(xn[off], s[off], rn[off])
        assert np.array_equal(o[off].view(np.int32), fused.view(np.int32)), (what, "out is neither RN(x*s + res) nor RN(RN(x*s) + res)")


ROWS_DRAWS = ["straddle", "neighbours", "null", "kp1"]


@pytest.mark.parametrize("draws", ROWS_DRAWS)
@pytest.mark.parametrize("D", [4, 12])
def test_rows_scale_boundary_and_pointer_forms(D, draws):
    M, rps, kp = 6, 3, 0.7
    g = torch.Generator().manual_seed(D)
    x, res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    u = None if draws == "null" else dtr.boundary_draws(kp)["straddle" if draws == "kp1" else draws]
    if draws == "kp1":
        kp = 1.0
    s = dtr.rows_factor(u, kp, 2)
    if draws == "straddle":
        assert s[0] == 0 and s[1] > 1                           # sample 0 dropped, sample 1 kept
    if draws in ("null", "kp1"):
        assert (s == 1).all()
    for with_res in (False, True):
        for want_out, want_lp in ((True, False), (False, True), (True, True)):
            r = res if with_res else None
            out, lp = _rows_scale(x, u, kp, rps, r, want_out, want_lp)
            _check_rows_scale(x, u, kp, rps, r, out, lp, (D, draws, with_res, want_out, want_lp))


def test_rows_scale_past_one_grid():
    """M * D / 4 = 4,300,800 float4 groups > 16384 * 256: grid-stride, with out, lp and res, and the boundary pair among the draws."""
    M, D, rps, kp = 4200, 4096, 3, 0.7
    g = torch.Generator().manual_seed(9)
    x, res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    u = torch.rand(M // rps, generator=g).numpy()
    u[[0, 1, -2, -1]] = np.tile(dtr.boundary_draws(kp)["straddle"], 2)
    s = dtr.rows_factor(u, kp, M // rps)
    assert s[0] == 0 and s[1] > 1 and s[-2] == 0 and s[-1] > 1
    out, lp = _rows_scale(x, u, kp, rps, res, True, True)
    _check_rows_scale(x, u, kp, rps, res, out, lp, "past one grid")


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from eventpretrain_amd._lib import EVP_BF16, EVP_F32, EvpError, call, ptr, stream_ptr
    x = torch.zeros(16, device="cuda")
    out = torch.full((16,), float("nan"), device="cuda")
    mask = torch.zeros(16, dtype=torch.uint8, device="cuda")
    F64 = 2
    assert F64 not in (EVP_F32, EVP_BF16)
    bad_fwd = {"p = 1": (EVP_F32, 16, 1.0), "p < 0": (EVP_F32, 16, -0.1), "n = 0": (EVP_F32, 0, 0.1), "dtype": (F64, 16, 0.1)}
    for what, (dtype, n, p) in bad_fwd.items():
        with pytest.raises(EvpError):
            call("evp_dropout_fwd", ptr(x), dtype, ptr(out), ptr(mask), n, p, 1, None, 0, stream_ptr())
    for dtype, n in ((F64, 16), (EVP_F32, 0)):
        with pytest.raises(EvpError):
            call("evp_dropout_apply", ptr(x), dtype, ptr(mask), ptr(out), n, 2.0, stream_ptr())
    x2 = torch.zeros(4, 6, device="cuda")
    o2 = torch.full((4, 8), float("nan"), device="cuda")
    with pytest.raises(EvpError):                               # D % 4 != 0
        call("evp_rows_scale_f32", ptr(x2), None, 0.7, None, 4, 6, 2, ptr(o2), None, stream_ptr())
    for kp in (0.0, -0.5):                                      # keep_prob <= 0
        with pytest.raises(EvpError):
            call("evp_rows_scale_f32", ptr(o2), None, kp, None, 4, 8, 2, ptr(o2), None, stream_ptr())
    with pytest.raises(EvpError):                               # both outputs NULL
        call("evp_rows_scale_f32", ptr(o2), None, 0.7, None, 4, 8, 2, None, None, stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(o2).all()     # a refused call launches nothing

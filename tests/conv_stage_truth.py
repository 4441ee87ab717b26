"""Float64 truth, per-element bounds and the case list for the ConvViT stage kernels of csrc/conv.hip: the depthwise 5x5
convolution with the fused keep mask (band form and row walkers; forward, data, weight and bias gradient) and the NHWC patch
gather / scatter. Shared by test_conv_stage_truth_host.py (proves the truth, the case list and that the bounds bite, on the CPU) and
test_gpu_conv_stage_truth.py (runs the kernels).

Truth: F.conv2d(x * keep, w, b, padding=2, groups=C) and autograd in float64, on exactly the values the kernel receives (bf16 mode:
x and dy rounded to bf16 first; taps, bias and mask are f32 in both modes). keep = 1 - mask, upsampled by the mask scale.

Bounds, per ELEMENT, from the arithmetic alone (u = 2^-24; nothing here was measured):
  y, dx (f32)  a chain of 25 products and a bias, each product and each add rounded once (contraction is off), the keep factor one
               more: 2 * 26 * u * (|w| conv |keep * x| + |b|), obtained by running the same float64 convolution on absolute values
               (dx: the flipped taps on |dy|, times keep).
  dw, db       f32 in both modes. A thread sums at most 4 * W products, at most 16 LDS partials meet, then the nslab slab rows in
               dwconv_bwd_weight_finalize: (4 * W + 16 + nslab + 1) * u * sum |dy * keep * x| per tap, sum |dy| for db.
  y, dx (bf16) the f32 bound * (1 + 2^-8) + 2^-8 * |ref|: one round-to-nearest-even to 8 significant bits.
  fractional keep, bf16, BAND form: chunk_scale<bf16_t> rounds keep * x to bf16 while it stages the band, so
               y gets + 2^-8 * (|w| conv |keep * x|), and -- the same staged band feeds the weight-gradient band kernel --
               dw gets + 2^-8 * sum |dy * keep * x|. The row walkers keep the product in f32 and must meet the plain bound; dx never
               sees the staged product (the data gradient stages dy unmasked).
Every element is compared. Where the bound is 0 (a masked-out dx position, say) the result must be exactly the truth."""
import functools

import torch
import torch.nn.functional as F

U24, U8 = 2.0 ** -24, 2.0 ** -8
DTYPES = ("f32", "bf16")
CB = {"f32": 32, "bf16": 64}            # channels per band workgroup (128 bytes per position)
DW_ROWS = 16                            # rows per weight-gradient slab
FWD_ROWS = 8                            # rows per block of the forward / data-gradient row walker (4 waves x 2)

# (B, H, W, C, mask scale [0 = no mask], fractional keep): what each reaches
CASES = {
    "band_min": (1, 4, 8, 32, 0, False),      # smallest f32 band launch; bf16 -> rows (C % 64); B*H = 4 leaves two waves idle
    "odd_w": (3, 4, 9, 64, 1, False),         # odd W in the band (seg_x0 bump); mask at map resolution
    "w64": (1, 8, 64, 64, 4, False),          # W = 64: the largest LDS request of all three band kernels
    "w65": (1, 4, 65, 64, 0, False),          # just over the band limit: automatic fall-back with the switch on
    "ragged": (3, 5, 7, 68, 1, False),        # H % 4, W < 8, lane cut mid-wave, B*H = 15 (one-row wave, 3-row bwd-weight wave)
    "c96": (2, 12, 20, 96, 4, False),         # f32 band / bf16 rows at one shape; 3 x 5 mask grid
    "slabs": (5, 4, 8, 128, 2, False),        # B*H = 20: several bands per slab and a short last slab; two channel blocks
    "frac": (2, 8, 12, 64, 4, True),          # mask values from {0, 0.25, 1}: the chunk_scale branch
}


def band_ok(H, W, C, dtype):
    """csrc/conv.hip band_ok<T>, restated."""
    return H % 4 == 0 and 8 <= W <= 64 and C % CB[dtype] == 0


def form(case, dtype, band_switch):
    B, H, W, C, scale, frac = CASES[case]
    return "band" if band_switch and band_ok(H, W, C, dtype) else "rows"


def nslab(case):
    B, H = CASES[case][:2]
    return (B * H + DW_ROWS - 1) // DW_ROWS


@functools.lru_cache(maxsize=None)
def inputs(case, dtype):
    """Fixed-seed CPU float32 tensors of one case: x, dy [B,H,W,C] (rounded to bf16 in bf16 mode), w [C,25], b [C], mask [B, gh*gw]
    or None."""
    B, H, W, C, scale, frac = CASES[case]
    g = torch.Generator().manual_seed(sorted(CASES).index(case) + 17)
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)
    if dtype == "bf16":
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    w, b = torch.randn(C, 25, generator=g) * 0.2, torch.randn(C, generator=g)
    mask = None
    if scale:
        L = (H // scale) * (W // scale)
        r = torch.rand(B, L, generator=g)
        mask = torch.where(r < 0.4, 0.0, torch.where(r < 0.7, 0.25, 1.0)) if frac else (r < 0.5).float()
    return dict(x=x, dy=dy, w=w, b=b, mask=mask)


def keep_map(mask, B, H, W, scale, dt, swap_grid=False):
    """[B,1,H,W] keep factor of every position: 1 - mask[b, (y / s) * gw + x / s]. swap_grid (a planted fault): the row stride of
    the mask grid taken as gh instead of gw."""
    if mask is None:
        return torch.ones(B, 1, H, W, dtype=dt)
    gh, gw = H // scale, W // scale
    yy, xx = torch.meshgrid(torch.arange(H) // scale, torch.arange(W) // scale, indexing="ij")
    idx = (yy * (gh if swap_grid else gw) + xx) % (gh * gw)
    return (1 - mask.to(dt))[:, idx].unsqueeze(1)


def _conv(x, w, b, C, pad_fault=False):
    if pad_fault:                       # planted: only ONE halo column on the left (every tap reads one column off)
        return F.conv2d(F.pad(x, (1, 3, 2, 2)), w, b, groups=C)
    return F.conv2d(x, w, b, padding=2, groups=C)


def evaluate(case, dtype, dt=torch.float64, fault=None):
    """{y, dx [B,H,W,C], dw [C,25], db [C]} of one case in precision `dt`. fault: None or one planted fault of FAULTS."""
    B, H, W, C, scale, frac = CASES[case]
    t = inputs(case, dtype)
    x = t["x"].to(dt).permute(0, 3, 1, 2).clone().requires_grad_(True)
    dy = t["dy"].to(dt).permute(0, 3, 1, 2)
    w = t["w"].to(dt).view(C, 1, 5, 5).clone().requires_grad_(True)
    b = t["b"].to(dt).clone().requires_grad_(True)
    keep = keep_map(t["mask"], B, H, W, scale, dt, swap_grid=fault == "grid_swapped")
    taps = w.transpose(2, 3) if fault == "taps_transposed" else w
    y = _conv(x * keep, taps, b, C, pad_fault=fault == "pad_one_side")
    if fault == "bias_twice":
        y = y + b.view(1, C, 1, 1)
    y.backward(dy)
    dx = x.grad
    if fault == "dx_unflipped":         # the data gradient is the FLIPPED kernel on dy; planted: the taps as they are
        dx = keep * F.conv2d(dy, w.detach(), None, padding=2, groups=C)
    if fault == "dx_keep_on_input":     # planted: keep multiplies dy before the convolution instead of the result after it
        dx = F.conv2d(dy * keep, w.detach().flip(2, 3), None, padding=2, groups=C)
    return dict(y=y.detach().permute(0, 2, 3, 1).contiguous(), dx=dx.detach().permute(0, 2, 3, 1).contiguous(),
                dw=w.grad.view(C, 25), db=b.grad)


# planted fault -> the tensors it must push outside the bound, and whether it needs a mask to matter
FAULTS = {
    "taps_transposed": (("y", "dx", "dw"), False),
    "dx_unflipped": (("dx",), False),
    "dx_keep_on_input": (("dx",), True),
    "grid_swapped": (("y", "dx", "dw"), True),
    "pad_one_side": (("y", "dx", "dw"), False),
    "bias_twice": (("y",), False),
}


@functools.lru_cache(maxsize=None)
def truth(case, dtype):
    """(float64 reference, magnitudes) of one case, computed once and shared; nobody writes to it. Magnitudes: the same float64
    convolutions on absolute values -- A["y"] = |w| conv |keep x| (without |b|), A["b"] = |b|, A["dx"], A["dw"], A["db"]."""
    B, H, W, C, scale, frac = CASES[case]
    ref = evaluate(case, dtype)
    t = inputs(case, dtype)
    d = torch.float64
    keep = keep_map(t["mask"], B, H, W, scale, d)
    ax = ((t["x"].to(d).permute(0, 3, 1, 2) * keep).abs()).requires_grad_(True)
    ady = t["dy"].to(d).permute(0, 3, 1, 2).abs()
    aw = t["w"].to(d).view(C, 1, 5, 5).abs().requires_grad_(True)
    ay = F.conv2d(ax, aw, None, padding=2, groups=C)
    ay.backward(ady)                    # ax.grad = flipped |w| on |dy|;  aw.grad = sum |dy| * |keep x| per tap
    A = dict(y=ay.detach().permute(0, 2, 3, 1).contiguous(), b=t["b"].to(d).abs(),
             dx=(keep * ax.grad).permute(0, 2, 3, 1).contiguous(), dw=aw.grad.view(C, 25), db=ady.sum((0, 2, 3)))
    return ref, A


def bounds(case, dtype, kernel_form):
    """{y, dx, dw, db: per-element bound} for results of `kernel_form` ("band" / "rows") in mode `dtype`."""
    B, H, W, C, scale, frac = CASES[case]
    ref, A = truth(case, dtype)
    chain = 2 * 26 * U24
    red = (4 * W + 16 + nslab(case) + 1) * U24
    bd = dict(y=chain * (A["y"] + A["b"]), dx=chain * A["dx"], dw=red * A["dw"], db=red * A["db"])
    if dtype == "bf16":
        for k in ("y", "dx"):
            bd[k] = bd[k] * (1 + U8) + U8 * ref[k].abs()
        if frac and kernel_form == "band":
            bd["y"] = bd["y"] + U8 * A["y"]
            bd["dw"] = bd["dw"] + U8 * A["dw"]
    return bd


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; an element with bound 0 counts 0 when exact and inf when not."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    return ratio.max().item()


# ---- NHWC patch gather / scatter (pure copies: exact) ------------------------------------------------------------------------------
def patchify_ref(x, ids_keep, p):
    """x [B,H,W,C] -> cols [B * n_keep, C*p*p]: cols[(b,j), c*p*p + py*p + px] = x[b, gy*p + py, gx*p + px, c], (gy, gx) the grid
    position of token ids_keep[b,j] (all L tokens in order when ids_keep is None)."""
    B, H, W, C = x.shape
    gh, gw = H // p, W // p
    pt = x.view(B, gh, p, gw, p, C).permute(0, 1, 3, 5, 2, 4).reshape(B, gh * gw, C * p * p)
    if ids_keep is not None:
        pt = torch.gather(pt, 1, ids_keep.unsqueeze(-1).expand(-1, -1, C * p * p))
    return pt.reshape(-1, C * p * p).contiguous()


def unpatchify_ref(dcols, ids_keep, B, H, W, C, p, base=None):
    """The scatter back: dx [B,H,W,C] float32 = (base, or zeros) with dcols added at the kept patches (each patch once)."""
    gh, gw = H // p, W // p
    L = gh * gw
    pt = torch.zeros(B, L, C * p * p)
    d = dcols.float().view(B, -1, C * p * p)
    if ids_keep is None:
        pt = d.clone()
    else:
        pt.scatter_(1, ids_keep.unsqueeze(-1).expand(-1, -1, C * p * p), d)
    dx = pt.view(B, gh, gw, C, p, p).permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, C)
    return dx.contiguous() if base is None else base + dx

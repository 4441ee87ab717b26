#!/usr/bin/env python3
"""One SHA-256 per case and output tensor of the dense-prediction heads' kernels and autograd functions: the ten entry points of
csrc/dense.hip (each element type on either side, contiguous and as column slices of wider buffers), one cast-copy large enough for the
grid-stride loop to wrap, the bilinear view of csrc/augment.hip on crops whose taps are clamped at the crop's edge, and ops.LinearFn /
DenseClsFn / LinearBNFn / ConvBNFn with every gradient they deliver. Run it from two checkouts on the same GPU and compare the lists
line by line: the library is built with -ffp-contract=off, so a change that keeps the order of the floating-point operations keeps every
digest. Inputs are drawn on the CPU from fixed seeds, every output holds FILL before a launch, every case is launched twice and the two
launches must agree. Where evp_colsum (per-column atomics, any order) is on the path the gradient is integer-valued, |v| <= 8: every
partial sum is exact.

tests/test_gpu_dense_forms.py takes its shapes and launchers from here."""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from eventpretrain_amd import ops  # noqa: E402
from eventpretrain_amd._lib import call, dt, ptr, stream_ptr  # noqa: E402
from eventpretrain_amd.testing import det_normalish  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
FILL = 7.0                       # what every output holds before a launch
B, H, W, C = 2, 3, 5, 8
R = B * H * W
POOL_S = (1, 2, 3)               # s = 2 on H = 3: overlapping bins
RESIZE = ((7, 4), (3, 5))        # (3, 5) -> up along H and down along W; -> itself
IN_OFF, IN_PAD = 4, 8            # the strided form: the input is the columns [IN_OFF, IN_OFF + width) of a buffer IN_PAD wider,
OUT_OFF, OUT_PAD = 8, 16         # the output the columns [OUT_OFF, OUT_OFF + width) of a buffer OUT_PAD wider
WRAP = (8200, 520)               # > 16384 blocks x 256 threads: every thread of the map kernel takes a second element
VIEW = dict(C=5, H=37, W=53, size=(40, 300), rows=[(10, 8, 30, 20, 0, 0), (10, 8, 30, 20, 1, 1), (1, 1, 51, 35, 0, 1)])
HEAD_K = 24                      # input width of the autograd-level cases; their rows are R = B * H * W = 30


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def filled(*shape, dtype=F32):
    return torch.full(shape, FILL, dtype=dtype, device="cuda")


def _dn(d):
    return str(d)[6:]


# ---------------------------------------------------------------------------------------------------------------- raw entry points
def map_cases():
    """-> [(entry point, its options)]: every entry point of dense.hip on the one geometry."""
    cases = [("evp_im2col3x3", {}), ("evp_col2im3x3", {})]
    cases += [(e, dict(s=s)) for e in ("evp_adaptive_avgpool_fwd", "evp_adaptive_avgpool_bwd") for s in POOL_S]
    cases += [(e, dict(size=z)) for e in ("evp_upsample_bilinear_fwd", "evp_upsample_bilinear_bwd") for z in RESIZE]
    cases += [("evp_channel_scale", dict(table=t)) for t in (True, False)]
    cases += [(e, dict(relu=r)) for e in ("evp_batchnorm_eval", "evp_batchnorm_eval_bwd") for r in (0, 1)]
    return cases + [("evp_colsum_ordered", {})]


def map_shapes(entry, kw):
    """-> (input rows, input width, output rows, output width)."""
    small = B * kw["s"] ** 2 if "s" in kw else None
    big = B * kw["size"][0] * kw["size"][1] if "size" in kw else None
    return {"evp_im2col3x3": (R, C, R, 9 * C), "evp_col2im3x3": (R, 9 * C, R, C), "evp_adaptive_avgpool_fwd": (R, C, small, C),
            "evp_adaptive_avgpool_bwd": (small, C, R, C), "evp_upsample_bilinear_fwd": (R, C, big, C),
            "evp_upsample_bilinear_bwd": (big, C, R, C), "evp_colsum_ordered": (R, C, 1, C)}.get(entry, (R, C, R, C))


def map_operands(entry, kw):
    """The case's inputs on the CPU in float32: x [input rows, input width] and what else the entry point reads."""
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, entry + repr(sorted(kw.items())))))
    rows, width, _, _ = map_shapes(entry, kw)
    p = dict(x=torch.randn(rows, width, generator=gen))
    if kw.get("table"):
        p["m"] = (torch.rand(B, C, generator=gen) >= 0.3).float() / 0.7
    if "relu" in kw:
        p.update(gamma=1 + 0.2 * torch.randn(C, generator=gen), beta=0.1 * torch.randn(C, generator=gen),
                 rm=0.1 * torch.randn(C, generator=gen), rv=0.5 + torch.rand(C, generator=gen), y=torch.randn(R, C, generator=gen))
    return p


def _operand(t, dtype, strided):
    """t on the device in `dtype` -> (map, leading dimension): contiguous, or a column slice of a wider buffer."""
    if not strided:
        return t.to(dtype).cuda(), t.shape[1]
    wide = filled(t.shape[0], t.shape[1] + IN_PAD, dtype=dtype)
    wide[:, IN_OFF:IN_OFF + t.shape[1]] = t.to(dtype).cuda()
    return wide[:, IN_OFF:IN_OFF + t.shape[1]], wide.shape[1]


def map_launch(entry, kw, p, in_dtype=F32, out_dtype=F32, strided=False):
    """One launch -> (the whole output buffer, the slice the entry point was to write)."""
    _, _, orows, owidth = map_shapes(entry, kw)
    x, ldi = _operand(p["x"], in_dtype, strided)
    off, ldo = (OUT_OFF, owidth + OUT_PAD) if strided else (0, owidth)
    buf = filled(orows, ldo, dtype=out_dtype)
    view = buf[:, off:off + owidth]
    dev = {k: v.cuda() for k, v in p.items() if k not in ("x", "y")}
    s_ = stream_ptr()
    if entry == "evp_im2col3x3":            # no offset argument: the slice's own address (16-byte aligned at OUT_OFF = 8)
        call(entry, ptr(x), dt(x), ldi, B, H, W, C, ptr(view), dt(buf), ldo, s_)
    elif entry == "evp_col2im3x3":
        call(entry, ptr(x), dt(x), ldi, B, H, W, C, ptr(buf), dt(buf), ldo, off, s_)
    elif entry.startswith("evp_adaptive_avgpool"):
        call(entry, ptr(x), dt(x), ldi, B, H, W, C, kw["s"], ptr(buf), dt(buf), ldo, off, s_)
    elif entry.startswith("evp_upsample_bilinear"):
        call(entry, ptr(x), dt(x), ldi, B, H, W, kw["size"][0], kw["size"][1], C, ptr(buf), dt(buf), ldo, off, s_)
    elif entry == "evp_channel_scale":
        Bn, P = (B, H * W) if kw["table"] else (1, R)
        call(entry, ptr(x), dt(x), ldi, ptr(dev.get("m")), Bn, P, C, ptr(buf), dt(buf), ldo, off, s_)
    elif entry == "evp_batchnorm_eval":
        call(entry, ptr(x), dt(x), ldi, R, C, ptr(dev["gamma"]), ptr(dev["beta"]), ptr(dev["rm"]), ptr(dev["rv"]), EPS, kw["relu"],
             ptr(buf), dt(buf), ldo, off, s_)
    elif entry == "evp_batchnorm_eval_bwd":     # no offset argument
        y, ldy = _operand(p["y"], in_dtype, strided)
        call(entry, ptr(x), dt(x), ldi, ptr(y), dt(y), ldy, R, C, ptr(dev["gamma"]), ptr(dev["rv"]), EPS, kw["relu"], ptr(view), dt(buf),
             ldo, s_)
    else:                                       # evp_colsum_ordered: float32 [C]
        call(entry, ptr(x), dt(x), R, C, ldi, ptr(view), s_)
    return buf, view


def wrap_operand():
    return torch.randn(*WRAP, generator=torch.Generator().manual_seed(2000))


def wrap_launch(x, dtype=BF16):
    """evp_channel_scale without a table on WRAP: the cast-copy."""
    xd, out = x.cuda(), filled(*WRAP, dtype=dtype)
    call("evp_channel_scale", ptr(xd), dt(xd), WRAP[1], None, 1, WRAP[0], WRAP[1], ptr(out), dt(out), WRAP[1], 0, stream_ptr())
    return out


def view_launch():
    """evp_view_augment_bilinear_f32 on the boxes of tests/test_gpu_view_bilinear.py::test_taps_are_clamped_at_the_crop_edge."""
    v = VIEW
    x = det_normalish("gpu.bilinear.clamp", (len(v["rows"]), v["C"], v["H"], v["W"])).cuda()
    params = torch.tensor(v["rows"], dtype=torch.int32).cuda()
    out = filled(len(v["rows"]), v["C"], *v["size"])
    call("evp_view_augment_bilinear_f32", ptr(x), ptr(params), ptr(out), len(v["rows"]), v["C"], v["H"], v["W"], v["size"][0], v["size"][1], 1,
         stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------------------------- autograd level
def _leaf(t, dtype=F32):
    return t.to(dtype).cuda().requires_grad_(True)


def _grads(named):
    ops.flush_deferred_grads()
    return {"d" + k: t.grad for k, t in named.items()}


def linear(N, seed):
    """ops.LinearFn [2, 15, HEAD_K] -> N with an integer-valued gradient (its bias gradient is evp_colsum's)."""
    gen = torch.Generator().manual_seed(seed)
    x, w, b = torch.randn(2, 15, HEAD_K, generator=gen), 0.2 * torch.randn(N, HEAD_K, generator=gen), torch.randn(N, generator=gen)
    g = torch.randint(-8, 9, (2, 15, N), generator=gen).float().cuda()

    def run():
        t = dict(x=_leaf(x), w=_leaf(w), b=_leaf(b))
        y = ops.LinearFn.apply(t["x"], t["w"], t["b"])
        y.backward(g)
        return dict(y=y.detach(), **_grads(t))
    return run


def dense_cls(N, seed):
    gen = torch.Generator().manual_seed(seed)
    x, w, b = torch.randn(R, HEAD_K, generator=gen), 0.2 * torch.randn(N, HEAD_K, 1, 1, generator=gen), torch.randn(N, generator=gen)
    g = torch.randn(R, N, generator=gen).cuda()

    def run():
        t = dict(x=_leaf(x), w=_leaf(w), b=_leaf(b))
        y = ops.DenseClsFn.apply(t["x"], t["w"], t["b"])
        y.backward(g)
        return dict(y=y.detach(), **_grads(t))
    return run


def _bn_state(N, gen, affine=True):
    p = dict(gamma=1 + 0.2 * torch.randn(N, generator=gen), beta=0.1 * torch.randn(N, generator=gen)) if affine else {}
    return p, 0.1 * torch.randn(N, generator=gen), 0.5 + torch.rand(N, generator=gen)


def linear_bn(last, seed, N=16):
    """One stage of the contrastive heads: hidden (affine, ReLU, compute dtype out) or last (neither, float32 out)."""
    gen = torch.Generator().manual_seed(seed)
    x, w = torch.randn(2, 15, HEAD_K, generator=gen), 0.2 * torch.randn(N, HEAD_K, generator=gen)
    affine, rm, rv = _bn_state(N, gen, affine=not last)
    g = torch.randn(2, 15, N, generator=gen)

    def run():
        t = dict(x=_leaf(x), w=_leaf(w), **{k: _leaf(v) for k, v in affine.items()})
        rmd, rvd = rm.cuda(), rv.cuda()
        y = ops.LinearBNFn.apply(t["x"], t["w"], t.get("gamma"), t.get("beta"), rmd, rvd, EPS, 0.1, not last, last)
        y.backward(g.to(y.dtype).cuda())
        return dict(y=y.detach(), running_mean=rmd, running_var=rvd, **_grads(t))
    return run


def conv_bn(k, train, slot, seed, N=16):
    """ops.ConvBNFn on the [R, C] map, kernel k, into a buffer of its own or into the columns [OUT_OFF, OUT_OFF + N) of a wider one (the
    gradient then arrives as the same slice of a wider gradient, as CatFn hands it over)."""
    gen = torch.Generator().manual_seed(seed)
    x, w, b = torch.randn(R, C, generator=gen), 0.2 * torch.randn(N, C, k, k, generator=gen), torch.randn(N, generator=gen)
    affine, rm, rv = _bn_state(N, gen)
    gw = torch.randn(R, N + OUT_PAD, generator=gen)

    def run():
        T = ops.get_compute_dtype()
        t = dict(x=_leaf(x), w=_leaf(w), b=_leaf(b), **{k_: _leaf(v) for k_, v in affine.items()})
        rmd, rvd = rm.cuda(), rv.cuda()
        buf = filled(R, N + OUT_PAD, dtype=T) if slot else None
        y = ops.ConvBNFn.apply(t["x"], t["w"], t["b"], t["gamma"], t["beta"], rmd, rvd, B, H, W, EPS, 0.1, True, train,
                               (buf, OUT_OFF) if slot else None)
        gd = gw.to(T).cuda()[:, OUT_OFF:OUT_OFF + N]
        y.backward(gd if slot else gd.contiguous())
        return dict(y=(buf if slot else y.detach()), running_mean=rmd, running_var=rvd, **_grads(t))
    return run


def autograd_cases():
    """-> [(tag, launcher)]; run under each compute dtype."""
    cases = [(f"LinearFn N={N}", linear(N, 3000 + N)) for N in (10, 16)]
    cases += [(f"DenseClsFn N={N}", dense_cls(N, 3100 + N)) for N in (2, 11, 16)]
    cases += [(f"LinearBNFn {'last' if last else 'hidden'}", linear_bn(last, 3200 + last)) for last in (False, True)]
    cases += [(f"ConvBNFn k={k} {'train' if train else 'eval'} slot={int(slot)}", conv_bn(k, train, slot, 3300 + 10 * k + 2 * train + slot))
              for k, train, slot in itertools.product((1, 3), (True, False), (False, True))]
    return cases


# ---------------------------------------------------------------------------------------------------------------- the list
_differ = []


def _emit(tag, fn):
    """Launch twice, note outputs that differ, print one line with a digest per output that was asked for."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    parts = []
    for k, v in a.items():
        if v is None:
            continue
        if not torch.equal(v.contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)):
            _differ.append(f"{tag}: two launches differ in {k}")
        parts.append(f"{k} {digest(v)}")
    print(f"{tag:72s} " + " ".join(parts), flush=True)


def main():
    for entry, kw in map_cases():
        p = map_operands(entry, kw)
        outs = (F32,) if entry == "evp_colsum_ordered" else (F32, BF16)
        for ind, outd, strided in itertools.product((F32, BF16), outs, (False, True)):
            opts = " ".join(f"{k}={v}" for k, v in kw.items()).replace(" ", "")
            _emit(f"{entry} {opts} {_dn(ind)}->{_dn(outd)} strided={int(strided)}",
                  lambda: dict(buf=map_launch(entry, kw, p, ind, outd, strided)[0]))
    x = wrap_operand()
    _emit(f"evp_channel_scale cast-copy {WRAP[0]}x{WRAP[1]} float32->bfloat16", lambda: dict(out=wrap_launch(x)))
    _emit("evp_view_augment_bilinear_f32 clamp boxes 5x37x53 -> 40x300", lambda: dict(out=view_launch()))
    for T in (F32, BF16):
        ops.set_compute_dtype(T)
        for tag, fn in autograd_cases():
            _emit(f"{tag} compute={_dn(T)}", fn)
    ops.set_compute_dtype(F32)
    if _differ:
        print("\n".join(_differ))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""numpy float32 restatement of evp_view_augment_bilinear_f32 (include/evtpretrain.h): crop -> F.interpolate(mode='bilinear',
align_corners=None) of the cropped view -> horizontal flip of the resized view -> time flip (reversed bin order, negated on request).
Every operation is one float32 operation; fmaf is emulated through float64 (see `fmaf`). tests/test_view_bilinear_host.py pins it to the
reference's own outputs bit for bit, so the GPU tests can hold the kernel to equality on shapes no fixture covers."""
import numpy as np

F32, F64 = np.float32, np.float64


def fmaf(a, b, c):
    """round32(a * b + c) with ONE rounding, for float32 arrays. In float64 the product of two float32 is exact (48 bits); the sum is
    rounded to 53 bits, and rounding that again to float32 goes wrong only when the float64 sum sits exactly half-way between two
    float32 while the exact sum does not: there the TwoSum error term says on which side the exact sum lies."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.asarray(c, F32).astype(F64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # exact: a * b + c == s + err
    tie = (np.ascontiguousarray(s).view(np.int64) & ((1 << 29) - 1)) == (1 << 28)
    s = np.where(tie & (err > 0), np.nextafter(s, np.inf), np.where(tie & (err < 0), np.nextafter(s, -np.inf), s))
    return s.astype(F32)


def axis_taps(n_in, n_out):
    """-> (i0, i1 int64 [n_out], l0, l1 float32 [n_out]): the two taps and weights of every output index along one axis."""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32) + F32(0.5)
    src = np.maximum(F32(0), fmaf(np.full(n_out, scale, F32), dst, np.full(n_out, -0.5, F32)))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def bilinear_resize(view, out_hw):
    """view float32 [C,h,w] -> [C,Ho,Wo]: top = fmaf(lx0, a, lx1 * b), bot = fmaf(lx0, c, lx1 * d), out = fmaf(ly0, top, ly1 * bot)."""
    view = np.ascontiguousarray(view, F32)
    Ho, Wo = out_hw
    y0, y1, ly0, ly1 = axis_taps(view.shape[1], Ho)
    x0, x1, lx0, lx1 = axis_taps(view.shape[2], Wo)
    lx0, lx1 = lx0[None, None, :], lx1[None, None, :]
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    a, b = view[:, y0][:, :, x0], view[:, y0][:, :, x1]
    c, d = view[:, y1][:, :, x0], view[:, y1][:, :, x1]
    top = fmaf(lx0, a, (lx1 * b).astype(F32))
    bot = fmaf(lx0, c, (lx1 * d).astype(F32))
    return fmaf(ly0, top, (ly1 * bot).astype(F32))


def evg_bilinear(view, params, out_hw, negate=True):
    """view float32 [C,H,W], params (x0, y0, w, h, hflip, tflip) -> float32 [C,Ho,Wo], as evg_augment(mode='bilinear') transforms it
    given the decisions."""
    x0, y0, w, h, hflip, tflip = (int(v) for v in params)
    out = bilinear_resize(view[:, y0:y0 + h, x0:x0 + w], out_hw)
    if hflip:
        out = out[:, :, ::-1]
    if tflip:
        out = out[::-1]
        if negate:
            out = -out
    return np.ascontiguousarray(out, dtype=F32)

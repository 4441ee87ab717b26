"""numpy restatement of the event-count images (include/evtpretrain.h K30: evp_event_image_count, _finish, _normalize) in integer
arithmetic: counts are int64 sums, the hot-pixel statistics are exact integer sums and a float64 threshold, and the normalisation is
one float32 operation after the other. tests/test_count_image_host.py pins it to the reference's own outputs
(tests/golden/ft_count_images.npz) exactly, so the GPU tests can hold the kernels to equality on inputs no fixture covers."""
import numpy as np

F32, F64 = np.float32, np.float64


def count_planes(events, size, scale=(1.0, 1.0)):
    """events float64 [n,4] (x,y,t,p) -> (planes int64 [3,H,W] for p == 1, p == 0, p == -1, rows with p == 0, rows outside the grid).
    lin = trunc(x * sx) + trunc(y * sy) * W with the products in float64; a row counts when 0 <= lin < H * W."""
    H, W = int(size[0]), int(size[1])
    ev = np.asarray(events, F64).reshape(-1, 4)
    planes = np.zeros((3, H * W), np.int64)
    outside = 0
    for k, pol in enumerate((1.0, 0.0, -1.0)):
        rows = ev[ev[:, 3] == pol]
        xs, ys = rows[:, 0] * F64(scale[0]), rows[:, 1] * F64(scale[1])
        fine = (np.abs(xs) < 4.0e18) & (np.abs(ys) < 2.0e9)
        outside += int((~fine).sum())
        lin = np.trunc(xs[fine]).astype(np.int64) + np.trunc(ys[fine]).astype(np.int64) * W
        inside = (lin >= 0) & (lin < H * W)
        outside += int((~inside).sum())
        np.add.at(planes[k], lin[inside], 1)
    return planes.reshape(3, H, W), int((ev[:, 3] == 0.0).sum()), outside


def hot_threshold(pos, neg):
    """The float64 threshold of remove_hot_pixel_mem on the values k / 255 of the two integer planes: mean + 10 * unbiased std."""
    k = np.concatenate([np.asarray(pos, np.int64).reshape(-1), np.asarray(neg, np.int64).reshape(-1)])
    n = F64(k.size)
    s1, s2 = F64(int(k.sum())), F64(int((k * k).sum()))
    mean = s1 / n / F64(255.0)
    var = (s2 - s1 * s1 / n) / (n - F64(1.0)) / F64(255.0 * 255.0)
    return mean + F64(10.0) * np.sqrt(var if var > 0 else F64(0.0))


def raw_image(events, num_bins, size, scale=(1.0, 1.0)):
    """-> (float32 [num_bins,H,W], rows outside the grid): events_to_image_ecdp (2), or events_to_image_mem, / 255 and
    remove_hot_pixel_mem (3). The negative plane is the p == 0 plane when the clip has a p == 0 row, else the p == -1 plane."""
    planes, n_zero, outside = count_planes(events, size, scale)
    pos, neg = planes[0], planes[1] if n_zero > 0 else planes[2]
    if int(num_bins) == 2:
        return np.stack([pos, neg]).astype(F32), outside
    fa, fb = pos.astype(F32) / F32(255.0), neg.astype(F32) / F32(255.0)
    hot = (fa.astype(F64) > hot_threshold(pos, neg)) | (fb.astype(F64) > hot_threshold(pos, neg))
    fa, fb = np.where(hot, F32(0), fa), np.where(hot, F32(0), fb)
    return np.stack([fa, np.zeros_like(fa), fb]).astype(F32), outside


def normalize(view, guard=False):
    """The datasets' tail on a view float32 [C,S,S] -> (float32 [C,S,S], 1 if a 3-channel view is all zero else 0)."""
    v = np.ascontiguousarray(view, F32)
    if v.shape[0] == 2:
        d = (v.max(axis=(1, 2), keepdims=True) + F32(1.0)).astype(F32)
        return (((v / d).astype(F32) - F32(0.5)).astype(F32) * F32(2.0)).astype(F32), 0
    m = F32(v[0::2].max())
    with np.errstate(divide="ignore", invalid="ignore"):
        f = F32(1000.0) if (m == 0 and guard) else F32(1.0) / m
        out = v.copy()
        out[0::2] = (v[0::2] * f).astype(F32)
    return out, int(m == 0)

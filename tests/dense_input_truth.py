"""numpy restatements the dense-input kernels are held to with array_equal (csrc/labels.hip).

The two label views restate the reference's semseg_label_augment, flow_label_augment (with evg_augment's time-flip flag) and
flow_label_valid_augment of the dataset's valid mask (dataset/augmentation/view_augment.py:91-134) for GIVEN crop rows
{x0, y0, w, h, hflip, tflip}; tests/test_dense_input_host.py holds them to tests/golden/dense_label_views.npz, made by the reference's own
functions, bit for bit.

`rectify_compact` restates ft_dsec_dataset.py:211-226 (look every event up in the rectify map, keep what lands in the sensor, stack the
survivors) and ft_ddd17_dataset.py:116-127 (crop mask, then the tail) LINE BY LINE: the reference has no callable for either outside its
h5py-backed __getitem__, so this one truth is a restatement and not a fixture."""
import numpy as np

from oracle.augment_oracle import nearest_index


GOLDEN_SHAPES = ((11, 14), (5, 300), (44, 64), (26, 35))      # (H, W) of tests/golden/dense_label_views.npz
GOLDEN_SEEDS = tuple(range(12))
F32_BELOW_1000 = np.float32(999.99994)                         # the largest float32 below 1000


def label_input(H, W):
    """uint8 [1,H,W] labels in 0..11 from the package's deterministic fill, 255 (the ignore label) planted in the corners and inside."""
    from eventpretrain_amd.testing import det_uniform
    lab = (det_uniform(f"dense_label_{H}x{W}", (1, H, W), 0.0, 12.0).numpy()).astype(np.uint8)
    lab[0, 0, 0] = lab[0, -1, -1] = lab[0, 0, -1] = lab[0, H // 2, W // 2] = 255
    return lab


def flow_input(H, W):
    """float32 [2,H,W] flow in (-30, 30) from the package's deterministic fill, seven pixels in ten exact zeros in both components (a
    flow map is sparse, and the fixture stays small), and the edges of the valid rule planted along the first and the last row: +-1000,
    999.99994, 1e-6 next to a zero component, an exact zero."""
    from eventpretrain_amd.testing import det_uniform
    flow = det_uniform(f"dense_flow_{H}x{W}", (2, H, W), -30.0, 30.0).numpy().copy()
    flow[:, det_uniform(f"dense_flow_zero_{H}x{W}", (H, W), 0.0, 1.0).numpy() < 0.7] = 0.0
    plants = ((1000.0, 2.0), (-1000.0, 0.0), (F32_BELOW_1000, -F32_BELOW_1000), (1e-6, 0.0), (0.0, -1e-6), (0.0, 0.0), (3.0, 1000.0), (0.0, 5.0))
    for row in (0, H - 1):
        for k, (fx, fy) in enumerate(plants):
            flow[:, row, (1 + k) % W] = (fx, fy)
    return flow.astype(np.float32)


def _gather_index(params, out_hw):
    x0, y0, w, h, hflip, _ = (int(v) for v in params)
    Ho, Wo = out_hw
    ys = y0 + nearest_index(Ho, h)
    xs = x0 + nearest_index(Wo, w)
    return ys, xs[::-1] if hflip else xs


def semseg_label_view(label, params, out_hw):
    """label uint8 [1,H,W] (or [H,W]) -> int64 [1,Ho,Wo]: view_crop -> view_resize('nearest') -> view_horizontal_flip -> .long()."""
    lab = np.asarray(label).reshape((1,) + tuple(np.shape(label)[-2:]))
    ys, xs = _gather_index(params, out_hw)
    return np.ascontiguousarray(lab[:, ys][:, :, xs]).astype(np.int64)


def flow_valid_mask(flow):
    """The dataset's mask (ft_mvsec_dataset.py:275-278): (torch.norm(flow, dim=0) > 0) & (|fx| < 1000) & (|fy| < 1000) as float32 [1,H,W].
    norm > 0 iff the float32 sum of squares is > 0 wherever no square underflows (the pinned range: exact zeros, magnitudes >= 1e-6)."""
    fx, fy = np.asarray(flow[0], np.float32), np.asarray(flow[1], np.float32)
    sq = (fx * fx).astype(np.float32) + (fy * fy).astype(np.float32)
    return ((sq > 0) & (np.abs(fx) < 1000) & (np.abs(fy) < 1000)).astype(np.float32)[None]


def flow_label_view(flow, params, out_hw):
    """flow float32 [2,H,W] -> (float32 [2,Ho,Wo], valid float32 [1,Ho,Wo]): the nearest view of the flow times float32(new_w / org_w),
    float32(new_h / org_h) (python doubles rounded once by torch.tensor), x negated on a horizontal flip, both on a time flip; and the same
    view of the valid mask."""
    x0, y0, w, h, hflip, tflip = (int(v) for v in params)
    Ho, Wo = out_hw
    ys, xs = _gather_index(params, out_hw)
    src = np.asarray(flow, np.float32)[:, ys][:, :, xs]
    scale = np.array([Wo / w, Ho / h], dtype=np.float32)
    out = (src * scale[:, None, None]).astype(np.float32)
    if hflip:
        out = out * np.array([-1.0, 1.0], np.float32)[:, None, None]
    if tflip:
        out = out * np.array([-1.0, -1.0], np.float32)[:, None, None]
    valid = flow_valid_mask(flow)[:, ys][:, :, xs]
    return np.ascontiguousarray(out, dtype=np.float32), np.ascontiguousarray(valid, dtype=np.float32)


def rectify_compact(events, offsets, extent, keep_last, rectify_map=None):
    """events float64 [n,4], offsets [B+1] -> (rows float64 [m,4], offsets int64 [B+1], status [clips without a survivor, rows outside
    the map]). Per clip, as the reference:
        xy_rect = rectify_ev_maps[y, x]; mask = (x_rect >= 0) & (x_rect < W) & (y_rect >= 0) & (y_rect < H)       (DSEC, with a map)
        mask = (x >= 0) & (x < W) & (y >= 0) & (y < H)                                                             (DDD17, without)
        events = np.stack([x_rect, y_rect, t, p], -1)[mask];  events = events[max(len(events) - keep_last, 0):]
    A row whose (int)x, (int)y names no cell of the map -- where the reference asserts -- is dropped and counted."""
    H, W = extent
    rows, offs, empty, outside = [], [0], 0, 0
    for c in range(len(offsets) - 1):
        e = np.asarray(events[int(offsets[c]):int(offsets[c + 1])], dtype=np.float64)
        x, y = e[:, 0], e[:, 1]
        if rectify_map is not None:
            mh, mw = rectify_map.shape[:2]
            with np.errstate(invalid="ignore"):
                inside = (x > -1) & (x < mw) & (y > -1) & (y < mh)              # (int) truncates toward zero; a NaN names no cell
            outside += int((~inside).sum())
            e = e[inside]
            xy = rectify_map[np.trunc(e[:, 1]).astype(np.int64), np.trunc(e[:, 0]).astype(np.int64)]
            x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            mask = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        kept = np.stack([x, y, e[:, 2], e[:, 3]], axis=-1)[mask]
        kept = kept[max(kept.shape[0] - int(keep_last), 0):]
        empty += int(mask.sum() == 0)
        rows.append(kept)
        offs.append(offs[-1] + kept.shape[0])
    return (np.concatenate(rows, 0) if rows else np.zeros((0, 4))), np.asarray(offs, np.int64), np.asarray([empty, outside], np.int32)

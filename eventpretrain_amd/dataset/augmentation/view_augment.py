"""Voxel-grid view augmentation on the GPU (reference dataset/augmentation/view_augment.py:9-95: `view_crop` ->
`view_resize(mode='nearest' | 'bilinear')` -> `view_horizontal_flip` -> `evg_time_flip`), batched: one kernel launch
(evp_view_augment_f32, or evp_view_augment_bilinear_f32 for the fine-tuning recipe's mode) for B grids that K1 left in HBM.

The reference draws its random decisions from the process-global legacy numpy stream inside each DataLoader worker.
Here they are explicit, host-drawn int32 rows {x0, y0, w, h, hflip, tflip}:
  * `draw_evg_params(rs, ...)`  -- the reference's exact call order on a `numpy.random.RandomState`, so
    `RandomState(seed)` reproduces `evg_augment(..., seed=seed)` bit for bit (pinned by tests/golden/evg_augment.npz);
  * `draw_evg_params_batch(seed, step, B, ...)` -- a counter-based stream (Philox keyed by (seed, step, sample)): the
    decisions of a sample do not depend on worker scheduling or on how many draws other samples consumed.
The dense fine-tuning labels ride with the grid (view_augment.py:91-134: the reference re-seeds numpy with the sample's seed, so a label gets
the grid's crop box and flip coins): `semseg_label_augment_batch` and `flow_label_augment_batch` take the same rows (csrc/labels.hip).
The event-level augmentations (erase / add correlated events) are in events_augment.py next to this file."""
import math

import numpy as np
import torch

from ... import _lib
from ..._lib import call, ptr, stream_ptr


def draw_evg_params(rs, H, W, crop_min=0.8, ratio=(3 / 4, 4 / 3)):
    """Decisions of one evg_augment call, in the reference's draw order (view_augment.py:14-31,41,49)."""
    x0, y0, w, h = 0, 0, W, H
    area = W * H
    for _ in range(10):
        target_area = rs.uniform(crop_min, 1.0) * area
        aspect = rs.uniform(W / H * ratio[0], W / H * ratio[1])
        cw, ch = int(round(math.sqrt(target_area * aspect))), int(round(math.sqrt(target_area / aspect)))
        if rs.randint(0, 10) < 5:
            cw, ch = ch, cw
        if cw < W and ch < H:
            x0, y0, w, h = rs.randint(0, W - cw), rs.randint(0, H - ch), cw, ch
            break
    hflip = int(rs.random_sample() < 0.5)
    tflip = int(rs.random_sample() < 0.5)
    return x0, y0, w, h, hflip, tflip


def draw_evg_params_batch(seed, step, B, H, W, crop_min=0.8, first_sample=0, ratio=(3 / 4, 4 / 3), U=None):
    """int32 [B,6] rows for samples first_sample .. first_sample+B-1 of optimizer step `step`: sample i uses the Philox
    stream keyed by (seed, step, i). Same distribution as the reference's (same accept / reject rule: up to ten tries of
    (area, aspect, swap coin), the first box that fits is placed uniformly, else the whole view; then the two flip coins), vectorised
    over the batch: every sample draws the uniforms of all ten tries, the first accepted one is used.
    `H`, `W`: the view's size, scalars, or int arrays of length B -- a view of its own per sample (N-Cars: the window's extent; what
    evp_events_window_geometry draws on the device); row i then equals the scalar call for (H[i], W[i])."""
    if U is None:
        U = evg_uniforms(seed, step, B, first_sample)
    T = U[:, :50].reshape(B, 10, 5)
    if np.ndim(H) or np.ndim(W):
        H, W = (np.broadcast_to(np.asarray(v, dtype=np.int64), (B,)) for v in (H, W))
        return _draw_rows(U, T, H, W, H[:, None], W[:, None], crop_min, ratio)
    return _draw_rows(U, T, H, W, H, W, crop_min, ratio)


def _draw_rows(U, T, H, W, Ht, Wt, crop_min, ratio):
    """draw_evg_params_batch's arithmetic: (H, W) as they meet the per-sample columns, (Ht, Wt) as they meet the [B, 10] tries."""
    B = U.shape[0]
    area = Wt * Ht
    target = (crop_min + T[..., 0] * (1.0 - crop_min)) * area
    aspect = Wt / Ht * ratio[0] + T[..., 1] * (Wt / Ht * ratio[1] - Wt / Ht * ratio[0])
    cw = np.rint(np.sqrt(target * aspect)).astype(np.int64)
    ch = np.rint(np.sqrt(target / aspect)).astype(np.int64)
    swap = (T[..., 2] * 10).astype(np.int64) < 5
    cw, ch = np.where(swap, ch, cw), np.where(swap, cw, ch)
    ok = (cw < Wt) & (ch < Ht)
    first = np.argmax(ok, axis=1)
    any_ok = ok.any(axis=1)
    r = np.arange(B)
    cw1, ch1 = cw[r, first], ch[r, first]
    x0 = np.minimum((T[r, first, 3] * np.maximum(W - cw1, 1)).astype(np.int64), np.maximum(W - cw1 - 1, 0))
    y0 = np.minimum((T[r, first, 4] * np.maximum(H - ch1, 1)).astype(np.int64), np.maximum(H - ch1 - 1, 0))
    out = np.zeros((B, 6), dtype=np.int32)
    out[:, 0], out[:, 1] = np.where(any_ok, x0, 0), np.where(any_ok, y0, 0)
    out[:, 2], out[:, 3] = np.where(any_ok, cw1, W), np.where(any_ok, ch1, H)
    out[:, 4], out[:, 5] = U[:, 50] < 0.5, U[:, 51] < 0.5
    return out


def evg_uniforms(seed, step, B, first_sample=0):
    """float64 [B, 52] in [0, 1): the uniforms behind one sample's crop box and flip coins (shared counter stream, purpose 4). The frame's
    box is drawn from the SAME uniforms scaled to the frame's size (the reference re-seeds numpy with the sample's seed before
    frame_augment), so a caller that needs both passes this array to draw_evg_params_batch twice."""
    from .events_augment import philox_words
    return philox_words(seed, step, first_sample + np.arange(B), 4, 10 * 5 + 2).astype(np.float64) * 2.3283064365386963e-10


VIEW_KERNELS = {"nearest": "evp_view_augment_f32", "bilinear": "evp_view_augment_bilinear_f32"}     # evg_augment's `mode` -> the kernel


def evg_augment_batch(voxels, params, size, negate=None, out=None, mode="nearest"):
    """voxels float32 [B,C,H,W] on the GPU, params int32 [B,6] (host array or device tensor) -> float32
    [B,C,size[0],size[1]]; negate=None applies the reference's rule (5- or 6-bin grids are negated on a time flip).
    `mode`: the reference's resize mode -- "nearest" (the pre-training datasets) or "bilinear" (the fine-tuning default,
    main_finetune_cls.py:48), each equal to F.interpolate on the CPU bit for bit."""
    if mode not in VIEW_KERNELS:
        raise ValueError(f"evg_augment_batch: mode must be one of {sorted(VIEW_KERNELS)} (got {mode!r})")
    _lib.require_device()
    if not voxels.is_cuda or voxels.dtype != torch.float32 or not voxels.is_contiguous():
        raise _lib.EvpError("evg_augment_batch: voxels must be a contiguous float32 tensor in device memory")
    B, C, H, W = voxels.shape
    if not torch.is_tensor(params):
        p = np.ascontiguousarray(params, dtype=np.int32).reshape(B, 6)
        if ((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 2] < 1) | (p[:, 3] < 1) | (p[:, 0] + p[:, 2] > W) | (p[:, 1] + p[:, 3] > H)).any():
            raise ValueError("evg_augment_batch: crop box outside the view")
        params = torch.from_numpy(p).to(voxels.device, non_blocking=True)
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 6) or not params.is_contiguous():
        raise ValueError("evg_augment_batch: params must be int32 [B,6]")
    Ho, Wo = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty(B, C, Ho, Wo, dtype=torch.float32, device=voxels.device)
    if negate is None:
        negate = C in (5, 6)
    call(VIEW_KERNELS[mode], ptr(voxels), ptr(params), ptr(out), B, C, H, W, Ho, Wo, int(bool(negate)), stream_ptr())
    return out


def frame_augment_batch(frames, params, size, out=None):
    """Difference-map targets of the batch (reference view_augment.py:79-89 `frame_augment`): frames float32 [B,C,H,W] on the
    GPU, params int32 [B,6] -- THE SAME rows that went to evg_augment_batch (the reference re-seeds numpy with the sample's
    seed, so the crop box and the flip coin repeat; column 5 is evg_augment's time-flip flag, which negates the frame) ->
    float32 [B,C,size[0],size[1]], bicubic (ATen upsample_bicubic2d, align_corners=False)."""
    _lib.require_device()
    if not frames.is_cuda or frames.dtype != torch.float32 or not frames.is_contiguous():
        raise _lib.EvpError("frame_augment_batch: frames must be a contiguous float32 tensor in device memory")
    B, C, H, W = frames.shape
    if not torch.is_tensor(params):
        p = np.ascontiguousarray(params, dtype=np.int32).reshape(B, 6)
        if ((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 2] < 1) | (p[:, 3] < 1) | (p[:, 0] + p[:, 2] > W) | (p[:, 1] + p[:, 3] > H)).any():
            raise ValueError("frame_augment_batch: crop box outside the frame")
        params = torch.from_numpy(p).to(frames.device, non_blocking=True)
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 6) or not params.is_contiguous():
        raise ValueError("frame_augment_batch: params must be int32 [B,6]")
    Ho, Wo = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty(B, C, Ho, Wo, dtype=torch.float32, device=frames.device)
    call("evp_frame_augment_f32", ptr(frames), ptr(params), ptr(out), B, C, H, W, Ho, Wo, stream_ptr())
    return out


def _label_rows(who, params, B, H, W, device):
    """The label wrappers' share of evg_augment_batch's params handling: host rows are range-checked and uploaded, device rows taken as they are."""
    if not torch.is_tensor(params):
        p = np.ascontiguousarray(params, dtype=np.int32).reshape(B, 6)
        if ((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 2] < 1) | (p[:, 3] < 1) | (p[:, 0] + p[:, 2] > W) | (p[:, 1] + p[:, 3] > H)).any():
            raise ValueError(f"{who}: crop box outside the view")
        params = torch.from_numpy(p).to(device, non_blocking=True)
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 6) or not params.is_contiguous() or not params.is_cuda:
        raise ValueError(f"{who}: params must be int32 [B,6]")
    return params


def _label_out(who, out, shape, dtype, device):
    if out is None:
        return torch.empty(*shape, dtype=dtype, device=device)
    if tuple(out.shape) != shape or out.dtype != dtype or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous {dtype} tensor of shape {shape} in device memory")
    return out


def semseg_label_augment_batch(labels, params, size, out=None):
    """Segmentation labels of the batch (reference view_augment.py:91-99 `semseg_label_augment`): labels uint8 [B,1,H,W] on the GPU,
    params int32 [B,6] (host array or device tensor) -- THE SAME rows that went to evg_augment_batch (the reference re-seeds numpy with the
    sample's seed, so the crop box and the flip coin repeat; column 5, the time flip, does not touch a label) -> int64
    [B,1,size[0],size[1]]: crop, nearest resize, horizontal flip; equal to the reference's function (tests/golden/dense_label_views.npz)."""
    who = "semseg_label_augment_batch"
    _lib.require_device()
    if not labels.is_cuda or labels.dtype != torch.uint8 or labels.dim() != 4 or labels.shape[1] != 1 or not labels.is_contiguous():
        raise _lib.EvpError(f"{who}: labels must be a contiguous uint8 [B,1,H,W] tensor in device memory")
    B, _, H, W = labels.shape
    params = _label_rows(who, params, B, H, W, labels.device)
    Ho, Wo = int(size[0]), int(size[1])
    out = _label_out(who, out, (B, 1, Ho, Wo), torch.int64, labels.device)
    call("evp_semseg_label_augment", ptr(labels), ptr(params), ptr(out), B, H, W, Ho, Wo, stream_ptr())
    return out


def flow_label_augment_batch(flow, params, size, out=None, valid_out=None):
    """Flow labels of the batch and their valid mask in one pass (reference view_augment.py:101-134 `flow_label_augment` with evg_augment's
    time-flip flag, `flow_label_valid_augment` of the dataset's `norm > 0 & |flow| < 1000` mask): flow float32 [B,2,H,W] on the GPU, params
    int32 [B,6] as semseg_label_augment_batch takes them (column 5 = the time-flip flag: both components change sign) -> (float32
    [B,2,size[0],size[1]] scaled by (size[1] / w, size[0] / h) of the crop box, float32 [B,1,size[0],size[1]] of 1.0 / 0.0); equal to the
    reference's functions (tests/golden/dense_label_views.npz)."""
    who = "flow_label_augment_batch"
    _lib.require_device()
    if not flow.is_cuda or flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[1] != 2 or not flow.is_contiguous():
        raise _lib.EvpError(f"{who}: flow must be a contiguous float32 [B,2,H,W] tensor in device memory")
    B, _, H, W = flow.shape
    params = _label_rows(who, params, B, H, W, flow.device)
    Ho, Wo = int(size[0]), int(size[1])
    out = _label_out(who, out, (B, 2, Ho, Wo), torch.float32, flow.device)
    valid_out = _label_out(who, valid_out, (B, 1, Ho, Wo), torch.float32, flow.device)
    call("evp_flow_label_augment_f32", ptr(flow), ptr(params), ptr(out), ptr(valid_out), B, H, W, Ho, Wo, stream_ptr())
    return out, valid_out

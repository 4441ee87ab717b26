"""Event stream -> event-count image on the GPU (csrc/evimage.hip), the 2- and 3-channel representations of the reference's
classification fine-tuning datasets (reference dataset/dataset_utils/events_to_image.py:6-75 as dataset/finetune_cls/* call it):

    num_bins == 2   events_to_image_ecdp: {count of p == 1, count of p == 0 (or of p == -1 where the clip has no p == 0 row)} as floats
    num_bins == 3   events_to_image_mem, / 255, remove_hot_pixel_mem: {pos / 255, 0, neg / 255} with the hot pixels of both planes zeroed

`event_image_batch` is the batched device-resident entry point the loader chain uses (two launches and the clears for a whole batch of
clips); `event_image_normalize_` is the datasets' tail after the view stage. The reference's function names are thin single-clip forms
with its signatures. Every count is an integer sum, so results repeat bit for bit from launch to launch."""
import numpy as np
import torch

from ... import _lib
from ..._lib import call, ptr, stream_ptr


def event_image_batch(events, clip_offsets, num_bins, size, scale=None, out=None, status=None, max_rows_per_clip=None):
    """events: float64 CUDA tensor [n_total,4] (x,y,t,p); clip_offsets: int64 CUDA tensor [n_clips+1] -> float32 [n_clips,num_bins,H,W],
    the raw images of evp_event_image_count + evp_event_image_finish (include/evtpretrain.h K30). scale=(sx, sy): the sensor -> input
    rescale (reference events_augment.py:22-26) applied to x and y in float64 before the truncation, as rescaling the array first.
    A row whose linear index trunc(x) + trunc(y) * W leaves [0, H * W) is where the reference raises: it is left out and counted in
    `status` (int32 [1] on the device, accumulated; the caller reads it when it likes). With status=None the count is read back here and
    a ValueError raised (one synchronisation: not for a captured chain). `max_rows_per_clip` sizes the launch grid (default: all rows)."""
    _lib.require_device()
    if int(num_bins) not in (2, 3):
        raise ValueError(f"event_image_batch: num_bins must be 2 or 3 (got {num_bins}); voxel grids are voxel_grid_batch's")
    if events.dtype != torch.float64 or events.dim() != 2 or events.shape[1] != 4 or not events.is_contiguous():
        raise _lib.EvpError("events must be a contiguous float64 [N,4] tensor")
    if clip_offsets.dtype != torch.int64:
        raise _lib.EvpError("clip_offsets must be int64")
    H, W, C = int(size[0]), int(size[1]), int(num_bins)
    n_clips = clip_offsets.numel() - 1
    dev = events.device
    if out is None:
        out = torch.empty(n_clips, C, H, W, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n_clips, C, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"event_image_batch: out must be a contiguous float32 tensor of shape {(n_clips, C, H, W)}")
    check = status is None
    if check:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_total = int(events.shape[0])
    work = torch.empty(n_clips * (3 * H * W + 1), dtype=torch.int32, device=dev)      # the three planes of every clip | the p == 0 counts
    planes, zero_rows = work[:n_clips * 3 * H * W], work[n_clips * 3 * H * W:]
    sx, sy = (1.0, 1.0) if scale is None else (float(scale[0]), float(scale[1]))
    call("evp_event_image_count", ptr(events), n_total, ptr(clip_offsets), n_clips, n_total if max_rows_per_clip is None else int(max_rows_per_clip),
         H, W, sx, sy, ptr(planes), ptr(zero_rows), ptr(status), stream_ptr())
    call("evp_event_image_finish", ptr(planes), ptr(zero_rows), n_clips, C, H, W, ptr(out), stream_ptr())
    if check:
        bad = int(status.item())
        if bad:
            raise ValueError(f"event_image_batch: {bad} row(s) fall outside the {H} x {W} grid (the reference's bincount / reshape raises there)")
    return out


def event_image_normalize_(views, guard=False, status=None):
    """The datasets' tail on the views float32 [B,C,S,S] (C = 2 or 3), in place (evp_event_image_normalize): C = 2 per channel
    ((v / (max + 1)) - 0.5) * 2; C = 3 planes 0 and 2 times 1.0 / their common max. `guard`: the `factor = 1.0 / 0.001` of the datasets
    that have it for an all-zero view; without it such a view becomes NaN, as in the reference. `status` (int32 [1], device, accumulated)
    counts the all-zero 3-channel views."""
    _lib.require_device()
    if not views.is_cuda or views.dtype != torch.float32 or views.dim() != 4 or not views.is_contiguous() or views.shape[1] not in (2, 3):
        raise _lib.EvpError("event_image_normalize_: views must be a contiguous float32 [B,2|3,H,W] tensor in device memory")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=views.device)
    B, C, H, W = views.shape
    call("evp_event_image_normalize", ptr(views), B, C, H, W, int(bool(guard)), ptr(status), stream_ptr())
    return views


def _single(events, size, is_txyp, num_bins):
    ev = np.ascontiguousarray(events, dtype=np.float64)
    if ev.ndim != 2 or ev.shape[1] != 4:
        raise AssertionError("events must be [N,4]")
    if is_txyp:
        ev = np.ascontiguousarray(ev[:, [1, 2, 0, 3]])
    dev = torch.device("cuda", torch.cuda.current_device())
    off = torch.tensor([0, ev.shape[0]], dtype=torch.int64, device=dev)
    return event_image_batch(torch.from_numpy(ev).to(dev), off, num_bins, size)[0]


def events_to_image_ecdp(args, events, size, is_txyp=False):
    """Drop-in for the reference function: numpy float64 [N,4] (x,y,t,p) or (t,x,y,p) -> float32 [2,H,W] in device memory."""
    _lib.require_device()
    return _single(events, size, is_txyp, 2)


def events_to_image_mem(args, events, size, is_txyp=False):
    """Drop-in for the reference function: -> float32 [3,H,W] in device memory, {pos, 0, neg} counts as floats (the caller divides by 255
    and calls remove_hot_pixel_mem, as the datasets do; event_image_batch(..., num_bins=3) does all three at once)."""
    _lib.require_device()
    two = _single(events, size, is_txyp, 2)
    out = torch.zeros(3, int(size[0]), int(size[1]), dtype=torch.float32, device=two.device)
    out[0::2] = two
    return out


def remove_hot_pixel_mem(hist, num_stds=10):
    """Drop-in for the reference function on what the datasets hand it: hist float32 [3,H,W] in device memory whose planes 0 and 2 hold
    k / 255 for integer counts k. The statistics are taken on the integers (include/evtpretrain.h K30), so any other content is refused."""
    _lib.require_device()
    if num_stds != 10:
        raise NotImplementedError("remove_hot_pixel_mem: the kernel's threshold is mean + 10 std, the only value the reference's datasets use")
    if not hist.is_cuda or hist.dtype != torch.float32 or hist.dim() != 3 or hist.shape[0] != 3:
        raise _lib.EvpError("remove_hot_pixel_mem: hist must be a float32 [3,H,W] tensor in device memory")
    k = torch.round(hist[0::2] * 255.0)
    if not torch.equal(k / 255, hist[0::2]) or bool((k < 0).any()) or bool((k >= 2 ** 31).any()):
        raise ValueError("remove_hot_pixel_mem: planes 0 and 2 must hold counts / 255 (events_to_image_mem(...) / 255)")
    _, H, W = hist.shape
    planes = torch.zeros(3, H, W, dtype=torch.int32, device=hist.device)
    planes[0], planes[2] = k[0].to(torch.int32), k[1].to(torch.int32)
    zero_rows = torch.zeros(1, dtype=torch.int32, device=hist.device)              # (the p == -1 plane carries the negatives here)
    out = torch.empty(1, 3, H, W, dtype=torch.float32, device=hist.device)
    call("evp_event_image_finish", ptr(planes), ptr(zero_rows), 1, 3, H, W, ptr(out), stream_ptr())
    hist.copy_(out[0])
    return hist

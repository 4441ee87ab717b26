"""MVSEC's flow label from resident ground-truth flow frames: the host half of what the reference's FinetuneMVSECSeqDataset does per
sample between its h5py reads and flow_label_augment (dataset/finetune_flow/ft_mvsec_dataset.py:264-272 and gen_correspond_gt_flow,
:121-188). The 20 Hz flow frames are not synchronised with the grayscale frames, so the reference propagates a pixel grid through the
frames between the two image timestamps with cv2.remap(..., INTER_NEAREST). Here a sequence's frames are uploaded once, a sample's label
costs the two timestamps: `mvsec_flow_hops` turns them into a short table of (frame, float64 scale) hops in numpy, and
evp_mvsec_flow_propagate (include/evtpretrain.h K29, csrc/labels.hip) walks every output pixel through them on the GPU.

    frames, scales, n = mvsec_flow_hops(flow_ts, image1_ts, image2_ts)            # per sample, float64
    label = mvsec_flow_propagate_batch(d_frames, d_hop_frame, d_hop_scale, d_n_hops, out, status)

GpuDenseLoader(task="flow", gt_flow=...) does both per batch. The nearest rule of cv2.remap (cvRound: half to even) is stated from
OpenCV's source and has not been checked against a real cv2: see the header."""
import numpy as np
import torch

from ..._lib import EVP_F32, EVP_F64, EvpError, call, ptr, require_device, stream_ptr

MAX_HOPS = 8                       # rows of a sample's hop table: args.skip_num = 4 at 45 Hz spans 2-3 frames of 20 Hz, i.e. 2-3 hops


def mvsec_flow_hops(flow_ts, image1_ts, image2_ts, max_hops=MAX_HOPS, name=None):
    """The reference's schedule for one sample, in float64. flow_ts: the sequence's flow_dist_ts (float64 [N], ascending); image1_ts,
    image2_ts: the sample's two image timestamps. -> (frames int64 [max_hops], scales float64 [max_hops], n_hops), frame indices into the
    sequence, rows past the used ones zero:
      n_hops == 0   the direct branch (image1_ts > ts[left] and image2_ts <= ts[left + 1]): label = frame frames[0] * scales[0];
      n_hops >= 2   hops (left, (ts[left+1] - t1) / (ts[left+1] - ts[left])), (left + i, 1.0) for the frames strictly between,
                    (right - 1, (t2 - ts[right-1]) / (ts[right] - ts[right-1])); with one frame (t1 == ts[left]) both go through it.
    left = searchsorted(ts, t1, 'right') - 1 and right = searchsorted(ts, t2, 'right') as the reference takes them; what it asserts
    (and what it would index out of range) is a ValueError naming the sample, and so is a schedule of more than max_hops rows."""
    ts = np.asarray(flow_ts)
    if ts.dtype != np.float64 or ts.ndim != 1 or ts.shape[0] < 2:
        raise ValueError(f"mvsec_flow_hops: flow_ts must be float64 [N >= 2] (got {ts.dtype} {list(ts.shape)})")
    who = f"mvsec_flow_hops: sample {name!r}" if name is not None else "mvsec_flow_hops: the sample"
    t1, t2 = np.float64(image1_ts), np.float64(image2_ts)
    n = int(ts.shape[0])
    left = int(np.searchsorted(ts, t1, side="right")) - 1
    right = int(np.searchsorted(ts, t2, side="right"))
    if left < 0:
        raise ValueError(f"{who} starts at {float(t1)!r}, before the sequence's first flow frame ({float(ts[0])!r})")
    if not (left < n and right < n):            # (the reference: flow_left_index < flow_length, flow_right_index < flow_length)
        raise ValueError(f"{who} ends at {float(t2)!r}, at or after the sequence's last flow frame ({float(ts[-1])!r})")
    F = right - left
    if F < 1:                                   # (flow_left_index <= flow_right_index; an empty slice has no frame 0 to read)
        raise ValueError(f"{who} ends ({float(t2)!r}) before it starts ({float(t1)!r}): no flow frame lies between")
    if max_hops < 1:
        raise ValueError(f"mvsec_flow_hops: max_hops = {max_hops}")
    frames, scales = np.zeros(int(max_hops), np.int64), np.zeros(int(max_hops), np.float64)
    if t1 > ts[left] and t2 <= ts[left + 1]:
        frames[0], scales[0] = left, (t2 - t1) / (ts[left + 1] - ts[left])
        return frames, scales, 0
    n_hops = max(F, 2)
    if n_hops > max_hops:
        raise ValueError(f"{who} spans {F} flow frames = {n_hops} hops, more than max_hops = {max_hops}: raise the capacity")
    frames[:n_hops] = [left] + [left + i for i in range(1, F - 1)] + [right - 1]
    scales[:n_hops] = 1.0
    scales[0] = (ts[left + 1] - t1) / (ts[left + 1] - ts[left])
    scales[n_hops - 1] = (t2 - ts[right - 1]) / (ts[right] - ts[right - 1])
    return frames, scales, n_hops


def mvsec_flow_propagate_batch(frames, hop_frame, hop_scale, n_hops, out, status):
    """evp_mvsec_flow_propagate on device tensors: frames float32 | float64 [N,2,H,W] (every sequence back to back), hop_frame int64
    [B,max_hops] (ABSOLUTE frame indices), hop_scale float64 [B,max_hops], n_hops int32 [B] -> out float32 [B,2,H,W]; status int32 [1]
    accumulates the samples whose table names no frame (skipped: their rows of `out` stay as they were). -> out."""
    require_device()
    who = "mvsec_flow_propagate_batch"
    if not frames.is_cuda or frames.dtype not in (torch.float32, torch.float64) or frames.dim() != 4 or frames.shape[1] != 2 or not frames.is_contiguous():
        raise EvpError(f"{who}: frames must be a contiguous float32 or float64 [N,2,H,W] tensor in device memory")
    N, _, H, W = (int(v) for v in frames.shape)
    for t, dtype, what in ((hop_frame, torch.int64, "hop_frame"), (hop_scale, torch.float64, "hop_scale"), (n_hops, torch.int32, "n_hops"),
                           (out, torch.float32, "out"), (status, torch.int32, "status")):
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise EvpError(f"{who}: {what} must be a contiguous {dtype} tensor in device memory")
    B = int(n_hops.numel())
    if hop_frame.dim() != 2 or hop_frame.shape[0] != B or tuple(hop_scale.shape) != tuple(hop_frame.shape) or hop_frame.shape[1] < 1:
        raise EvpError(f"{who}: hop_frame and hop_scale must be [B,max_hops] with B = n_hops' {B} (got {list(hop_frame.shape)}, {list(hop_scale.shape)})")
    if tuple(out.shape) != (B, 2, H, W) or status.numel() != 1:
        raise EvpError(f"{who}: out must be [{B},2,{H},{W}] (got {list(out.shape)}), status [1]")
    call("evp_mvsec_flow_propagate", ptr(frames), EVP_F64 if frames.dtype == torch.float64 else EVP_F32, N, H, W, ptr(hop_frame),
         ptr(hop_scale), ptr(n_hops), B, int(hop_frame.shape[1]), ptr(out), ptr(status), stream_ptr())
    return out

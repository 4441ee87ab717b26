"""A loader for the dense fine-tuning loops (semantic segmentation on DSEC / DDD17, optical flow on MVSEC) that starts from RAW EVENT
CLIPS with their label maps: what the reference's dense Dataset.__getitem__ does per sample on a DataLoader worker
(dataset/finetune_semseg/ft_dsec_dataset.py:192-290, ft_ddd17_dataset.py:111-190, dataset/finetune_flow/ft_mvsec_dataset.py:190-315)
happens here per BATCH on the GPU, with the pack / upload machinery of dataset.pretrain.gpu_event_loader and the chain of
dataset.finetune_cls.gpu_event_loader.GpuFinetuneLoader's grid="sensor" recipe in bilinear mode:

    tail window -> [DSEC: rectify through the map, keep what lands in the sensor | DDD17: crop mask, then the tail] ->
    [train: erase / add] -> voxel grid at the sensor's (H, W) -> [train: evg_augment | val: view_resize] to S x S, bilinear ->
    the LABEL under the same crop box and flip coins, nearest, back at (H, W)

    samples = iterable of (events float64 [n,4] (x,y,t,p) time-sorted numpy array, label, seq_name)
              task="semseg": label uint8 [H,W];  task="flow": label float32 [2,H,W], what the reader's gen_correspond_gt_flow returns --
              or, with gt_flow={seq_name: (flow_dist frames, flow_dist_ts)}, the pair (image1_ts, image2_ts): the label is then made here
    recipe  = dense_recipe(args)                            # args.dataset_type in {"dsec", "ddd17", "mvsec"}
    train   = GpuDenseLoader(args, samples, 64, len(dataset) // 64, True, seed=args.seed, rectify_map=map_or_None, **recipe)
    ft_semseg_train_one_epoch(args, model, train, optimizer, epoch, loss_scaler);  ft_semseg_val(args, model, val, epoch)

What differs from the classification loader:
  * the window is the clip's TAIL (the last fix_events_num rows; for MVSEC every row between the two frames, `max_events` being the
    capacity), not get_random_index's random start: `_window_start`;
  * with `rectify_map` (DSEC, float32 [org_h, org_w, 2]) or `raw_rows` (DDD17) the uploaded rows go through
    evp_events_rectify_compact_f64 on the consumer's stream into the chain's event buffer and offsets before the replay: DSEC uploads
    the tail of fix rows and keeps the rows whose rectified coordinates land in the sensor (the reference cuts before it rectifies);
    DDD17 uploads the tail of `raw_rows` rows, masks them to the sensor and keeps the last fix survivors (the reference masks first and
    cuts second -- over the whole clip; `raw_rows` bounds how far back the mask looks, and a clip that loses more than raw_rows - fix
    rows of its tail to the mask comes out shorter than the reference's);
  * labels travel with the windows (pinned slot -> one device tensor) and are augmented by evp_semseg_label_augment /
    evp_flow_label_augment_f32 under `chain.crop_rows`, the rows the chain's plan kernel drew for the grids on the device (the reference
    re-seeds numpy with the sample's seed before each of evg_augment, semseg_label_augment, flow_label_augment and
    flow_label_valid_augment); the flow kernel makes the valid mask (norm > 0 and |flow| < 1000) on the way, so no third plane travels;
  * with `gt_flow` (MVSEC) no flow label travels either: every sequence's ground-truth flow frames are uploaded once at construction, a
    sample carries its two image timestamps, the pack turns them into a row of hops (mvsec_flow.mvsec_flow_hops, float64 numpy) and
    evp_mvsec_flow_propagate fills the label buffer from the resident frames in front of the label view -- gen_correspond_gt_flow's
    propagation (ft_mvsec_dataset.py:121-188), whose cv2.remap nearest rule (half to even) is stated from OpenCV's source, unchecked
    against a real cv2 (include/evtpretrain.h K29).
Train: float32 cells. Clean validation: K1 with float64 cells (algo 3) + the bilinear view under the full box, the label kernel under the
full-box rows (it only widens / makes the mask): a pass repeats bit for bit.

Yields static device tensors the next batch overwrites:
  task="semseg": {"events_voxel_grid" float32 [B,bins,S,S], "semseg_label" int64 [B,1,H,W], "seq_name"}
  task="flow":   misc.FLOW_BATCH_KEYS: "events_voxel_grid", "events_voxel_grid_org", "flow_label" float32 [B,2,H,W], "flow_label_valid"
                 float32 [B,1,H,W], "seq_name". In validation events_voxel_grid_org IS the raw sensor-size grid K1 wrote (no copy); in
                 training it is yielded with org_view=True only (one more bilinear view of the raw grids under the same rows to (H, W), what
                 the reference makes for its visualiser; the trainer drops the key).

Windows are checked on the host before upload (empty; without a compaction, coordinates outside the sensor; with a map, coordinates
outside the map: ValueError naming the clip); the device's status words (clips without a survivor, rows outside the map) are read once
at the end of a pass and raise ValueError when non-zero. With gt_flow a timestamp outside its sequence's flow frames, an unknown
sequence name and a sample of more than `max_hops` hops are ValueErrors of the pack.

Out of scope (NotImplementedError): the 2- and 3-bin representations, EvRepSL, and args.val_event_noise -- the reference's dense noisy
validation clips the added rows to N-Caltech101's cal_sensor_h / cal_sensor_w (ft_dsec_dataset.py:233, ft_mvsec_dataset.py:214), which
looks like an oversight and is not reproduced. The file readers (h5py, PIL) stay with the caller."""
import numpy as np
import torch

from ..._lib import EvpError, call, ptr, require_device, stream_ptr
from ..augmentation.view_augment import evg_augment_batch, flow_label_augment_batch, semseg_label_augment_batch
from ..dataset_utils.events_to_voxel_grid import voxel_grid_batch
from ..pretrain.gpu_event_loader import ClipWindowLoader
from ..pretrain.gpu_input_pipeline import GpuInputPipeline
from .mvsec_flow import MAX_HOPS, mvsec_flow_hops, mvsec_flow_propagate_batch

DDD17_MASK_MARGIN = 10000          # rows of tail the DDD17 recipe uploads beyond the window, for the crop mask to eat into
MVSEC_MAX_EVENTS = 200_000         # capacity of an MVSEC sample where the namespace has no max_events


def dense_recipe(args):
    """-> GpuDenseLoader's recipe keywords for args.dataset_type, read from the reference's own argument names for that dataset:
    task, sensor=(h, w), org_sensor=(h, w) | None, rectify (the caller must pass the dataset's rectify_map), raw_rows (rows of tail
    uploaded per clip where that is more than the window) and, for MVSEC, max_events. The loader never calls this on its own."""
    kind = args.dataset_type
    if kind == "dsec":
        return dict(task="semseg", sensor=(int(args.dsec_sensor_h), int(args.dsec_sensor_w)),
                    org_sensor=(int(args.dsec_org_sensor_h), int(args.dsec_org_sensor_w)), rectify=True, raw_rows=None)
    if kind == "ddd17":
        fix = max(int(args.fix_events_num), int(getattr(args, "val_fix_events_num", args.fix_events_num)))
        return dict(task="semseg", sensor=(int(args.ddd17_sensor_h), int(args.ddd17_sensor_w)), org_sensor=None, rectify=False,
                    raw_rows=fix + DDD17_MASK_MARGIN)
    if kind == "mvsec":
        return dict(task="flow", sensor=(int(args.mvsec_sensor_h), int(args.mvsec_sensor_w)), org_sensor=None, rectify=False, raw_rows=None,
                    max_events=int(getattr(args, "max_events", MVSEC_MAX_EVENTS)))
    raise ValueError(f"dense_recipe: unknown dataset_type {kind!r} (one of ['ddd17', 'dsec', 'mvsec'])")


def rectify_compact_batch(events, clip_offsets, max_rows_per_clip, keep_last, extent, out, offsets_out, status, rectify_map=None,
                          workspace=None):
    """evp_events_rectify_compact_f64 on device tensors: events float64 [n,4], clip_offsets int64 [B+1], `extent` = the kept (H, W),
    rectify_map float32 [org_h, org_w, 2] or None (the plain crop mask) -> the survivors' last `keep_last` rows per clip in `out`
    (float64 [.,4], at least min(n, B * keep_last) rows), their offsets in `offsets_out` (int64 [B+1]); `status` int32 [2] accumulates
    (clips without a survivor, rows outside the map). -> offsets_out."""
    require_device()
    B = clip_offsets.numel() - 1
    for t, dtype, who in ((events, torch.float64, "events"), (out, torch.float64, "out"), (clip_offsets, torch.int64, "clip_offsets"),
                          (offsets_out, torch.int64, "offsets_out"), (status, torch.int32, "status")):
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise EvpError(f"rectify_compact_batch: {who} must be a contiguous {dtype} tensor in device memory")
    if events.dim() != 2 or events.shape[1] != 4 or out.dim() != 2 or out.shape[1] != 4 or offsets_out.numel() != B + 1 or status.numel() != 2:
        raise EvpError("rectify_compact_batch: events / out must be [.,4], offsets_out [B+1], status [2]")
    if out.shape[0] < min(int(events.shape[0]), B * int(keep_last)):
        raise EvpError(f"rectify_compact_batch: out holds {out.shape[0]} rows, the survivors may need {min(int(events.shape[0]), B * int(keep_last))}")
    mh = mw = 0
    if rectify_map is not None:
        if not rectify_map.is_cuda or rectify_map.dtype != torch.float32 or rectify_map.dim() != 3 or rectify_map.shape[2] != 2 or not rectify_map.is_contiguous():
            raise EvpError("rectify_compact_batch: rectify_map must be a contiguous float32 [org_h, org_w, 2] tensor in device memory")
        mh, mw = int(rectify_map.shape[0]), int(rectify_map.shape[1])
    words = call("evp_events_rectify_compact_ws_words", B, int(max_rows_per_clip))
    if workspace is None:
        workspace = torch.empty(words, dtype=torch.int32, device=events.device)
    elif workspace.dtype != torch.int32 or workspace.numel() < words or not workspace.is_cuda:
        raise EvpError(f"rectify_compact_batch: workspace must be int32 [{words}] in device memory")
    call("evp_events_rectify_compact_f64", ptr(events), int(events.shape[0]), ptr(clip_offsets), B, int(max_rows_per_clip), ptr(rectify_map), mh, mw,
         int(extent[0]), int(extent[1]), int(keep_last), ptr(out), int(out.shape[0]), ptr(offsets_out), ptr(status), ptr(workspace), stream_ptr())
    return offsets_out


class _CheckedSamples:
    """The caller's samples with MVSEC's capacity check in front of the pack (which only ever sees a window)."""

    def __init__(self, samples, max_events):
        self.samples, self.max_events = samples, max_events

    def __iter__(self):
        for events, label, name in self.samples:
            if events.shape[0] > self.max_events:
                raise ValueError(f"GpuDenseLoader: sample {name!r} holds {events.shape[0]} events, more than max_events = {self.max_events} "
                                 "(a flow sample is every row between its two frames: raise the capacity)")
            yield events, label, name


class _GtFlowSamples:
    """(events, (image1_ts, image2_ts), seq_name) -> (events, the sample's hop row, seq_name): the schedule is made where the sample is
    drawn (the pack's worker thread), with the sequence's base index added to its frame indices."""

    def __init__(self, samples, flow_ts, base, max_hops):
        self.samples, self.flow_ts, self.base, self.max_hops = samples, flow_ts, base, max_hops

    def __iter__(self):
        for events, stamps, name in self.samples:
            if name not in self.flow_ts:
                raise ValueError(f"GpuDenseLoader: sample of sequence {name!r}, gt_flow holds {sorted(self.flow_ts)}")
            if np.shape(stamps) != (2,):
                raise ValueError(f"GpuDenseLoader: with gt_flow a sample of {name!r} carries (image1_ts, image2_ts) in the label's place")
            frames, scales, n_hops = mvsec_flow_hops(self.flow_ts[name], stamps[0], stamps[1], self.max_hops, name=name)
            frames[:max(n_hops, 1)] += self.base[name]
            yield events, (frames, scales, n_hops), name


class GpuDenseLoader(ClipWindowLoader):
    def __init__(self, args, samples, batch_size, n_batches, is_train, task, sensor, seed=0, first_sample=0, step0=0, rectify_map=None,
                 org_sensor=None, raw_rows=None, max_events=None, rectify=None, org_view=False, gt_flow=None, max_hops=MAX_HOPS):
        """`samples`: a re-iterable (one pass per epoch) of (events, label, seq_name); `n_batches`: batches per pass (a short last batch is
        dropped). `task`: "semseg" | "flow". `sensor`: the (H, W) the grids are binned at and the labels have. `step0`: the counter
        stream's step of the first batch (a training loader continues across epochs, a validation loader restarts there).
        `rectify_map` (float32 [org_h, org_w, 2], numpy or tensor) with `org_sensor` = its (org_h, org_w): DSEC's rectification;
        `raw_rows`: rows of tail uploaded per clip for the crop mask (DDD17); `max_events`: the window's capacity in place of
        args.fix_events_num / val_fix_events_num (MVSEC, which has no fixed count: a longer sample raises ValueError). `rectify`: what
        dense_recipe says about the map (True needs rectify_map). `org_view`: yield events_voxel_grid_org in training (flow).
        `gt_flow` (task="flow"): {seq_name: (frames float32 | float64 [F,2,H,W], flow_ts float64 [F])}, a sequence's flow_dist and
        flow_dist_ts whole -- uploaded once; a sample is then (events, (image1_ts, image2_ts), seq_name) and may span `max_hops` hops."""
        if task not in ("semseg", "flow"):
            raise ValueError(f"GpuDenseLoader: task must be 'semseg' or 'flow' (got {task!r})")
        if int(args.num_bins) in (2, 3):
            raise NotImplementedError("GpuDenseLoader: the 2- and 3-bin event representations are out of scope (voxel grids only)")
        if getattr(args, "use_evrepsl", False):
            raise NotImplementedError("GpuDenseLoader: EvRepSL preprocessing is out of scope")
        if not is_train and getattr(args, "val_event_noise", False):
            raise NotImplementedError("GpuDenseLoader: val_event_noise is out of scope for the dense datasets: the reference clips the added rows of "
                                      "its dense noisy validation to N-Caltech101's cal_sensor_h / cal_sensor_w, which looks like an oversight")
        if rectify and rectify_map is None:
            raise ValueError("GpuDenseLoader: this recipe rectifies its events (rectify=True): pass the dataset's rectify_map")
        self.task, self.is_train, self.step0, self.org_view = task, bool(is_train), int(step0), bool(org_view)
        H, W = self.sensor = (int(sensor[0]), int(sensor[1]))
        self._gt_host, self.max_hops = None, int(max_hops)
        if gt_flow is not None:
            samples = self._gt_flow_checked(gt_flow, samples)
        fix = int(max_events) if max_events is not None else int(args.fix_events_num if self.is_train else args.val_fix_events_num)
        self.keep = fix
        self.compact = rectify_map is not None or raw_rows is not None
        raw = max(int(raw_rows), fix) if raw_rows is not None else fix
        pipe = GpuInputPipeline(args, seed=seed, resize_mode="bilinear", grid="sensor", sensor=self.sensor, fix_events_num=fix,
                                view_augment=self.is_train, voxel_cells="f32" if self.is_train else "f64")
        if max_events is not None:
            samples = _CheckedSamples(samples, int(max_events))
        self._setup(args, samples, batch_size, n_batches, seed, first_sample, step0, raw, raw)      # (the pack's window: the tail of `raw` rows)
        B, dev = self.B, self.dev
        self.S, self.bins, self.pipe = int(args.input_size), int(args.num_bins), pipe
        self.map = self.org_sensor = None
        if rectify_map is not None:
            m = rectify_map if torch.is_tensor(rectify_map) else torch.from_numpy(np.ascontiguousarray(rectify_map, dtype=np.float32))
            if m.dtype != torch.float32 or m.dim() != 3 or m.shape[2] != 2:
                raise ValueError("GpuDenseLoader: rectify_map must be float32 [org_h, org_w, 2]")
            if org_sensor is not None and tuple(m.shape[:2]) != (int(org_sensor[0]), int(org_sensor[1])):
                raise ValueError(f"GpuDenseLoader: rectify_map is {tuple(m.shape[:2])}, org_sensor says {tuple(org_sensor)}")
            self.map = m.to(dev).contiguous()
            self.org_sensor = (int(m.shape[0]), int(m.shape[1]))
        # the buffer the grids are binned from: the uploaded windows themselves, or what the compaction leaves of them
        self.cev = torch.zeros(B * fix, 4, dtype=torch.float64, device=dev) if self.compact else self.ev
        self.status = torch.zeros(2, dtype=torch.int32, device=dev) if self.compact else None
        self._ws = (torch.zeros(call("evp_events_rectify_compact_ws_words", B, raw), dtype=torch.int32, device=dev) if self.compact else None)
        self.chain = self.raw = self._full = None
        if self.is_train:
            self.chain = pipe.capture(self.cev, B, clip_offsets=np.zeros(B + 1, np.int64))
            self.c_off, self.raw = self.chain.d_off, self.chain.raw
            self.org = torch.zeros(B, self.bins, H, W, dtype=torch.float32, device=dev) if self.org_view else None
        else:
            self.c_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            self.raw = torch.zeros(B, self.bins, H, W, dtype=torch.float32, device=dev)
            self.out = self.raw if (H, W) == (self.S, self.S) else torch.zeros(B, self.bins, self.S, self.S, dtype=torch.float32, device=dev)
            self._full = pipe.full_rows(B, dev)
        if not self.compact:
            self.d_off = self.c_off           # the uploaded offsets are the chain's (K1's)
        if task == "semseg":
            self.label = torch.zeros(B, 1, H, W, dtype=torch.int64, device=dev)
        else:
            self.label = torch.zeros(B, 2, H, W, dtype=torch.float32, device=dev)
            self.valid = torch.zeros(B, 1, H, W, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------------------------------------ host half
    def _window_start(self, n, fix, w0):
        return max(n - fix, 0)            # the tail (ft_dsec_dataset.py:202-209, ft_ddd17_dataset.py:126-127); MVSEC: fix is the capacity

    def _gt_flow_checked(self, gt_flow, samples):
        """The sequences' frames as one host array (uploaded in _alloc_extra) + the samples wrapped so that a hop row travels."""
        if self.task != "flow":
            raise ValueError("GpuDenseLoader: gt_flow (MVSEC's ground-truth flow frames) goes with task='flow'")
        if not gt_flow:
            raise ValueError("GpuDenseLoader: gt_flow holds no sequence")
        if self.max_hops < 2:
            raise ValueError(f"GpuDenseLoader: max_hops = {self.max_hops} (a propagated label takes at least 2 hops)")
        parts, flow_ts, base, n = [], {}, {}, 0
        for name, (frames, ts) in gt_flow.items():
            f = frames.numpy() if torch.is_tensor(frames) else np.asarray(frames)
            ts = np.ascontiguousarray(ts.numpy() if torch.is_tensor(ts) else ts)
            if f.dtype not in (np.float32, np.float64) or f.ndim != 4 or f.shape[1] != 2 or tuple(f.shape[2:]) != self.sensor:
                raise ValueError(f"GpuDenseLoader: gt_flow[{name!r}] frames must be float32 or float64 [F,2,{self.sensor[0]},{self.sensor[1]}] "
                                 f"(got {f.dtype} {list(f.shape)})")
            if parts and f.dtype != parts[0].dtype:
                raise ValueError(f"GpuDenseLoader: gt_flow[{name!r}] frames are {f.dtype}, the sequences before it {parts[0].dtype}: one dtype for all")
            if ts.dtype != np.float64 or ts.shape != (f.shape[0],) or f.shape[0] < 2:
                raise ValueError(f"GpuDenseLoader: gt_flow[{name!r}] flow_ts must be float64 [{f.shape[0]}], one per frame, at least two "
                                 f"(got {ts.dtype} {list(ts.shape)})")
            parts.append(f), flow_ts.update({name: ts}), base.update({name: n})
            n += int(f.shape[0])
        self._gt_host, self.gt_base = parts, base
        return _GtFlowSamples(samples, flow_ts, base, self.max_hops)

    def _alloc_extra(self):
        H, W = self.sensor
        shape, dtype = ((self.B, 1, H, W), torch.uint8) if self.task == "semseg" else ((self.B, 2, H, W), torch.float32)
        self._lab = torch.zeros(*shape, dtype=dtype, device=self.dev)
        self.gt_frames = self.gt_status = None
        if self._gt_host is not None:
            # every sequence's frames back to back, uploaded once; a batch's hop rows in ONE pinned buffer of int64 words:
            # [B, max_hops] frame indices | [B, max_hops] float64 scales | B int32 hop counts
            self.gt_frames = torch.cat([torch.from_numpy(np.ascontiguousarray(f)).to(self.dev) for f in self._gt_host], 0).contiguous()
            self._gt_host = None
            B, mh = self.B, self.max_hops
            self._hops = torch.zeros(2 * B * mh + (B + 1) // 2, dtype=torch.int64, device=self.dev)
            self._pin_hops = [torch.zeros_like(self._hops, device="cpu").pin_memory() for _ in range(2)]
            self._hop_frame, self._hop_scale, self._n_hops = self._hop_views(self._hops)
            self.gt_status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            return
        self._pin_lab = [torch.zeros(*shape, dtype=dtype).pin_memory() for _ in range(2)]

    def _hop_views(self, words):
        """One buffer of int64 words (a tensor or a numpy array) -> (frames int64 [B,mh], scales float64 [B,mh], n_hops int32 [B])."""
        B, mh = self.B, self.max_hops
        f64, i32 = (torch.float64, torch.int32) if torch.is_tensor(words) else (np.float64, np.int32)
        return words[:B * mh].reshape(B, mh), words[B * mh:2 * B * mh].view(f64).reshape(B, mh), words[2 * B * mh:].view(i32)[:B]

    def _pack_extra(self, slot, i, label):
        if self.gt_frames is not None:
            frames, scales, n_hops = self._hop_views(self._pin_hops[slot].numpy())
            frames[i], scales[i], n_hops[i] = label[0], label[1], label[2]
            return
        dst = self._pin_lab[slot][i].numpy()
        lab = label.numpy() if torch.is_tensor(label) else np.asarray(label)
        # semseg: uint8 [H,W] (or [1,H,W]); flow: float32 [2,H,W]
        want, shapes = (np.uint8, (dst.shape[1:], dst.shape)) if self.task == "semseg" else (np.float32, (dst.shape,))
        if lab.dtype != want or tuple(lab.shape) not in shapes:
            raise ValueError(f"GpuDenseLoader: a {self.task} label must be {np.dtype(want).name} {list(shapes[0])} (got {lab.dtype} {list(lab.shape)})")
        dst[...] = lab.reshape(dst.shape)

    def _upload_extra(self, slot):
        if self.gt_frames is not None:
            self._hops.copy_(self._pin_hops[slot], non_blocking=True)       # a few KB in the label planes' place
            return
        self._lab.copy_(self._pin_lab[slot], non_blocking=True)

    def _check_window(self, window, name):
        """On the host before upload: what the device would only count (status words) or bin out of bounds."""
        if window.shape[0] == 0:
            raise ValueError(f"GpuDenseLoader: clip {name!r} has an empty window")
        x, y = window[:, 0], window[:, 1]
        if self.map is not None:
            oh, ow = self.org_sensor
            # (int) truncates toward zero; a NaN fails every comparison
            if not bool(((x > -1) & (x < ow) & (y > -1) & (y < oh)).all()):
                raise ValueError(f"GpuDenseLoader: clip {name!r} has an event outside the {oh} x {ow} rectify map")
        elif not self.compact:
            H, W = self.sensor
            if not bool(((x >= 0) & (x < W) & (y >= 0) & (y < H)).all()):
                raise ValueError(f"GpuDenseLoader: clip {name!r} has an event outside the {H} x {W} sensor")

    def _status_checked(self):
        """End of a pass: the device's status words, read once."""
        if self.gt_status is not None:
            skipped = int(self.gt_status.item())
            if skipped:
                self.gt_status.zero_()
                raise ValueError(f"GpuDenseLoader: evp_mvsec_flow_propagate skipped {skipped} sample(s) of this pass whose hop table names "
                                 f"no frame of gt_flow ({self.gt_frames.shape[0]} frames, max_hops = {self.max_hops})")
        if self.status is None:
            return
        empty, outside = (int(v) for v in self.status.tolist())
        if empty or outside:
            self.status.zero_()
            raise ValueError(f"GpuDenseLoader: evp_events_rectify_compact_f64 left {empty} clip(s) of this pass without an event inside the "
                             f"{self.sensor[0]} x {self.sensor[1]} sensor and refused {outside} row(s) / clip(s) outside the map or the buffer")

    # ------------------------------------------------------------------------------------------------ device half
    def __iter__(self):
        if not self.is_train:
            self.step = self.step0
        if self.chain is not None:
            self.chain.set_state(self.step, self.first_sample)
        self._mark_read(torch.cuda.current_stream(self.dev))      # (a pass that was left early: its last step is behind this event)
        H, W = self.sensor
        for b, slot, n, names, cur in self._batches():
            if self.compact:
                rectify_compact_batch(self.ev[:n], self.d_off, self.cap, self.keep, self.sensor, self.cev, self.c_off, self.status,
                                      rectify_map=self.map, workspace=self._ws)
            if self.chain is not None:
                vox, _ = self.chain.run_next()
                rows = self.chain.crop_rows
            else:
                # float64 cells: an order-independent sum, so a validation pass repeats bit for bit
                voxel_grid_batch(self.cev, self.c_off, self.bins, self.sensor, out=self.raw, algo=3)
                vox = self.out if self.out is self.raw else evg_augment_batch(self.raw, self._full, (self.S, self.S), out=self.out, mode="bilinear")
                rows = self._full
            self.step += 1
            batch = {"events_voxel_grid": vox}
            if self.task == "semseg":
                batch["semseg_label"] = semseg_label_augment_batch(self._lab, rows, (H, W), out=self.label)
            else:
                if not self.is_train:
                    batch["events_voxel_grid_org"] = self.raw
                elif self.org_view:
                    batch["events_voxel_grid_org"] = evg_augment_batch(self.raw, rows, (H, W), out=self.org, mode="bilinear")
                if self.gt_frames is not None:
                    # the label itself, from the resident frames and the uploaded hop rows, into the buffer the label view reads
                    mvsec_flow_propagate_batch(self.gt_frames, self._hop_frame, self._hop_scale, self._n_hops, self._lab, self.gt_status)
                batch["flow_label"], batch["flow_label_valid"] = flow_label_augment_batch(self._lab, rows, (H, W), out=self.label, valid_out=self.valid)
            batch["seq_name"] = names
            yield batch
            # the consumer has queued its step: what reads the grids and the labels (and, before it, the uploaded rows) is on its stream now
            self._mark_read(torch.cuda.current_stream(self.dev))
        self._status_checked()

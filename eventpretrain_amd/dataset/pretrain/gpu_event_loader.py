"""A loader for the pre-training epoch loops that starts from RAW EVENT CLIPS: what the reference's Dataset.__getitem__ does per sample on
a DataLoader worker (dataset/pretrain/pr_n_imagenet_dataset.py:76-107: window pick -> erase / add -> rescale -> voxel grid -> view
augmentation; the seeded frame target of pr_ef_imagenet_dataset.py:187-206) happens here per BATCH on the GPU, by one replay of the
self-driven loader chain (gpu_input_pipeline.CapturedChain). The workers are left with what only they can do -- reading and decoding
the clip files.

    samples = iterable of (events float64 [n,4] (x,y,t,p) time-sorted numpy array, frame float32 [C,Hf,Wf] array / tensor or None, name)
    loader  = GpuEventLoader(args, samples, batch_size=64, n_batches=len(dataset) // 64, seed=args.seed, first_sample=rank * 64)
    pr_rec_one_epoch(args, model, loader, optimizer, epoch, loss_scaler)          # yields the dict batches the trainers take

Per batch: each clip's window is picked on the host and only its rows are packed into a pinned slot on a worker thread (one batch
ahead), uploaded on a copy stream while the previous training step runs, and turned into (events_voxel_grid [B,bins,S,S],
sub_frame [B,C,S,S]) by one graph replay. The decisions come from the counter stream keyed by (seed, step, first_sample + i):
reproducible per sample, independent of worker scheduling. The window start is the plan kernel's own rule (word 0 of the stream,
s0 = (w0 * (n - fix)) >> 32, uniform over the WHOLE clip as get_random_index draws it); the plan then sees a clip of fix rows, which it
takes whole, and draws the same counts and crop boxes it would have drawn for the uncut clip.

The pack / upload half (ClipWindowLoader) is shared with dataset.finetune_cls.gpu_event_loader.GpuFinetuneLoader, whose samples carry a
label in the frame's place, and with dataset.finetune_dense.gpu_dense_loader.GpuDenseLoader, whose samples carry a label MAP and whose
window is the clip's tail (`_window_start`)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import _lib
from ..augmentation.events_augment import philox_words
from .gpu_input_pipeline import GpuInputPipeline


class ClipWindowLoader:
    """What every raw-event loader shares: B clips per batch -> each clip's window (the plan kernel's own rule, word 0 of the counter
    stream) packed into one of two pinned slots on a worker thread, one batch ahead, and uploaded on a copy stream into the ONE device
    event buffer `self.ev` the batch's kernels read. A subclass says what else travels with a sample (`_alloc_extra`, `_pack_extra`,
    `_upload_extra`: a frame target, a label) and turns an uploaded batch into tensors (`_run`).

    Lifetimes: the pinned slot is reused once the upload out of it has run (`_slot_free`); the upload of the next batch waits for the
    event the subclass left in `_readers_done` -- recorded on the consumer's stream behind the last launch that reads what the upload
    overwrites."""
    yields_device_batches = True       # static device tensors, overwritten by the next batch: the epoch loop must not read one batch ahead

    def _setup(self, args, samples, batch_size, n_batches, seed, first_sample, step0, fix, cap):
        _lib.require_device()
        self.args, self.samples, self.B, self.n_batches = args, samples, int(batch_size), int(n_batches)
        self.dev = torch.device(args.device)
        self.fix, self.cap = int(fix), int(cap)
        self.seed, self.first_sample, self.step = int(seed), int(first_sample), int(step0)
        B = self.B
        self.ev = torch.zeros(B * self.cap, 4, dtype=torch.float64, device=self.dev)
        self.d_off = torch.zeros(B + 1, dtype=torch.int64, device=self.dev)       # where the uploaded offsets land (a chain: its own d_off)
        # two pinned slots: one being uploaded, one being packed
        self._pin_ev = [torch.zeros(B * self.cap, 4, dtype=torch.float64).pin_memory() for _ in range(2)]
        self._pin_off = [torch.zeros(B + 1, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._slot_free = [None, None]            # event: the upload out of this slot has run
        self._alloc_extra()
        self.copy_stream = torch.cuda.Stream(self.dev)
        self._readers_done = None
        self._pool = ThreadPoolExecutor(max_workers=1)

    def __len__(self):
        return self.n_batches

    def _alloc_extra(self):
        pass

    def _pack_extra(self, slot, i, extra):
        pass

    def _upload_extra(self, slot):
        pass

    def _check_window(self, window, name):
        pass

    def _window_start(self, n, fix, w0):
        """First row of the window of `fix` rows in a clip of `n`: the plan kernel's rule on word 0 of the sample's counter stream, uniform
        over the whole clip as get_random_index draws it. (The dense loaders take the clip's tail instead.)"""
        return (w0 * (n - fix)) >> 32 if n > fix else 0

    def _pack(self, it, slot, step):
        """Host half of one batch (worker thread): B samples -> their windows in the pinned slot. `step`: the counter stream's step of
        THIS batch (the pack runs one batch ahead). -> (rows, names) or None at the end of the pass."""
        if self._slot_free[slot] is not None:
            self._slot_free[slot].synchronize()
        ev_h, off_h = self._pin_ev[slot].numpy(), self._pin_off[slot].numpy()
        fix = self.fix
        w0 = philox_words(self.seed, step, self.first_sample + np.arange(self.B), 0, 1)[:, 0]      # evp_events_plan_batch's window word
        names, n = [], 0
        off_h[0] = 0
        for i in range(self.B):
            try:
                events, extra, name = next(it)
            except StopIteration:
                return None
            e = np.asarray(events, dtype=np.float64)
            if e.ndim != 2 or e.shape[1] != 4:
                raise ValueError(f"{type(self).__name__}: events must be float64 [n,4] (x,y,t,p)")
            s0 = self._window_start(e.shape[0], fix, int(w0[i]))
            k = min(e.shape[0], fix)
            self._check_window(e[s0:s0 + k], name)
            ev_h[n:n + k] = e[s0:s0 + k]
            n += k
            off_h[i + 1] = n
            self._pack_extra(slot, i, extra)
            names.append(name)
        return n, names

    def _upload(self, slot, n):
        cs = self.copy_stream
        if self._readers_done is not None:
            cs.wait_event(self._readers_done)         # whatever read the event buffer, the offsets and the extras of the last batch has run
        with torch.cuda.stream(cs):
            self.ev[:n].copy_(self._pin_ev[slot][:n], non_blocking=True)
            self.d_off.copy_(self._pin_off[slot], non_blocking=True)
            self._upload_extra(slot)
            done = torch.cuda.Event()
            done.record(cs)
        self._slot_free[slot] = done
        return done

    def _batches(self):
        """-> (batch index, pinned slot, rows, names, the consumer's stream) per batch, the upload done as far as that stream is
        concerned and the next batch being packed."""
        it = iter(self.samples)
        fut = self._pool.submit(self._pack, it, 0, self.step)
        for b in range(self.n_batches):
            slot = b & 1
            packed = fut.result()
            if packed is None:
                return
            n, names = packed
            up = self._upload(slot, n)
            if b + 1 < self.n_batches:
                fut = self._pool.submit(self._pack, it, slot ^ 1, self.step + 1)      # the next batch is packed while this one is uploaded and trained on
            cur = torch.cuda.current_stream(self.dev)
            cur.wait_event(up)
            yield b, slot, n, names, cur

    def _mark_read(self, cur):
        ev = torch.cuda.Event()
        ev.record(cur)
        self._readers_done = ev


class GpuEventLoader(ClipWindowLoader):
    def __init__(self, args, samples, batch_size, n_batches, seed=0, first_sample=0, max_events_per_clip=None, frame_shape=None,
                 frame_key="sub_frame", step0=0):
        """`samples`: a re-iterable (one pass per epoch) of (events, frame, name); `n_batches`: batches per epoch (a short last batch is
        dropped, as the reference's training loader does: drop_last=True). `max_events_per_clip`: capacity per clip of the device
        buffer, at least (and by default) fix_events_num -- only the picked window of a clip is uploaded. `frame_shape` = (C,Hf,Wf)
        when the samples carry frame targets. `step0`: the counter stream's step of the first batch (continues across epochs)."""
        fix = int(args.fix_events_num)
        cap = int(max_events_per_clip or fix)
        if cap < fix:
            raise ValueError(f"GpuEventLoader: max_events_per_clip ({cap}) must hold a window of fix_events_num ({fix}) rows")
        self.frame_key, self.frame_shape = frame_key, None if frame_shape is None else tuple(int(v) for v in frame_shape)
        self._setup(args, samples, batch_size, n_batches, seed, first_sample, step0, fix, cap)
        self.pipe = GpuInputPipeline(args, seed=seed)
        self.chain = self.pipe.capture(self.ev, self.B, frames=self.frames, clip_offsets=np.zeros(self.B + 1, np.int64))
        self.d_off = self.chain.d_off

    def _alloc_extra(self):
        B = self.B
        self.frames = None if self.frame_shape is None else torch.zeros(B, *self.frame_shape, dtype=torch.float32, device=self.dev)
        self._pin_fr = [None if self.frames is None else torch.zeros(B, *self.frame_shape, dtype=torch.float32).pin_memory() for _ in range(2)]

    def _pack_extra(self, slot, i, frame):
        fr_h = self._pin_fr[slot]
        if fr_h is not None:
            f = frame.numpy() if torch.is_tensor(frame) else np.asarray(frame, dtype=np.float32)
            if tuple(f.shape) != self.frame_shape:
                raise ValueError(f"GpuEventLoader: frame of shape {tuple(f.shape)}, expected {self.frame_shape}")
            fr_h[i].numpy()[...] = f

    def _upload_extra(self, slot):
        if self.frames is not None:
            self.frames.copy_(self._pin_fr[slot], non_blocking=True)

    def __iter__(self):
        self.chain.set_state(self.step, self.first_sample)
        for b, slot, n, names, cur in self._batches():
            vox, tgt = self.chain.run_next()
            self._mark_read(cur)                      # the replay has read the event buffer, the frames and the offsets
            self.step += 1
            batch = {"events_voxel_grid": vox}
            if tgt is not None:
                batch[self.frame_key] = tgt
            batch["image_name"] = names
            # static tensors: the consumer's launches are queued on this stream before the next replay overwrites them
            yield batch

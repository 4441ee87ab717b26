"""A loader for the classification fine-tuning loops that starts from RAW EVENT CLIPS with their labels: what the reference's fine-tuning
Dataset.__getitem__ does per sample on a DataLoader worker (dataset/finetune_cls/ft_n_imagenet_dataset.py:79-133 and its sibling
datasets: window pick -> [train: erase / add] -> rescale -> voxel grid -> [train: evg_augment(mode=args.resize_mode) | val: view_resize])
happens here per BATCH on the GPU, with the pack / upload machinery of dataset.pretrain.gpu_event_loader.

    samples = iterable of (events float64 [n,4] (x,y,t,p) time-sorted numpy array, label int, name)
    train   = GpuFinetuneLoader(args, samples, batch_size=64, n_batches=len(dataset) // 64, is_train=True, seed=args.seed)
    val     = GpuFinetuneLoader(args, val_samples, batch_size=64, n_batches=len(val_set) // 64, is_train=False, seed=args.seed)
    ft_train_one_epoch(args, model, train, optimizer, epoch, loss_scaler);  ft_val(args, model, val, epoch)

Train: one replay of the self-driven captured chain (gpu_input_pipeline.CapturedChain) with `resize_mode=args.resize_mode` -- the
reference's fine-tuning default is 'bilinear' (main_finetune_cls.py:48) -- and windows of args.fix_events_num rows.
Val: the window pick with args.val_fix_events_num (get_random_index(is_train=False), events_augment.py:9-20; the same rule on word 0 of
the counter stream), no erase / add, and ONE K1 call with the sensor -> input rescale. No view kernel runs: the reference's
view_resize of an S x S grid to S x S is the identity in both modes (scale 1: every source coordinate is the pixel's own, weight 1).
A validation pass restarts the counter stream at `step0` and bins with K1's float64 cells (algo 3, an order-independent sum), so an
evaluation set gives the same windows and the same grids, bit for bit, every epoch.

Labels travel with the windows: packed into the pinned slot, uploaded into a per-slot device tensor. They are read by the CONSUMER's
step, which is queued after this loader yields -- so the event the next upload waits for is recorded on the consumer's stream after
the generator resumes, behind that step, not behind the chain replay.

Out of scope (NotImplementedError): --val_event_noise (add_noise_events), EvRepSL, the 2- and 3-bin representations."""
import numpy as np
import torch

from ..dataset_utils.events_to_voxel_grid import voxel_grid_batch
from ..pretrain.gpu_event_loader import ClipWindowLoader
from ..pretrain.gpu_input_pipeline import GpuInputPipeline


class GpuFinetuneLoader(ClipWindowLoader):
    def __init__(self, args, samples, batch_size, n_batches, is_train, seed=0, first_sample=0, step0=0):
        """`samples`: a re-iterable (one pass per epoch) of (events, label, name); `n_batches`: batches per pass (a short last batch is
        dropped). `step0`: the counter stream's step of the first batch (a training loader continues across epochs, a validation
        loader restarts there). Yields {"events_voxel_grid": float32 [B,bins,S,S], "label": int64 [B], "image_name": [B names]}:
        device tensors the next batch overwrites."""
        if int(args.num_bins) in (2, 3):
            raise NotImplementedError("GpuFinetuneLoader: the 2- and 3-bin event representations are out of scope (voxel grids only)")
        if getattr(args, "val_event_noise", False) or getattr(args, "use_evrepsl", False):
            raise NotImplementedError("GpuFinetuneLoader: --val_event_noise and EvRepSL preprocessing are out of scope")
        self.is_train, self.step0 = bool(is_train), int(step0)
        fix = int(args.fix_events_num if self.is_train else args.val_fix_events_num)
        self._setup(args, samples, batch_size, n_batches, seed, first_sample, step0, fix, fix)
        self.S, self.bins = int(args.input_size), int(args.num_bins)
        self.sensor = (int(args.img_sensor_h), int(args.img_sensor_w))
        self.pipe = self.chain = self.out = None
        if self.is_train:
            self.pipe = GpuInputPipeline(args, seed=seed, resize_mode=getattr(args, "resize_mode", "bilinear"))
            self.chain = self.pipe.capture(self.ev, self.B, clip_offsets=np.zeros(self.B + 1, np.int64))
            self.d_off = self.chain.d_off
        else:
            self.out = torch.zeros(self.B, self.bins, self.S, self.S, dtype=torch.float32, device=self.dev)

    def _alloc_extra(self):
        self._lab = [torch.zeros(self.B, dtype=torch.int64, device=self.dev) for _ in range(2)]
        self._pin_lab = [torch.zeros(self.B, dtype=torch.int64).pin_memory() for _ in range(2)]

    def _pack_extra(self, slot, i, label):
        self._pin_lab[slot][i] = int(label)

    def _upload_extra(self, slot):
        self._lab[slot].copy_(self._pin_lab[slot], non_blocking=True)

    def __iter__(self):
        H, W = self.sensor
        if self.is_train:
            self.chain.set_state(self.step, self.first_sample)
        else:
            self.step = self.step0
        self._mark_read(torch.cuda.current_stream(self.dev))      # (a pass that was left early: its last step is behind this event)
        for b, slot, n, names, cur in self._batches():
            if self.is_train:
                vox, _ = self.chain.run_next()
            else:
                # algo 3: float64 cells in K1's LDS tile -- the sum no longer depends on the order its atomics arrive in, so a pass repeats
                # bit for bit (the float32 cells of the default differ by an ulp or two from launch to launch); 1.2 x the K1 time
                vox = voxel_grid_batch(self.ev[:n], self.d_off, self.bins, (self.S, self.S), scale=(self.S / W, self.S / H), out=self.out,
                                       algo=3)
            self.step += 1
            yield {"events_voxel_grid": vox, "label": self._lab[slot], "image_name": names}
            # the consumer has queued its step: what reads the grids, the labels and (before it) the event buffer is on its stream now
            self._mark_read(torch.cuda.current_stream(self.dev))

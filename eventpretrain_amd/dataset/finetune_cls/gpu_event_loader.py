"""A loader for the classification fine-tuning loops that starts from RAW EVENT CLIPS with their labels: what the reference's fine-tuning
Dataset.__getitem__ does per sample on a DataLoader worker (dataset/finetune_cls/ft_n_imagenet_dataset.py:79-133 and its sibling
datasets: window pick -> [train: erase / add] -> rescale -> voxel grid -> [train: evg_augment(mode=args.resize_mode) | val: view_resize])
happens here per BATCH on the GPU, with the pack / upload machinery of dataset.pretrain.gpu_event_loader.

    samples = iterable of (events float64 [n,4] (x,y,t,p) time-sorted numpy array, label int, name)
    train   = GpuFinetuneLoader(args, samples, batch_size=64, n_batches=len(dataset) // 64, is_train=True, seed=args.seed)
    val     = GpuFinetuneLoader(args, val_samples, batch_size=64, n_batches=len(val_set) // 64, is_train=False, seed=args.seed)
    ft_train_one_epoch(args, model, train, optimizer, epoch, loss_scaler);  ft_val(args, model, val, epoch)

Two recipes, chosen by the caller (`grid`, `sensor`; `finetune_recipe(args)` maps the reference's dataset_type strings to them):
  grid="input"   N-ImageNet (ft_n_imagenet_dataset.py:79-133): events_reshape sensor -> input_size, voxelise at S x S, crop boxes on S x S;
                 validation's view_resize of an S x S grid to S x S is the identity in both modes, so no view kernel runs there.
  grid="sensor"  N-Caltech101, CIFAR10-DVS, DVS128-Gesture, UCF101-DVS, ES-ImageNet with 5 bins (ft_n_caltech101_dataset.py:61-91,
                 ft_dvs128_gesture_dataset.py:63-89 and siblings): no events_reshape, voxelise at the sensor's (H, W), crop boxes on the
                 H x W grid, evg_augment (train) / view_resize (val) resizes H x W -> S x S in args.resize_mode.

  grid="window"  N-Cars (ft_n_cars_dataset.py:61-87; `ncars_recipe(args)`): as grid="sensor", but every sample's grid is its own window's
                 extent, H_c = int(max y) + 1 by W_c = int(max x) + 1, taken before the event augmentation -- the bound of the added rows,
                 the voxel grid's size and the view view_crop draws its box on. `sensor` is the CAPACITY (cap_h, cap_w): K1 and the view
                 kernels run on padded cap_h x cap_w grids of which a clip fills the top-left H_c x W_c, the per-clip geometry travels in
                 the crop rows (evp_events_window_geometry writes them; evp_events_build_added_hw_f64 clips the added rows per clip).
                 Bit for bit the reference's chain (tests/golden/ft_ncars_recipe.npz) except a 1 x 1 window grid in bilinear mode, where
                 ATen takes another path and differs by 1 ulp. Every window is checked on the host before upload (non-empty, coordinates
                 >= 0 and inside the capacity: ValueError naming the clip); the device's own count of refused windows is read once at the
                 end of a pass. Clean validation: the geometry kernel on the uploaded windows, K1 algo 3 at the capacity, the view kernel
                 under the clips' full boxes.

Train: one replay of the self-driven captured chain (gpu_input_pipeline.CapturedChain) with `resize_mode=args.resize_mode` -- the
reference's fine-tuning default is 'bilinear' (main_finetune_cls.py:48) -- and windows of args.fix_events_num rows.
Val: the window pick with args.val_fix_events_num (get_random_index(is_train=False), events_augment.py:9-20; the same rule on word 0 of
the counter stream), no erase / add, ONE K1 call (with the sensor -> input rescale, or unscaled at the sensor's size) and, where the grid
is not S x S already, the view kernel under the constant full-box rows -- view_resize alone.
A validation pass restarts the counter stream at `step0` and bins with K1's float64 cells (algo 3, an order-independent sum), so an
evaluation set gives the same windows and the same grids, bit for bit, every epoch.
Noisy val (args.val_event_noise, the reference's robustness evaluation): events_augment's erase / add on the validation window as well,
then the validation view -- the self-driven captured chain with windows of args.val_fix_events_num rows, no view augmentation and the
fused K1's float64 cells (evp_voxel_scatter_fused_algo_f32 algo 3), its counter stream reset to (step0, first_sample) at the start of
every pass: a pass redraws the same erase / add decisions and gives the same bits.

Labels travel with the windows: packed into the pinned slot, uploaded into a per-slot device tensor. They are read by the CONSUMER's
step, which is queued after this loader yields -- so the event the next upload waits for is recorded on the consumer's stream after
the generator resumes, behind that step, not behind the chain replay.

Event-count images (args.num_bins 2 or 3; finetune_recipe gives each dataset's grid, `rescale` and `norm_guard`): the representation
stage is dataset_utils.events_to_image.event_image_batch (csrc/evimage.hip) in K1's place -- events_to_image_ecdp, or
events_to_image_mem, / 255 and remove_hot_pixel_mem -- and the datasets' normalisation (per-channel ((v / (max + 1)) - 0.5) * 2, or planes
0 and 2 over their common max) follows the view stage. Train and noisy validation replay the captured chain in its merged-clip form
(evp_events_erase_add_win_f64 -> count -> finish -> view -> normalise), clean validation counts the uploaded windows directly. The
counts are integer sums, so every pass repeats bit for bit. A row whose linear cell index leaves the grid is where the reference
raises: the device counts such rows and the loader raises ValueError at the end of the pass; `loader.empty_views` is the pass's count
of all-zero 3-channel views (NaN without the dataset's guard, as in the reference). A time flip reverses the channel order and negates
nothing (evg_time_flip negates 5- and 6-bin grids only).

Out of scope (NotImplementedError): EvRepSL, event-count images for N-Cars (grid="window"). The
reference's add_noise_events (events_augment.py) is called by none of its datasets and is not what --val_event_noise means."""
import numpy as np
import torch

from ..._lib import call, ptr, stream_ptr
from ..dataset_utils.events_to_image import event_image_batch
from ..dataset_utils.events_to_voxel_grid import voxel_grid_batch
from ..pretrain.gpu_event_loader import ClipWindowLoader
from ..augmentation.view_augment import evg_augment_batch
from ..pretrain.gpu_input_pipeline import GpuInputPipeline

# the reference's dataset_type strings (main_finetune_cls.py) -> (grid, the prefix of its own sensor arguments)
_RECIPES = {"n-imagenet": ("input", "img"), "n-caltech101": ("sensor", "cal"), "cifar10-dvs": ("sensor", "cifar"),
            "dvs128_gesture": ("sensor", "gesture"), "ucf101_dvs": ("sensor", "ucf"), "es-imagenet": ("sensor", "esimg")}


# event-count images: dataset_type -> ((grid, rescale) with 2 channels, (grid, rescale) with 3 channels, the `factor = 1.0 / 0.001` guard),
# read off the reference's files: ft_n_imagenet_dataset.py:92-115 (events_reshape ahead of both branches), ft_n_caltech101_dataset.py:71-98
# (both at the sensor's size), ft_cifar10_dvs_dataset.py:69-92, ft_dvs128_gesture_dataset.py:73-96 and ft_ucf101_dvs_dataset.py:75-101
# (events_reshape inside the 2-channel branch only; UCF101-DVS alone has the `else`), ft_es_imagenet_dataset.py:109-131 (2 channels on
# input_size x input_size with no events_reshape at all; `if max > 0` skips the product, which on an all-zero view is the guard's result)
_COUNT_RECIPES = {"n-imagenet": (("input", True), ("input", True), False), "n-caltech101": (("sensor", True), ("sensor", True), False),
                  "cifar10-dvs": (("input", True), ("sensor", True), False), "dvs128_gesture": (("input", True), ("sensor", True), False),
                  "ucf101_dvs": (("input", True), ("sensor", True), True), "es-imagenet": (("input", False), ("sensor", True), True)}


def finetune_recipe(args):
    """-> dict(grid=..., sensor=(h, w)): GpuFinetuneLoader's recipe keywords for args.dataset_type, the sensor read from the reference's
    own argument names for that dataset (cal_sensor_h / _w for N-Caltech101, ...). The loader never calls this on its own.
    With args.num_bins in (2, 3) (event-count images) the grid is the one the dataset's own branch for that representation counts on,
    and two more keywords come along: rescale (False: the events are counted at their sensor coordinates on the S x S grid) and
    norm_guard (the dataset multiplies an all-zero 3-channel view by 1.0 / 0.001 where the others divide by zero)."""
    kind = args.dataset_type
    count = int(getattr(args, "num_bins", 5)) in (2, 3)
    if kind == "n-cars":
        if count:
            raise NotImplementedError("finetune_recipe: n-cars event-count images (num_bins 2 / 3) are out of scope: its per-clip window grids "
                                      "(ncars_recipe) are voxel grids only")
        raise NotImplementedError("finetune_recipe: n-cars sizes each grid from the window's own max(x) + 1 and max(y) + 1, so its recipe carries "
                                  "a capacity in the sensor's place: use ncars_recipe(args)")
    if kind not in _RECIPES:
        raise ValueError(f"finetune_recipe: unknown dataset_type {kind!r} (one of {sorted(_RECIPES)})")
    grid, prefix = _RECIPES[kind]
    sensor = (int(getattr(args, prefix + "_sensor_h")), int(getattr(args, prefix + "_sensor_w")))
    if not count:
        return dict(grid=grid, sensor=sensor)
    two, three, guard = _COUNT_RECIPES[kind]
    grid, rescale = two if int(args.num_bins) == 2 else three
    return dict(grid=grid, sensor=sensor, rescale=rescale, norm_guard=guard)


def ncars_recipe(args):
    """-> dict(grid="window", sensor=(cap_h, cap_w)): GpuFinetuneLoader's recipe keywords for N-Cars, the capacity of the padded grids read
    from the reference's own cars_sensor_h / cars_sensor_w (100 x 120 where the namespace has none)."""
    return dict(grid="window", sensor=(int(getattr(args, "cars_sensor_h", 100)), int(getattr(args, "cars_sensor_w", 120))))


class GpuFinetuneLoader(ClipWindowLoader):
    def __init__(self, args, samples, batch_size, n_batches, is_train, seed=0, first_sample=0, step0=0, grid="input", sensor=None,
                 rescale=True, norm_guard=False):
        """`samples`: a re-iterable (one pass per epoch) of (events, label, name); `n_batches`: batches per pass (a short last batch is
        dropped). `step0`: the counter stream's step of the first batch (a training loader continues across epochs, a validation
        loader restarts there). Yields {"events_voxel_grid": float32 [B,bins,S,S], "label": int64 [B], "image_name": [B names]}:
        device tensors the next batch overwrites. `grid` / `sensor` / `rescale` / `norm_guard`: the recipe (module docstring), passed
        to GpuInputPipeline; the last two matter for event-count images (args.num_bins 2 or 3) only."""
        if int(args.num_bins) in (2, 3) and grid == "window":
            raise NotImplementedError("GpuFinetuneLoader: event-count images (num_bins 2 / 3) on N-Cars' per-clip window grids are out of scope "
                                      "(voxel grids only)")
        if getattr(args, "use_evrepsl", False):
            raise NotImplementedError("GpuFinetuneLoader: EvRepSL preprocessing is out of scope")
        self.is_train, self.step0 = bool(is_train), int(step0)
        self.noisy_val = not self.is_train and bool(getattr(args, "val_event_noise", False))
        fix = int(args.fix_events_num if self.is_train else args.val_fix_events_num)
        mode = getattr(args, "resize_mode", "bilinear")
        # (the pipeline validates grid / sensor / mode before any device memory is taken)
        pipe = GpuInputPipeline(args, seed=seed, resize_mode=mode, grid=grid, sensor=sensor, fix_events_num=fix,
                                view_augment=self.is_train, voxel_cells="f32" if self.is_train else "f64", rescale=rescale,
                                norm_guard=norm_guard, representation="count" if int(args.num_bins) in (2, 3) else "voxel")
        self._setup(args, samples, batch_size, n_batches, seed, first_sample, step0, fix, fix)
        self.S, self.bins, self.resize_mode = int(args.input_size), int(args.num_bins), mode
        self.sensor, self.grid_hw, self.scale, self.window = pipe.sensor, (pipe.gh, pipe.gw), pipe.scale, pipe.grid == "window"
        self.pipe = self.chain = self.out = self.raw = self.ext = self.geom_status = None
        # event-count images: the pipeline's device counts {rows outside the grid, all-zero 3-channel views}, read at the end of a pass
        self.count, self._clean_pipe, self.empty_views = pipe.count, pipe, 0
        self.image_status = pipe._status(self.dev) if pipe.count else None
        if self.is_train or self.noisy_val:
            self.pipe = pipe
            self.chain = pipe.capture(self.ev, self.B, clip_offsets=np.zeros(self.B + 1, np.int64))
            self.d_off = self.chain.d_off
            self.ext, self.geom_status = self.chain.ext, self.chain.geom_status
        else:
            self.out = torch.zeros(self.B, self.bins, self.S, self.S, dtype=torch.float32, device=self.dev)
            if pipe.resize:                               # view_resize is a real resize: K1 into the sensor-sized grids, then the view kernel
                self.raw = torch.zeros(self.B, self.bins, *self.grid_hw, dtype=torch.float32, device=self.dev)
                # the full-box rows: one constant row, or (window) the clips' own (0, 0, W_c, H_c, 0, 0), written per batch by the geometry kernel
                self._full = torch.zeros(self.B, 6, dtype=torch.int32, device=self.dev) if self.window else pipe.full_rows(self.B, self.dev)
            if self.window:
                self.ext = torch.zeros(self.B, 2, dtype=torch.int32, device=self.dev)
                self.geom_status = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def _alloc_extra(self):
        self._lab = [torch.zeros(self.B, dtype=torch.int64, device=self.dev) for _ in range(2)]
        self._pin_lab = [torch.zeros(self.B, dtype=torch.int64).pin_memory() for _ in range(2)]

    def _pack_extra(self, slot, i, label):
        self._pin_lab[slot][i] = int(label)

    def _upload_extra(self, slot):
        self._lab[slot].copy_(self._pin_lab[slot], non_blocking=True)

    def _check_window(self, window, name):
        """grid="window", on the host before upload: what evp_events_window_geometry would refuse (and only count) on the device."""
        if not self.window:
            return
        cap_h, cap_w = self.sensor
        if window.shape[0] == 0:
            raise ValueError(f"GpuFinetuneLoader: clip {name!r} has an empty window (grid='window' sizes the grid from the window's rows)")
        x0, x1, y0, y1 = window[:, 0].min(), window[:, 0].max(), window[:, 1].min(), window[:, 1].max()
        if not (x0 >= 0 and y0 >= 0):
            raise ValueError(f"GpuFinetuneLoader: clip {name!r} has a negative coordinate (min x {x0}, min y {y0})")
        if not (x1 < cap_w and y1 < cap_h):
            raise ValueError(f"GpuFinetuneLoader: clip {name!r} reaches past the capacity {cap_h} x {cap_w} (max x {x1}, max y {y1})")

    def _geometry_checked(self):
        """End of a pass with grid="window": the device's count of refused windows, read once (the host check above should leave it 0)."""
        if self.geom_status is None:
            return
        bad = int(self.geom_status.item())
        if bad:
            self.geom_status.zero_()
            raise ValueError(f"GpuFinetuneLoader: evp_events_window_geometry refused {bad} window(s) of this pass (empty, a negative coordinate, "
                             f"or an extent above the capacity {self.sensor[0]} x {self.sensor[1]}); their grids were clamped")

    def _images_checked(self):
        """End of a pass with event-count images: the two device counts, read once and cleared."""
        if self.image_status is None:
            return
        outside, self.empty_views = (int(v) for v in self.image_status.tolist())
        self.image_status.zero_()
        if outside:
            raise ValueError(f"GpuFinetuneLoader: {outside} event row(s) of this pass fall outside the {self.grid_hw[0]} x {self.grid_hw[1]} grid "
                             "the images are counted on (the reference's bincount / reshape raises there); they were left out")

    def __iter__(self):
        if not self.is_train:
            self.step = self.step0
        if self.chain is not None:
            self.chain.set_state(self.step, self.first_sample)     # (noisy validation: every pass redraws the same erase / add decisions)
        self._mark_read(torch.cuda.current_stream(self.dev))      # (a pass that was left early: its last step is behind this event)
        for b, slot, n, names, cur in self._batches():
            if self.chain is not None:
                vox, _ = self.chain.run_next()
            else:
                # algo 3: float64 cells in K1's LDS tile -- the sum no longer depends on the order its atomics arrive in, so a pass repeats
                # bit for bit (the float32 cells of the default differ by an ulp or two from launch to launch); 1.2 x the K1 time
                if self.window:
                    call("evp_events_window_geometry", ptr(self.ev), ptr(self.d_off), ptr(self.d_off[1:]), self.B, self.sensor[0], self.sensor[1], 0,
                         1.0, 0, 0, 0, None, ptr(self.ext), ptr(self._full), ptr(self.geom_status), stream_ptr())
                if self.count:
                    vox = event_image_batch(self.ev[:n], self.d_off, self.bins, self.grid_hw, scale=self.scale,
                                            out=self.out if self.raw is None else self.raw, status=self.image_status[:1], max_rows_per_clip=self.fix)
                else:
                    vox = voxel_grid_batch(self.ev[:n], self.d_off, self.bins, self.grid_hw, scale=self.scale,
                                           out=self.out if self.raw is None else self.raw, algo=3)
                if self.raw is not None:
                    vox = evg_augment_batch(vox, self._full, (self.S, self.S), out=self.out, mode=self.resize_mode)
                self._clean_pipe._tail(vox)
            self.step += 1
            yield {"events_voxel_grid": vox, "label": self._lab[slot], "image_name": names}
            # the consumer has queued its step: what reads the grids, the labels and (before it) the event buffer is on its stream now
            self._mark_read(torch.cuda.current_stream(self.dev))
        self._geometry_checked()
        self._images_checked()

"""Skipping the optimizer step on non-finite gradients, on the device (reference utils/misc.py:290: GradScaler.step leaves
optimizer.step() out when a gradient holds an Inf or NaN): evp_grad_guard_multi against the oracle norm and evp_grad_clip_multi,
FusedAdamW(skip_nonfinite=True) against a torch.optim.AdamW that steps only on finite gradients, and the guarded recipes running as
captured HIP graphs -- one rank and two. Only non-finite VALUES are injected."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------------------ 1. kernel
def _tables(grads):
    numel = np.array([g.numel() for g in grads], dtype=np.int64)
    ct = np.concatenate([np.full((int(n) + CHUNK - 1) // CHUNK, t, dtype=np.int32) for t, n in enumerate(numel)])
    co = np.concatenate([np.arange(0, int(n), CHUNK, dtype=np.int64) for n in numel])
    dev = grads[0].device
    return dict(ptrs=torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64, device=dev), numel=torch.from_numpy(numel).to(dev),
                ct=torch.from_numpy(ct).to(dev), co=torch.from_numpy(co).to(dev), n=int(ct.shape[0]),
                ws=torch.empty(int(ct.shape[0]), dtype=torch.float32, device=dev))


def _guard(T, max_norm, betas, hyper, out, guard):
    from eventpretrain_amd._lib import call, stream_ptr
    call("evp_grad_guard_multi", T["ptrs"].data_ptr(), T["numel"].data_ptr(), T["ct"].data_ptr(), T["co"].data_ptr(), T["n"], CHUNK,
         T["ws"].data_ptr(), float(max_norm), float(betas[0]), float(betas[1]), hyper.data_ptr(), out.data_ptr(), guard.data_ptr(),
         stream_ptr())


def _clip(T, max_norm, hyper, out):
    from eventpretrain_amd._lib import call, stream_ptr
    call("evp_grad_clip_multi", T["ptrs"].data_ptr(), T["numel"].data_ptr(), T["ct"].data_ptr(), T["co"].data_ptr(), T["n"], CHUNK,
         T["ws"].data_ptr(), float(max_norm), hyper.data_ptr(), out.data_ptr(), stream_ptr())


def _bias_corrections(betas, t):
    """FusedAdamW.stage_scalars' host formulas, rounded to float32 once."""
    return np.float32(1.0 - betas[0] ** t), np.float32(math.sqrt(1.0 - betas[1] ** t))


@pytest.fixture(scope="module")
def kernel_case():
    """The shapes of the clip test's parameter groups and one view that starts 4 bytes off a 16-byte boundary (3 head elements, 1024
    float4, 3 tail elements); the float64 oracle norm of the clean set, computed once."""
    from oracle import model_oracle as mo
    g = torch.Generator().manual_seed(31)
    host = [torch.randn(*s, generator=g) * (0.2 + 0.1 * i) for i, s in enumerate([(37, 19), (129,), (5, 4100), (1,)])]
    base = torch.randn(5010, generator=g)
    dev = [h.cuda() for h in host]
    b = base.cuda()
    view = b[1:1 + 4102]
    assert view.data_ptr() % 16 == 4 and all(d.data_ptr() % 16 == 0 for d in dev)
    grads = dev + [view]
    total = float(mo.grad_norm([h.double() for h in host] + [base[1:1 + 4102].double()]))
    return dict(grads=grads, T=_tables(grads), total=total, keep=b)


def test_guard_kernel_flags_every_planting_and_leaves_the_tables_alone(kernel_case):
    """NaN / +Inf / -Inf at a scalar-head, a float4-body and a scalar-tail element, at both sides of the chunk boundary of the
    20500-element tensor, and in the one-element tensor: guard[0] = 1, guard[1] up by one, guard[2] and hyper unchanged bit for bit,
    out = {NaN, 0}."""
    grads, T = kernel_case["grads"], kernel_case["T"]
    # (tensor, flat index): 703 = 175 * 4 + 3 and 129 = 32 * 4 + 1 end in scalar tails; the view's first 3 elements are its head
    places = [(4, 1), (4, 100), (4, 4101), (0, 8), (0, 702), (1, 128), (2, 16383), (2, 16384), (2, 20499), (3, 0)]
    hyper0 = torch.tensor([0.25, 0.75, 0.5, 1.0], dtype=torch.float32)
    for max_norm in (5.0, 0.0):
        for ti, idx in places:
            flat = grads[ti].view(-1)
            saved = flat[idx].clone()
            for k, poison in enumerate((NAN, INF, -INF)):
                flat[idx] = poison
                hyper, out = hyper0.cuda(), torch.full((2,), -1.0, device="cuda")
                guard = torch.tensor([0, 7 + k, 41, 0], dtype=torch.int64, device="cuda")
                _guard(T, max_norm, (0.9, 0.999), hyper, out, guard)
                assert guard.tolist() == [1, 8 + k, 41, 0], (max_norm, ti, idx, poison, guard.tolist())
                assert hyper.cpu().numpy().tobytes() == hyper0.numpy().tobytes(), (ti, idx, poison)
                o = out.tolist()
                assert math.isnan(o[0]) and o[1] == 0.0, (ti, idx, poison, o)
            flat[idx] = saved


def test_guard_kernel_on_clean_gradients_matches_the_oracle_and_the_clip_entry(kernel_case):
    """Clean gradients: guard = {0, same, +1}; out[0] within 1e-5 relative of oracle.grad_norm in float64 (the clip test's bound);
    coefficient and hyper[2] equal, bit for bit, to evp_grad_clip_multi's on the same input; hyper[0:2] are the bias corrections of
    the new t; max_norm = 0 clips nothing. Two launches give the same bits."""
    T, total = kernel_case["T"], kernel_case["total"]
    betas = (0.9, 0.999)
    for gs in (1.0, 0.5):
        for max_norm in (0.37 * total * gs, 2.5 * total * gs, 0.0):
            runs = []
            for _ in range(2):
                hyper = torch.tensor([0.25, 0.75, gs, 1.0], dtype=torch.float32, device="cuda")
                out = torch.full((2,), -1.0, device="cuda")
                guard = torch.tensor([1, 7, 41, 0], dtype=torch.int64, device="cuda")
                _guard(T, max_norm, betas, hyper, out, guard)
                assert guard.tolist() == [0, 7, 42, 0]
                runs.append((out.cpu().numpy().copy(), hyper.cpu().numpy().copy()))
            (o, h), (o2, h2) = runs
            assert o.tobytes() == o2.tobytes() and h.tobytes() == h2.tobytes()
            print("gs", gs, "max_norm", max_norm, "norm", float(o[0]), "oracle", total * gs, "coef", float(o[1]))
            assert abs(float(o[0]) - total * gs) <= 1e-5 * total * gs, (gs, float(o[0]), total * gs)
            bc1, bc2 = _bias_corrections(betas, 42)
            assert abs(int(h[:2].view(np.int32)[0]) - int(np.array([bc1]).view(np.int32)[0])) <= 1
            assert abs(int(h[:2].view(np.int32)[1]) - int(np.array([bc2]).view(np.int32)[0])) <= 1
            assert h[3] == 1.0
            if max_norm == 0.0:
                assert o[1] == 1.0 and h[2] == np.float32(gs)
                continue
            hyper_c = torch.tensor([0.25, 0.75, gs, 1.0], dtype=torch.float32, device="cuda")
            out_c = torch.full((2,), -1.0, device="cuda")
            _clip(T, max_norm, hyper_c, out_c)
            assert out_c.cpu().numpy().tobytes() == o.tobytes(), (out_c.tolist(), o)
            assert hyper_c.cpu().numpy()[2:].tobytes() == h[2:].tobytes()
            assert (o[1] < 1.0) == (max_norm < total * gs)


def test_guard_kernel_overflowed_but_finite_norm_is_a_zero_gradient_not_a_skip():
    """Every element 3e19 (finite; its square is not): clip_grad_norm_ on the CPU gives norm inf and scales every gradient to 0. The
    guard does the same: not skipped, out = {inf, 0}, hyper[2] = 0."""
    ref = torch.nn.Parameter(torch.zeros(100))
    ref.grad = torch.full((100,), 3e19)
    assert torch.isinf(torch.nn.utils.clip_grad_norm_([ref], 5.0)) and float(ref.grad.abs().max()) == 0.0
    g = torch.full((100,), 3e19, device="cuda")
    T = _tables([g])
    hyper = torch.tensor([0.25, 0.75, 1.0, 1.0], dtype=torch.float32, device="cuda")
    out, guard = torch.full((2,), -1.0, device="cuda"), torch.tensor([0, 2, 9, 0], dtype=torch.int64, device="cuda")
    _guard(T, 5.0, (0.9, 0.999), hyper, out, guard)
    assert guard.tolist() == [0, 2, 10, 0]
    assert out.tolist() == [INF, 0.0] and float(hyper[2]) == 0.0


def test_guard_kernel_bias_corrections_follow_the_host_formulas():
    """t = 1 .. 2000 with betas (0.9, 0.95) and (0.9, 0.999): the device-written hyper[0:2] against numpy.float32 of stage_scalars'
    formulas, at most one float32 ulp apart (both sides evaluate in double from the same double betas; a few double ulps cannot move
    a float by more than one ulp). Prints how many of the 4000 differ at all."""
    g = torch.ones(5, device="cuda")
    T = _tables([g])
    for betas in ((0.9, 0.95), (0.9, 0.999)):
        hyper = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float32, device="cuda")
        out, guard = torch.zeros(2, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
        got = torch.zeros(2000, 2, device="cuda")
        for t in range(2000):
            _guard(T, 0.0, betas, hyper, out, guard)
            got[t].copy_(hyper[:2])
        assert guard.tolist() == [0, 0, 2000, 0]
        got = got.cpu().numpy()
        want = np.array([_bias_corrections(betas, t) for t in range(1, 2001)], dtype=np.float32)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print("betas", betas, ":", int((ulps != 0).sum()), "of 4000 bias corrections differ from the host's; worst", int(ulps.max()), "ulp")
        assert np.isfinite(got).all() and int(ulps.max()) <= 1, (betas, int(ulps.max()), int(ulps.argmax()))


# --------------------------------------------------------------------------------------------------------------- 2. optimizer
def _loss(ps, x, step):
    return (torch.nn.functional.linear(x, ps[0]) ** 2).mean() + (ps[1] ** 2).sum() * 0.01 + (ps[2].sin() * (1 + step)).sum() * 1e-3 + ps[3].sum()


def _groups(q):
    return [{"params": [q[0], q[2]], "weight_decay": 0.05}, {"params": [q[1], q[3]], "weight_decay": 0.0}]


POISONS = {1: (2, 16384, NAN), 2: (1, 128, INF)}      # step -> (tensor, flat index, value): one NaN, one Inf, in different tensors


def _everything(opt, ps):
    out = []
    for p in ps:
        out += [p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
        if getattr(p, "_evp_lp", None) is not None:
            out.append(p._evp_lp.clone())
    return out


@pytest.mark.parametrize("clip", [None, 0.05])
def test_guarded_update_matches_torch_adamw_stepped_on_finite_gradients_only(clip):
    """FusedAdamW(skip_nonfinite=True) against torch.optim.AdamW on the CPU, fed the GPU's gradients and stepped only when every
    gradient is finite (GradScaler._maybe_opt_step's rule). The clip test's parameter groups, five steps, the second and third
    poisoned. A poisoned step leaves parameters, moments and bf16 shadows bit-identical; clean steps match at rtol 1e-5 / atol 1e-6
    (the bound of the clip test's comparison); the checkpoint carries the applied count and a resumed optimizer continues from it."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(23)
    init = [torch.randn(*s, generator=g) for s in [(37, 19), (129,), (5, 4100), (1,)]]
    x = torch.randn(8, 19, generator=g).cuda()
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    ops.set_compute_dtype(torch.bfloat16)
    try:
        for p in (ps[0], ps[2]):                 # bf16 shadows on two of the four, as the GEMM weights of a bf16 run have
            ops.lp_weight(p)
    finally:
        ops.set_compute_dtype(torch.float32)
    opt = FusedAdamW(_groups(ps), lr=1e-2, betas=(0.9, 0.95), max_grad_norm=clip, skip_nonfinite=True)
    ropt = torch.optim.AdamW(_groups(ref), lr=1e-2, betas=(0.9, 0.95), eps=1e-8)

    def one_step(o, q, step, poison):
        o.zero_grad(set_to_none=True)
        _loss(q, x, step).backward()
        if poison is not None:
            q[poison[0]].grad.view(-1)[poison[1]] = poison[2]
        for r, p in zip(ref, q):
            r.grad = p.grad.detach().cpu().clone()
        finite = all(bool(torch.isfinite(r.grad).all()) for r in ref)
        before = _everything(o, q) if step else None
        o.step()
        if finite:
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(ref, clip)
            ropt.step()
        return finite, before

    applied = 0
    for step in range(5):
        finite, before = one_step(opt, ps, step, POISONS.get(step))
        assert finite == (step not in POISONS)
        applied += finite
        gs = opt.guard_state.tolist()
        assert gs[:3] == [0 if finite else 1, step + 1 - applied, applied], (step, gs)
        if not finite:
            after = _everything(opt, ps)
            assert len(after) == len(before) == 14
            assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                                   b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16)) for a, b in zip(after, before)), step
            assert math.isnan(float(opt.last_grad_norm[0])) and float(opt.last_grad_norm[1]) == 0.0
        else:
            for r, p in zip(ref, ps):
                assert torch.allclose(p.detach().cpu(), r.detach(), rtol=1e-5, atol=1e-6), (clip, step, tuple(p.shape))
            for p in (ps[0], ps[2]):             # the shadow is the updated weight, rounded once
                assert torch.equal(p._evp_lp, p.detach().to(torch.bfloat16))
    assert opt.skipped_steps() == 2
    sd = opt.state_dict()
    assert [float(st["step"]) for st in sd["state"].values()] == [3.0] * 4
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = FusedAdamW(_groups(ps2), lr=1e-2, betas=(0.9, 0.95), max_grad_norm=clip, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    finite, _ = one_step(opt2, ps2, 5, None)
    assert finite and opt2.guard_state.tolist()[:3] == [0, 0, 4]
    for r, p in zip(ref, ps2):
        assert torch.allclose(p.detach().cpu(), r.detach(), rtol=1e-5, atol=1e-6), (clip, "resumed", tuple(p.shape))
    assert {float(st["step"]) for st in opt2.state_dict()["state"].values()} == {4.0}
    # reset_state zeroes the guard in place
    addr = opt2.guard_state.data_ptr()
    opt2.reset_state()
    assert opt2.guard_state.data_ptr() == addr and opt2.guard_state.tolist() == [0, 0, 0, 0] and opt2.skipped_steps() == 0


def test_unguarded_update_applies_the_poison():
    """The same poisoned steps with skip_nonfinite=False leave NaN in the parameters: the test's poison does reach the update."""
    from eventpretrain_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(23)
    init = [torch.randn(*s, generator=g) for s in [(37, 19), (129,), (5, 4100), (1,)]]
    x = torch.randn(8, 19, generator=g).cuda()
    for step, (ti, idx, value) in POISONS.items():
        ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        opt = FusedAdamW(_groups(ps), lr=1e-2, betas=(0.9, 0.95))
        _loss(ps, x, step).backward()
        ps[ti].grad.view(-1)[idx] = value
        opt.step()
        assert bool(torch.isnan(ps[ti].detach().view(-1)[idx])), (step, value)


# ------------------------------------------------------------------------------------------------------------------- 3. loops
class _GuardRecordingLoader:
    """A list of batches that notes, each time the loop comes for a batch (and at the end of the epoch), clones of two weights and the
    optimizer's guard_state as the step before left them (the executor's `guard_state` is the same tensor)."""

    def __init__(self, batches, watched, opt):
        self.batches, self.watched, self.opt, self.log = batches, watched, opt, []

    def __len__(self):
        return len(self.batches)

    def _note(self):
        torch.cuda.synchronize()
        g = self.opt.guard_state
        self.log.append(([w.detach().clone() for w in self.watched], None if g is None else [int(v) for v in g.cpu()][:3]))

    def __iter__(self):
        for b in self.batches:
            self._note()
            yield b
        self._note()


def _watched(m):
    """The first and the last attention input projection of the backbone."""
    qkv = [p for k, p in m.named_parameters() if k.startswith("backbone") and k.endswith("attn.qkv.weight") and p.requires_grad]
    return [qkv[0], qkv[-1]]


def _check_log(log, poisoned, applied0, skipped0, guarded=True):
    """log[i] = state in front of step i, log[-1] behind the last: weights bit-identical across the poisoned step and changed across
    every other; the counters follow."""
    applied, skipped = applied0, skipped0
    for i in range(len(log) - 1):
        same = all(torch.equal(a, b) for a, b in zip(log[i][0], log[i + 1][0]))
        moved = all(not torch.equal(a, b) for a, b in zip(log[i][0], log[i + 1][0]))
        if i == poisoned:
            assert same, i
            skipped += 1
        else:
            assert moved, i
            applied += 1
        if guarded:
            assert log[i + 1][1] == [1 if i == poisoned else 0, skipped, applied], (i, log[i + 1][1])
    return applied, skipped


def _ft_batches():
    from eventpretrain_amd.testing import det_normalish
    batches = [dict(events_voxel_grid=det_normalish(f"ft.x.{i}", (4, 5, 224, 224)) * 0.5, label=torch.tensor([i % 10, 3, 7, (2 * i) % 10]), image_name=["i"] * 4)
               for i in range(4)]
    batches[1]["events_voxel_grid"][2, 3, 100, 100] = INF        # one +inf cell in one sample of batch 1
    return batches


def _ft_run(clip, graph, skip):
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, make_args
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    ops.set_compute_dtype(torch.float32)
    a = make_args(phase="finetune_cls", model_size="small", backbone_type="vit", num_classes=10, mask_ratio=0.0, device="cuda",
                  dataset_type="n-caltech101", clip_grad=clip, smoothing=0.1, drop_path_rate=0.0, drop_rate=0.0)
    # (no warm-up epoch, unlike the clip test: its schedule gives the very first step lr = 0, and a step that cannot move a weight
    # cannot show that the weights "changed across every other step")
    a.epochs, a.warmup_epochs, a.lr, a.min_lr, a.graph_step = 4, 0, 1e-3, 1e-6, graph
    a.prefetch_to_device = False         # the recording loader reads the state step i left when the loop asks for batch i + 1
    if skip:
        a.skip_nonfinite = True
    m = ft.finetune_cls_hub_model_small_patch16(a)
    det_fill_module_(m)
    m = m.cuda()
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, 0.05, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
    loader = _GuardRecordingLoader(_ft_batches(), _watched(m), opt)
    stats, logs = [], []
    for ep in range(2):
        loader.log = []
        stats.append(ft_train_one_epoch(a, m, loader, opt, ep, NativeScalerWithGradNormCount()))
        logs.append(loader.log)
    assert opt.skip_nonfinite is False and opt.max_grad_norm is None        # the loop leaves the caller's optimizer as it found it
    return m, opt, stats, logs, getattr(m, "_evp_auto_executor", (None, None))[1]


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("clip", [5, None], ids=["clip5", "noclip"])
def test_guarded_finetune_epochs_skip_the_poisoned_batch_and_stay_finite(graph, clip):
    """Set-up of test_gpu_grad_clip.py::_ft_run (ViT-Small hub, f32, det_fill_module_, four batches of four, drop rates 0) with one
    +inf cell in one sample of batch 1 and args.skip_nonfinite: the watched weights are bit-identical across the poisoned step and
    changed across every other, guard_state reads {1, 1, 1} behind it, then {0, 1, 2}, ...; after two epochs every parameter is
    finite and each epoch's dict reports skipped_steps == 1. The epoch's loss_cls is non-finite -- the poisoned batch's loss is
    metered as it is, as in the reference: the guard protects the weights, not the log."""
    m, opt, stats, logs, ex = _ft_run(clip, graph, True)
    if graph:
        assert ex.note.startswith("hip-graph") and ex.eager_fallbacks == 0, (ex.note, ex.eager_fallbacks)
        assert ex.guard_state is opt.guard_state
    else:
        assert ex is None
    applied, skipped = _check_log(logs[0], 1, 0, 0)
    assert logs[0][2][1] == [1, 1, 1] and logs[0][3][1] == [0, 1, 2]
    assert _check_log(logs[1], 1, applied, skipped) == (6, 2)
    for st in stats:
        assert st["skipped_steps"] == 1 and not math.isfinite(st["loss_cls"]), st
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert opt.skipped_steps() == 2 and {float(st["step"]) for st in opt.state_dict()["state"].values()} == {6.0}


def test_unguarded_finetune_epochs_end_with_non_finite_weights():
    """The same run with the option off: the poison reaches the weights, and the dict is today's (no skipped_steps key)."""
    m, opt, stats, logs, ex = _ft_run(5, True, False)
    assert ex.note.startswith("hip-graph") and ex.guard_state is None
    assert all("skipped_steps" not in st and sorted(st) == ["loss_cls", "lr"] for st in stats)
    assert not all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_guarded_masked_modeling_epoch_skips_the_poisoned_batch():
    """pr_rec_one_epoch on the tiny hub (64 x 64, f32, set-up of test_gpu_epoch_loop.py), captured, args.skip_nonfinite, one +inf cell
    per patch of one sample of batch 1 of four: same assertions on the weights and the counter."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.pretrain import pr_hub_model as hub
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, det_normalish, make_args
    from eventpretrain_amd.trainer.pretrain.pr_trainer import pr_rec_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    ops.set_compute_dtype(torch.float32)
    batches = [dict(events_voxel_grid=det_normalish(f"loop.voxels.{s}", (2, 5, 64, 64)) * 0.5, sub_frame=det_normalish(f"loop.sub_frame.{s}", (2, 1, 64, 64)),
                    image_name=[f"s{s}"] * 2) for s in range(4)]
    # (the encoder sees the half of the patches the mask keeps: one cell in each of the sample's 16 patches, so that whatever the
    # draw, the poison is in a patch that is kept)
    batches[1]["events_voxel_grid"][1, 2, 8::16, 8::16] = INF
    a = make_args(model_size="tiny", pr_phase="rec", patch_size=16, device="cuda", input_size=64, print_freq=2, log_freq=3)
    a.batch_size, a.epochs, a.warmup_epochs, a.lr, a.min_lr = 2, 4, 0, 1e-3, 1e-6      # (no warm-up: the first step's lr is not 0)
    a.prefetch_to_device, a.skip_nonfinite = False, True
    m = hub.pretrain_hub_model_tiny_patch16_64(a, emb_frames_dim=512, queue_length=8, T=0.07)
    det_fill_module_(m)
    m = m.cuda().train()
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, a.weight_decay, layer_decay=1), lr=a.lr, betas=(0.9, 0.95))
    loader = _GuardRecordingLoader(batches, _watched(m), opt)
    torch.manual_seed(11)
    stats = pr_rec_one_epoch(a, m, loader, opt, 0, NativeScalerWithGradNormCount())
    ex = m._evp_auto_executor[1]
    assert ex.note.startswith("hip-graph") and ex.eager_fallbacks == 0, (ex.note, ex.eager_fallbacks)
    assert _check_log(loader.log, 1, 0, 0) == (3, 1)
    assert stats["skipped_steps"] == 1 and not math.isfinite(stats["reconstruct_loss"])
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ------------------------------------------------------------------------------------------------- 4. two ranks on one card
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_guarded_finetune_steps(tmp_path):
    """Two ranks on this card (gloo, started as tests/dp_clip_worker.py is), ViT-Small fine-tune hub in f32, three captured steps, one
    +inf cell in RANK 1's batch of step 1 only: the NaN reaches rank 0 through the SUM, both ranks report guard_state {1, 1, ...} for
    that step, their weights are bit-identical to their own pre-step clones and to each other's checksums, and the update is the
    single launch behind the last all-reduce."""
    out = tmp_path / "dpguard.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dp_guard_worker.py"), "--out", str(out), "--steps", "3"]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    ranks = json.load(open(out))
    assert len(ranks) == 2
    for g in ranks:
        print(g["note"], g["guards"], g["unchanged"], g["losses"])
        assert g["note"].startswith("hip-graph") and "hip-graph (skip on non-finite gradients + AdamW)" in g["note"], g["note"]
        assert not g["parts"] and "AdamW per reduced buffer" not in g["note"]
        assert [x[:3] for x in g["guards"]] == [[0, 0, 1], [1, 1, 1], [0, 1, 2]], g["guards"]
        assert g["unchanged"] == [False, True, False]
        assert g["ranks_equal"] and g["finite"] and abs(g["grad_scale"] - 0.5) < 1e-12 and g["skip_after"] is False
        assert g["applied"] == 2 and g["skipped"] == 1
    assert math.isfinite(ranks[0]["losses"][1]) and not math.isfinite(ranks[1]["losses"][1])      # the poison is rank 1's alone

"""Gradient clipping on the device (reference utils/misc.py:289-290, the fine-tune default --clip_grad 5): evp_grad_clip_multi against
the oracle, FusedAdamW(max_grad_norm) against clip_grad_norm_ + torch.optim.AdamW, and the clipped fine-tune recipe running as a
captured HIP graph -- one rank and two."""
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


def _tables(grads):
    numel = np.array([g.numel() for g in grads], dtype=np.int64)
    ct = np.concatenate([np.full((int(n) + CHUNK - 1) // CHUNK, t, dtype=np.int32) for t, n in enumerate(numel)])
    co = np.concatenate([np.arange(0, int(n), CHUNK, dtype=np.int64) for n in numel])
    dev = grads[0].device
    return dict(ptrs=torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64, device=dev), numel=torch.from_numpy(numel).to(dev),
                ct=torch.from_numpy(ct).to(dev), co=torch.from_numpy(co).to(dev), n=int(ct.shape[0]),
                ws=torch.empty(int(ct.shape[0]), dtype=torch.float32, device=dev))


def _clip(T, max_norm, hyper, out):
    from eventpretrain_amd._lib import call, stream_ptr
    call("evp_grad_clip_multi", T["ptrs"].data_ptr(), T["numel"].data_ptr(), T["ct"].data_ptr(), T["co"].data_ptr(), T["n"], CHUNK,
         T["ws"].data_ptr(), float(max_norm), hyper.data_ptr(), out.data_ptr(), stream_ptr())


def test_clip_kernel_matches_the_oracle_and_is_reproducible():
    """Awkward sizes (1, 3, one chunk -1 / exactly / +1, a few million), several tensors, views that start 4 and 12 bytes off a
    16-byte boundary. out[0] against oracle.grad_norm in float64 (1e-5 rel, as the scaler test); out[1] and the scaled hyper[2] equal
    oracle.clip_coef evaluated on the returned float norm, rounded to float once; two launches give the same bits."""
    from oracle import model_oracle as mo
    g = torch.Generator().manual_seed(5)
    sizes = (1, 3, 16383, 16384, 16385, 3_000_001)
    host = [torch.randn(n, generator=g) * (0.3 + 0.1 * i) for i, n in enumerate(sizes)]
    base1, base3 = torch.randn(50_010, generator=g), torch.randn(40_000, generator=g)
    dev = [h.cuda() for h in host]
    b1, b3 = base1.cuda(), base3.cuda()
    v1, v3 = b1[1:50_002], b3[3:3 + 16_385]
    assert v1.data_ptr() % 16 == 4 and v3.data_ptr() % 16 == 12 and v1.is_contiguous()
    sets = {"all": (dev + [v1, v3], host + [base1[1:50_002], base3[3:3 + 16_385]]),
            "tiny": (dev[:2], host[:2]), "views": ([v3, v1], [base3[3:3 + 16_385], base1[1:50_002]]), "big": (dev[5:], host[5:])}
    for tag, (gd, gh) in sets.items():
        T = _tables(gd)
        total = float(mo.grad_norm([h.double() for h in gh]))
        for gs in (1.0, 0.5):
            for max_norm in (0.37 * total * gs, 2.5 * total * gs):
                outs = []
                for _ in range(2):
                    hyper = torch.tensor([0.1, 0.2, gs, 1.0], dtype=torch.float32, device="cuda")
                    out = torch.full((2,), -1.0, device="cuda")
                    _clip(T, max_norm, hyper, out)
                    torch.cuda.synchronize()
                    outs.append((out.cpu().numpy().copy(), hyper.cpu().numpy().copy()))
                (o, h), (o2, h2) = outs
                assert o.tobytes() == o2.tobytes() and h.tobytes() == h2.tobytes(), (tag, gs, max_norm)
                assert abs(float(o[0]) - total * gs) <= 1e-5 * total * gs, (tag, gs, float(o[0]), total * gs)
                coef = mo.clip_coef(float(o[0]), max_norm)
                assert (coef < 1.0) == (max_norm < total * gs)
                assert o[1] == np.float32(coef), (tag, gs, o[1], coef)
                assert h[2] == np.float32(np.float64(np.float32(gs)) * coef), (tag, gs, h[2], coef)
                assert h[0] == np.float32(0.1) and h[1] == np.float32(0.2) and h[3] == 1.0


def test_clipped_update_matches_clip_grad_norm_and_torch_adamw():
    """FusedAdamW(max_grad_norm=c).step() against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (what reference utils/misc.py:289-290
    calls) on the CPU, fed the gradients the GPU produced; rtol 1e-5 / atol 1e-6 as the scaler test. Two steps, so the second one
    starts from non-zero moments and a fresh gradient scale."""
    from eventpretrain_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(23)
    shapes = [(37, 19), (129,), (5, 4100), (1,)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    x = torch.randn(8, 19, generator=g)
    for clip in (0.05, 1e6):
        ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        ref = [torch.nn.Parameter(t.clone()) for t in init]
        groups = lambda q: [{"params": [q[0], q[2]], "weight_decay": 0.05}, {"params": [q[1], q[3]], "weight_decay": 0.0}]
        opt = FusedAdamW(groups(ps), lr=1e-2, betas=(0.9, 0.95), max_grad_norm=clip)
        ropt = torch.optim.AdamW(groups(ref), lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
        for step in range(2):
            opt.zero_grad(set_to_none=True)
            loss = (torch.nn.functional.linear(x.cuda(), ps[0]) ** 2).mean() + (ps[1] ** 2).sum() * 0.01 + (ps[2].sin() * (1 + step)).sum() * 1e-3 + ps[3].sum()
            loss.backward()
            for r, p in zip(ref, ps):
                r.grad = p.grad.detach().cpu().clone()
            opt.step()
            total = torch.nn.utils.clip_grad_norm_(ref, clip)
            ropt.step()
            norm, coef = [float(v) for v in opt.last_grad_norm.cpu()]
            assert abs(norm - float(total)) <= 1e-5 * float(total), (clip, step)
            assert (coef < 1.0) == (clip < 1.0)
            for r, p in zip(ref, ps):
                assert torch.allclose(p.detach().cpu(), r.detach(), rtol=1e-5, atol=1e-6), (clip, step, tuple(p.shape))
        assert opt.grad_scale == 1.0 and opt.max_grad_norm == clip
    # the attribute is per launch: switched off, the same optimizer does not clip
    opt.max_grad_norm = None
    before = opt.last_grad_norm.clone()
    opt.step()
    assert torch.equal(opt.last_grad_norm, before)


class _RecordingLoader:
    """A list of batches that notes, each time the loop comes back for the next batch (and at the end of the epoch), the {norm, coef}
    the step before left on the device: the executor's `grad_norm` where the loop built one, else the optimizer's `last_grad_norm`
    (the same tensor)."""

    def __init__(self, batches, model, opt):
        self.batches, self.model, self.opt, self.log = batches, model, opt, []

    def __len__(self):
        return len(self.batches)

    def _note(self):
        ex = getattr(self.model, "_evp_auto_executor", (None, None))[1]
        t = ex.grad_norm if ex is not None else self.opt.last_grad_norm
        self.log.append([float(v) for v in t.cpu()])

    def __iter__(self):
        for i, b in enumerate(self.batches):
            if i:
                self._note()
            yield b
        self._note()


def _ft_run(clip, graph, batches):
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_fill_module_, make_args
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    from helpers import checksums
    ops.set_compute_dtype(torch.float32)
    a = make_args(phase="finetune_cls", model_size="small", backbone_type="vit", num_classes=10, mask_ratio=0.0, device="cuda",
                  dataset_type="n-caltech101", clip_grad=clip, smoothing=0.1, drop_path_rate=0.0, drop_rate=0.0)
    a.epochs, a.warmup_epochs, a.lr, a.min_lr, a.graph_step = 4, 1, 1e-3, 1e-6, graph
    a.prefetch_to_device = False         # the recording loader reads the norm of step i when the loop asks for batch i + 1
    m = ft.finetune_cls_hub_model_small_patch16(a)
    det_fill_module_(m)
    m = m.cuda()
    opt = FusedAdamW(lrd.param_groups_lrd(a, m, 0.05, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
    loader = _RecordingLoader(batches, m, opt)
    losses = [ft_train_one_epoch(a, m, loader, opt, ep, NativeScalerWithGradNormCount())["loss_cls"] for ep in range(2)]
    ex = getattr(m, "_evp_auto_executor", (None, None))[1]
    assert opt.max_grad_norm is None and opt.grad_scale == 1.0        # the loop leaves the caller's optimizer as it found it
    return dict(losses=losses, norms=loader.log, note=None if ex is None else ex.note,
                wsum={k: checksums(p)[2] for k, p in m.named_parameters()}, scale={k: p.detach().abs().sum().item() for k, p in m.named_parameters()})


def test_clipped_finetune_recipe_runs_captured_and_follows_the_eager_loop():
    """The reference's fine-tune default clips (main_finetune_cls.py:145 --clip_grad 5). Set-up of part (a) of
    test_gpu_round4.py::test_finetune_epoch_runs_captured_and_follows_the_eager_loop (ViT-Small hub, det_fill_module_, f32, four
    batches of four, two epochs) with clip_grad set: the loop builds its executor and the step is ONE HIP graph. The clip value comes
    from the recorded norms of the same trajectory run with a clip that never engages (1e9): midway between the two norms around the
    median, so some steps clip and some do not, and no norm sits on the threshold. Captured against eager (graph_step=False) with the
    tolerances of the unclipped pair: losses rel 2e-5, worst weight-checksum deviation 5e-6. The clipped trajectory differs from the
    unclipped one (a coefficient computed but not applied would not).
    Measured on an MI355X: unclipped norms 16.8 .. 58.3, clip 29.196, four of the eight steps clip in both runs; clipped against
    unclipped 3.9e-3. The worst captured / eager weight-checksum deviation (bound 5e-6, always on a qkv bias) is not the same from
    run to run, because the f32 backward itself is not (two EAGER runs of this recipe differ by 1.4e-6 .. 2.4e-6): five runs of
    this test gave 1.8e-6, 5.1e-6 (a miss), 2.0e-6, 1.4e-6, 0.5e-6; the UNCLIPPED pair the bound comes from gave 1.7e-6, 2.7e-6,
    4.4e-6 in the same session. The clip kernel adds none of it (its output is bit-identical for identical gradients)."""
    from eventpretrain_amd.testing import det_normalish
    batches = [dict(events_voxel_grid=det_normalish(f"ft.x.{i}", (4, 5, 224, 224)) * 0.5, label=torch.tensor([i % 10, 3, 7, (2 * i) % 10]), image_name=["i"] * 4)
               for i in range(4)]
    free = _ft_run(1e9, True, batches)
    assert free["note"] == "hip-graph"
    assert len(free["norms"]) == 8 and all(n[1] == 1.0 and n[0] > 0 and math.isfinite(n[0]) for n in free["norms"]), free["norms"]
    srt = sorted(n[0] for n in free["norms"])
    clip = 0.5 * (srt[3] + srt[4])
    print("unclipped norms", srt, "-> clip_grad", clip)
    assert srt[4] - srt[3] > 1e-3 * clip, ("the two norms around the median are too close to put a threshold between them", srt)
    res = {mode: _ft_run(clip, mode == "graph", batches) for mode in ("eager", "graph")}
    assert res["graph"]["note"] == "hip-graph" and res["eager"]["note"] is None
    for mode, r in res.items():
        print(mode, "losses", r["losses"], "norms/coefs", r["norms"])
        coefs = [n[1] for n in r["norms"]]
        assert len(coefs) == 8 and any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), (mode, r["norms"])
        # no step of either run sits on the threshold: the captured / eager difference (1e-5 class) cannot flip a branch
        assert all(abs(n[0] - clip) > 1e-4 * clip for n in r["norms"]), (mode, clip, r["norms"])
        assert all((n[1] < 1.0) == (n[0] > clip) for n in r["norms"])
    assert [n[1] < 1.0 for n in res["graph"]["norms"]] == [n[1] < 1.0 for n in res["eager"]["norms"]]
    assert res["graph"]["losses"] == pytest.approx(res["eager"]["losses"], rel=2e-5)
    worst = max(abs(res["graph"]["wsum"][k] - v) / max(res["eager"]["scale"][k], 1e-6) for k, v in res["eager"]["wsum"].items())
    print("worst weight-checksum deviation captured vs eager", worst)
    assert worst <= 5e-6, worst
    moved = max(abs(res["graph"]["wsum"][k] - v) / max(free["scale"][k], 1e-6) for k, v in free["wsum"].items())
    print("clipped vs unclipped weight-checksum deviation", moved)
    assert moved > 1e-4, moved        # 20x the captured-vs-eager bound: the coefficient reached the update


def test_swin_tiny_clipped_bf16_step_is_captured():
    """Swin-T fine-tune hub, bf16, the reference's drop_path_rate 0.1 and clip_grad 5: captured, finite, a positive norm."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_cls import ft_cls_hub_model as ft
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_normalish, make_args
    from eventpretrain_amd.trainer.finetune_cls.ft_cls_trainer import ft_train_one_epoch
    from eventpretrain_amd.utils import lr_decay as lrd
    from eventpretrain_amd.utils.misc import NativeScalerWithGradNormCount
    ops.set_compute_dtype(torch.bfloat16)
    try:
        a = make_args(phase="finetune_cls", model_size="tiny", backbone_type="swin", num_classes=10, mask_ratio=0.0, device="cuda",
                      dataset_type="n-caltech101", clip_grad=5, smoothing=0.1, drop_path_rate=0.1, drop_rate=0.0)
        a.epochs, a.warmup_epochs, a.lr, a.min_lr = 4, 0, 1e-3, 1e-6
        torch.manual_seed(0)
        m = ft.finetune_cls_hub_model_swin_tiny_window7(a).cuda()
        opt = FusedAdamW(lrd.param_groups_lrd(a, m, 0.05, layer_decay=0.75), lr=a.lr, betas=(0.9, 0.999))
        x = det_normalish("ft.voxels", (2, 5, 224, 224)) * 0.5
        loader = [dict(events_voxel_grid=x, label=torch.tensor([3, 7]), image_name=["a", "b"])]
        st = ft_train_one_epoch(a, m, loader, opt, 0, NativeScalerWithGradNormCount())
        ex = m._evp_auto_executor[1]
        assert ex.note == "hip-graph", ex.note
        norm, coef = [float(v) for v in ex.grad_norm.cpu()]
        assert math.isfinite(st["loss_cls"]) and math.isfinite(norm) and norm > 0.0 and 0.0 < coef <= 1.0
        assert coef == np.float32(min(1.0, 5.0 / (norm + 1e-6)))
        assert all(torch.isfinite(p).all() for p in m.parameters())
    finally:
        ops.set_compute_dtype(torch.float32)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_clipped_finetune_steps(tmp_path):
    """Two ranks on this card (gloo, started as tests/dp_cuda_worker.py is), different batches per rank, ViT-Small fine-tune hub in
    f32, four steps with a clip value between the recorded norms: the captured data-parallel step takes the non-parts order (the
    global norm needs every buffer reduced before any update) and follows the eager data-parallel step; both ranks report the same
    norms and end with the same weights; the norm of step 0 is the oracle norm of the AVERAGE of the two ranks' gradients (computed
    here in one process; 2e-5 rel -- the bound the loss of a captured step is held to against the eager one, since the two
    processes sum the same f32 products in different orders)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dp_clip_worker as w
    from oracle import model_oracle as mo
    out = tmp_path / "dpclip.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dp_clip_worker.py"), "--out", str(out), "--steps", "4"]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    got = json.load(open(out))
    e, g, clip = got["eager"], got["graph"], got["clip"]
    print("clip", clip, "free norms", got["free"]["norms"], "eager", e["norms"], "graph", g["norms"], g["note"])
    assert g["note"].startswith("hip-graph") and "hip-graph (clip to the norm of the mean gradient + AdamW)" in g["note"], g["note"]
    assert not g["parts"] and "AdamW per reduced buffer" not in g["note"]
    for r_ in (e, g, got["free"]):
        assert r_["ranks_equal"] and abs(r_["grad_scale"] - 0.5) < 1e-12 and r_["max_grad_norm_after"] is None
    assert all(n[1] == 1.0 for n in got["free"]["norms"])
    for r_ in (e, g):
        coefs = [n[1] for n in r_["norms"]]
        assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), r_["norms"]
        assert all(abs(n[0] - clip) > 1e-4 * clip for n in r_["norms"]), (clip, r_["norms"])
    assert g["losses"] == pytest.approx(e["losses"], rel=2e-5)
    assert [n[0] for n in g["norms"]] == pytest.approx([n[0] for n in e["norms"]], rel=2e-5)
    worst = max(abs(g["wsums"][k] - v) / max(e["scale"][k], 1e-6) for k, v in e["wsums"].items())
    assert worst <= 5e-6, worst
    # step 0: the norm of the mean gradient over both ranks' batches
    a, m, opt = w.build()
    grads = []
    for rank in range(2):
        x, y = w.batch_of(rank, 0)
        m.zero_grad(set_to_none=True)
        w.forward(m, x.cuda(), y.cuda())[0].backward()
        from eventpretrain_amd import ops
        ops.flush_deferred_grads()
        torch.cuda.synchronize()
        grads.append({k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None})
    total = float(mo.grad_norm([0.5 * (grads[0][k] + grads[1][k]) for k in grads[0]]))
    for r_ in (got["free"], e, g):
        assert abs(r_["norms"][0][0] - total) <= 2e-5 * total, (r_["norms"][0], total)

"""The bf16 forward and backward of whole small Swin and ConvViT backbones and of the fine-tuning step (FtClsHubModel.forward +
CrossEntropyFn) against the float64 run of the CPU oracle, tensor by tensor: the output, the stage taps, pred and loss, the returned
attention map and every parameter gradient on its own; mask, ids_restore and the Swin stage coordinates equal. The bound of every tensor
is the error of the oracle under CPU autocast to bf16 against the same truth (tests/block_truth.py: whole tensor, sub-blocks, scale; one
constant, FACTOR = 3). Cases and references: tests/backbone_truth.py; what the comparator accepts and rejects on them:
tests/test_backbone_truth_host.py.

Each test prints the worst ratio e_hip / e_ref over all tensors and gates (bound: 3) and the tensor it belongs to; the docstrings record
the figures of an MI355X run."""
import contextlib
import copy

import pytest
import torch

import backbone_truth as kt
import block_truth as bt

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _bf16(fused_attention=True, window_mfma=True, grad_side=True, deferred=True):
    from eventpretrain_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    ops.set_fused_attention(fused_attention)
    ops.set_window_mfma(window_mfma)
    ops.set_grad_side(grad_side)
    ops.set_deferred_grads(deferred)
    try:
        yield ops
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.set_fused_attention(True)
        ops.set_window_mfma(True)
        ops.set_grad_side(True)
        ops.set_deferred_grads(True)


def _hip(name, static_plan=False, **switches):
    """The case's module on the device in bf16 mode: -> {tensor name: tensor}, named as the reference names them."""
    c = kt.make_case(name)
    ref = kt.reference(name)
    mod = copy.deepcopy(c["module"]).cuda().train()
    x = c["x"].cuda()
    got = {}
    with _bf16(**switches) as ops:
        if c["kind"] == "masked":
            noise = c["noise"]
            if static_plan:
                prepare = mod.enable_static_plan("cuda")
                assert prepare(noise) is True
                noise = noise.cuda()
            elif c["backbone"] != "swin":
                noise = noise.cuda()          # Swin takes the host noise: the window plan is host work
            out = mod(x, mask=True, noise=noise)
            if c["backbone"] == "swin":
                taps, emb, coords, (mask, ids_restore, got["attn"]) = out[0:4], out[4], out[5:9], out[9:12]
                for i, co in enumerate(coords):
                    assert torch.equal(co.cpu().reshape(-1, 2).long(), ref.T[f"_coords{i + 1}"]), f"stage {i + 1} coordinates"
                if static_plan:
                    assert mod._static is not None and mod._static.loads == 1 and mod._static.overflows == 0
            else:
                taps, emb, mask, ids_restore = out[0:2], out[2], out[3], out[4]
            assert torch.equal(mask.cpu(), ref.T["_mask"]) and torch.equal(ids_restore.cpu(), ref.T["_ids_restore"])
            got["act:emb_lh"] = emb
            loss = kt.quadratic_loss(emb.float(), c["w"].cuda())
        else:
            out = mod(x)
            taps, emb, pred, got["attn"] = out[:-3], out[-3], out[-2], out[-1]
            loss = ops.CrossEntropyFn.apply(pred, c["label"].cuda(), kt.SMOOTHING)
            got["act:emb_h"], got["pred"], got["loss"] = emb, pred, loss
        got.update({f"act:l{i + 1}": kt.tokens(t) for i, t in enumerate(taps)})
        loss.backward()
        ops.flush_deferred_grads()
        torch.cuda.synchronize()
    for k, p in mod.named_parameters():
        if p.grad is not None:
            got["grad:" + k] = p.grad
    return {k: v.detach().float().cpu() for k, v in got.items()}


def _gate(name, got, what, factors=None):
    ref = kt.reference(name)
    assert sorted(got) == sorted(ref.tensors), sorted(set(got) ^ set(ref.tensors))
    fails, worst, table = kt.compare_all(name, got, factors=factors)
    print(f"\n[{what}] worst e_hip / e_ref = {worst[0]:.2f} at {worst[1]} (bound {bt.FACTOR:g})\n{table}")
    assert not fails, "\n".join(fails)


SWIN_RUNS = {
    "defaults": {},
    "lds_window_kernels": dict(window_mfma=False),
    "undeferred": dict(deferred=False),
    "side_off": dict(grad_side=False),
    "static_plan": dict(static_plan=True),
}


@pytest.mark.parametrize("run", list(SWIN_RUNS))
def test_swin_masked_bf16_against_float64_truth(run):
    """The small Swin (widths 32 - 256, 1 - 8 heads, input 224, B = 2), masked forward with feature fusion + backward of a quadratic loss
    on emb_lh: PatchProjFn at the visible tokens, grouping mode with padding (1536, 384 tokens) and masking mode (96, 24), three shifted
    stages, PatchMerging x 3, SwinFuseConvFn x 3, AddFn and the three-input LayerNormFn; LayerNorm at D = 32 and 64, GEMMs at N = 96.
    defaults; the f32 LDS window kernels; deferred gradients off; the LayerNorm side data off; the static plan (fixed-shape tables with
    fully masked padding groups, noise as a device tensor).
    Measured on an MI355X, worst e_hip / e_ref over all tensors and gates (bound 3): defaults, undeferred, side off and static plan 1.14
    (stage 1 block 1 mlp.fc2.bias, whole), LDS window kernels 1.15 (stage 1 block 1 norm1.bias, whole); emb_lh 0.61, the taps 0.59 -
    0.66, the attention map 0.64. No tensor needed a factor of its own, and no argument check refused the widths 32 and 64."""
    _gate("swin_masked", _hip("swin_masked", **SWIN_RUNS[run]), f"swin_masked {run}")


CONVVIT_RUNS = {"defaults": {}, "unfused_attention": dict(fused_attention=False), "undeferred": dict(deferred=False)}


@pytest.mark.parametrize("run", list(CONVVIT_RUNS))
def test_convvit_masked_bf16_against_float64_truth(run):
    """The small ConvViT (widths 64 / 128 / 192, 6 heads, input 64, B = 3, 8 of 16 tokens kept), masked forward with feature fusion +
    backward of a quadratic loss on emb_lh: PatchEmbedFn, PatchEmbedNHWCFn x 2 (the second at the kept tokens), the keep map at scales 4
    and 2 in the conv blocks, AddPosGatherFn, StridedConvTokensFn x 2, the three-input LayerNormFn.
    Measured on an MI355X, worst e_hip / e_ref (bound 3): defaults and undeferred 0.97 (vit_block.0 qkv.bias, head slice), unfused
    attention 0.93 (vit_block.1 norm1.bias, whole); emb_lh 0.68, the taps 0.63 - 0.65."""
    _gate("convvit_masked", _hip("convvit_masked", **CONVVIT_RUNS[run]), f"convvit_masked {run}")


FT_RUNS = {
    "swin_ft": ("swin_ft", {}),
    "swin_ft_lds_window_kernels": ("swin_ft", dict(window_mfma=False)),
    "convvit_ft": ("convvit_ft", {}),
    "vit_ft": ("vit_ft", {}),
}


@pytest.mark.parametrize("run", list(FT_RUNS))
def test_ft_cls_step_bf16_against_float64_truth(run):
    """FtClsHubModel.forward over the small Swin (dense: 3136 / 784 / 196 / 49 tokens), the small ConvViT and vit_tiny_patch16_64, then
    TokenMeanFn, the head LinearFn with 101 classes and CrossEntropyFn with smoothing 0.1: pred, loss, emb_h, the taps, the attention
    map and every gradient. The loss is measured against the yardstick's loss error pooled over the three cases
    (backbone_truth.loss_yardstick, 1.08e-3).
    Measured on an MI355X, worst e_hip / e_ref (bound 3): swin_ft 1.08 and on the LDS window kernels 1.25 (stage 1 block 1
    norm1.weight, whole), convvit_ft 0.98 (conv_block1.1 depthwise bias, whole), vit_ft 1.32 (vit_block.5 qkv.weight, 128 x 128
    tiles); pred 0.76 - 0.91, the loss 0.04 - 0.33, emb_h 0.61 - 0.83, the attention maps 0.64 - 0.82."""
    name, kw = FT_RUNS[run]
    _gate(name, _hip(name, **kw), run)

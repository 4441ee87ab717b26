"""The bf16 forward and backward of ViTBlockFn, ConvBlockFn, SwinBlockFn and of a whole tiny reconstruction step against the float64
run of the CPU oracle, tensor by tensor: output, dx, every parameter gradient, the returned attention map. The bound of every tensor
is the error of the oracle under CPU autocast to bf16 against the same truth (tests/block_truth.py: whole tensor, sub-blocks, scale;
one constant, FACTOR = 3). The host half (tests/test_block_truth_host.py) shows what the comparator accepts and rejects.

Each test prints, per case, the worst ratio e_hip / e_ref over all tensors and gates (bound: 3) and the tensor it belongs to; the
docstrings record the figures of an MI355X run."""
import contextlib
import copy

import pytest
import torch

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


def _block_drop(ops, c):
    if "u1" not in c:
        return None
    return ops.BlockDrop(c["u1"].cuda(), c["u2"].cuda(), keep_prob=bt.KEEP_PROB, drop=bt.P_DROP, seed=1,
                         masks={k: v.cuda() for k, v in c["masks"].items()})


def _hip(name, want_attn=False, **switches):
    """The case's module on the device in bf16 mode: -> {tensor name: tensor}, named as the reference names them."""
    c = bt.make_case(name)
    mod = copy.deepcopy(c["module"]).cuda().train()
    got = {}
    with _bf16(**switches) as ops:
        rd = _block_drop(ops, c)
        if c["kind"] == "rec":
            out = mod(c["x"].cuda(), c["y"].cuda(), is_rec=True, noise=c["noise"].cuda())
            loss, got["loss"], got["pred"] = out[0], out[0].detach(), out[4].detach()
            ref = bt.reference(name)
            assert torch.equal(out[5].cpu(), ref.T["_mask"]) and torch.equal(out[6].cpu(), ref.T["_ids_restore"])
        else:
            x = c["x"].cuda().requires_grad_(True)
            if c["kind"] == "vit":
                t = x
                for blk in mod:
                    t = blk(t, return_attn=want_attn, block_drop=rd)
                    if want_attn:
                        t, got["attn"] = t
            elif c["kind"] == "conv":
                s = c["spec"]
                coarse = (1.0 - c["keep_coarse"]).reshape(s["B"], -1).contiguous().cuda() if "keep_coarse" in c else None
                t = mod.forward_tokens(x, s["H"], s["W"], coarse, 2 if coarse is not None else 1, block_drop=rd)
            else:
                rel = torch.where(c["blocked"], torch.full_like(c["rel"], -1), c["rel"]).to(torch.int32).cuda()
                t = mod(x, rel, block_drop=rd)
            got["out"] = t.detach()
            loss = (t * c["w"].cuda()).sum()
        loss.backward()
        ops.flush_deferred_grads()
        torch.cuda.synchronize()
    if c["kind"] != "rec":
        got["dx"] = x.grad
    for k, p in mod.named_parameters():
        if p.grad is not None:
            got["grad:" + k] = p.grad
    return {k: v.detach().float().cpu() for k, v in got.items()}


def _gate(name, got, what, factors=None):
    ref = bt.reference(name)
    want = [t for t in ref.tensors if t != "attn" or "attn" in got]
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    fails, worst, table = bt.compare_all(got, ref, heads=bt.heads_of(name), factors=factors, blocks=name != "rec_tiny")
    print(f"\n[{what}] worst e_hip / e_ref = {worst[0]:.2f} at {worst[1]} (bound {bt.FACTOR:g})\n{table}")
    assert not fails, "\n".join(fails)


VIT_RUNS = {
    "a_fused_deferred": ("vit_a", {}),
    "a_fused_undeferred": ("vit_a", dict(deferred=False)),
    "b_head_pairs": ("vit_b", {}),
    "c_unfused": ("vit_a", dict(fused_attention=False)),
    "d_attention_map": ("vit_a", dict(want_attn=True)),
    "e_given_drops": ("vit_e", {}),
    "f_stacked_side_on": ("vit_f", dict(grad_side=True)),
    "f_stacked_side_off": ("vit_f", dict(grad_side=False)),
}


@pytest.mark.parametrize("run", list(VIT_RUNS))
def test_vit_block_bf16_against_float64_truth(run):
    """ViTBlockFn in bf16 mode. a: M = 150 rows (ragged against the 16 / 128-row tiles), N = 50 padded to 64 in the fused attention,
    deferred gradients on and off; b: N = 197, d_h = 32; c: the unfused attention core; d: the returned attention map; e: given
    drop-path draws (one sample dropped per branch) and dropout masks, which switch the side path off and the dropout backward on;
    f: two stacked blocks, the lower consuming the upper's bf16 gradient copy and column-sum partials (side data on) or casting and
    summing itself (off) -- dx and all gradients of BOTH blocks, each setting on its own.
    Measured on an MI355X, worst e_hip / e_ref over all tensors and gates (bound 3): a deferred 1.04 and undeferred 1.04 (norm1.weight,
    whole), b 1.01 (norm2.weight, whole), c 1.00 (qkv.bias, head slice), d 1.04 (norm1.weight, whole; the map itself 0.94), e 1.02
    (norm2.bias, whole), f side on 1.06 and off 1.06 (lower block's norm1.bias, whole)."""
    name, kw = VIT_RUNS[run]
    _gate(name, _hip(name, **kw), f"vit {run}")


@pytest.mark.parametrize("name", list(bt.CONV))
def test_conv_block_bf16_against_float64_truth(name):
    """ConvBlockFn in bf16 mode (bf16 I/O of the depthwise 5 x 5): keep map at scale 2 on 14 x 14, C = 128 on 12 x 20 without a
    mask, given drop-path draws and CMlp dropout masks.
    Measured on an MI355X, worst e_hip / e_ref (bound 3): conv_keep 1.18 (norm2.bias, whole), conv_nomask 0.94 and conv_drops 0.97
    (dx, 16 x 64 tiles)."""
    _gate(name, _hip(name), f"conv {name}")


@pytest.mark.parametrize("name", list(bt.SWIN))
def test_swin_block_bf16_against_float64_truth(name):
    """SwinBlockFn in bf16 mode on the MFMA window kernels, d_h = 32, ~30 % of the pairs blocked: N = 24 (padded to 32) with 3 x 2
    grouped rows, N = 98 (padded to 128) with 2 x 2, given drops; the relative-position bias table's gradient included.
    Measured on an MI355X, worst e_hip / e_ref (bound 3): swin_24 1.15 (norm2.weight, whole), swin_98 1.07 (norm2.bias, whole),
    swin_drops 1.11 (norm1.weight, whole)."""
    _gate(name, _hip(name), f"swin {name}")


def test_rec_tiny_step_bf16_against_float64_truth():
    """The whole tiny reconstruction step (input 64, patch 16, dim 192, depth 12 + decoder, B = 5) in bf16 mode against mo.rec_step
    in float64: loss, pred and EVERY parameter gradient on its own (whole-tensor and scale gates); mask and ids_restore equal.
    Measured on an MI355X, worst e_hip / e_ref (bound 3): 1.19 (decoder block 2 norm2.weight, whole); the loss 0.84, pred 0.90."""
    _gate("rec_tiny", _hip("rec_tiny"), "rec_tiny")

#!/usr/bin/env python3
"""Fixtures of the dense-prediction heads, made by the REFERENCE's own classes (model/finetune_dense/ft_dense_decoder.py,
ft_dense_hub_model.py) in float64 on the CPU -> tests/golden/ft_dense_heads.npz, tests/golden/ft_dense_vit_small.npz.

Runs where a checkout of the reference is at hand (EVP_REFERENCE=<its root>), never on the GPU machine. Nothing of the reference is
copied: the fixtures hold arrays and lists of names. The reference modules get the weights eventpretrain_amd.testing.det_fill_module_
gives the same-named module here; the inputs are re-made by the tests (tests/dense_truth.py: case_inputs).

ft_dense_heads.npz, per case "<head>.<shape>.<train|eval>" (dense_truth.FIXTURE_CASES): the prediction, the input gradients, every
parameter gradient and the running statistics after the call, dropout_ratio = 0, in float64. A tensor of more than dense_truth.BIG
elements (the 3x3 weight gradients) is held as four float64 checksums plus every SAMPLE-th element, to keep the file small.
ft_dense_vit_small.npz: FtDenseHubModel (ViT-Small, finetune_semseg, 11 classes) on the input of tests/test_gpu_finetune.py."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_truth as dt  # noqa: E402
from eventpretrain_amd.testing import det_fill_module_, det_normalish, make_args  # noqa: E402
from oracle import gen_golden  # noqa: E402  (the timm stand-in and the reference's import path)

OUT = os.path.join(ROOT, "tests", "golden")


def ref_head(head):
    from model.finetune_dense.ft_dense_decoder import FCNHead, UPerHead
    s = dt.HEADS[head]
    a = make_args(sample_mode="bilinear")
    if s["kind"] == "uper":
        m = UPerHead(args=a, in_channels=s["in_channels"], channels=s["channels"], out_channels=s["out_channels"], in_index=[0, 1, 2, 3],
                     pool_scales=dt.POOL_SCALES, dropout_ratio=0)
    else:
        m = FCNHead(args=a, in_channels=s["in_channels"], channels=s["channels"], out_channels=s["out_channels"], in_index=2,
                    num_convs=s["num_convs"], kernel_size=3, concat_input=s["concat_input"], dropout_ratio=0)
    ours = dt.build_head(head)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ours.state_dict().items()}, head
    det_fill_module_(m)
    return m.double()


def gen_heads():
    out, cases = {}, []
    for head, shape, train in dt.FIXTURE_CASES:
        B, H, W = dt.SHAPES[shape]
        m = ref_head(head).train(train)
        xs_tok, w, _ = dt.case_inputs(head, shape)
        used = range(4) if dt.HEADS[head]["kind"] == "uper" else (2,)
        toks = [t.double().requires_grad_(i in used) for i, t in enumerate(xs_tok)]
        pred = m([dt.tokens_to_frame(t, H, W) for t in toks])
        pred_tok = pred.permute(0, 2, 3, 1).reshape(B * H * W, -1)
        (pred_tok * w.double()).sum().backward()
        res = {"act:out": pred_tok}
        res.update({f"act:dx{i}": toks[i].grad.reshape(B * H * W, -1) for i in used})
        res.update({"grad:" + k: p.grad for k, p in m.named_parameters()})
        res.update({"stat:" + k: v for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))})
        tag = f"{head}.{shape}.{'train' if train else 'eval'}"
        for k, v in res.items():
            v = v.detach().double()
            if v.numel() > dt.BIG:
                out[f"{tag}|{k}|sample"] = v.flatten()[::dt.SAMPLE].numpy()
                out[f"{tag}|{k}|sums"] = dt.checksums(v).numpy()
            else:
                out[f"{tag}|{k}"] = v.numpy()
        cases.append(dict(tag=tag, tensors=list(res)))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(OUT, "ft_dense_heads.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def gen_hub():
    from model.finetune_dense.ft_dense_hub_model import finetune_dense_hub_model_small_patch16
    a = make_args(phase="finetune_semseg", model_size="small", backbone_type="vit", num_classes=11, mask_ratio=0.0, sample_mode="bilinear")
    hub = finetune_dense_hub_model_small_patch16(a)
    for head in (hub.decode_head, hub.auxiliary_head):
        head.dropout = None          # dropout_ratio forced to 0
    det_fill_module_(hub)
    hub.train(True)
    x = det_normalish("ft.voxels", (2, 5, 224, 224)) * 0.5
    res = hub(x)
    dec, aux = res[-2], res[-1]
    w1, w2 = dt.hub_loss_weights(dec.shape)
    ((dec * w1).sum() + 0.4 * (aux * w2).sum()).backward()
    out = dict(decode_predict=dec.detach(), aux_predict=aux.detach())
    names, gn = [], []
    for n, p in hub.named_parameters():
        if p.grad is not None:
            names.append(n)
            gn.append(p.grad.double().norm().item())
    out["grad_names"], out["grad_norms"] = np.array(json.dumps(names)), np.array(gn)
    for k in ("decode_head.conv_dense.weight", "decode_head.conv_dense.bias", "auxiliary_head.conv_dense.weight", "auxiliary_head.conv_dense.bias"):
        out["grad::" + k] = dict(hub.named_parameters())[k].grad.detach().numpy()
    out["state_keys"] = np.array(json.dumps({k: list(v.shape) for k, v in hub.state_dict().items()}))
    path = os.path.join(OUT, "ft_dense_vit_small.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    if not os.path.isdir(gen_golden.REF):
        raise SystemExit("set EVP_REFERENCE to the root of a checkout of the reference")
    gen_golden._ref()
    torch.set_num_threads(1)
    which = sys.argv[1:] or ["heads", "hub"]
    if "heads" in which:
        gen_heads()
    if "hub" in which:
        gen_hub()

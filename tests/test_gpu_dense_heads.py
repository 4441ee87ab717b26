"""The dense-prediction heads on the GPU (csrc/dense.hip, ops.ConvBNFn & co., model/finetune_dense) against tests/dense_truth.py, whose
float64 restatement tests/test_dense_truth_host.py pins to the reference's own classes (tests/golden/ft_dense_heads.npz).

float32 rule (the project's): 1e-4 relative per tensor and allclose(atol = 1e-6 |ref|_inf, rtol = 1e-4) elementwise. bf16: the three gates
of block_truth.compare with FACTOR = 3 against the autocast yardstick computed at run time."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_truth as dtr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, BF16 = 0, 1


@pytest.fixture(autouse=True)
def _f32_after():
    yield
    from eventpretrain_amd import ops
    ops.set_compute_dtype(torch.float32)


def close_f32(got, ref, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    scale = ref.abs().max().item()
    assert (got - ref).norm().item() <= 1e-4 * ref.norm().item(), (what, dtr.rel_err(got, ref))
    assert torch.allclose(got, ref, atol=1e-6 * scale, rtol=1e-4), (what, (got - ref).abs().max().item(), scale)


def call(name, *args):
    from eventpretrain_amd import _lib
    return _lib.call(name, *args, _lib.stream_ptr())


def tok(x):
    """(B, C, H, W) -> contiguous token-major [B*H*W, C]."""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------- 1. kernels, f32
@pytest.mark.parametrize("B,H,W,C", [(2, 14, 14, 40), (3, 6, 10, 8), (1, 1, 1, 8), (2, 3, 70, 72)])
def test_im2col_and_col2im(B, H, W, C):
    x = randn(B, C, H, W, seed=1)
    # the input as a channel slice of a wider map (ld = C + 8), the way a concat buffer hands it over
    wide = torch.zeros(B * H * W, C + 8)
    wide[:, 8:] = tok(x)
    wide = wide.cuda()
    cols = torch.full((B * H * W, C * 9), float("nan"), device="cuda")
    call("evp_im2col3x3", wide.data_ptr() + 8 * 4, F32, C + 8, B, H, W, C, cols.data_ptr(), F32, C * 9)
    ref = dtr.im2col3x3(x.double())
    assert torch.equal(cols.cpu().double(), ref)                 # a gather: exact
    g = randn(B * H * W, C * 9, seed=2)
    xr = x.double().requires_grad_(True)
    (dtr.im2col3x3(xr) * g.double()).sum().backward()
    out = torch.full((B * H * W, C + 8), float("nan"), device="cuda")
    gd = g.cuda()
    call("evp_col2im3x3", gd.data_ptr(), F32, C * 9, B, H, W, C, out.data_ptr(), F32, C + 8, 8)
    torch.cuda.synchronize()
    close_f32(out[:, 8:], tok(xr.grad), "col2im")
    assert torch.isnan(out[:, :8]).all()                       # nothing outside the slice is written


@pytest.mark.parametrize("H,W,s", dtr.GEOMETRY)
def test_adaptive_avgpool_and_bilinear_upsample(H, W, s):
    B, C = 2, 40
    x = randn(B, C, H, W, seed=3)
    xr = x.double().requires_grad_(True)
    p = F.adaptive_avg_pool2d(xr, s)
    u = F.interpolate(p, size=(H, W), mode="bilinear", align_corners=False)
    gp, gu = randn(B, C, s, s, seed=4), randn(B, C, H, W, seed=5)
    (dxp,) = torch.autograd.grad((p * gp.double()).sum(), xr, retain_graph=True)
    (dpu,) = torch.autograd.grad((u * gu.double()).sum(), p)
    xd = tok(x).cuda()
    pooled = torch.empty(B * s * s, C, device="cuda")
    call("evp_adaptive_avgpool_fwd", xd.data_ptr(), F32, C, B, H, W, C, s, pooled.data_ptr(), F32, C, 0)
    close_f32(pooled, tok(p), "pool")
    dx = torch.empty(B * H * W, C, device="cuda")
    gpd, gud = tok(gp).cuda(), tok(gu).cuda()
    call("evp_adaptive_avgpool_bwd", gpd.data_ptr(), F32, C, B, H, W, C, s, dx.data_ptr(), F32, C, 0)
    close_f32(dx, tok(dxp), "pool bwd")
    # upsample from the truth's pooled map, into a slice of a wider buffer
    pin = tok(p.detach().float()).cuda()
    wide = torch.full((B * H * W, C + 16), float("nan"), device="cuda")
    call("evp_upsample_bilinear_fwd", pin.data_ptr(), F32, C, B, s, s, H, W, C, wide.data_ptr(), F32, C + 16, 16)
    close_f32(wide[:, 16:], tok(u), "upsample")
    assert torch.isnan(wide[:, :16]).all()
    dp = torch.empty(B * s * s, C, device="cuda")
    call("evp_upsample_bilinear_bwd", gud.data_ptr(), F32, C, B, s, s, H, W, C, dp.data_ptr(), F32, C, 0)
    torch.cuda.synchronize()
    close_f32(dp, tok(dpu), "upsample bwd")


def test_upsample_from_one_pixel_and_at_equal_size():
    B, C = 2, 8
    one = randn(B, C, 1, 1, seed=6)
    out = torch.empty(B * 196, C, device="cuda")
    oned, gd, xd = tok(one).cuda(), tok(randn(B, C, 14, 14, seed=7)).cuda(), tok(randn(B, C, 6, 10, seed=8)).cuda()
    call("evp_upsample_bilinear_fwd", oned.data_ptr(), F32, C, B, 1, 1, 14, 14, C, out.data_ptr(), F32, C, 0)
    close_f32(out, tok(F.interpolate(one.double(), size=(14, 14), mode="bilinear", align_corners=False)), "1x1 fwd")      # a constant map
    g = randn(B, C, 14, 14, seed=7)
    d1 = torch.empty(B, C, device="cuda")
    call("evp_upsample_bilinear_bwd", gd.data_ptr(), F32, C, B, 1, 1, 14, 14, C, d1.data_ptr(), F32, C, 0)
    close_f32(d1, g.double().sum((2, 3)), "1x1 bwd")
    x = randn(B, C, 6, 10, seed=8)
    same = torch.empty(B * 60, C, device="cuda")
    call("evp_upsample_bilinear_fwd", xd.data_ptr(), F32, C, B, 6, 10, 6, 10, C, same.data_ptr(), F32, C, 0)
    torch.cuda.synchronize()
    assert torch.equal(same.cpu(), tok(x))


def test_channel_scale_and_batchnorm_eval():
    B, P, C = 3, 60, 24
    x = randn(B * P, C, seed=9)
    keep = (torch.rand(B, C, generator=torch.Generator().manual_seed(10)) >= 0.3).float()
    m = keep / 0.7
    out = torch.full((B * P, C + 8), float("nan"), device="cuda")
    xd, md = x.cuda(), m.cuda()
    call("evp_channel_scale", xd.data_ptr(), F32, C, md.data_ptr(), B, P, C, out.data_ptr(), F32, C + 8, 8)
    close_f32(out[:, 8:], (x.double().view(B, P, C) * m.double()[:, None, :]).view(B * P, C), "channel scale")
    assert torch.isnan(out[:, :8]).all()
    lp = torch.empty(B * P, C, dtype=torch.bfloat16, device="cuda")
    call("evp_channel_scale", xd.data_ptr(), F32, C, None, 1, B * P, C, lp.data_ptr(), BF16, C, 0)
    assert torch.equal(lp.cpu(), x.bfloat16())                               # without a table: the cast
    gamma, beta = 1 + 0.2 * randn(C, seed=11), 0.1 * randn(C, seed=12)
    rm, rv = 0.1 * randn(C, seed=13), 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(14))
    gd, bd, rmd, rvd = gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda()
    for relu in (0, 1):
        y = torch.empty(B * P, C, device="cuda")
        call("evp_batchnorm_eval", xd.data_ptr(), F32, C, B * P, C, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(),
             rvd.data_ptr(), 1e-5, relu, y.data_ptr(), F32, C, 0)
        ref = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, 1e-5)
        close_f32(y, F.relu(ref) if relu else ref, f"bn eval relu={relu}")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 2 / 3. heads
def run_gpu(head, shape, train, dtype, drop=False):
    """Our head on the device on the case's inputs -> the tensors dense_truth.run_head names."""
    from eventpretrain_amd import ops
    B, H, W = dtr.SHAPES[shape]
    ops.set_compute_dtype(dtype)
    m = dtr.build_head(head, dropout_ratio=dtr.P_DROP if drop else 0.0).cuda().train(train)
    xs_tok, w, keep = dtr.case_inputs(head, shape)
    used = range(4) if dtr.HEADS[head]["kind"] == "uper" else (2,)
    toks = [t.cuda().requires_grad_(i in used) for i, t in enumerate(xs_tok)]
    if drop:
        m.given_keep = keep.cuda()
    out = m([dtr.tokens_to_frame(t, H, W) for t in toks])
    assert tuple(out.shape) == (B, dtr.HEADS[head]["out_channels"], H, W) and out.dtype == torch.float32
    out_tok = out.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    (out_tok * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    res = {"act:out": out_tok}
    res.update({f"act:dx{i}": toks[i].grad.reshape(B * H * W, -1) for i in used})
    res.update({"grad:" + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    res.update({"stat:" + k: v for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))})
    return {k: v.detach().cpu() for k, v in res.items()}


def _is_bn_affine(key):
    return key.endswith(("norm_layer.weight", "norm_layer.bias"))


@pytest.mark.parametrize("head,shape,train", dtr.FIXTURE_CASES)
def test_heads_f32_match_truth(head, shape, train):
    got = run_gpu(head, shape, train, torch.float32)
    T, _ = dtr.reference(head, shape, train)
    golden = np.load(os.path.join(GOLDEN, "ft_dense_heads.npz"))
    tag = f"{head}.{shape}.{'train' if train else 'eval'}"
    # the prediction against the fixture itself (whole, or the fixture's sample of it), everything against the truth the fixture pins
    if f"{tag}|act:out" in golden.files:
        close_f32(got["act:out"], torch.from_numpy(golden[f"{tag}|act:out"]), "out (fixture)")
    else:
        assert dtr.rel_err(got["act:out"].double().flatten()[::dtr.SAMPLE], torch.from_numpy(golden[f"{tag}|act:out|sample"])) <= 1e-4
    for k, t in T.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(t), k
        elif k.startswith("grad:") and _is_bn_affine(k) and not train:
            assert k not in got, k       # eval(): the BatchNorm affine parameters get no gradient (ops.ConvBNFn)
        elif k.startswith("grad:") and dtr.is_prebn_bias(k) and train:
            bound = 1e-4 * T[k[:-len("bias")] + "weight"].abs().max().item()
            assert got[k].abs().max().item() <= bound, (k, got[k].abs().max().item(), bound)
        else:
            close_f32(got[k], t, k)


@pytest.mark.parametrize("head,shape,train,drop", dtr.BF16_CASES)
def test_heads_bf16_within_three_times_the_autocast_yardstick(head, shape, train, drop):
    """Outputs, input gradients, parameter gradients and (training mode) running statistics in bf16 mode through the three gates of
    block_truth.compare. Worst gate value as a share of its bound, e_got / (FACTOR * e_ref), measured on an MI355X (the test prints the
    four worst tensors of each case):
      uper  sq train 0.4x  sq eval 0.44 (fpn_convs.0 bias)  rect train 0.64 (fpn_convs.2 norm bias)  rect eval 0.84 (fpn_convs.2 weight)
      fcn / fcn_flow, every shape and mode: 0.33 - 0.36 (the yardstick's own figure is 0.33)
      fcn_cat  sq train 0.75 (dx2)  sq eval 0.34  rect train 0.39 (conv_cat running_var)  rect eval 0.35
      given channel masks, dropout_ratio 0.1: uper 0.45 (psp_modules norm weights)  fcn 0.38  fcn_cat 0.41  fcn_flow 0.36"""
    got = run_gpu(head, shape, train, torch.bfloat16, drop)
    T, Y = dtr.reference(head, shape, train, drop)
    got = {k: v for k, v in got.items() if k in T}
    if not train:
        assert not any(k.startswith("grad:") and _is_bn_affine(k) for k in got)
        T = {k: v for k, v in T.items() if not (k.startswith("grad:") and _is_bn_affine(k))}
    assert set(k for k in T if dtr.gated(k, train)) <= set(got)
    fails, worst = dtr.compare_case(got, T, Y, train)
    print(f"{head}.{shape}.{'train' if train else 'eval'}{'.drop' if drop else ''}: " +
          "  ".join(f"{k} {v / dtr.FACTOR:.2f}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:4]))
    assert not fails, fails
    assert all(int(v) == int(train) for k, v in got.items() if k.endswith("num_batches_tracked"))


# ------------------------------------------------------------------------------------------------------------- 4. hub model
def _hub(phase="finetune_semseg", size="small", backbone="vit", dropout=False):
    from eventpretrain_amd.model.finetune_dense.ft_dense_hub_model import FtDenseHubModel
    from eventpretrain_amd.testing import det_fill_module_, make_args
    a = make_args(phase=phase, model_size=size, backbone_type=backbone, num_classes=11, mask_ratio=0.0, sample_mode="bilinear")
    m = FtDenseHubModel(a)
    if not dropout:
        for h in (m.decode_head, m.auxiliary_head):
            h.dropout = None
    det_fill_module_(m)
    return a, m.cuda().train()


_W = {}


def _surrogate(res):
    dec, aux = res[-2], res[-1]
    if tuple(dec.shape) not in _W:           # made once, outside any capture
        _W[tuple(dec.shape)] = tuple(w.cuda() for w in dtr.hub_loss_weights(dec.shape))
    w1, w2 = _W[tuple(dec.shape)]
    return (dec * w1).sum() + 0.4 * (aux * w2).sum()


def test_dense_hub_vit_small_f32_matches_reference():
    """The tolerances of test_ft_cls_step_f32_matches_reference, except for the convolution biases in front of a BatchNorm: measured on
    an MI355X their |g|_inf is 8e-7 .. 2e-5 against bounds of 7e-4 .. 4e-3, and 3.1e-3 against 1.1e-2 for psp_modules.0 (BatchNorm over
    the two rows of the pooled 1 x 1 map); the reference's float32 norms of the same gradients differ from ours by up to 3 x."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.testing import det_normalish
    d = np.load(os.path.join(GOLDEN, "ft_dense_vit_small.npz"))
    a, m = _hub()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == json.loads(str(d["state_keys"]))
    x = (det_normalish("ft.voxels", (2, 5, 224, 224)) * 0.5).cuda()
    ops.set_compute_dtype(torch.float32)
    res = m(x)
    assert len(res) == 7 and len(res[3]) == 4
    _surrogate(res).backward()
    torch.cuda.synchronize()
    for got, key in ((res[-2], "decode_predict"), (res[-1], "aux_predict")):
        assert tuple(got.shape) == (2, 11, 14, 14)
        assert torch.allclose(got.cpu(), torch.from_numpy(d[key]), atol=1e-4, rtol=1e-4), key
    params = dict(m.named_parameters())
    for n, gn in zip(json.loads(str(d["grad_names"])), d["grad_norms"]):
        assert params[n].grad is not None, n
        if dtr.is_prebn_bias(n):
            # zero in exact arithmetic (the bias sits in front of a batch-statistics BatchNorm): the fixture's norm is the reference's own
            # float32 residue, not a quantity. Held by the head-level rule instead: |g|_inf <= 1e-4 |dW|_inf of the same convolution.
            got, bound = params[n].grad.abs().max().item(), 1e-4 * params[n[:-len("bias")] + "weight"].grad.abs().max().item()
            print(f"{n}: |g|_inf {got:.3e}  bound {bound:.3e}  norm {params[n].grad.double().norm().item():.4e} (fixture {gn:.4e})")
            assert got <= bound, (n, got, bound)
            continue
        assert params[n].grad.double().norm().item() == pytest.approx(gn, rel=5e-3, abs=2e-7), n
    for k in ("decode_head.conv_dense.weight", "decode_head.conv_dense.bias", "auxiliary_head.conv_dense.weight", "auxiliary_head.conv_dense.bias"):
        ref = torch.from_numpy(d["grad::" + k])
        assert torch.allclose(params[k].grad.cpu(), ref, atol=1e-6 + 1e-3 * ref.abs().max().item(), rtol=1e-3), k


def test_dense_hub_flow_base_and_the_refused_backbones():
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.finetune_dense.ft_dense_hub_model import FtDenseHubModel
    from eventpretrain_amd.testing import det_normalish, make_args
    a, m = _hub(phase="finetune_flow")
    ops.set_compute_dtype(torch.float32)
    with torch.no_grad():
        res = m.eval()((det_normalish("ft.voxels", (2, 5, 224, 224)) * 0.5).cuda())
    assert tuple(res[-2].shape) == tuple(res[-1].shape) == (2, 2, 14, 14) and torch.isfinite(res[-2]).all()
    base = FtDenseHubModel(make_args(phase="finetune_flow", model_size="base", backbone_type="vit", num_classes=11, sample_mode="bilinear"))
    assert base.decode_head.conv_dense.weight.shape == (2, 384, 1, 1) and base.auxiliary_head.convs[0].conv_layer.weight.shape == (256, 768, 3, 3)
    for bt, size in (("convvit", "small"), ("swin", "tiny")):
        with pytest.raises(NotImplementedError):
            FtDenseHubModel(make_args(phase="finetune_semseg", model_size=size, backbone_type=bt, num_classes=11, sample_mode="bilinear"))
    with pytest.raises(NotImplementedError):
        FtDenseHubModel(make_args(phase="finetune_semseg", backbone_type="vit", num_classes=11, sample_mode="nearest"))


# ------------------------------------------------------------------------------------------------------------- 5. captured step
def _stepper(use_graph, dropout):
    from eventpretrain_amd.engine import GraphedStep
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.testing import det_normalish
    a, m = _hub(dropout=dropout)
    opt = FusedAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    x = (det_normalish("ft.voxels", (2, 5, 224, 224)) * 0.5).cuda()
    ex = GraphedStep(m, opt, lambda mm, xx, noise: (_surrogate(mm(xx)),), [x], use_graph=use_graph, warmup=2)
    return m, ex


def test_captured_dense_step_replays_bit_equal_to_eager():
    from eventpretrain_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    runs = {}
    for mode in ("eager", "graph"):
        m, ex = _stepper(mode == "graph", dropout=False)
        if mode == "graph":
            assert ex.note.startswith("hip-graph"), ex.note
        for _ in range(2):
            ex.step()
        torch.cuda.synchronize()
        runs[mode] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in runs["eager"].items():
        assert torch.equal(v, runs["graph"][k]), k


def test_captured_dense_step_draws_fresh_channel_masks():
    from eventpretrain_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    m, ex = _stepper(True, dropout=True)
    assert ex.note.startswith("hip-graph"), ex.note
    masks = []
    for _ in range(2):
        ex.step()
        torch.cuda.synchronize()
        masks.append((m.decode_head.last_keep.clone(), m.auxiliary_head.last_keep.clone()))
    for i, width in ((0, 2 * 384), (1, 2 * 256)):
        a, b = masks[0][i], masks[1][i]
        assert a.numel() == b.numel() == width and not torch.equal(a, b)
        for k in (a, b):
            assert set(k.unique().tolist()) <= {0, 1} and 0.75 * width <= int(k.sum()) <= width


# ------------------------------------------------------------------------------------------------------------- 6. a batch of one
def test_batch_of_one_raises_in_train_and_runs_in_eval():
    from eventpretrain_amd import ops
    ops.set_compute_dtype(torch.float32)
    m = dtr.build_head("uper").cuda()
    xs = [dtr.tokens_to_frame(t[:1].cuda(), 14, 14) for t in dtr.case_inputs("uper", "sq")[0]]
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.train()(xs)
    out = m.eval()(xs)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 11, 14, 14) and torch.isfinite(out).all()

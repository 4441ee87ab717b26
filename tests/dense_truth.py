"""Truth for the dense-prediction heads (tests/test_dense_truth_host.py, tests/test_gpu_dense_heads.py): a restatement of the UPerNet /
FCN decoders with plain torch functions (F.conv2d, F.batch_norm, F.adaptive_avg_pool2d, F.interpolate, given channel scales), run in
float64 (truth), float32, or float32 under torch.autocast("cpu", bfloat16) (the yardstick of tests/block_truth.py, whose comparator and
constants are used as they are). The restatement itself is pinned to the reference's own classes by tests/golden/ft_dense_heads.npz
(tools/gen_dense_golden.py) in the host tests. `mut`: named mutations of the restatement, each of which the comparator must catch.

Tensors are presented token-major -- "act:out" [B*H*W, out_channels], "act:dx{i}" [B*H*W, C_i] -- and gradients as "grad:<key>", so that
block_truth.families() tiles them as it tiles the blocks' tensors; "stat:<key>" are the running statistics after the call."""
import contextlib
import functools

import torch
import torch.nn.functional as F

from block_truth import FACTOR, FLOOR, MAX_EXCLUDED, ACT_TILE, W_TILE, compare, rel_err  # noqa: F401  (re-exported to the tests)
from eventpretrain_amd.testing import det_fill_module_, det_normalish, det_uniform, make_args

POOL_SCALES = (1, 2, 3, 6)
HEADS = dict(
    uper=dict(kind="uper", in_channels=[40, 40, 40, 40], channels=24, out_channels=11),
    fcn=dict(kind="fcn", in_channels=40, channels=24, num_convs=1, concat_input=False, out_channels=11),
    fcn_cat=dict(kind="fcn", in_channels=40, channels=24, num_convs=2, concat_input=True, out_channels=11),
    fcn_flow=dict(kind="fcn", in_channels=40, channels=24, num_convs=1, concat_input=False, out_channels=2),
)
SHAPES = dict(sq=(2, 14, 14), rect=(3, 6, 10))        # overlapping bins at 14 -> 3, 6; non-square, scale 6 = identity along H
P_DROP = 0.1
MUTANTS = ("bins_no_overlap", "align_corners", "replicate_pad", "kykxc_weight", "cat_reversed", "no_drop_scale", "biased_running_var")
# where each mutant shows: (head, shape, training, with dropout)
MUTANT_CASE = dict(bins_no_overlap=("uper", "sq", True, False), align_corners=("uper", "sq", True, False),
                   replicate_pad=("fcn", "rect", True, False), kykxc_weight=("fcn", "rect", True, False),
                   cat_reversed=("fcn_cat", "rect", True, False), no_drop_scale=("fcn", "sq", True, True),
                   biased_running_var=("fcn", "rect", True, False))


# tests/golden/ft_dense_heads.npz (tools/gen_dense_golden.py): every head at both shapes in both modes. A tensor of more than BIG elements
# is held as four float64 checksums plus every SAMPLE-th element in float64 (the file stays small); the others whole, in float64.
FIXTURE_CASES = tuple((h, s, t) for h in HEADS for s in SHAPES for t in (True, False))
BIG, SAMPLE = 512, 16
# pooling / resize geometry of the kernel tests (H, W, s), and the cases of the bf16 comparator: (head, shape, training, given channel masks)
GEOMETRY = ((14, 14, 3), (14, 14, 6), (6, 10, 6), (6, 10, 3), (5, 7, 1))
BF16_CASES = tuple((h, s, t, False) for h, s, t in FIXTURE_CASES) + tuple((h, "rect" if h == "fcn_cat" else "sq", True, True) for h in HEADS)


def checksums(t):
    """Layout-sensitive checksums of a tensor in float64: sum, sum |.|, a fixed random projection, sum of squares."""
    d = t.detach().double().flatten()
    w = det_uniform("dense.checksum.weights", (d.numel(),)).double()
    return torch.stack([d.sum(), d.abs().sum(), (d * w).sum(), (d * d).sum()])


def hub_loss_weights(shape):
    """Fixed weights of the surrogate loss (decode * w1).sum() + 0.4 * (aux * w2).sum() of the hub-model tests; `shape` = a prediction's."""
    return det_normalish("dense.hub.w1", tuple(shape)), det_normalish("dense.hub.w2", tuple(shape))


def build_head(head, dropout_ratio=0.0):
    """Our module for a head-level case, on the CPU, with closed-form parameters and buffers."""
    from eventpretrain_amd.model.finetune_dense import ft_dense_decoder as dec
    s = HEADS[head]
    a = make_args(sample_mode="bilinear")
    if s["kind"] == "uper":
        m = dec.UPerHead(args=a, in_channels=s["in_channels"], channels=s["channels"], out_channels=s["out_channels"],
                         in_index=[0, 1, 2, 3], pool_scales=POOL_SCALES, dropout_ratio=dropout_ratio)
    else:
        m = dec.FCNHead(args=a, in_channels=s["in_channels"], channels=s["channels"], out_channels=s["out_channels"], in_index=2,
                        num_convs=s["num_convs"], kernel_size=3, concat_input=s["concat_input"], dropout_ratio=dropout_ratio)
    det_fill_module_(m)
    return m


def case_inputs(head, shape):
    """-> (four token tensors [B, H*W, 40] float32, loss weights [B*H*W, out_channels] float32, keep mask uint8 [B, channels])."""
    B, H, W = SHAPES[shape]
    s = HEADS[head]
    xs = [det_normalish(f"dense.{shape}.x{i}", (B, H * W, 40)) for i in range(4)]
    w = det_normalish(f"dense.{head}.{shape}.w", (B * H * W, s["out_channels"]))
    keep = (det_uniform(f"dense.{head}.{shape}.keep", (B, s["channels"]), 0.0, 1.0) >= P_DROP).to(torch.uint8)
    return xs, w, keep


def tokens_to_frame(t, H, W):
    B, L, C = t.shape
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------- the restatement
def pool_bins(n, s, overlap=True):
    """nn.AdaptiveAvgPool2d's bins along one axis: [floor(i n / s), ceil((i + 1) n / s)); overlap=False: the mutant's floor at both ends."""
    return [((i * n) // s, -((-(i + 1) * n) // s) if overlap else max(((i + 1) * n) // s, (i * n) // s + 1)) for i in range(s)]


def pool_matrix(n, s, overlap=True, dtype=torch.float64):
    m = torch.zeros(s, n, dtype=dtype)
    for i, (a, b) in enumerate(pool_bins(n, s, overlap)):
        m[i, a:b] = 1.0 / (b - a)
    return m


def bilinear_matrix(n_in, n_out, dtype=torch.float64):
    """F.interpolate(mode="bilinear", align_corners=False) along one axis as an [n_out, n_in] matrix: src = max(0, (d + 0.5) n_in / n_out -
    0.5), taps i0 = min(floor(src), n_in - 1), i1 = i0 + (i0 < n_in - 1), weights 1 - (src - i0), src - i0."""
    m = torch.zeros(n_out, n_in, dtype=dtype)
    for d in range(n_out):
        src = max(0.0, (d + 0.5) * n_in / n_out - 0.5)
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        m[d, i0] += 1.0 - (src - i0)
        m[d, i1] += src - i0
    return m


def pool2d(x, s, overlap=True):
    if overlap:
        return F.adaptive_avg_pool2d(x, s)
    ph, pw = pool_matrix(x.shape[2], s, False, x.dtype), pool_matrix(x.shape[3], s, False, x.dtype)
    return torch.einsum("ih,bchw,jw->bcij", ph, x, pw)


def resize(x, size, align=False):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=align)


def im2col3x3(x):
    """(B, C, H, W) -> [B*H*W, C*9], inner order (c, ky, kx)."""
    B, C, H, W = x.shape
    return F.unfold(x, 3, padding=1).permute(0, 2, 1).reshape(B * H * W, C * 9)


def conv_module(sd, p, x, train, mut=()):
    w, b = sd[p + "conv_layer.weight"], sd[p + "conv_layer.bias"]
    k = w.shape[-1]
    if k == 3 and "kykxc_weight" in mut:
        w = w.reshape(w.shape[0], 3, 3, w.shape[1]).permute(0, 3, 1, 2)      # the stored (c, ky, kx) run read as (ky, kx, c)
    if k == 3 and "replicate_pad" in mut:
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b)
    else:
        y = F.conv2d(x, w, b, padding=k // 2)
    rm, rv = sd[p + "norm_layer.running_mean"], sd[p + "norm_layer.running_var"]
    biased = train and "biased_running_var" in mut
    rv_old = rv.clone()
    z = F.batch_norm(y.to(rm.dtype), rm, rv.clone() if biased else rv, sd[p + "norm_layer.weight"], sd[p + "norm_layer.bias"], train, 0.1, 1e-5)
    if train:
        sd[p + "norm_layer.num_batches_tracked"] += 1
        if biased:
            with torch.no_grad():
                rv.copy_(0.9 * rv_old + 0.1 * y.detach().to(rv.dtype).var((0, 2, 3), unbiased=False))
    return F.relu(z)


def cls_dense(sd, p, feat, scale, mut=()):
    if scale is not None:
        s = scale.to(feat.dtype)
        if "no_drop_scale" in mut:
            s = (s > 0).to(feat.dtype)
        feat = feat * s[:, :, None, None]
    return F.conv2d(feat, sd[p + "conv_dense.weight"], sd[p + "conv_dense.bias"])


def uper_head(sd, p, xs, train, scale=None, mut=()):
    overlap, align = "bins_no_overlap" not in mut, "align_corners" in mut
    x = xs[-1]
    outs = [x]
    for i, s in enumerate(POOL_SCALES):
        c = conv_module(sd, f"{p}psp_modules.{i}.1.", pool2d(x, s, overlap), train, mut)
        outs.append(resize(c, x.shape[2:], align))
    lat = [conv_module(sd, f"{p}lateral_convs.{i}.", xs[i], train, mut) for i in range(len(xs) - 1)]
    lat.append(conv_module(sd, p + "psp_bottleneck.", torch.cat(outs[::-1] if "cat_reversed" in mut else outs, 1), train, mut))
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + resize(lat[i], lat[i - 1].shape[2:], align)
    fo = [conv_module(sd, f"{p}fpn_convs.{i}.", lat[i], train, mut) for i in range(len(lat) - 1)] + [lat[-1]]
    fo = [fo[0]] + [resize(f, fo[0].shape[2:], align) for f in fo[1:]]
    feats = conv_module(sd, p + "fpn_bottleneck.", torch.cat(fo[::-1] if "cat_reversed" in mut else fo, 1), train, mut)
    return cls_dense(sd, p, feats, scale, mut)


def fcn_head(sd, p, xs, spec, train, scale=None, mut=()):
    x = xs[2]
    f = x
    for i in range(spec["num_convs"]):
        f = conv_module(sd, f"{p}convs.{i}.", f, train, mut)
    if spec["concat_input"]:
        f = conv_module(sd, p + "conv_cat.", torch.cat([f, x] if "cat_reversed" in mut else [x, f], 1), train, mut)
    return cls_dense(sd, p, f, scale, mut)


def run_head(head, shape, train, mode="truth", drop=False, mut=()):
    """One forward + backward of the restatement on the case's module state. mode: "truth" (float64), "f32", "yardstick" (float32 under
    CPU autocast to bfloat16). -> {"act:out", "act:dx0".., "grad:<key>", "stat:<key>"} in float64."""
    spec = HEADS[head]
    B, H, W = SHAPES[shape]
    dt_ = torch.float64 if mode == "truth" else torch.float32
    mod = build_head(head)
    sd = {k: v.detach().clone().to(dt_) if v.is_floating_point() else v.detach().clone() for k, v in mod.state_dict().items()}
    params = [k for k, _ in mod.named_parameters()]
    for k in params:
        sd[k].requires_grad_(True)
    xs_tok, w, keep = case_inputs(head, shape)
    used = range(4) if spec["kind"] == "uper" else (2,)
    toks = [t.to(dt_).clone().requires_grad_(i in used) for i, t in enumerate(xs_tok)]
    xs = [tokens_to_frame(t, H, W) for t in toks]
    scale = keep.to(dt_) / (1.0 - P_DROP) if (drop and train) else None
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if mode == "yardstick" else contextlib.nullcontext()
    with ctx:
        out = uper_head(sd, "", xs, train, scale, mut) if spec["kind"] == "uper" else fcn_head(sd, "", xs, spec, train, scale, mut)
    out_tok = out.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    (out_tok.to(dt_) * w.to(dt_)).sum().backward()
    res = {"act:out": out_tok}
    for i in used:
        res[f"act:dx{i}"] = toks[i].grad.reshape(B * H * W, -1)
    for k in params:
        res["grad:" + k] = sd[k].grad
    for k, v in sd.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            res["stat:" + k] = v
    return {k: v.detach().double() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def reference(head, shape, train, drop=False):
    """(truth, yardstick) of a case: computed once per process and shared; nobody writes into them."""
    return run_head(head, shape, train, "truth", drop), run_head(head, shape, train, "yardstick", drop)


def is_prebn_bias(key):
    """A convolution bias in front of a BatchNorm: in training mode its gradient is zero up to rounding."""
    return key.endswith("conv_layer.bias")


def gated(tensor, train):
    """The tensors the bf16 comparator gates: activations, gradients that have a norm to measure against, and in training mode the
    running statistics (in eval() they do not move: the yardstick equals truth there)."""
    if tensor.startswith("stat:"):
        return train and not tensor.endswith("num_batches_tracked")
    return not (train and is_prebn_bias(tensor))


def compare_case(got, T, Y, train):
    """The block_truth comparator over every gated tensor of a case. -> (failures, {tensor: worst ratio to the yardstick's own figure})."""
    fails, worst = [], {}
    for t, g in got.items():
        if not gated(t, train):
            continue
        rows, f = compare(t, g, T[t], Y[t])
        fails += f
        worst[t] = max(r[3] for r in rows)
    return fails, worst

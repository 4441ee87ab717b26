"""Shared by the CPU and GPU tests that pin the bf16 blocks to float64 truth (tests/test_block_truth_host.py,
tests/test_gpu_block_bf16_truth.py): the cases, their references and the comparator.

For every case three runs of the SAME oracle function (oracle/model_oracle.py) on the CPU, on the module's own f32 parameters:
  truth      T: everything in float64;
  yardstick  Y: float32 under torch.autocast("cpu", dtype=torch.bfloat16) -- the reference project's own notion of bf16 training;
  f32        F: plain float32 (shows that T is truth: F sits at ~1e-6 of it).
Per tensor t (output, dx, every parameter gradient, the attention map where returned):
  e_ref(t) = |Y_t - T_t|_2 / |T_t|_2,   e_got(t) = |got_t - T_t|_2 / |T_t|_2.
Gates, all measured against the yardstick, FACTOR being the only constant:
  1. whole tensor  e_got <= FACTOR * e_ref. The HIP path rounds to bf16 at a handful of points autocast keeps in f32 (LN outputs,
     stored qkv / h_pre, probabilities inside the MFMA chain, dln, the handed-down gradient copy). Independent roundings add in
     quadrature: twice as many rounding points is a factor ~1.4; FACTOR = 3 leaves 2x on top. A dropped tile, a wrong scale or a
     swapped slice moves a tensor by an order of magnitude more.
  2. sub-blocks    every block's error relative to THAT block's truth norm <= FACTOR * the LARGEST block error of Y in the same
     family of blocks of the same tensor. Families: 16 x 64 tiles of [M, D] tensors (output, dx), 128 x 128 tiles of weight
     gradients, the (sample, head) slices of an attention map, and for the qkv weight / bias gradients the q, k, v thirds and each
     head's slice of each third (bias: q and v only, see families()). Blocks whose truth norm is below FLOOR of the family's RMS block norm are left out (dropped samples,
     masked positions); at most MAX_EXCLUDED of a family may be left out -- a condition on the INPUTS, asserted. The tensors of the
     attention cores ("core:...", tests/attention_truth.py) have families of their own, _core_families.
  3. scale         |<got, T> / <T, T> - 1| <= FACTOR * e_ref. Rounding noise is near zero-mean; a missing 1 / keep_prob, 1 / R or
     d_h^-0.5 is not.
The yardstick is computed here at run time (milliseconds at these shapes), never from the code under test."""
import collections.abc
import contextlib
import functools
import math

import torch

from eventpretrain_amd.testing import det_fill_module_, det_normalish, make_args
from oracle import model_oracle as mo

FACTOR = 3.0            # the one constant of the three gates
ACT_TILE = (16, 64)     # rows x columns of an [M, D] tensor
W_TILE = (128, 128)     # of a weight gradient
FLOOR = 1e-3            # of the family's RMS block norm
MAX_EXCLUDED = 0.10

# DropPath draws of the f32 tests (tests/test_gpu_round4.py): keep_prob 0.7, floor(0.7 + u) ->
U1 = (0.05, 0.9, 0.5, 0.2, 0.31, 0.95)       # 0, 1, 1, 0, 1, 1
U2 = (0.95, 0.1, 0.31, 0.6, 0.29, 0.7)       # 1, 0, 1, 1, 0, 1
KEEP_PROB, P_DROP = 0.7, 0.25

VIT = dict(
    vit_a=dict(B=3, N=50, D=128, heads=2),               # M = 150: ragged against 16 / 128-row tiles; N padded to 64 in the fused kernel
    vit_b=dict(B=2, N=197, D=128, heads=4),              # d_h = 32: head pairs; the largest tile count
    vit_e=dict(B=3, N=50, D=128, heads=2, drops=True),   # given drop-path draws and dropout masks
    vit_f=dict(B=2, N=24, D=64, heads=2, stack=2),       # two blocks: the lower one takes the upper one's gradient
)
CONV = dict(
    conv_keep=dict(B=4, C=64, H=14, W=14, keep=True),    # keep map at scale 2 (7 x 7 cells)
    conv_nomask=dict(B=2, C=128, H=12, W=20),
    conv_drops=dict(B=4, C=64, H=14, W=14, keep=True, drops=True),
)
SWIN = dict(
    swin_24=dict(Bn=3, nG=2, N=24, D=64, heads=2),       # NP = 32
    swin_98=dict(Bn=2, nG=2, N=98, D=64, heads=2),       # NP = 128
    swin_drops=dict(Bn=3, nG=2, N=24, D=64, heads=2, drops=True),
)
REC_CFG = dict(input=64, patch=16, dim=192, depth=12, heads=3, dec_dim=128, dec_depth=4, dec_heads=4, mask_ratio=0.5, B=5)
BLOCK_CASES = tuple(VIT) + tuple(CONV) + tuple(SWIN)
CASES = BLOCK_CASES + ("rec_tiny",)


# ------------------------------------------------------------------------------------------------------------- the cases
def _seed(name):
    return 1000 + CASES.index(name)


def _given_masks(g, rows, widths):
    return {k: (torch.rand(rows * w, generator=g) >= P_DROP).to(torch.uint8) for k, w in widths.items()}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict(kind, spec, module (on the CPU, closed-form weights), x, w = weights of the loss (y * w).sum(), and what the case needs
    besides). Deterministic; the GPU tests move the module and the inputs to the device."""
    g = torch.Generator().manual_seed(_seed(name))
    if name in VIT:
        from eventpretrain_amd.model.sub_module.vit_block import ViTBlock
        s = VIT[name]
        drops = s.get("drops", False)
        mod = torch.nn.ModuleList([ViTBlock(dim=s["D"], num_heads=s["heads"], mlp_ratio=4., qkv_bias=True, drop=P_DROP if drops else 0.,
                                            drop_path=0.3 if drops else 0.) for _ in range(s.get("stack", 1))])
        det_fill_module_(mod)
        c = dict(kind="vit", spec=s, module=mod.train(), x=torch.randn(s["B"], s["N"], s["D"], generator=g),
                 w=torch.randn(s["B"], s["N"], s["D"], generator=g))
        if drops:
            c.update(u1=torch.tensor(U1[:s["B"]]), u2=torch.tensor(U2[:s["B"]]),
                     masks=_given_masks(g, s["B"] * s["N"], {"proj": s["D"], "hidden": 4 * s["D"], "fc2": s["D"]}))
        return c
    if name in CONV:
        from eventpretrain_amd.model.sub_module.conv_block import ConvBlock
        s = CONV[name]
        drops = s.get("drops", False)
        B, C, H, W = s["B"], s["C"], s["H"], s["W"]
        mod = ConvBlock(input_size=C, kernel_size=5, mlp_ratio=4., drop=P_DROP if drops else 0., drop_path=0.3 if drops else 0.)
        det_fill_module_(mod)
        c = dict(kind="conv", spec=s, module=mod.train(), x=det_normalish(name + ".x", (B, H * W, C)), w=torch.randn(B, H * W, C, generator=g))
        if s.get("keep"):
            c["keep_coarse"] = (det_normalish(name + ".keep", (B, 1, H // 2, W // 2)) > -0.3).float()      # 1 = kept, one cell = 2 x 2
        if drops:
            c.update(u1=torch.tensor(U1[:B]), u2=torch.tensor(U2[:B]), masks=_given_masks(g, B * H * W, {"hidden": 4 * C, "fc2": C}))
        return c
    if name in SWIN:
        from eventpretrain_amd.model.sub_module.swin_block import SwinTransformerBlock
        s = SWIN[name]
        drops = s.get("drops", False)
        Bg, nG, N, D = s["Bn"] * s["nG"], s["nG"], s["N"], s["D"]
        mod = SwinTransformerBlock(dim=D, input_resolution=(14, 14), num_heads=s["heads"], window_size=7, shift_size=0, mlp_ratio=4.,
                                   drop=P_DROP if drops else 0., drop_path=0.3 if drops else 0.)
        det_fill_module_(mod)
        x = torch.randn(Bg, N, D, generator=g)
        rel = torch.randint(0, 169, (nG, N, N), generator=g)
        blocked = torch.rand(nG, N, N, generator=g) < 0.3
        blocked[:, torch.arange(N), torch.arange(N)] = False             # every token sees itself
        c = dict(kind="swin", spec=s, module=mod.train(), x=x, w=torch.randn(Bg, N, D, generator=g), rel=rel, blocked=blocked)
        if drops:
            c.update(u1=torch.tensor(U1[:Bg]), u2=torch.tensor(U2[:Bg]),
                     masks=_given_masks(g, Bg * N, {"proj": D, "hidden": 4 * D, "fc2": D}))
        return c
    assert name == "rec_tiny", name
    from eventpretrain_amd.model.pretrain import pr_hub_model as hub
    cfg = REC_CFG
    a = make_args(model_size="tiny", pr_phase="rec", mask_ratio=cfg["mask_ratio"], patch_size=cfg["patch"], device="cpu")
    mod = hub.pretrain_hub_model_tiny_patch16_64(a, emb_frames_dim=512, queue_length=1024, T=0.07)
    det_fill_module_(mod)
    S, B = cfg["input"], cfg["B"]
    return dict(kind="rec", spec=cfg, module=mod.train(), x=torch.randn(B, 5, S, S, generator=g), y=torch.randn(B, 1, S, S, generator=g),
                noise=torch.rand(B, (S // cfg["patch"]) ** 2, generator=g))


def heads_of(name):
    spec = make_case(name)["spec"]
    return spec.get("heads")


# ------------------------------------------------------------------------------------------------------------- oracle runs
def _drops(c, dt):
    if "u1" not in c:
        return None
    d = dict(u1=c["u1"].to(dt), u2=c["u2"].to(dt), keep_prob=KEEP_PROB, p=P_DROP)
    d.update({k: v.to(dt) for k, v in c["masks"].items()})
    return d


def _oracle(name, mode):
    """One run of the case's oracle function: mode "truth" (float64), "f32", or "yardstick" (f32 under CPU autocast to bf16).
    -> {tensor name: float64 tensor}; gradients of the loss (out * w).sum() (the model's own loss for rec_tiny)."""
    c = make_case(name)
    dt = torch.float64 if mode == "truth" else torch.float32
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if mode == "yardstick" else contextlib.nullcontext()
    sd = {k: v.detach().clone().to(dt) if v.is_floating_point() else v.detach().clone() for k, v in c["module"].state_dict().items()}
    params = [k for k, p in c["module"].named_parameters() if p.requires_grad]
    for k in params:
        sd[k].requires_grad_(True)
    x = c["x"].to(dt).clone().requires_grad_(c["kind"] != "rec")
    res = {}
    with ctx:
        if c["kind"] == "vit":
            s, t = c["spec"], x
            for i in range(s.get("stack", 1)):
                t = mo.vit_block(sd, f"{i}.", t, s["heads"], eps=c["module"][i].norm1.eps, want_attn=True, drops=_drops(c, dt))
                t, res["attn"] = t
            if s.get("stack", 1) > 1 or s.get("drops"):
                del res["attn"]                  # returned by the single plain block only
            out = t
        elif c["kind"] == "conv":
            s = c["spec"]
            B, C, H, W = s["B"], s["C"], s["H"], s["W"]
            keep = c["keep_coarse"].to(dt).repeat_interleave(2, 2).repeat_interleave(2, 3) if "keep_coarse" in c else None
            drops = _drops(c, dt)
            o = mo.conv_block(sd, "", x.view(B, H, W, C).permute(0, 3, 1, 2), keep, drops=drops)
            out = o.permute(0, 2, 3, 1).reshape(B, H * W, C)
        elif c["kind"] == "swin":
            mask = torch.where(c["blocked"], torch.tensor(-100.0, dtype=dt), torch.tensor(0.0, dtype=dt))
            out, _ = mo.swin_block(sd, "", x, dict(mode="plain", mask=mask, rel=c["rel"]), c["spec"]["heads"], eps=c["module"].norm1.eps,
                                   drops=_drops(c, dt))
        else:
            r = mo.rec_step(sd, x, c["y"].to(dt), c["noise"], c["spec"])
            loss, res["loss"], res["pred"] = r[0].to(dt), r[0], r[4]
            res["_mask"], res["_ids_restore"] = r[5], r[6]
    if c["kind"] != "rec":
        res["out"] = out
        loss = (out.to(dt) * c["w"].to(dt)).sum()
    loss.backward()
    if c["kind"] != "rec":
        res["dx"] = x.grad
    for k in params:
        if sd[k].grad is not None:
            res["grad:" + k] = sd[k].grad
    return {k: v.detach().double() if not k.startswith("_") else v for k, v in res.items()}


class Reference:
    def __init__(self, name):
        self.name = name
        self.T, self.Y, self.F = _oracle(name, "truth"), _oracle(name, "yardstick"), _oracle(name, "f32")
        self.tensors = [k for k in self.T if not k.startswith("_")]
        assert self.tensors == [k for k in self.Y if not k.startswith("_")]

    def e_ref(self, t):
        return rel_err(self.Y[t], self.T[t])


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per process and shared; nobody writes into it."""
    return Reference(name)


# ------------------------------------------------------------------------------------------------------------- the comparator
def rel_err(got, T):
    return float((got.double() - T).norm() / T.norm())


def scale_coef(got, T):
    return float((got.double() * T).sum() / (T * T).sum())


def _tiles(shape, tile):
    return [(slice(r, min(r + tile[0], shape[0])), slice(c, min(c + tile[1], shape[1])))
            for r in range(0, shape[0], tile[0]) for c in range(0, shape[1], tile[1])]


CORE_STRIP = 16         # rows of one query / key strip of the fused attention kernels


def _core_families(kind, shape):
    """The tensors of an attention core, handed over as [B, heads, N, d_h] (out and the q, k, v thirds of dqkv), [B, heads, N] (lse),
    [B, heads, N, N] (attn), [R, heads] (dtable), and anything else (dqkv as a whole) without sub-blocks."""
    fam = {}
    if kind in ("out", "dq", "dk", "dv"):
        planes, N = shape[0] * shape[1], shape[2]
        v = (planes * N, shape[3])
        fam["head"] = [(slice(p * N, (p + 1) * N), slice(0, v[1])) for p in range(planes)]
        fam["strip16"] = [(slice(p * N + r, p * N + min(r + CORE_STRIP, N)), slice(0, v[1])) for p in range(planes) for r in range(0, N, CORE_STRIP)]
    elif kind == "lse":
        v = (shape[0] * shape[1], shape[2])
        fam["head"] = [(slice(p, p + 1), slice(0, v[1])) for p in range(v[0])]
    elif kind == "attn":
        v = (math.prod(shape[:-1]), shape[-1])
        fam["head"] = [(slice(r, r + shape[-2]), slice(0, shape[-1])) for r in range(0, v[0], shape[-2])]
    elif kind == "dtable":
        v = tuple(shape)
        fam["head_col"] = [(slice(0, v[0]), slice(h, h + 1)) for h in range(v[1])]
    else:
        v = (math.prod(shape), 1)
    return v, fam


def families(tensor, shape, heads=None):
    """-> (the 2-D view's shape, {family: [(row slice, column slice), ...]}) for the tensor called `tensor`."""
    fam = {}
    if tensor.startswith("core:"):                   # the attention cores' own tensors (tests/attention_truth.py), [B, heads, N, ...]
        return _core_families(tensor[5:], shape)
    if tensor in ("out", "dx") or tensor.startswith("act:"):      # "act:...": the [M, D] tensors of tests/contrast_truth.py
        v = (math.prod(shape[:-1]), shape[-1])
        fam["tile16x64"] = _tiles(v, ACT_TILE)
    elif tensor == "attn":
        v = (math.prod(shape[:-1]), shape[-1])            # [B * heads * N, N]: one block per (sample, head)
        fam["head"] = [(slice(r, r + shape[-2]), slice(0, shape[-1])) for r in range(0, v[0], shape[-2])]
    elif tensor.startswith("grad:") and len(shape) >= 2:
        v = (shape[0], math.prod(shape[1:]))
        fam["tile128x128"] = _tiles(v, W_TILE)
    else:
        v = (math.prod(shape), 1) if len(shape) else (1, 1)
    if tensor.endswith(("attn.qkv.weight", "attn.qkv.bias")) and heads:
        D = shape[0] // 3
        dh = D // heads
        # the k third of the BIAS gradient is zero in exact arithmetic (a shift of every key by the same vector moves each row of
        # scores by a constant, which the softmax removes): no norm to measure against, so it has no slices of its own; what the
        # code under test leaves there counts in the whole-tensor gate
        thirds = (0, 2) if tensor.endswith("bias") else (0, 1, 2)
        fam["third"] = [(slice(i * D, (i + 1) * D), slice(0, v[1])) for i in thirds]
        fam["third_head"] = [(slice(i * D + h * dh, i * D + (h + 1) * dh), slice(0, v[1])) for i in thirds for h in range(heads)]
    return v, fam


def compare(tensor, got, T, Y, heads=None, factor=FACTOR, blocks=True):
    """-> (rows, failures): rows = [(gate, value of got, bound, value / (bound / factor))] -- the last one is the ratio to the
    yardstick's own figure, the number the docstrings record --, failures = strings of the violated gates."""
    got = got.detach().double().cpu()
    assert got.shape == T.shape, (tensor, tuple(got.shape), tuple(T.shape))
    assert torch.isfinite(got).all(), f"{tensor}: not finite"
    e_ref = rel_err(Y, T)
    assert e_ref > 0, f"{tensor}: the yardstick equals truth; no scale to measure with"
    rows = [("whole", rel_err(got, T), factor * e_ref), ("scale", abs(scale_coef(got, T) - 1.0), factor * e_ref)]
    if blocks:
        v, fam = families(tensor, tuple(T.shape), heads)
        g2, T2, Y2 = got.reshape(v), T.reshape(v), Y.reshape(v)
        for f, blks in fam.items():
            tn = torch.stack([T2[b].norm() for b in blks])
            kept = tn >= FLOOR * tn.pow(2).mean().sqrt()
            share = 1.0 - kept.double().mean().item()
            assert share <= MAX_EXCLUDED, f"{tensor}/{f}: {share:.0%} of the blocks of TRUTH are empty -- choose other inputs"
            ey = max(float((Y2[b] - T2[b]).norm() / n) for b, n, k in zip(blks, tn, kept) if k)
            eg = max(float((g2[b] - T2[b]).norm() / n) for b, n, k in zip(blks, tn, kept) if k)
            rows.append((f, eg, factor * ey))
    rows = [(gate, val, bound, val / (bound / factor)) for gate, val, bound in rows]
    fails = [f"{tensor}/{gate}: {val:.3e} > {bound:.3e} ({ratio:.2f} x the yardstick's)" for gate, val, bound, ratio in rows if not val <= bound]
    return rows, fails


def heads_for(heads, tensor):
    """`heads` as compare_all takes it -- one number, a mapping or a callable from tensor name to head count -- for one tensor."""
    if callable(heads):
        return heads(tensor)
    if isinstance(heads, collections.abc.Mapping):
        return heads.get(tensor)
    return heads


def compare_all(got, ref, heads=None, factors=None, blocks=True):
    """Every tensor of `got` against the reference. `heads`: one head count for all tensors, or a mapping / callable from tensor name
    to head count (tests/backbone_truth.py: the Swin stages differ). -> (failures, (worst ratio, "tensor/gate"), table as text)."""
    fails, worst, lines = [], (0.0, ""), []
    for t, g in got.items():
        rows, f = compare(t, g, ref.T[t], ref.Y[t], heads=heads_for(heads, t), factor=(factors or {}).get(t, FACTOR), blocks=blocks)
        fails += f
        for gate, val, bound, ratio in rows:
            worst = max(worst, (ratio, f"{t}/{gate}"))
        lines.append(f"  {t:44s} e_ref {ref.e_ref(t):.2e}  " + "  ".join(f"{gate} {ratio:.2f}" for gate, _, _, ratio in rows))
    return fails, worst, "\n".join(lines)

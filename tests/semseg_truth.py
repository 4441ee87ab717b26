"""Truth for the segmentation objective (tests/test_semseg_truth_host.py, tests/test_gpu_semseg_objective.py): a float64 restatement in
plain torch functions of what the reference computes from a head's low-resolution logits -- F.interpolate to the label size, the cross
entropy over the valid pixels, the batch-wide Dice loss, the confusion table with mIoU / mAcc -- with gradients by autograd. The
restatement is pinned to the reference's own SemsegLoss / resize / semseg_compute_confusion by tests/golden/ft_semseg_objective.npz
(tools/gen_semseg_golden.py) in the host tests. `mut`: named mutations of the restatement, each of which the comparator the GPU test
uses must catch. The inputs of every case are closed-form (eventpretrain_amd.testing.det_*), so the fixture holds no inputs."""
import functools

import torch
import torch.nn.functional as F

from eventpretrain_amd.testing import det_normalish, det_uniform

IGNORE = 255
# name -> B, C, ld (leading dimension the GPU test stores the map with), h x w -> H x W
CASES = dict(
    slice=dict(B=2, C=11, ld=16, h=14, w=14, H=40, W=56),      # one label row fully ignored, class 7 absent from the labels
    odd=dict(B=3, C=6, ld=8, h=5, w=7, H=33, W=45),            # odd sizes, partial waves; sample 1 entirely ignored
    wide=dict(B=1, C=19, ld=24, h=4, w=6, H=17, W=23),         # the 32-class kernel form
    ident=dict(B=1, C=2, ld=8, h=3, w=3, H=3, W=3),            # identity taps
    down=dict(B=2, C=11, ld=16, h=9, w=9, H=4, W=5),           # downsampling: cells with no pixel
)
UPSTREAM = ((1.0, 1.0), (0.4, 0.4), (0.3, 1.7))               # (g_ce, g_dice)
MUTANTS = ("dice_per_sample", "ignored_as_class0", "ce_mean_all", "confusion_transposed", "weights_swapped")
REL_LOSS = 1e-4           # ce, dice: relative
REL_GRAD = 1e-4           # the map gradient: of the truth's largest magnitude, per tensor
UNSURE = 1e-5             # a pixel is unsure when its two largest logits lie within UNSURE * the largest |logit|
MAX_UNSURE = 1e-3         # at most this share of the valid pixels may be unsure in a case


@functools.lru_cache(maxsize=None)
def case_inputs(name, all_ignored=False):
    """-> (logits float32 [B*h*w, C], label int64 [B, 1, H, W]): normal-ish logits times 3, uniform labels, about 20 % ignored."""
    s = CASES[name]
    B, C, h, w, H, W = (s[k] for k in ("B", "C", "h", "w", "H", "W"))
    logits = (det_normalish(f"semseg.{name}.logits", (B * h * w, C)) * 3.0).float()
    label = (det_uniform(f"semseg.{name}.label", (B, 1, H, W), 0.0, 1.0) * C).floor().clamp(0, C - 1).long()
    # (".0": the draw under the plain name ignores none of the nine pixels of `ident`)
    label[det_uniform(f"semseg.{name}.ignore.0", (B, 1, H, W), 0.0, 1.0) < 0.2] = IGNORE
    if name == "slice":
        label[label == 7] = 3
        label[0, 0, 5, :] = IGNORE
    if name == "odd":
        label[1] = IGNORE
    if all_ignored:
        label[:] = IGNORE
    return logits, label


def interpolate(logits, B, h, w, H, W):
    """[B*h*w, C] -> the resized logits, pixel-major [B, H, W, C]."""
    x = logits.view(B, h, w, -1).permute(0, 3, 1, 2)
    return F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def objective(logits, B, h, w, label, ignore=IGNORE, mut=None):
    """-> (ce, dice) of the resized logits, in the dtype of `logits`, differentiable."""
    H, W = label.shape[2:]
    z = interpolate(logits, B, h, w, H, W)
    C = z.shape[-1]
    lab = label[:, 0]
    valid = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != ignore
    zv, yv = z[valid], lab[valid]
    nll = torch.logsumexp(zv, 1) - zv.gather(1, yv[:, None])[:, 0]
    ce = nll.sum() / (lab.numel() if mut == "ce_mean_all" else valid.sum())

    def dice_of(zs, ys, n_ignored):
        p = torch.softmax(zs, 1)
        hot = F.one_hot(ys, C).to(p.dtype)
        A, Q, T = (p * hot).sum(0), (p * p).sum(0), hot.sum(0)
        if mut == "ignored_as_class0":
            T = T + F.one_hot(torch.zeros((), dtype=torch.long), C).to(p.dtype) * n_ignored
        return (1.0 - (2.0 * A + 1.0) / (Q + T + 1.0)).mean()
    if mut == "dice_per_sample":
        dice = torch.stack([dice_of(z[b][valid[b]], lab[b][valid[b]], int((~valid[b]).sum())) for b in range(B)]).mean()
    else:
        dice = dice_of(zv, yv, int((~valid).sum()))
    return ce, dice


def confusion_of(z, label, ignore=IGNORE, only=None):
    """int64 [C, C], rows = label, columns = argmax, over the valid pixels (and those of the boolean map `only`)."""
    C = z.shape[-1]
    lab = label[:, 0]
    valid = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != ignore
    if only is not None:
        valid = valid & only
    return torch.bincount(lab[valid] * C + z.argmax(-1)[valid], minlength=C * C).view(C, C)


def miou_macc(confusion):
    t = confusion.double()
    d, r, c = t.diagonal(), t.sum(1), t.sum(0)
    return (100.0 * d / (r + c - d).clamp(min=1e-12)).mean(), (100.0 * d / r.clamp(min=1e-12)).mean()


def truth(logits, B, h, w, label, ignore=IGNORE, upstream=UPSTREAM, mut=None, dtype=torch.float64, need_grad=True):
    """Everything the GPU test compares, from float32-valued logits [B*h*w, C], computed in `dtype`:
    ce, dice, grad[(g_ce, g_dice)] of g_ce * ce + g_dice * dice in the map, confusion, confusion over the sure pixels, n_valid,
    n_unsure, miou, macc."""
    x = logits.detach().to(dtype).requires_grad_(need_grad)
    ce, dice = objective(x, B, h, w, label, ignore, mut)
    out = dict(ce=ce.detach(), dice=dice.detach(), grad={})
    if need_grad:
        for g_ce, g_dice in upstream:
            a, b = (g_dice, g_ce) if mut == "weights_swapped" else (g_ce, g_dice)
            (out["grad"][(g_ce, g_dice)],) = torch.autograd.grad(a * ce + b * dice, x, retain_graph=True)
    H, W = label.shape[2:]
    z = interpolate(x.detach(), B, h, w, H, W)
    top2 = z.topk(2, -1).values
    sure = (top2[..., 0] - top2[..., 1]) > UNSURE * z.abs().max()
    conf, conf_sure = confusion_of(z, label, ignore), confusion_of(z, label, ignore, only=sure)
    if mut == "confusion_transposed":
        conf, conf_sure = conf.t().contiguous(), conf_sure.t().contiguous()
    n_valid = int(label.numel() if ignore is None else (label != ignore).sum())
    out.update(confusion=conf, confusion_sure=conf_sure, n_valid=n_valid, n_unsure=n_valid - int(conf_sure.sum()))
    out["miou"], out["macc"] = miou_macc(conf)
    return out


def compare(got, want):
    """The comparator of the GPU test -> list of failures (empty = pass). `got`: ce, dice (floats), grad {(g_ce, g_dice): [R, C]},
    confusion int64 [C, C]; `want`: a truth() dict. A NaN ce must be met by a NaN."""
    bad = []
    for k in ("ce", "dice"):
        g, t = float(got[k]), float(want[k])
        if t != t:
            if g == g:
                bad.append(f"{k}: {g} where the truth is NaN")
        elif not abs(g - t) <= REL_LOSS * abs(t):
            bad.append(f"{k}: {g} against {t} (rel {abs(g - t) / abs(t):.2e})")
    for key, t in want["grad"].items():
        if key not in got.get("grad", {}):
            continue
        err = (got["grad"][key].double().cpu() - t).abs().max().item()
        bound = REL_GRAD * t.abs().max().item()
        if not err <= bound:
            bad.append(f"grad{key}: max |err| {err:.3e} over the bound {bound:.3e}")
    if "confusion" in got:
        c = got["confusion"].cpu()
        if not bool((c >= want["confusion_sure"]).all()):
            bad.append("confusion: below the count of sure pixels somewhere")
        if int(c.sum()) != want["n_valid"]:
            bad.append(f"confusion: sums to {int(c.sum())}, {want['n_valid']} pixels are valid")
        if int(c.sum()) - int(want["confusion_sure"].sum()) != want["n_unsure"]:
            bad.append("confusion: does not exceed the sure count by the number of unsure pixels")
    return bad


def as_got(t):
    """A truth() dict (of a mutant, or in another dtype) presented to compare() as a result."""
    return dict(ce=t["ce"], dice=t["dice"], grad=t["grad"], confusion=t["confusion"])

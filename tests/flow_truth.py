"""Truth for the optical-flow objective (tests/test_flow_truth_host.py, tests/test_gpu_flow_objective.py): a float64 restatement in plain
torch functions of what the reference computes from a head's low-resolution two-channel prediction -- resize_flow (F.interpolate to the
label size, x times W / w and y times H / h through a float32 tensor), the masked L1 loss, and the validation's end-point error and
outlier share over the sparse mask -- with gradients by autograd. The restatement is pinned to the reference's own resize_flow /
FlowLoss / flow_compute_aee_outlier by tests/golden/ft_flow_objective.npz (tools/gen_flow_golden.py) in the host tests. `mut`: named
mutations of the restatement, each of which the comparator the GPU test uses must catch in at least one case. The inputs of every case
are closed-form (eventpretrain_amd.testing.det_*), so the fixture holds no inputs."""
import functools

import torch
import torch.nn.functional as F

from eventpretrain_amd.testing import det_normalish, det_uniform

# name -> B, ld (leading dimension the GPU test stores the map with), h x w -> H x W, channels of the event grid, max_flow
CASES = dict(
    slice=dict(B=2, ld=8, h=14, w=14, H=40, W=56, E=3, max_flow=40.0),      # x and y factors differ (4 and 20/7)
    odd=dict(B=3, ld=8, h=5, w=7, H=33, W=45, E=2, max_flow=70.0),          # inexact float32 factors, partial waves; sample 1 entirely invalid
    sensor=dict(B=1, ld=8, h=14, w=14, H=65, W=87, E=5, max_flow=60.0),     # the MVSEC aspect (260 x 346) at quarter size
    ident=dict(B=1, ld=2, h=3, w=3, H=3, W=3, E=1, max_flow=14.0),          # identity taps, factors 1, a map with no pad
    down=dict(B=2, ld=8, h=9, w=9, H=4, W=5, E=2, max_flow=6.0),            # downsampling: cells no pixel names
)
UPSTREAM = (1.0, 0.4, 1.7)      # the gradient that reaches the loss (a head's loss weight among them)
MUTANTS = ("scale_swapped", "no_scale", "valid_nonzero_in_loss", "no_max_flow", "mean_over_pixels",
           "max_flow_in_metrics", "valid_ge_half_in_metrics", "outlier_or", "events_mask_ignored")
REL_LOSS = 1e-4           # l1, aee: relative
REL_GRAD = 1e-4           # the map gradient: of the truth's largest magnitude
TIE = 1e-5                # a component with |p - t| <= TIE * max(|p|, |t|) could change sign in float32: none may exist
NEAR_MAX_FLOW = 1e-4      # no target magnitude within this relative distance of max_flow
UNSURE = 1e-5             # a sparse pixel is unsure when epe is within UNSURE of 3.0, or epe / mag of 0.05, relative
MAX_UNSURE = 1e-3         # at most this share of a case's sparse pixels may be unsure
REL_PERCENT = 1e-6        # the outlier share is a count over a count rounded to float32 (mean, then times 100: 2 ulp = 2.4e-7)
VALID_LEVELS = (0.0, 0.25, 0.75, 1.0)
MAP_SCALE, NOISE = 10.0, 6.0


def scale_factors(h, w, H, W, dtype, mut=None):
    """resize_flow's factors for (x, y): Python's double quotients stored into a float32 tensor."""
    f = torch.tensor([W / w, H / h])
    if mut == "scale_swapped":
        f = f.flip(0)
    if mut == "no_scale":
        f = torch.ones(2)
    return f.to(dtype)


def resize_flow(flow_map, B, h, w, H, W, mut=None):
    """[B*h*w, 2] -> the resized and scaled prediction [B, 2, H, W], in the dtype of `flow_map`."""
    x = flow_map.view(B, h, w, 2).permute(0, 3, 1, 2)
    z = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
    return z * scale_factors(h, w, H, W, z.dtype, mut).view(1, 2, 1, 1)


@functools.lru_cache(maxsize=None)
def case_inputs(name, all_invalid=False, no_events=False):
    """-> (map float32 [B*h*w, 2], target float32 [B, 2, H, W], valid float32 [B, 1, H, W], org float32 [B, E, H, W]).
    The targets are the float64-resized prediction plus noise of up to a few pixels, so that epe straddles 3.0 and epe / mag 0.05."""
    s = CASES[name]
    B, h, w, H, W, E = (s[k] for k in ("B", "h", "w", "H", "W", "E"))
    flow_map = (det_normalish(f"flow.{name}.map", (B * h * w, 2)) * MAP_SCALE).float()
    p = resize_flow(flow_map.double(), B, h, w, H, W)
    amp = 0.05 + NOISE * det_uniform(f"flow.{name}.amp", (B, 1, H, W), 0.0, 1.0).double() ** 2
    target = (p + amp * det_normalish(f"flow.{name}.noise", (B, 2, H, W)).double()).float()
    # by construction: no magnitude next to max_flow, no component next to its prediction
    mag = target.double().pow(2).sum(1, keepdim=True).sqrt()
    target = torch.where((mag - s["max_flow"]).abs() <= NEAR_MAX_FLOW * s["max_flow"], target * 1.01, target)
    t64 = target.double()
    tied = (p - t64).abs() <= TIE * torch.maximum(p.abs(), t64.abs())
    target = torch.where(tied, target + 1e-2, target)
    level = (det_uniform(f"flow.{name}.valid", (B, 1, H, W), 0.0, 1.0) * 4).floor().clamp(0, 3).long()
    valid = torch.tensor(VALID_LEVELS)[level]
    if name == "odd":
        valid[1] = 0.0
    if all_invalid:
        valid[:] = 0.25          # below FlowLoss's 0.5, but non-zero: the sparse mask still has pixels
    org = det_normalish(f"flow.{name}.org", (B, E, H, W))
    org = torch.sign(org) * (org.abs() + 1e-3)
    org = org * (det_uniform(f"flow.{name}.events", (B, 1, H, W), 0.0, 1.0) >= 0.5)
    if no_events:
        org = torch.zeros_like(org)
    # (F.interpolate of the permuted map answers channels-last, and the targets inherit that: the C ABI takes plain NCHW)
    return flow_map, target.contiguous(), valid, org.float().contiguous()


def loss_mask(target, valid, max_flow, mut=None):
    """FlowLoss's mask [B, 1, H, W]: valid >= 0.5 and |t| < max_flow."""
    mag = target.pow(2).sum(1, keepdim=True).sqrt()
    ok = valid != 0 if mut == "valid_nonzero_in_loss" else valid >= 0.5
    return ok if mut == "no_max_flow" else ok & (mag < max_flow)


def objective(flow_map, B, h, w, target, valid, max_flow, mut=None):
    """-> the L1 loss of the resized prediction, in the dtype of `flow_map`, differentiable."""
    H, W = target.shape[2:]
    p = resize_flow(flow_map, B, h, w, H, W, mut)
    t = target.to(p.dtype)
    m = loss_mask(t, valid, max_flow, mut).repeat(1, 2, 1, 1)
    l1 = (p[m] - t[m]).abs().mean()
    return l1 * 2.0 if mut == "mean_over_pixels" else l1


def sparse_mask(target, valid, org, max_flow, mut=None):
    """The validation's mask [B, H, W]: valid NON-ZERO and an event at the pixel; max_flow plays no part."""
    events = org.double().pow(2).sum(1) > 0
    ok = valid[:, 0] >= 0.5 if mut == "valid_ge_half_in_metrics" else valid[:, 0] != 0
    if mut != "events_mask_ignored":
        ok = ok & events
    if mut == "max_flow_in_metrics":
        ok = ok & (target.double().pow(2).sum(1).sqrt() < max_flow)
    return ok


def truth(flow_map, B, h, w, target, valid, org, max_flow, upstream=UPSTREAM, mut=None, dtype=torch.float64, need_grad=True):
    """Everything the GPU test compares, from a float32-valued map [B*h*w, 2], computed in `dtype`: l1, grad[g] of g * l1 in the map,
    aee, outlier (percent), n_valid, n_sparse, the outlier count with its sure part and the number of unsure pixels."""
    x = flow_map.detach().to(dtype).requires_grad_(need_grad)
    l1 = objective(x, B, h, w, target, valid, max_flow, mut)
    out = dict(l1=l1.detach(), grad={})
    if need_grad:
        for g in upstream:
            (out["grad"][g],) = torch.autograd.grad(g * l1, x, retain_graph=True)
    H, W = target.shape[2:]
    p, t = resize_flow(x.detach(), B, h, w, H, W, mut), target.to(dtype)
    sm = sparse_mask(target, valid, org, max_flow, mut)
    epe, mag = (p - t).pow(2).sum(1).sqrt()[sm], t.pow(2).sum(1).sqrt()[sm]
    ratio = epe / mag
    hit = (epe > 3.0) | (ratio > 0.05) if mut == "outlier_or" else (epe > 3.0) & (ratio > 0.05)
    unsure = ((epe - 3.0).abs() <= UNSURE * 3.0) | ((ratio - 0.05).abs() <= UNSURE * 0.05)
    n = int(sm.sum())
    out.update(aee=epe.mean(), outlier=hit.to(dtype).mean() * 100, n_valid=int(loss_mask(t, valid, max_flow, mut).sum()), n_sparse=n,
               n_outlier=int(hit.sum()), n_outlier_sure=int((hit & ~unsure).sum()), n_unsure=int(unsure.sum()))
    return out


def compare(got, want):
    """The comparator of the GPU test -> list of failures (empty = pass). `got`: l1 (float), grad {g: [R, 2]}, and, where metrics were
    taken, aee and outlier (floats); `want`: a truth() dict. A NaN must be met by a NaN. The outlier share, read as a count over
    want's n_sparse, must lie between the sure count and the sure count plus the unsure pixels."""
    bad = []
    for k in ("l1", "aee"):
        if k not in got:
            continue
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
            bad.append(f"grad({key}): max |err| {err:.3e} over the bound {bound:.3e}")
    if "outlier" in got:
        g, n = float(got["outlier"]), want["n_sparse"]
        if n == 0:
            if g == g:
                bad.append(f"outlier: {g} where the mask is empty")
        else:
            lo, hi = 100.0 * want["n_outlier_sure"] / n, 100.0 * (want["n_outlier_sure"] + want["n_unsure"]) / n
            if not lo * (1.0 - REL_PERCENT) <= g <= hi * (1.0 + REL_PERCENT):
                bad.append(f"outlier: {g} % outside [{lo}, {hi}] % ({want['n_outlier_sure']} sure + {want['n_unsure']} unsure of {n})")
    return bad


def as_got(t):
    """A truth() dict (of a mutant, or in another dtype) presented to compare() as a result."""
    return dict(l1=t["l1"], grad=t["grad"], aee=t["aee"], outlier=t["outlier"])

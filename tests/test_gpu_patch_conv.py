"""The patch convolutions that only whole-model fixtures reached (ops.StridedConvTokensFn, ops.PatchEmbedNHWCFn,
ops.PatchProjFn) against torch.nn.functional on the CPU in float64: a convolution with kernel = stride, evaluated at the kept
tokens only. Smallest shapes that still exercise every index computation: non-square patch grid, B > 1, n_keep < L with
unsorted ids_keep, Kc and D multiples of 8.

f32 mode (deferred gradients off): the tolerances of the sibling op tests (test_patchify_embed_post_unshuffle_loss,
test_fuse_conv_matches_dense_formulation).
bf16 mode (deferred gradients on, leaf Parameters -- the path the benchmark runs): the same float64 computation on inputs
rounded to bf16; error = max|got - ref| / max|ref| per tensor. Each bound in BF16_BOUNDS is twice the worst error measured
over the function's cases at the commit before the five patch-convolution classes were folded onto shared helpers, rounded up
to one significant digit (the headroom covers the summation order of grouped against plain weight-gradient launches); the
measured value stands beside it. The bf16 cases also pin which gradients arrive through the deferred queue."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# tensor: (bound, measured worst error)
BF16_BOUNDS = {
    "strided": {"y": (1e-7, 4.831e-08), "dx": (9e-3, 4.177e-03), "dw": (4e-3, 1.681e-03), "db": (3e-7, 1.488e-07)},
    "embed": {"y": (3e-7, 1.416e-07), "dx": (8e-3, 3.822e-03), "dw": (4e-3, 1.618e-03), "db": (4e-3, 1.556e-03),
              "dgamma": (5e-7, 2.351e-07), "dbeta": (3e-7, 1.478e-07)},
    "proj": {"y": (2e-7, 6.838e-08), "dw": (5e-3, 2.016e-03), "db": (2e-7, 8.898e-08)},
}
# (db: the embed form sums the compute-dtype dy, the other two the f32 gradient -- hence 1e-3 against 1e-7)
N_KEEP = 7


def _inputs(seed, x_shape, w_shape, L, norm, bf16):
    """Fixed-seed CPU tensors; with `bf16` the inputs and weights are rounded to bf16 (kept as f32), so that the float64
    reference and the kernels start from the same numbers. The incoming gradients stay f32: a bias gradient summed from the f32
    gradient is then accurate to f32, one summed from a bf16 copy is not."""
    g = torch.Generator().manual_seed(seed)
    D = w_shape[0]
    t = {"x": torch.randn(*x_shape, generator=g), "w": torch.randn(*w_shape, generator=g) * 0.2,
         "b": torch.randn(D, generator=g) * 0.1}
    if norm:
        t.update(gamma=torch.rand(D, generator=g) + 0.5, beta=torch.randn(D, generator=g) * 0.1,
                 pos=torch.randn(1, L, D, generator=g))
    if bf16:
        t = {k: v.bfloat16().float() for k, v in t.items()}
    t["ids_keep"] = torch.rand(x_shape[0], L, generator=g).argsort(dim=1)[:, :N_KEEP].contiguous()   # unsorted, distinct
    t["g_all"] = torch.randn(x_shape[0], L, D, generator=g)
    t["g_keep"] = torch.randn(x_shape[0], N_KEEP, D, generator=g)
    return t


@functools.lru_cache(maxsize=None)
def _reference(kind, bf16, keep, pos):
    """(inputs, {name: float64 reference}) of one case, computed once and shared; nobody writes to it."""
    if kind == "proj":
        B, C, H, W, p, D = 2, 5, 16, 24, 4, 16
        L = (H // p) * (W // p)
        t = _inputs(31, (B, C, H, W), (D, C, p, p), L, False, bf16)
    else:
        B, H, W, C, p, D = 2, 8, 12, 8, 2, 16
        L = (H // p) * (W // p)
        t = _inputs(29 if kind == "strided" else 30, (B, H * W, C), (D, C, p, p), L, kind == "embed", bf16)
    leaves = {k: t[k].double().requires_grad_(True) for k in ("x", "w", "b", "gamma", "beta") if k in t}
    img = leaves["x"] if kind == "proj" else leaves["x"].view(B, H, W, C).permute(0, 3, 1, 2)
    y = F.conv2d(img, leaves["w"], leaves["b"], stride=p).flatten(2).transpose(1, 2)
    if kind == "embed":
        y = F.gelu(F.layer_norm(y, (D,), leaves["gamma"], leaves["beta"], 1e-5))
        if pos:
            y = y + t["pos"].double()
    if keep:
        y = torch.gather(y, 1, t["ids_keep"].unsqueeze(-1).expand(-1, -1, D))
    y.backward((t["g_keep"] if keep else t["g_all"]).double())
    ref = {"y": y.detach()}
    ref.update({"d" + k: v.grad for k, v in leaves.items()})
    dims = dict(B=B, H=H, W=W, C=C, p=p, D=D, L=L)
    return t, ref, dims


def _dropped_rows(dx, ids_keep, d):
    """dx [B, H*W, C] of a channels-last map -> the entries that belong to patches outside ids_keep."""
    B, H, W, C, p = d["B"], d["H"], d["W"], d["C"], d["p"]
    kept = torch.zeros(B, d["L"], dtype=torch.bool)
    kept.scatter_(1, ids_keep, True)
    patches = dx.view(B, H // p, p, W // p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(B, d["L"], p * p * C)
    return patches[~kept]


def _run(kind, bf16, keep, pos=False, need_dx=True):
    """-> (inputs, reference, dims, {name: result on the CPU, or None where no gradient arrived}, queued names)."""
    from eventpretrain_amd import ops
    t, ref, d = _reference(kind, bf16, keep, pos)
    ids = t["ids_keep"].cuda() if keep else None
    gout = (t["g_keep"] if keep else t["g_all"]).cuda()
    x = t["x"].clone().cuda().requires_grad_(need_dx and kind != "proj")
    names = ("w", "b", "gamma", "beta") if kind == "embed" else ("w", "b")
    if bf16:
        prm = {k: torch.nn.Parameter(t[k].clone().cuda()) for k in names}
    else:
        prm = {k: t[k].clone().cuda().requires_grad_(True) for k in names}
    ops.set_compute_dtype(torch.bfloat16 if bf16 else torch.float32)
    ops.set_deferred_grads(bf16)
    ops.hold_deferred_grads(bf16)               # keep the queue at the end of backward: shows what went through it
    try:
        if kind == "strided":
            y = ops.StridedConvTokensFn.apply(x, ids, prm["w"], prm["b"], d["p"], d["H"], d["W"])
        elif kind == "embed":
            y = ops.PatchEmbedNHWCFn.apply(x, ids, prm["w"], prm["b"], prm["gamma"], prm["beta"],
                                           t["pos"].cuda() if pos else None, d["p"], d["H"], d["W"])
        else:
            y = ops.PatchProjFn.apply(x, ids, prm["w"], prm["b"], d["p"])
        y.backward(gout)
        queued = {k for k in names if prm[k].grad is None}
    finally:
        ops.hold_deferred_grads(False)
        ops.flush_deferred_grads()
        ops.set_deferred_grads(True)
        ops.set_compute_dtype(torch.float32)
    got = {"y": y.detach().cpu(), "dx": None if x.grad is None else x.grad.cpu()}
    got.update({"d" + k: prm[k].grad.cpu() for k in names})
    return t, ref, d, got, queued


def _check(kind, bf16, keep, got, ref, checked):
    for k in checked:
        assert got[k].shape == ref[k].shape, (kind, k, tuple(got[k].shape))
    if bf16:
        errs = {k: ((got[k].double() - ref[k]).abs().max() / ref[k].abs().max()).item() for k in checked}
        print(f"{kind} bf16 keep={keep}: " + "  ".join(f"{k} {e:.3e}" for k, e in errs.items()))
        for k, e in errs.items():
            assert e <= BF16_BOUNDS[kind][k][0], (kind, k, e)
        return
    for k in checked:
        r = ref[k]
        if k in ("y", "dx"):
            tol = dict(atol=2e-5, rtol=1e-5)
        elif k in ("dgamma", "dbeta"):
            tol = dict(atol=1e-4 * r.abs().max().item() + 1e-6, rtol=1e-4)
        else:
            tol = dict(atol=5e-5, rtol=1e-5)
        err = (got[k].double() - r).abs().max().item()
        print(f"{kind} f32 keep={keep}: {k} max|err| {err:.3e} (max|ref| {r.abs().max().item():.3e})")
        assert got[k].shape == r.shape and torch.allclose(got[k].double(), r, **tol), (kind, k, err)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_strided_conv_tokens(bf16, keep):
    t, ref, d, got, queued = _run("strided", bf16, keep)
    _check("strided", bf16, keep, got, ref, ("y", "dx", "dw", "db"))
    if keep:
        assert torch.count_nonzero(_dropped_rows(got["dx"], t["ids_keep"], d)) == 0
    assert queued == ({"w", "b"} if bf16 else set())


@pytest.mark.parametrize("keep,pos,need_dx", [(False, False, True), (True, False, True), (True, True, True),
                                              (True, False, False), (True, True, False)])
@pytest.mark.parametrize("bf16", [False, True])
def test_patch_embed_nhwc(bf16, keep, pos, need_dx):
    t, ref, d, got, queued = _run("embed", bf16, keep, pos, need_dx)
    _check("embed", bf16, keep, got, ref, ("y", "dw", "db", "dgamma", "dbeta") + (("dx",) if need_dx else ()))
    if not need_dx:
        assert got["dx"] is None
    elif keep:
        assert torch.count_nonzero(_dropped_rows(got["dx"], t["ids_keep"], d)) == 0
    assert queued == ({"w", "b"} if bf16 else set())       # d gamma / d beta of this form are reduced in its own kernel


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_patch_proj(bf16, keep):
    t, ref, d, got, queued = _run("proj", bf16, keep)
    _check("proj", bf16, keep, got, ref, ("y", "dw", "db"))
    assert queued == ({"w", "b"} if bf16 else set())

"""Shared by the CPU and GPU tests that pin the seams of the reconstruction step and the optimizer update to float64 truth
(tests/test_pretrain_truth_host.py, tests/test_gpu_pretrain_truth.py): the cases, their float64 references written from the
reference's formulas, a float32 CPU restatement of every kernel in the kernel's own order, the gates (contrast_truth's classes) and
the single mutations of the restatement which the gates have to reject. Every case exists twice: with small integers, where sums
are exact in any order and the comparison is equality, and with random values, where the gates apply.

Kernel -> the cases that reach it:
  evp_rec_loss (loss.hip)          REC_SHAPES x norm_pix 0 / 1 x REC_MASKS (no mask, half, all ones, a single one); REC_SPECIAL.
      1 x 1 x 2 x 2 / 2 one row, P = 4; 2 x 2 x 3 x 5 / 1 P = 2 (the variance divides by 1), 30 rows, gw != gh; 2 x 3 x 8 x 12 / 4
      P = 48 < one wave, C = 3; 2 x 2 x 16 x 16 / 8 P = 128; 3 x 1 x 64 x 96 / 16 P = 256; 1 x 5 x 16 x 32 / 16 P = 1280 (20 passes
      of the wave's 64 lanes); 3 x 3 x 128 x 128 / 2 12288 rows > the 2048 blocks x 4 rows of one pass and > the 1024
      threads of the reduce. REC_SPECIAL: a constant patch (variance 0) and a patch of variance 1e-6 (where the place of eps shows)
      under norm_pix. Integer version: norm_pix = 0 only (a normalised target is no integer).
  evp_unshuffle_fwd / _bwd         UNSH_SHAPES (slabs of UM_ROWS = 64 rows: 1 partial, 1 full, 2 with a last slab of one row, 16, 17
      (tokens.hip)                 with a last slab of one row, 33; D / 4 = 1, 2, 16, 65, 257; D > 256 = a second column block of the
                                   mask-token sum; n_keep = L: nothing removed); UNSH_NULL_SHAPE with dmask_token = workspace = NULL.
  evp_add_rows_gather_f32          GATHER_CASES (ids NULL / unsorted; D / 4 = 1, 16, 65, 257).
  evp_patchify                     PATCHIFY_CASES x f32 / bf16 output (Kc = 16; unsorted ids; ids NULL with Kc = 1280 > 256 x 4).
  evp_density_noise                DENS_SHAPES x both signs (one cell; p * p = 16 < one wave; p * p = 1024).
  evp_mask_from_noise              MASK_CASES (L = 257 and 4096; len_keep = 0 with ids_keep NULL; len_keep = L; MASK_SPECIAL_ROW
                                   of +-0, +-Inf and NaN against torch.argsort(stable=True)).
  adamw_kernel (optim.hip)         ADAM_NUMEL in two groups through FusedAdamW.launch, launch_part and the C ABI without dev_hyper:
                                   numel 1, 3 (tail only), 4, 5, CHUNK - 1, CHUNK, CHUNK + 1 and CHUNK + 3 (a tail in the last of
                                   two chunks), 2 CHUNK + 2; bf16 shadows on numel 5, CHUNK + 1, CHUNK + 3; grad_scale 0.5; step
                                   1, 2, 3 and 100001; gradients of 1e-6 on numel 5 (where the place of eps shows); ADAM_RECIPE.
  evp_add_f32, evp_scale_f32       EW_SIZES (1 .. 5: no vector body / no tail; 2048 x 1024 + 5: past ew_grid's 2048 blocks x 256).
  evp_cast                         CAST_SIZES both ways, CAST_SPECIALS in the vector body and in the scalar tail.
  evp_transpose                    TRANSPOSE_SHAPES x f32 / bf16.

Gates (contrast_truth.Report): gathers, scatters, casts, transposes, sums of two: exact; losses rel_class (1e-5 relative); dpred
grad_class (|got - T| <= 1e-7 + 1e-4 |T|); dmask_token, density noise, per-row losses, exp_avg, parameters f32_class (|got - T| <=
1e-5 max(1, max|T|)); exp_avg_sq, a sum of positive terms, elementwise relative at V_RTOL = 2e-6 -- the float32 restatement measures
2.5e-7 here on the CPU over the four steps of the main case, 2.7e-7 over the 5 of ADAM_RECIPE (the parameters: 2.9e-7 absolute), and
has to keep a factor of 4. exp_avg cancels near 0 and stays absolute.
Condition on the INPUTS, asserted on the host for every case: the float32 restatement alone stays at or below HEADROOM = 1 / 4 of
every gate. Targets under norm_pix carry no offset (randn * 2): with randn + 3 at P = 12 the restatement's own dpred sits at 0.9 x
its gate.

Measured on an MI355X by tests/test_gpu_pretrain_truth.py, worst error over the bound per tensor (the test prints them):
  evp_rec_loss        loss 0.015 (2 x 2 x 16 x 16 / 8), per-row losses 0.115 at P = 2 (2 x 2 x 3 x 5 / 1: two terms, each a difference
                      of near-equal numbers) and 0.017 elsewhere, dpred 0.013 (2 x 3 x 8 x 12 / 4); 12288 rows: loss 0.013, dpred 0.001;
                      the special patches: loss 0.006, per-row 0.010, dpred 0.004; every integer comparison equal.
  evp_unshuffle_bwd   dmask_token 0.018 (4 x 16 / D 260), 0.017 (last slab of one row, D 1028), 0.011 / 0.016 / 0.015 at 16 / 17 / 33
                      slabs; forward, demb and the integer versions equal.
  evp_density_noise   0.005 (one cell), 0.009 (p * p = 16), 0.030 (p * p = 1024); integers equal.
  adamw_kernel        FusedAdamW.launch and evp_adamw_multi without dev_hyper alike: p 0.029, exp_avg 0.004, exp_avg_sq 0.124 (of
                      V_RTOL), shadows equal; launch_part (two steps) p 0.017, exp_avg_sq 0.088, bit-identical to launch;
                      ADAM_RECIPE: p 0.029, exp_avg 0.007, exp_avg_sq 0.135. These are the figures of the float32 restatement on the CPU.
  evp_add_f32         a + b + c against truth 0.007 (n = 2048 x 1024 + 5), equal to (a + b) + c; everything else under `exact` equal.
"""
import functools
import math

import torch

import contrast_truth as ct
from contrast_truth import Report, _gen  # noqa: F401  (the gates are contrast_truth's, not redefined)

HEADROOM = 0.25
V_RTOL = 2e-6
UPSTREAM = 0.25


def f32(x):
    """What a C `float` argument holds."""
    return float(torch.tensor(x, dtype=torch.float32))


def rel_elem(rep, name, got, T, rtol=V_RTOL):
    """Elementwise relative gate for a tensor whose elements are sums of positive terms (exp_avg_sq)."""
    T = T.double()
    assert got.shape == T.shape, (name, tuple(got.shape), tuple(T.shape))
    rep._add(name, "relv", (got.double() - T).abs(), rtol * T.abs())


def bits_equal(rep, name, got, want):
    """Equality bit for bit (so -0 is not +0), NaN against NaN by position and not by payload."""
    want = want.to(got.dtype)
    ok = got.shape == want.shape
    if ok:
        gn, wn = torch.isnan(got), torch.isnan(want)
        it = torch.int32 if got.dtype == torch.float32 else torch.int16
        ok = torch.equal(gn, wn) and bool(((got.contiguous().view(it) == want.contiguous().view(it)) | gn).all())
    if not ok:
        rep.fails.append(f"{rep.what} {name}/bits: differs")
    rep.rows.append((name, "bits", 0.0))


def _rand(shape, g, kind, spread=1.0):
    if kind == "int":
        return torch.randint(-4, 5, shape, generator=g).float()
    return torch.randn(shape, generator=g) * spread


# ================================================================================================================ reductions
def _wave_sum(acc):
    """wave_sum of evp_common.h on [R, 64]: the xor butterfly 32, 16, .., 1. -> [R]."""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


def _lane_strided(t):
    """[R, P] -> [R, 64]: lane j adds elements j, j + 64, .. in turn."""
    R, P = t.shape
    n = (P + 63) // 64
    p = torch.zeros(R, n * 64)
    p[:, :P] = t
    acc = torch.zeros(R, 64)
    for k in range(n):
        acc = acc + p[:, 64 * k:64 * k + 64]
    return acc


def _block_sum_1024(v):
    """[n] -> scalar as rec_loss_reduce does it: thread t adds rows t, t + 1024, ..; wave_sum; the 16 wave sums added in turn."""
    n = v.numel()
    p = torch.zeros((n + 1023) // 1024 * 1024)
    p[:n] = v
    p = p.view(-1, 1024)
    acc = torch.zeros(1024)
    for k in range(p.shape[0]):
        acc = acc + p[k]
    w = _wave_sum(acc.view(16, 64))
    t = torch.zeros(())
    for i in range(16):
        t = t + w[i]
    return t


# ================================================================================================================ evp_rec_loss
REC_SHAPES = ((1, 1, 2, 2, 2), (2, 2, 3, 5, 1), (2, 3, 8, 12, 4), (2, 2, 16, 16, 8), (3, 1, 64, 96, 16), (1, 5, 16, 32, 16),
              (3, 3, 128, 128, 2))           # B, C, H, W, p
REC_MASKS = ("none", "half", "ones", "single")
REC_SPECIAL = (2, 3, 8, 12, 4)              # + a constant patch (b 0, l 1) and a patch of standard deviation 1e-3 (b 0, l 2)
REC_PASS_ROWS = 2048 * 4                    # rows one pass of rec_loss_rows covers: the grid cap x 4 waves
REC_REDUCE_THREADS = 1024


def frame2emb(frame, p):
    """(B, C, H, W) -> (B, L, p * p * C), inner order (py, px, c)."""
    B, C, H, W = frame.shape
    gh, gw = H // p, W // p
    return frame.reshape(B, C, gh, p, gw, p).permute(0, 2, 4, 3, 5, 1).reshape(B, gh * gw, p * p * C)


def rec_truth(pred, target, mask, p, norm_pix):
    """float64: unbiased variance, (var + 1e-6) ** 0.5, masked mean or the plain mean when mask is None; dpred by autograd."""
    tgt = frame2emb(target.double(), p)
    if norm_pix:
        mu = tgt.mean(-1, keepdim=True)
        var = tgt.var(-1, keepdim=True, unbiased=True)
        tgt = (tgt - mu) / (var + 1e-6) ** 0.5
    pr = pred.double().clone().requires_grad_(True)
    per = ((pr - tgt) ** 2).mean(-1)
    loss = per.mean() if mask is None else (mask.double() * per).sum() / mask.double().sum()
    loss.backward()
    return dict(loss=loss.detach(), per_row=per.detach().reshape(-1), dpred=pr.grad)


@functools.lru_cache(maxsize=None)
def rec_case(B, C, H, W, p, norm_pix, mask_kind, kind="random", special=False):
    g = _gen(B, C, H, W, p, norm_pix, REC_MASKS.index(mask_kind), kind == "int", special, 29)
    gh, gw = H // p, W // p
    L, P = gh * gw, p * p * C
    pred = _rand((B, L, P), g, kind)
    target = _rand((B, C, H, W), g, kind, 2.0)
    if special:
        target[0, :, 0:p, p:2 * p] = 3.0                                                    # l = 1: variance 0
        target[0, :, 0:p, 2 * p:3 * p] = 1e-3 * torch.randn(C, p, p, generator=g)           # l = 2: variance 1e-6
    if mask_kind == "none":
        mask = None
    elif mask_kind == "ones":
        mask = torch.ones(B, L)
    elif mask_kind == "single":
        mask = torch.zeros(B, L)
        mask[B - 1, L // 2] = 1.0                 # 3 x 4096 rows: row 10240, in the second pass
    else:
        mask = torch.zeros(B, L)
        for b in range(B):
            mask[b, torch.randperm(L, generator=g)[:max(1, L // 2)]] = 1.0
        if special:
            mask[0, 1:3] = 1.0
    T = rec_truth(pred, target, mask, p, norm_pix)
    c = dict(B=B, C=C, H=H, W=W, p=p, L=L, P=P, rows=B * L, norm_pix=norm_pix, mask_kind=mask_kind, kind=kind, pred=pred, target=target,
             mask=mask, T=T)
    if kind == "int":
        # integers: every sum below is exact, each division and product is one float32 rounding in the kernel's order
        assert not norm_pix
        d = pred.reshape(B * L, P) - frame2emb(target, p).reshape(B * L, P)
        w = torch.ones(B * L) if mask is None else mask.reshape(-1)
        per = (d * d).sum(1) / float(P)
        inv_den = 1.0 / w.sum()
        c["E"] = dict(per_row=per, dpred=((w * inv_den * 2.0 / float(P))[:, None] * d).view(B, L, P))
        if P & (P - 1) == 0:                      # P a power of two: the row losses are exact too, the loss is one division
            c["E"]["loss"] = (w * per).sum() / w.sum()
    return c


def rec_cases():
    out = []
    for s in REC_SHAPES:
        for mk in REC_MASKS:
            out += [s + (0, mk, "random"), s + (1, mk, "random"), s + (0, mk, "int")]
    return out + [REC_SPECIAL + (1, "half", "random", True)]


def check_rec(c, got, upstream=1.0, rep=None):
    """got: loss, dpred (times `upstream`, a power of two) and, from the C ABI, per_row."""
    rep = rep or Report("rec %dx%dx%dx%d/%d norm%d %s %s" % (c["B"], c["C"], c["H"], c["W"], c["p"], c["norm_pix"], c["mask_kind"], c["kind"]))
    T, E = c["T"], c.get("E", {})
    rep.rel_class("loss", got["loss"], T["loss"])
    rep.grad_class("dpred", got["dpred"], T["dpred"] * upstream)
    if "per_row" in got:
        rep.f32_class("per_row", got["per_row"], T["per_row"])
    for k, v in E.items():
        if k in got:
            rep.exact(k + " (integers)", got[k], v * upstream if k == "dpred" else v)
    if c["mask"] is not None:
        rep.zero("dpred[unmasked rows]", got["dpred"][c["mask"] == 0])
    return rep


def _tgt_rows(target, p, mutant=None):
    """tgt_at of loss.hip for every (row, j): the address arithmetic itself."""
    B, C, H, W = target.shape
    gw = (H if mutant == "gw_from_H" else W) // p
    L, P = (H // p) * (W // p), p * p * C
    j = torch.arange(P)
    if mutant == "order_c_py_px":
        c, q = j // (p * p), j % (p * p)
    else:
        c, q = j % C, j // C
    px, py = q % p, q // p
    l = torch.arange(L)
    gy, gx = l // gw, l % gw
    b = torch.arange(B)
    idx = ((b[:, None, None] * C + c[None, None, :]) * H + gy[None, :, None] * p + py[None, None, :]) * W + gx[None, :, None] * p + px[None, None, :]
    return target.reshape(-1)[idx % target.numel()].reshape(B * L, P)


def rec_restated(c, mutant=None):
    """rec_loss_rows (one wave per row, lane-strided sums, the butterfly) + rec_loss_reduce + the gradient pass, in float32."""
    p, P, rows = c["p"], c["P"], c["rows"]
    t = _tgt_rows(c["target"], p, mutant)
    pr = c["pred"].reshape(rows, P)
    if c["norm_pix"]:
        mu = _wave_sum(_lane_strided(t)) / float(P)
        d = t - mu[:, None]
        v = _wave_sum(_lane_strided(d * d)) / float(P if mutant == "biased_variance" else P - 1)
        inv = 1.0 / (torch.sqrt(v) + 1e-6) if mutant == "eps_outside_sqrt" else 1.0 / torch.sqrt(v + 1e-6)
        t = (t - mu[:, None]) * inv[:, None]
    d = pr - t
    per = _wave_sum(_lane_strided(d * d)) / float(P)
    if mutant == "rows_past_one_pass_not_written":
        per[REC_PASS_ROWS:] = float("nan")
    w = torch.ones(rows) if c["mask"] is None else c["mask"].reshape(-1)
    a, m = _block_sum_1024(w * per), _block_sum_1024(w)
    if mutant == "mean_over_all_rows":
        m = torch.tensor(float(rows))
    inv_den = 1.0 / m
    sc = w * inv_den * 2.0 / float(P)
    if mutant == "no_2_over_P":
        sc = w * inv_den
    if mutant == "dpred_ignores_mask":
        sc = torch.ones(rows) * inv_den * 2.0 / float(P)
    dpred = sc[:, None] * d
    if mutant == "rows_past_one_pass_not_written":
        dpred[REC_PASS_ROWS:] = float("nan")
    return dict(loss=a / m, per_row=per, dpred=dpred.view(c["B"], c["L"], P))


# ================================================================================================================ unshuffle, gathers
UM_ROWS, FOLD_GROUPS, UM_COLS = 64, 16, 256
UNSH_SHAPES = ((1, 1, 1, 4), (2, 7, 3, 4), (3, 24, 12, 64), (4, 16, 8, 260), (5, 13, 6, 1028), (16, 64, 16, 8), (5, 205, 100, 8),
               (3, 700, 1, 8), (2, 9, 9, 8))         # B, L, n_keep, D
UNSH_NULL_SHAPE = (3, 24, 12, 64)
GATHER_CASES = ((1, 1, 1, 4, False), (3, 7, 24, 64, True), (2, 5, 9, 260, True), (2, 9, 9, 1028, False))      # B, n, L, D, ids given
PATCHIFY_CASES = ((1, 1, 4, 4, 4, 1, True), (2, 3, 8, 16, 4, 3, True), (1, 5, 16, 32, 16, 2, False))          # B, C, H, W, p, n_keep, ids


def unsh_slabs(B, L):
    return (B * L + UM_ROWS - 1) // UM_ROWS


@functools.lru_cache(maxsize=None)
def unsh_case(B, L, n_keep, D, kind="random"):
    """ids_restore: one random permutation per sample; the very last row is a removed one wherever anything is removed, so that a last
    slab of one row carries a term of the mask-token sum. Truth: cat / gather + pos in float64 and its autograd."""
    g = _gen(B, L, n_keep, D, kind == "int", 23)
    ids = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    if n_keep < L and ids[-1, -1] < n_keep:
        j = int(torch.argmax(ids[-1]))
        ids[-1, -1], ids[-1, j] = ids[-1, j].clone(), ids[-1, -1].clone()
    emb, mt, pos, gr = (_rand(s, g, kind) for s in ((B, n_keep, D), (D,), (L, D), (B, L, D)))
    e, m = emb.double().clone().requires_grad_(True), mt.double().clone().requires_grad_(True)
    cat = torch.cat([e, m.view(1, 1, D).expand(B, L - n_keep, D)], 1)
    out = torch.gather(cat, 1, ids.unsqueeze(-1).expand(-1, -1, D)) + pos.double()
    out.backward(gr.double())
    T = dict(out=out.detach(), demb=e.grad, dmask_token=m.grad if m.grad is not None else torch.zeros(D, dtype=torch.float64))
    return dict(B=B, L=L, n_keep=n_keep, D=D, kind=kind, ids=ids, emb=emb, mask_token=mt, pos=pos, g=gr, T=T)


def check_unsh(c, got, rep=None):
    """got: any of out, demb, dmask_token."""
    rep = rep or Report("unshuffle B%d L%d keep%d D%d %s" % (c["B"], c["L"], c["n_keep"], c["D"], c["kind"]))
    T = c["T"]
    for k in ("out", "demb"):
        if k in got:
            rep.exact(k, got[k], T[k])
    if "dmask_token" in got:
        if c["kind"] == "int" or c["n_keep"] == c["L"]:
            rep.exact("dmask_token", got["dmask_token"], T["dmask_token"])
        else:
            rep.f32_class("dmask_token", got["dmask_token"], T["dmask_token"])
    return rep


def unsh_restated(c, mutant=None):
    """unshuffle_fwd_kernel, unshuffle_bwd_scatter, and the mask-token sum in its two stages: per slab of UM_ROWS rows the removed rows
    added in turn, then sum_partials: 16 groups of every 16th slab, the groups added in turn."""
    B, L, n_keep, D, ids = c["B"], c["L"], c["n_keep"], c["D"], c["ids"]
    src = torch.cat([c["emb"], c["mask_token"].view(1, 1, D).expand(B, L, D)], 1)
    out = torch.gather(src, 1, torch.where(ids < n_keep, ids, torch.full_like(ids, n_keep)).unsqueeze(-1).expand(-1, -1, D)) + c["pos"]
    demb = torch.full((B, n_keep, D), float("nan"))
    for b in range(B):
        kept = ids[b] < n_keep
        demb[b, ids[b][kept]] = c["g"][b][kept]
    rows = B * L
    flat = ids.reshape(-1)
    rem = flat > n_keep if mutant == "threshold_gt_n_keep" else flat >= n_keep
    if mutant == "kept_rows_in_mask_token_sum":
        rem = torch.ones_like(rem)
    nb = unsh_slabs(B, L)
    gp = torch.zeros(nb * UM_ROWS, D)
    gp[:rows] = torch.where(rem[:, None], c["g"].reshape(rows, D), torch.zeros(()))
    gp = gp.view(nb, UM_ROWS, D)
    part = torch.zeros(nb, D)
    for i in range(UM_ROWS):
        part = part + gp[:, i]
    if mutant == "last_slab_dropped" and nb > 1:
        part = part[:-1]
    if mutant == "slabs_past_16_dropped":
        part = part[:FOLD_GROUPS]
    grp = torch.zeros(FOLD_GROUPS, D)
    for s in range(part.shape[0]):
        grp[s % FOLD_GROUPS] = grp[s % FOLD_GROUPS] + part[s]
    tot = torch.zeros(D)
    for i in range(FOLD_GROUPS):
        tot = tot + grp[i]
    if mutant == "columns_past_256_dropped":
        tot[UM_COLS:] = float("nan")
    return dict(out=out, demb=demb, dmask_token=tot)


@functools.lru_cache(maxsize=None)
def gather_case(B, n, L, D, with_ids, kind="random"):
    g = _gen(B, n, L, D, with_ids, kind == "int", 31)
    x, table = _rand((B, n, D), g, kind), _rand((L, D), g, kind)
    ids = torch.stack([torch.randperm(L, generator=g)[:n] for _ in range(B)]) if with_ids else None
    tok = ids if with_ids else torch.arange(L).expand(B, L)
    return dict(B=B, n=n, L=L, D=D, x=x, table=table, ids=ids, T=x.double() + table.double()[tok], restated=x + table[tok])


@functools.lru_cache(maxsize=None)
def patchify_case(B, C, H, W, p, n_keep, with_ids):
    """cols[(b, j), c * p * p + py * p + px] = x[b, c, gy * p + py, gx * p + px] for token ids_keep[b, j] (or j)."""
    g = _gen(B, C, H, W, p, n_keep, with_ids, 37)
    gh, gw = H // p, W // p
    L = gh * gw
    x = torch.randn(B, C, H, W, generator=g)
    ids = torch.stack([torch.randperm(L, generator=g)[:n_keep] for _ in range(B)]) if with_ids else None
    cols = x.reshape(B, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, L, C * p * p)
    if with_ids:
        cols = torch.gather(cols, 1, ids.unsqueeze(-1).expand(-1, -1, C * p * p))
    assert with_ids or n_keep == L
    return dict(B=B, C=C, H=H, W=W, p=p, n_keep=n_keep, x=x, ids=ids, T=cols.reshape(B * n_keep, C * p * p).contiguous())


# ================================================================================================================ density noise, masking
DENS_SHAPES = ((1, 1, 4, 4, 4), (2, 5, 8, 12, 4), (1, 3, 64, 32, 32))
MASK_CASES = ((1, 257, 128), (1, 4096, 2048), (2, 9, 0), (2, 9, 9))         # B, L, len_keep
MASK_SPECIAL_ROW = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, -0.0, float("nan"), 0.0, float("-inf"), float("inf"), -1.0)
MASK_SPECIAL_KEEP = 6


@functools.lru_cache(maxsize=None)
def density_case(B, C, H, W, p, sign, kind="random"):
    """|sum over bins| averaged per patch, negated for sign < 0. Integers: the exact integer sum divided once in float32."""
    g = _gen(B, C, H, W, p, kind == "int", 41)
    x = torch.randint(-3, 4, (B, C, H, W), generator=g).float() if kind == "int" else torch.randn(B, C, H, W, generator=g)
    gh, gw = H // p, W // p
    s = x.double().sum(1).abs().reshape(B, gh, p, gw, p).sum((2, 4)).reshape(B, gh * gw)
    c = dict(B=B, C=C, H=H, W=W, p=p, sign=sign, kind=kind, x=x, T=sign * s / (p * p))
    if kind == "int":
        c["E"] = sign * (s.float() / float(p * p))
    return c


def check_density(c, got, rep=None):
    rep = rep or Report("density %dx%dx%dx%d/%d sign%+d %s" % (c["B"], c["C"], c["H"], c["W"], c["p"], c["sign"], c["kind"]))
    rep.f32_class("noise", got, c["T"])
    if "E" in c:
        rep.exact("noise (integers)", got, c["E"])
    return rep


def density_restated(c, mutant=None):
    """density_kernel: the bins added in order, abs, the window's p * p values added one after the other row-major, one division."""
    x, p = c["x"], c["p"]
    B, C, H, W = x.shape
    t = x[:, 0].abs() if mutant == "abs_before_bin_sum" else x[:, 0]
    for ch in range(1, C):
        t = t + (x[:, ch].abs() if mutant == "abs_before_bin_sum" else x[:, ch])
    gh, gw = H // p, W // p
    cells = t.abs().reshape(B, gh, p, gw, p).permute(0, 1, 3, 2, 4).reshape(B, gh * gw, p * p)
    s = torch.zeros(B, gh * gw)
    for e in range(p * p):
        s = s + cells[:, :, e]
    m = s / float(p * p)
    return -m if c["sign"] < 0 else m


@functools.lru_cache(maxsize=None)
def mask_case(B, L, len_keep, special=False):
    """Truth: torch.argsort(stable=True), its inverse, mask = 1 where the rank is >= len_keep. Noise with ties (two decimals)."""
    if special:
        noise = torch.tensor([MASK_SPECIAL_ROW, MASK_SPECIAL_ROW[::-1]])
        B, L = noise.shape
    else:
        noise = (torch.rand(B, L, generator=_gen(B, L, len_keep, 43)) * 100).round() / 100
    order = torch.argsort(noise, dim=1, stable=True)
    restore = torch.argsort(order, dim=1, stable=True)
    return dict(B=B, L=L, len_keep=len_keep, noise=noise,
                T=dict(ids_keep=order[:, :len_keep].contiguous(), mask=(restore >= len_keep).float(), ids_restore=restore))


def mask_cases():
    return [mask_case(*k) for k in MASK_CASES] + [mask_case(0, 0, MASK_SPECIAL_KEEP, True)]


def mask_restated(c):
    """mask_kernel's rank rule: rank[i] = #{j: noise[j] sorts before noise[i], or equals it with j < i}, NaN last and equal to NaN."""
    v, L, keep = c["noise"], c["L"], c["len_keep"]
    a, b = v[:, None, :], v[:, :, None]                    # a = u (index j, last dim), b = v (index i)
    nan_a, nan_b = a != a, b != b
    lt = (a < b) | (~nan_a & nan_b)
    eq = (a == b) | (nan_a & nan_b)
    j_lt_i = torch.arange(L)[None, None, :] < torch.arange(L)[None, :, None]
    rank = (lt | (eq & j_lt_i)).sum(-1)
    ids_keep = torch.zeros(c["B"], keep, dtype=torch.int64)
    for bb in range(c["B"]):
        sel = rank[bb] < keep
        ids_keep[bb, rank[bb][sel]] = torch.arange(L)[sel]
    return dict(ids_keep=ids_keep, mask=(rank >= keep).float(), ids_restore=rank)


def check_mask(c, got, rep=None):
    rep = rep or Report("mask B%d L%d keep%d" % (c["B"], c["L"], c["len_keep"]))
    for k, v in got.items():
        rep.exact(k, v, c["T"][k])
    return rep


# ================================================================================================================ element-wise entries
EW_GRID_ITEMS = 2048 * 256                 # items one pass of a capped ew_grid launch covers
EW_SIZES = (1, 2, 3, 4, 5, 1003, 2048 * 1024 + 5)
CAST_SIZES = (1, 3, 5, 2048 * 1024 + 5)
TRANSPOSE_SHAPES = ((1, 1), (1, 65), (63, 64), (64, 65), (65, 63))
# -0, NaN, +Inf, 1 + 2^-8 (a tie: down to the even 1), -Inf, 1 + 3 * 2^-8 (a tie: up to the even 1 + 2^-6), 3.4e38 (rounds to Inf),
# 1 + 2^-8 + 2^-20 (above the tie: up)
CAST_SPECIALS = (-0.0, float("nan"), float("inf"), 1.0 + 2.0 ** -8, float("-inf"), 1.0 + 3 * 2.0 ** -8, 3.4e38, 1.0 + 2.0 ** -8 + 2.0 ** -20)
SCALE = f32(0.3)


@functools.lru_cache(maxsize=None)
def ew_case(n, kind="random"):
    g = _gen(n, kind == "int", 47)
    a, b, c = (_rand((n,), g, kind) for _ in range(3))
    ad, bd, cd = a.double(), b.double(), c.double()
    return dict(n=n, kind=kind, a=a, b=b, c=c, T=dict(add2=ad + bd, add3=ad + bd + cd, scale=ad * SCALE),
                restated=dict(add2=a + b, add3=(a + b) + c, scale=a * SCALE))


def check_ew(c, got, rep=None):
    """Sums of two and the product: one rounding, equal to the rounded truth. The sum of three rounds twice: equal to the restatement
    (a + b) + c, f32 class against truth; with integers equal to truth."""
    rep = rep or Report("element-wise n%d %s" % (c["n"], c["kind"]))
    for k, v in got.items():
        if k == "add3" and c["kind"] != "int":
            rep.f32_class(k, v, c["T"][k])
            rep.exact(k + " (a + b) + c", v, c["restated"][k])
        else:
            rep.exact(k, v, c["T"][k])
    return rep


@functools.lru_cache(maxsize=None)
def cast_case(n):
    """float32 data with CAST_SPECIALS at the front (the vector body) and one of them at the very end (the scalar tail where n % 4
    != 0: NaN at n = 1, the tie at n = 3, 1 + 3 * 2^-8 at n = 5 and at the large n)."""
    x = torch.randn(n, generator=_gen(n, 53)) * 3
    sp = torch.tensor(CAST_SPECIALS)
    x[:min(n, sp.numel())] = sp[:n]
    x[n - 1] = sp[n % sp.numel()]
    return dict(n=n, x=x, T=x.bfloat16())


def cast_restated(x, mutant=None):
    if mutant == "cast_truncates":
        return (x.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    return x.bfloat16()


@functools.lru_cache(maxsize=None)
def transpose_case(R, C):
    return torch.randn(R, C, generator=_gen(R, C, 59))


# ================================================================================================================ AdamW
from eventpretrain_amd.optim import CHUNK  # noqa: E402

ADAM_NUMEL = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, 2 * CHUNK + 2)
ADAM_GROUPS = (dict(lr=0.1, weight_decay=0.05), dict(lr=0.03, weight_decay=0.0))
ADAM_GROUP_OF = (0, 1, 0, 1, 0, 1, 0, 1, 0)         # tensor -> group; the parameter without a gradient joins group 1
ADAM_SHADOWS = (3, 6, 7)                            # numel 5, CHUNK + 1, CHUNK + 3
ADAM_TINY = 3                                       # this tensor's gradients are 1e-6: sqrt(v) / bc2_sqrt ~ 1e-7, where eps = 1e-8 shows
ADAM_BETAS, ADAM_EPS, ADAM_GRAD_SCALE = (0.9, 0.95), 1e-8, 0.5
ADAM_LR_FACTORS = (1.0, 0.7, 0.4)                   # three steps with changing lr
ADAM_RESUME_STEP = 100000                           # then load_state_dict with this step and one more step (bias corrections ~ 1)
ADAM_RECIPE = dict(numel=(5, CHUNK + 3), lr=1e-3, weight_decay=0.05, steps=5, grad_scale=1.0)


def adam_truth_step(p, g, m, v, step, lr, wd, grad_scale):
    """torch.optim.AdamW in float64; lr, wd, betas, eps at the float32 values the C ABI's arguments hold. -> p, m, v."""
    b1, b2, eps = f32(ADAM_BETAS[0]), f32(ADAM_BETAS[1]), f32(ADAM_EPS)
    lr, wd = f32(lr), f32(wd)
    g = g.double() * grad_scale
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


def adam_restated_step(p, g, m, v, lp, step, lr, wd, grad_scale, mutant=None):
    """adamw_kernel in float32, operation by operation; the bias corrections as FusedAdamW stages them (from the Python floats, then
    float32). lp: the bf16 shadow before the step or None. -> p, m, v, lp."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    sb = max(step - 1, 1) if mutant == "bias_corrections_of_previous_step" else step
    bc1 = t(1.0 - ADAM_BETAS[0] ** sb)
    bc2_sqrt = t(1.0 - ADAM_BETAS[1] ** sb) if mutant == "bc2_without_sqrt" else t(math.sqrt(1.0 - ADAM_BETAS[1] ** sb))
    b1, b2, eps, lr, wd, gs = t(ADAM_BETAS[0]), t(ADAM_BETAS[1]), t(ADAM_EPS), t(lr), t(wd), t(grad_scale)
    decay, step_size = 1.0 - lr * wd, lr / bc1
    gr = g * gs
    if mutant == "coupled_l2":
        gr, decay = gr + wd * p, t(1.0)
    me = b1 * m + (1.0 - b1) * gr
    gq = g if mutant == "no_grad_scale_in_square" else gr
    ve = b2 * v + (1.0 - b2) * gq * gq
    denom = (torch.sqrt(ve) + eps) / bc2_sqrt if mutant == "eps_inside_bc2_division" else torch.sqrt(ve) / bc2_sqrt + eps
    if mutant == "decay_after_update":
        pe = (p - step_size * (me / denom)) * decay
    else:
        pe = p * decay - step_size * (me / denom)
    tail = p.numel() - p.numel() % 4
    if mutant == "tail_not_updated":
        pe[tail:], me[tail:], ve[tail:] = p[tail:], m[tail:], v[tail:]
    new_lp = None
    if lp is not None:
        new_lp = pe.bfloat16()
        if mutant == "no_shadow_on_tail":
            new_lp[tail:] = lp[tail:]
    return pe, me, ve, new_lp


@functools.lru_cache(maxsize=None)
def adam_case(recipe=False):
    """Parameters of magnitude 0.5 to 1 (so the f32 class on a parameter is 1e-5 absolute = 1e-4 of an update of lr = 0.1), gradients
    ~ N(0, 1) per step, the moments' truth after every step. -> dict(p0, grads[step][tensor], steps: [(step number, lr per group)],
    T[step index][tensor] = (p, m, v))."""
    numel = ADAM_RECIPE["numel"] if recipe else ADAM_NUMEL
    g = _gen(len(numel), recipe, 61)
    p0 = [(torch.rand(n, generator=g) * 0.5 + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() for n in numel]
    if recipe:
        groups, group_of, gs = (dict(lr=ADAM_RECIPE["lr"], weight_decay=ADAM_RECIPE["weight_decay"]),), (0,) * len(numel), ADAM_RECIPE["grad_scale"]
        steps = [(k + 1, (ADAM_RECIPE["lr"],)) for k in range(ADAM_RECIPE["steps"])]
    else:
        groups, group_of, gs = ADAM_GROUPS, ADAM_GROUP_OF, ADAM_GRAD_SCALE
        steps = [(k + 1, tuple(gr["lr"] * f for gr in groups)) for k, f in enumerate(ADAM_LR_FACTORS)]
        steps.append((ADAM_RESUME_STEP + 1, tuple(gr["lr"] for gr in groups)))
    grads = []
    for _ in steps:
        grads.append([torch.randn(n, generator=g) * (1e-6 if (not recipe and i == ADAM_TINY) else 1.0) for i, n in enumerate(numel)])
    frozen = torch.rand(7, generator=g)               # a parameter that never gets a gradient
    state = [(p.double(), torch.zeros(p.numel(), dtype=torch.float64), torch.zeros(p.numel(), dtype=torch.float64)) for p in p0]
    T = []
    for (step, lrs), gk in zip(steps, grads):
        state = [adam_truth_step(p, gk[i], m, v, step, lrs[group_of[i]], groups[group_of[i]]["weight_decay"], gs)
                 for i, (p, m, v) in enumerate(state)]
        T.append(state)
    return dict(numel=numel, groups=groups, group_of=group_of, grad_scale=gs, p0=p0, grads=grads, steps=steps, frozen=frozen, T=T,
                shadows=() if recipe else ADAM_SHADOWS)


def adam_restated(c, mutant=None):
    """Every step of the case through adam_restated_step. -> [step index][tensor] = (p, m, v, lp)."""
    state = [(p.clone(), torch.zeros_like(p), torch.zeros_like(p), p.bfloat16() if i in c["shadows"] else None) for i, p in enumerate(c["p0"])]
    out = []
    for (step, lrs), gk in zip(c["steps"], c["grads"]):
        nxt = []
        for i, (p, m, v, lp) in enumerate(state):
            gi = 0 if mutant == "group_0_for_every_tensor" else c["group_of"][i]
            nxt.append(adam_restated_step(p, gk[i], m, v, lp, step, lrs[gi], c["groups"][gi]["weight_decay"], c["grad_scale"], mutant))
        state = nxt
        out.append(state)
    return out


def check_adam(c, k, got, rep=None, what="adamw"):
    """got[tensor] = (p, m, v, lp or None) after step index k. The shadow equals the step's own parameter in bf16."""
    rep = rep or Report(f"{what} step {c['steps'][k][0]}")
    for i, (p, m, v, lp) in enumerate(got):
        Tp, Tm, Tv = c["T"][k][i]
        n = c["numel"][i]
        rep.f32_class(f"p[{n}]", p, Tp)
        rep.f32_class(f"exp_avg[{n}]", m, Tm)
        rel_elem(rep, f"exp_avg_sq[{n}]", v, Tv)
        if i in c["shadows"]:
            assert lp is not None
            rep.exact(f"shadow[{n}]", lp, p.bfloat16())
    return rep


def worst_by_kind(rep):
    """-> {p, exp_avg, exp_avg_sq, ...: worst ratio} from a Report whose row names end in [numel]."""
    out = {}
    for n, _, w in rep.rows:
        k = n.split("[")[0]
        out[k] = max(out.get(k, 0.0), w)
    return out


# ================================================================================================================ the mutants
# name -> (area, what it is, the case that has to reject it)
MUTANTS = {
    "order_c_py_px": ("rec", "inner order (c, py, px)", (2, 3, 8, 12, 4, 0, "none", "int")),                  # only C > 1 sees it
    "gw_from_H": ("rec", "gw taken from H", (2, 2, 3, 5, 1, 0, "none", "int")),                                # gw != gh
    "biased_variance": ("rec", "biased variance", (2, 2, 3, 5, 1, 1, "none", "random")),                       # P = 2: a factor of 2
    "eps_outside_sqrt": ("rec", "1 / (sqrt(var) + 1e-6)", REC_SPECIAL + (1, "half", "random", True)),           # the patch of variance 1e-6
    "mean_over_all_rows": ("rec", "mean over all rows where the mask mean is due", (3, 1, 64, 96, 16, 0, "half", "random")),
    "no_2_over_P": ("rec", "2 / P missing from dpred", (2, 2, 16, 16, 8, 1, "ones", "random")),
    "rows_past_one_pass_not_written": ("rec", "rows >= 8192 not written", (3, 3, 128, 128, 2, 0, "single", "random")),
    "dpred_ignores_mask": ("rec", "dpred not zero on unmasked rows", (1, 5, 16, 32, 16, 1, "single", "random")),
    "kept_rows_in_mask_token_sum": ("unsh", "kept rows added into the mask-token sum", (3, 24, 12, 64, "int")),
    "last_slab_dropped": ("unsh", "last slab dropped", (5, 13, 6, 1028, "int")),                               # a last slab of one row
    "slabs_past_16_dropped": ("unsh", "slabs >= 16 dropped", (5, 205, 100, 8, "int")),                         # 17 slabs
    "columns_past_256_dropped": ("unsh", "columns >= 256 dropped", (4, 16, 8, 260, "random")),
    "threshold_gt_n_keep": ("unsh", "threshold > n_keep", (3, 700, 1, 8, "int")),
    "decay_after_update": ("adam", "decay applied after the update", 0),
    "coupled_l2": ("adam", "coupled L2 (g += wd p)", 0),
    "bc2_without_sqrt": ("adam", "bc2 without the square root", 0),
    "eps_inside_bc2_division": ("adam", "eps inside the division by bc2_sqrt", 0),                              # the tensor of tiny gradients
    "no_grad_scale_in_square": ("adam", "grad_scale missing from g * g", 0),
    "group_0_for_every_tensor": ("adam", "group 0's lr / wd used for every tensor", 0),
    "tail_not_updated": ("adam", "tail elements not updated", 0),
    "no_shadow_on_tail": ("adam", "shadow not written on the tail", 0),
    "bias_corrections_of_previous_step": ("adam", "bias corrections of step - 1", 1),                          # the second step
    "cast_truncates": ("cast", "truncation where round-to-nearest-even is due", 5),                             # 1 + 3 * 2^-8 in the tail
    "abs_before_bin_sum": ("density", "per-pixel abs taken before the sum over bins", (2, 5, 8, 12, 4, 1, "int")),
}

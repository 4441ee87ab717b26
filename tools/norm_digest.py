#!/usr/bin/env python3
"""One SHA-256 per case and output tensor of the kernels in csrc/norm.hip (LayerNorm forward / backward, the patch-embed pair, the plain
and grouped column sums, BatchNorm) and of the four other users of the 4-wide bf16 pack in evp_common.h (evp_cast, evp_rows_scale_f32,
patchify, the AdamW shadow store): run it from two checkouts on the same GPU and compare the lists line by line. The library is built
with -ffp-contract=off, so a change that keeps the order of the floating-point operations keeps every digest. Inputs are drawn on the
CPU from fixed seeds; the column sums, whose per-column atomics arrive in any order, get integer-valued data (|v| <= 8: every partial
sum is exact). Every case is launched twice and the two launches must agree.

tests/test_gpu_norm_forms.py takes its shapes and launchers from here."""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from eventpretrain_amd import ops, wgrad_plan  # noqa: E402
from eventpretrain_amd._lib import EVP_BF16, EVP_F32, EvpError, call, dt, ptr, stream_ptr  # noqa: E402
from eventpretrain_amd.optim import FusedAdamW  # noqa: E402

EPS = 1e-5
FILL = 7.0                                       # what outputs and workspaces hold before a launch
LN_D = (96, 260, 768, 772, 1100, 2052, 4096)     # every chunks-per-lane instantiation (1, 2, 4, 4, 8, 16, 16), whole and ragged last chunk
LN_FWD_M = (5, 8197)                             # 8197 > 4 rows x 2048 blocks: waves loop
LN_BWD_M = (5, 2053)                             # 2053 at the 512-block cap: five waves get a live second row, the others a dead one
LN_BWD_OPTIONS_AT = (772, 2053)                  # (D, M) where every option of the backward goes both ways
EMBED_D = (96, 772, 1100)
EMBED_M = (5, 2053)
FORMS_D, FORMS_M = (96, 772), (5, 2053)          # the shapes of tests/test_gpu_norm_forms.py
COLSUM_M = 300                                   # two row slabs
COLSUM_N_LD = ((136, 136), (134, 136))
BN_SHAPES = ((130, 260, 0), (130, 262, 0), (130, 260, 1))   # (R, C, view offset in elements); the last two take the scalar width


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def filled(*shape, dtype=torch.float32):
    return torch.full(shape, FILL, dtype=dtype, device="cuda")


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen).cuda()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_operands(M, D, seed):
    gen = torch.Generator().manual_seed(seed)
    p = {k: _randn(gen, M, D) for k in ("x", "x2", "x3", "dy", "gres")}
    p.update(M=M, D=D, gamma=_randn(gen, D), beta=_randn(gen, D))
    return p


def ln_fwd(p, x23, y_dtype):
    """-> dict(y, mean, rstd) of evp_layernorm_fwd on x (+ x2 + x3)."""
    M, D = p["M"], p["D"]
    y, mean, rstd = filled(M, D, dtype=y_dtype), filled(M), filled(M)
    x2, x3 = (p["x2"], p["x3"]) if x23 else (None, None)
    call("evp_layernorm_fwd", ptr(p["x"]), ptr(x2), ptr(x3), ptr(p["gamma"]), ptr(p["beta"]), M, D, EPS, ptr(y), dt(y), ptr(mean), ptr(rstd),
         stream_ptr())
    return dict(y=y, mean=mean, rstd=rstd)


def ln_bwd(p, stats, cs, dy_dtype=torch.float32, x23=False, gres=False, outs="both", affine=True):
    """evp_layernorm_bwd_cs (cs) or evp_layernorm_bwd -> dict(dx, dx_lp, ws [nblk, 3 or 2, D], dgamma, dbeta), None where not asked for.
    stats: the forward's (mean, rstd) of the same x23."""
    M, D = p["M"], p["D"]
    dy = p["dy"].to(dy_dtype)
    dx = filled(M, D) if outs in ("dx", "both") else None
    lp = filled(M, D, dtype=torch.bfloat16) if outs in ("lp", "both") else None
    ws = filled(call("evp_layernorm_bwd_nblk", M), 3 if cs else 2, D)
    dg, db = (filled(D), filled(D)) if affine and not cs else (None, None)
    x2, x3 = (p["x2"], p["x3"]) if x23 else (None, None)
    head = (ptr(dy), dt(dy), ptr(p["x"]), ptr(x2), ptr(x3), ptr(p["gamma"]), ptr(stats[0]), ptr(stats[1]), ptr(p["gres"] if gres else None),
            M, D, ptr(dx), ptr(lp))
    if cs:
        call("evp_layernorm_bwd_cs", *head, ptr(ws), stream_ptr())
    else:
        call("evp_layernorm_bwd", *head, ptr(dg), ptr(db), ptr(ws), stream_ptr())
    return dict(dx=dx, dx_lp=lp, ws=ws, dgamma=dg, dbeta=db)


# ---------------------------------------------------------------------------------------------------------------- patch embed
def embed_operands(M, D, seed):
    """One sample of n_keep = L = M tokens: y, the upstream gradient g, gamma, beta, a position table and a permutation as ids_keep."""
    gen = torch.Generator().manual_seed(seed)
    return dict(M=M, D=D, y=_randn(gen, M, D), g=_randn(gen, M, D), gamma=_randn(gen, D), beta=_randn(gen, D), pos=_randn(gen, M, D),
                ids=torch.randperm(M, generator=gen).view(1, M).cuda())


def embed_fwd(p, pos=False, ids=False):
    M, D = p["M"], p["D"]
    out, mean, rstd = filled(M, D), filled(M), filled(M)
    call("evp_embed_post_fwd", ptr(p["y"]), ptr(p["gamma"]), ptr(p["beta"]), ptr(p["pos"] if pos else None), ptr(p["ids"] if ids else None),
         1, M, M, D, EPS, ptr(out), ptr(mean), ptr(rstd), stream_ptr())
    return dict(out=out, mean=mean, rstd=rstd)


def embed_bwd(p, stats, dy_dtype=torch.float32, affine=True):
    M, D = p["M"], p["D"]
    dy, ws = filled(M, D, dtype=dy_dtype), filled(call("evp_layernorm_bwd_nblk", M), 2, D)
    dg, db = (filled(D), filled(D)) if affine else (None, None)
    call("evp_embed_post_bwd", ptr(p["g"]), ptr(p["y"]), ptr(p["gamma"]), ptr(p["beta"]), ptr(stats[0]), ptr(stats[1]), M, D, ptr(dy), dt(dy),
         ptr(dg), ptr(db), ptr(ws), stream_ptr())
    return dict(dy=dy, ws=ws, dgamma=dg, dbeta=db)


# ---------------------------------------------------------------------------------------------------------------- column sums
def colsum_operands():
    """[(x [M, ld] with integer values in -8..8, N)] over COLSUM_N_LD x (f32, bf16)."""
    gen = torch.Generator().manual_seed(31)
    return [(torch.randint(-8, 9, (COLSUM_M, ld), generator=gen).to(dtype).cuda(), N)
            for (N, ld) in COLSUM_N_LD for dtype in (torch.float32, torch.bfloat16)]


def colsum(x, N):
    """evp_colsum over the first N of x's ld columns -> out [N + 8]; the 8 behind N must keep FILL."""
    M, ld = x.shape
    out = filled(N + 8)
    call("evp_colsum", ptr(x), dt(x), M, N, ld, ptr(out), None, stream_ptr())
    return out


def colsum_grouped(problems):
    """One evp_colsum_grouped launch over [(x, N)] -> [out [N + 8]], each zero in front (the grouped form accumulates)."""
    probs = np.zeros(len(problems), dtype=wgrad_plan.COLSUM_DT)
    outs = []
    for i, (x, N) in enumerate(problems):
        outs.append(filled(N + 8))
        outs[-1][:N] = 0.0
        probs[i] = (x.data_ptr(), outs[-1].data_ptr(), x.shape[0], N, x.shape[1], dt(x), 0)
    items = np.ascontiguousarray(wgrad_plan.colsum_items([(x.shape[0], N) for x, N in problems]), dtype=np.int32)
    pt, it = torch.from_numpy(probs.view(np.uint8)).cuda(), torch.from_numpy(items).cuda()
    call(wgrad_plan.COLSUM, ptr(pt), ptr(it), int(items.shape[0]), stream_ptr())
    torch.cuda.synchronize()                     # pt / it die with this frame
    return outs


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def _view(t, off):
    """A copy of t whose first element sits `off` elements behind a 256-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def batchnorm(R, C, off, io, relu, affine, seed):
    """evp_batchnorm_fwd then _bwd with running statistics -> dict of every output and both workspaces."""
    gen = torch.Generator().manual_seed(seed)
    x, dy = _view(_randn(gen, R, C).to(io), off), _view(_randn(gen, R, C).to(io), off)
    gamma, beta = (_randn(gen, C), _randn(gen, C)) if affine else (None, None)
    rm, rv = _randn(gen, C), torch.rand(C, generator=gen).cuda() + 0.5
    y, dx = _view(filled(R, C, dtype=io), off), _view(filled(R, C, dtype=io), off)
    mean, invstd = filled(C), filled(C)
    dg, db = (filled(C), filled(C)) if affine else (None, None)
    nb = call("evp_batchnorm_nblk", R)
    ws1, ws2 = filled((2 * nb + 2) * C), filled((2 * nb + 2) * C)
    call("evp_batchnorm_fwd", ptr(x), dt(x), R, C, ptr(gamma), ptr(beta), EPS, 0.1, int(relu), ptr(y), ptr(mean), ptr(invstd), ptr(rm), ptr(rv),
         ptr(ws1), stream_ptr())
    call("evp_batchnorm_bwd", ptr(dy), ptr(x), ptr(y), dt(x), R, C, ptr(gamma), ptr(mean), ptr(invstd), int(relu), ptr(dx), ptr(dg), ptr(db),
         ptr(ws2), stream_ptr())
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, ws_fwd=ws1, dx=dx, dgamma=dg, dbeta=db, ws_bwd=ws2)


# ---------------------------------------------------------------------------------------------------------------- the other pack sites
def pack_sites():
    """One small case per user of the 4-wide pack outside norm.hip -> [(tag, dict of outputs)] (a list of launchers, see _emit)."""
    gen = torch.Generator().manual_seed(77)
    x = _randn(gen, 37, 52)
    u = torch.rand(3, generator=gen).cuda()
    res = _randn(gen, 37, 52)
    img = _randn(gen, 2, 3, 32, 32)
    ids = torch.stack([torch.randperm(16, generator=gen)[:7] for _ in range(2)]).cuda()
    w0, grad = torch.randn(1003, generator=gen), torch.randn(1003, generator=gen)

    def cast_there_and_back():
        lp = ops.cast(x.view(-1)[:1923], torch.bfloat16)         # 480 whole groups of four and a tail of three
        return dict(bf16=lp, f32=ops.cast(lp, torch.float32))

    def rows_scale():
        out, lp = ops.rows_scale(x, u, 0.7, 13, res=res, want_out=True, want_lp=True)
        return dict(out=out, lp=lp)

    def patchify():
        old = ops._compute_dtype
        ops.set_compute_dtype(torch.bfloat16)
        try:
            return dict(cols=ops._gather_nchw(img, ids, 8)[0])
        finally:
            ops.set_compute_dtype(old)

    def adamw():
        w = torch.nn.Parameter(w0.clone().cuda())
        w.grad = grad.clone().cuda()
        w._evp_lp, w._evp_lp_version = filled(1003, dtype=torch.bfloat16), w._version
        FusedAdamW([w], lr=1e-2, weight_decay=0.05).step()
        return dict(p=w.detach(), shadow=w._evp_lp)

    return [("evp_cast 1923 f32->bf16->f32", cast_there_and_back), ("evp_rows_scale_f32 37x52 + res + lp", rows_scale),
            ("evp_patchify 2x3x32x32 p=8 keep 7 bf16", patchify), ("FusedAdamW 1003 + shadow", adamw)]


# ---------------------------------------------------------------------------------------------------------------- the list
def _emit(tag, fn):
    """Launch twice, demand equal outputs, print one line with a digest per output that was asked for."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    parts = []
    for k, v in a.items():
        if v is None:
            continue
        assert torch.equal(v.view(torch.uint8), b[k].view(torch.uint8)), f"{tag}: two launches differ in {k}"
        parts.append(f"{k} {digest(v)}")
    print(f"{tag:72s} " + " ".join(parts), flush=True)


def _dn(d):
    return str(d)[6:]


def main():
    f32, bf16 = torch.float32, torch.bfloat16
    for D in LN_D:
        for M in LN_FWD_M:
            p = ln_operands(M, D, seed=100 + D)
            for x23, yd in itertools.product((False, True), (f32, bf16)):
                _emit(f"ln_fwd M={M} D={D} x23={int(x23)} y={_dn(yd)}", lambda: ln_fwd(p, x23, yd))
        for M in LN_BWD_M:
            p = ln_operands(M, D, seed=200 + D)
            stats = {x23: (lambda f: (f["mean"], f["rstd"]))(ln_fwd(p, x23, f32)) for x23 in (False, True)}
            every = (D, M) == LN_BWD_OPTIONS_AT
            for cs in (False, True):
                name = "ln_bwd_cs" if cs else "ln_bwd"
                if cs and D == 4096:
                    try:
                        ln_bwd(p, stats[True], True)
                        raise AssertionError("evp_layernorm_bwd_cs accepted D = 4096")
                    except EvpError as e:
                        print(f"{name} M={M} D={D} refused: {e}", flush=True)
                    continue
                opts = itertools.product((f32, bf16), (False, True), (False, True), ("dx", "lp", "both"), (True,) if cs else (False, True)) \
                    if every else [(f32, True, True, "both", True), (bf16, True, True, "both", True)]
                for dyd, x23, gres, outs, affine in opts:
                    _emit(f"{name} M={M} D={D} dy={_dn(dyd)} x23={int(x23)} gres={int(gres)} out={outs} affine={int(affine)}",
                          lambda: ln_bwd(p, stats[x23], cs, dyd, x23, gres, outs, affine))
    for D in EMBED_D:
        for M in EMBED_M:
            p = embed_operands(M, D, seed=300 + D)
            for pos, ids in itertools.product((False, True), (False, True)):
                _emit(f"embed_post_fwd M={M} D={D} pos={int(pos)} ids={int(ids)}", lambda: embed_fwd(p, pos, ids))
            f = embed_fwd(p)
            for dyd, affine in itertools.product((f32, bf16), (False, True)):
                _emit(f"embed_post_bwd M={M} D={D} dy={_dn(dyd)} affine={int(affine)}", lambda: embed_bwd(p, (f["mean"], f["rstd"]), dyd, affine))
    problems = colsum_operands()
    for x, N in problems:
        _emit(f"colsum M={x.shape[0]} N={N} ld={x.shape[1]} {_dn(x.dtype)}", lambda: dict(out=colsum(x, N)))
    for pair in (problems[0:2], problems[2:4], problems[1:3]):      # each one launch of two problems of mixed dtype
        tag = " + ".join(f"N={N} ld={x.shape[1]} {_dn(x.dtype)}" for x, N in pair)
        _emit(f"colsum_grouped M={COLSUM_M} {tag}", lambda: {f"out{i}": o for i, o in enumerate(colsum_grouped(pair))})
    for (R, C, off), io, relu, affine in itertools.product(BN_SHAPES, (f32, bf16), (0, 1), (False, True)):
        _emit(f"batchnorm R={R} C={C} offset={off} {_dn(io)} relu={relu} affine={int(affine)}",
              lambda: batchnorm(R, C, off, io, relu, affine, seed=400 + C))
    for tag, fn in pack_sites():
        _emit(tag, fn)


if __name__ == "__main__":
    main()

"""Thin Python layer over the C-ABI: tensor -> pointer plumbing and the torch.autograd.Function wrappers that make
the HIP kernels differentiable building blocks of the reference's modules.

Precision modes (set with `set_compute_dtype`):
  * torch.float32  -- "parity mode": exact-f32 MFMA GEMMs, f32 activations; checked against the CPU oracle to 1e-4.
  * torch.bfloat16 -- "throughput mode": bf16 MFMA GEMMs with f32 accumulation, bf16 GEMM operands, f32 residual
                      stream / LayerNorm statistics / softmax / loss / optimizer state.
Every tensor handed to a kernel is allocated by PyTorch; all arithmetic happens in libevtpretrain.so.
"""
import ctypes as C
import math
import os

import numpy as np

import torch

from . import _lib, wgrad_plan
from ._lib import (ACT_DGELU, ACT_DRELU, ACT_GELU, ACT_NONE, ACT_RELU, EVP_BF16, EVP_F32, GemmDesc, call, dt, ptr,
                   stream_ptr)

_compute_dtype = torch.float32


def set_compute_dtype(dtype):
    """torch.float32 (parity mode) or torch.bfloat16 (throughput mode)."""
    global _compute_dtype
    if isinstance(dtype, str):
        dtype = {"fp32": torch.float32, "f32": torch.float32, "float32": torch.float32,
                 "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}[dtype]
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be float32 or bfloat16")
    _compute_dtype = dtype


def get_compute_dtype():
    return _compute_dtype


def _code(dtype):
    return EVP_BF16 if dtype == torch.bfloat16 else EVP_F32


def _chk(t, dtype=None):
    if not t.is_cuda:
        raise _lib.EvpError("tensor is not in device memory; eventpretrain_amd has no CPU path")
    if not t.is_contiguous():
        raise _lib.EvpError("kernel operand must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise _lib.EvpError(f"expected {dtype}, got {t.dtype}")
    return t


# ----------------------------------------------------------------------------------------------------- raw calls
def gemm(a, b, out, *, M, N, K, trans_a=False, trans_b=False, lda=None, ldb=None, ldc=None, bias=None, act=ACT_NONE,
         aux=None, residual=None, alpha=1.0, accumulate=False, batch=(1, 1), stride_a=(0, 0), stride_b=(0, 0),
         stride_c=(0, 0), a_off=0, b_off=0, c_off=0, tile=0, splitk=0):
    """out = epilogue(alpha * A . B^T); offsets/strides in ELEMENTS. See include/evtpretrain.h (evp_gemm)."""
    if not (a.is_cuda and b.is_cuda and out.is_cuda):
        raise _lib.EvpError("gemm operands must be in device memory; eventpretrain_amd has no CPU path")
    if a.dtype != b.dtype:
        raise _lib.EvpError("gemm: A and B must share a dtype")
    d = GemmDesc()
    d.dtype = dt(a)
    d.transA, d.transB = int(trans_a), int(trans_b)
    d.M, d.N, d.K = int(M), int(N), int(K)
    es = a.element_size()
    d.A = a.data_ptr() + a_off * es
    d.lda = int(lda if lda is not None else (M if trans_a else K))
    d.strideA0, d.strideA1 = int(stride_a[0]), int(stride_a[1])
    d.B = b.data_ptr() + b_off * es
    d.ldb = int(ldb if ldb is not None else (N if trans_b else K))
    d.strideB0, d.strideB1 = int(stride_b[0]), int(stride_b[1])
    d.C = out.data_ptr() + c_off * out.element_size()
    d.c_dtype = dt(out)
    d.ldc = int(ldc if ldc is not None else N)
    d.strideC0, d.strideC1 = int(stride_c[0]), int(stride_c[1])
    d.batch0, d.batch1 = int(batch[0]), int(batch[1])
    d.alpha = float(alpha)
    d.bias = ptr(bias)
    d.act = int(act)
    d.aux = ptr(aux)
    d.ldaux = d.ldc
    d.residual = ptr(residual)
    d.ldres = d.ldc
    d.accumulate = int(accumulate)
    d.tile = int(tile)
    d.splitk = int(splitk)
    call("evp_gemm", C.byref(d), stream_ptr())
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    out = torch.empty_like(x, dtype=dtype)
    call("evp_cast", ptr(_chk(x)), dt(x), ptr(out), dt(out), x.numel(), stream_ptr())
    return out


def lp_weight(w):
    """Weight in the compute dtype. In bf16 mode the shadow copy is cached on the Parameter and kept current by
    FusedAdamW (which writes it in the same kernel that updates the f32 master weight)."""
    if _compute_dtype == torch.float32:
        return w.detach()
    sh = getattr(w, "_evp_lp", None)
    if sh is None or getattr(w, "_evp_lp_version", -1) != w._version or sh.device != w.device:
        sh = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
        call("evp_cast", ptr(_chk(w.detach())), EVP_F32, ptr(sh), EVP_BF16, w.numel(), stream_ptr())
        w._evp_lp = sh
        w._evp_lp_version = w._version
    return sh


def refresh_lp_shadows(params):
    """Re-cast the f32 master weights into their EXISTING bf16 shadow buffers (same addresses: captured HIP graphs keep
    reading them). Needed after weights were changed outside FusedAdamW, e.g. by load_state_dict."""
    for w in params:
        sh = getattr(w, "_evp_lp", None)
        if sh is not None and sh.device == w.device:
            call("evp_cast", ptr(_chk(w.detach())), EVP_F32, ptr(sh), EVP_BF16, w.numel(), stream_ptr())
            w._evp_lp_version = w._version


def colsum(x2d, out=None):
    M, N = x2d.shape
    out = torch.empty(N, dtype=torch.float32, device=x2d.device) if out is None else out
    nb = call("evp_colsum_nblk", M)
    ws = torch.empty(nb * N, dtype=torch.float32, device=x2d.device)
    call("evp_colsum", ptr(_chk(x2d)), dt(x2d), M, N, N, ptr(out), ptr(ws), stream_ptr())
    return out


def layernorm_fwd(x, gamma, beta, eps, out_dtype, x2=None, x3=None):
    M, D = x.shape
    y = torch.empty(M, D, dtype=out_dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    call("evp_layernorm_fwd", ptr(_chk(x, torch.float32)), ptr(x2), ptr(x3), ptr(gamma), ptr(beta), M, D, float(eps),
         ptr(y), dt(y), ptr(mean), ptr(rstd), stream_ptr())
    return y, mean, rstd


# Side record of a residual-stream gradient, set as an attribute on the tensor by the LayerNorm backward that made it: its
# bf16 copy (the next GEMM's operand, written by the same kernel), the per-block column sums of it (the proj / fc2 bias
# gradient) and the version it describes. Autograd hands the tensor object itself (or a view of it) to the one consumer; a
# gradient that autograd summed from several is a new tensor without the record, or an old one whose version has moved.
_use_grad_side = os.environ.get("EVP_GRAD_SIDE", "1") != "0"


def set_grad_side(flag):
    """A/B switch: bf16 copy + bias column sums of the residual-stream gradient handed from LayerNorm backward to the next
    block (default) or a cast kernel and a full column sum per use."""
    global _use_grad_side
    _use_grad_side = bool(flag)


def _side_put(dx, lp, colsum_part):
    dx._evp_side = (lp, colsum_part, dx._version)


def _side_take(g):
    """(bf16 copy, column-sum partials) of exactly `g`, once; (None, None) without a record that still describes it."""
    t = g if hasattr(g, "_evp_side") else g._base           # the block below returns g0.view(B, N, D): look on the base too
    rec = getattr(t, "_evp_side", None)
    if rec is None:
        return None, None
    del t._evp_side                                         # one use: the bf16 copy is not pinned beyond it
    lp, colsum_part, version = rec
    if version != g._version or not g.is_contiguous() or g.numel() != t.numel() or g.data_ptr() != t.data_ptr():
        return None, None
    return lp, colsum_part


def _norm_defer(params, D):
    return params is not None and D % 8 == 0 and _deferred.can_defer(params[0]) and _deferred.can_defer(params[1])


def _norm_grads(params, D, M, device, n_partial_rows=2):
    """Where a LayerNorm backward kernel over M rows leaves d gamma / d beta: -> (ws, dgamma, dbeta, finish). The kernel
    writes per-block partials into ws [nblk, n_partial_rows * D] (d gamma | d beta | ...). With `params=(weight, bias)` leaf
    Parameters that can take deferred gradients, dgamma and dbeta are None (the kernel skips its own reduction) and
    finish(), called after the kernel, queues the two partial rows for the step's grouped column-sum launch."""
    defer = _norm_defer(params, D)
    ws = torch.empty(call("evp_layernorm_bwd_nblk", M), n_partial_rows * D, dtype=torch.float32, device=device)
    dgamma = dbeta = None
    if not defer:
        dgamma = torch.empty(D, dtype=torch.float32, device=device)
        dbeta = torch.empty(D, dtype=torch.float32, device=device)

    def finish():
        if defer:
            _deferred.colsum(params[0], ws[:, :D])
            _deferred.colsum(params[1], ws[:, D:2 * D])
    return ws, dgamma, dbeta, finish


def layernorm_bwd(dy, x, gamma, mean, rstd, gres=None, x2=None, x3=None, want_lp=False, params=None, side=False):
    """Returns (dx f32, dx_lp bf16|None, dgamma, dbeta); dgamma / dbeta are None where `params` take them deferred (see
    _norm_grads). `side` (deferred mode only): the kernel also leaves per-block column sums of dx, and (bf16 copy, those
    partials) are recorded on dx for whoever receives it as its incoming gradient (_side_take)."""
    M, D = x.shape
    dx = torch.empty(M, D, dtype=torch.float32, device=x.device)
    dx_lp = torch.empty(M, D, dtype=torch.bfloat16, device=x.device) if want_lp else None
    # (the three-partial-row kernel keeps 4 rows x 3 D floats in LDS: D <= 3412; wider rows take the plain kernel below and the
    # consumer of dx casts / column-sums it itself)
    cs = side and _use_grad_side and 4 * 3 * D * 4 <= 160 * 1024 and _norm_defer(params, D)
    ws, dgamma, dbeta, finish = _norm_grads(params, D, M, x.device, 3 if cs else 2)
    if cs:
        call("evp_layernorm_bwd_cs", ptr(_chk(dy)), dt(dy), ptr(x), ptr(x2), ptr(x3), ptr(gamma), ptr(mean), ptr(rstd),
             ptr(gres), M, D, ptr(dx), ptr(dx_lp), ptr(ws), stream_ptr())
    else:
        call("evp_layernorm_bwd", ptr(_chk(dy)), dt(dy), ptr(x), ptr(x2), ptr(x3), ptr(gamma), ptr(mean), ptr(rstd),
             ptr(gres), M, D, ptr(dx), ptr(dx_lp), ptr(dgamma), ptr(dbeta), ptr(ws), stream_ptr())
    finish()
    if cs:
        _side_put(dx, dx_lp, ws[:, 2 * D:])
    return dx, dx_lp, dgamma, dbeta


_use_fused_attention = True
_use_window_mfma = True


def set_window_mfma(flag):
    """A/B switch: Swin window attention on the MFMA kernels (default, bf16 mode) or on the f32 LDS kernels."""
    global _use_window_mfma
    _use_window_mfma = bool(flag)


def set_fused_attention(flag):
    """A/B switch: the fused per-head kernels (default) or the batched-GEMM + softmax formulation."""
    global _use_fused_attention
    _use_fused_attention = bool(flag)


def fused_attention_ok(dtype, N, dh):
    return _use_fused_attention and bool(call("evp_attention_fused_supported", _code(dtype), int(N), int(dh)))


def attention_fused_fwd(qkv, B, N, heads, dh, want_probs=False):
    """-> (out [B*N, h*dh] bf16, lse [B,h,N] f32, probs [B,h,N,ldp] bf16 | None)."""
    dev = qkv.device
    out = torch.empty(B * N, heads * dh, dtype=qkv.dtype, device=dev)
    lse = torch.empty(B, heads, N, dtype=torch.float32, device=dev)
    ldp = (N + 7) // 8 * 8
    probs = torch.empty(B, heads, N, ldp, dtype=qkv.dtype, device=dev) if want_probs else None
    call("evp_attention_fused_fwd", ptr(_chk(qkv)), B, N, heads, dh, float(dh) ** -0.5, ptr(out), ptr(lse), ptr(probs), ldp,
         stream_ptr())
    return out, lse, probs


def attention_fused_bwd(qkv, out, dout, lse, B, N, heads, dh):
    dqkv = torch.empty_like(qkv)
    call("evp_attention_fused_bwd", ptr(qkv), ptr(out), ptr(_chk(dout)), ptr(lse), B, N, heads, dh, float(dh) ** -0.5, ptr(dqkv),
         stream_ptr())
    return dqkv


def attention_fwd(qkv, B, N, heads, dh):
    """qkv [B*N, 3*h*dh] (compute dtype) -> (probs [B,h,N,ldp], out [B*N, h*dh])."""
    ldp = (N + 7) // 8 * 8
    dev = qkv.device
    scores = torch.empty(B * heads * N * ldp, dtype=torch.float32, device=dev)
    probs = torch.empty(B, heads, N, ldp, dtype=qkv.dtype, device=dev)
    out = torch.empty(B * N, heads * dh, dtype=qkv.dtype, device=dev)
    call("evp_attention_fwd", ptr(_chk(qkv)), dt(qkv), B, N, heads, dh, float(dh) ** -0.5, ptr(scores), ptr(probs), ldp,
         ptr(out), stream_ptr())
    return probs, out


def attention_bwd(qkv, probs, dout, B, N, heads, dh):
    ldp = probs.shape[-1]
    dev = qkv.device
    dp = torch.empty(B * heads * N * ldp, dtype=torch.float32, device=dev)
    ds = dp if qkv.dtype == torch.float32 else torch.empty(B * heads * N * ldp, dtype=qkv.dtype, device=dev)
    dqkv = torch.empty_like(qkv)
    call("evp_attention_bwd", ptr(qkv), ptr(probs), ptr(_chk(dout)), dt(qkv), B, N, heads, dh, float(dh) ** -0.5, ldp,
         ptr(dp), ptr(ds), ptr(dqkv), stream_ptr())
    return dqkv


def attention_dropout_fwd(qkv, B, N, heads, dh, rd):
    """Attention core with dropout on the probabilities (vit_block.py:134-140 with attn_drop > 0): the batched-GEMM formulation, because
    the probabilities have to exist -- scores GEMM (f32), row softmax, evp_dropout_fwd on the probabilities (mask = rd.masks["attn"] when
    given, else drawn from rd's stream), dropped-probabilities x V. -> (P softmax, dropped P, keep mask uint8, out). The fused kernels
    stay what every attn_drop_rate = 0 run (all of the reference's scripts) uses."""
    T = qkv.dtype
    C_ = heads * dh
    tok = 3 * C_
    ldp = (N + 7) // 8 * 8
    dev = qkv.device
    scores = torch.empty(B * heads * N * ldp, dtype=torch.float32, device=dev)
    gemm(qkv, qkv, scores, M=N, N=N, K=dh, lda=tok, ldb=tok, ldc=ldp, batch=(B, heads), stride_a=(N * tok, dh), stride_b=(N * tok, dh),
         stride_c=(heads * N * ldp, N * ldp), b_off=C_, alpha=float(dh) ** -0.5)
    probs = torch.empty(B, heads, N, ldp, dtype=T, device=dev)
    call("evp_softmax_rows", ptr(scores), ptr(probs), dt(probs), B * heads * N, N, ldp, stream_ptr())
    sub = BlockDrop(drop=rd.attn_drop, seed=rd.seed_dev if rd.seed_dev is not None else rd.seed,
                    masks=None if (rd.masks is None or "attn" not in rd.masks) else {"attn": rd.masks["attn"]})
    sub._n = rd.next_offset(probs.numel())
    dropped, mk = dropout_fwd(probs, sub, "attn")
    out = torch.empty(B * N, C_, dtype=T, device=dev)
    gemm(dropped, qkv, out, M=N, N=dh, K=N, trans_b=True, lda=ldp, ldb=tok, ldc=C_, batch=(B, heads), stride_a=(heads * N * ldp, N * ldp),
         stride_b=(N * tok, dh), stride_c=(N * C_, dh), b_off=2 * C_)
    return probs, dropped, mk, out


def attention_dropout_bwd(qkv, probs, dropped, mk, dout, B, N, heads, dh, p_drop):
    """Backward of attention_dropout_fwd: dV = dropped^T dO; dP = mask / (1 - p) * (dO V^T); dS = P * (dP - rowsum(P dP)); dQ, dK."""
    T = qkv.dtype
    C_ = heads * dh
    tok = 3 * C_
    ldp = probs.shape[-1]
    dev = qkv.device
    sP = (heads * N * ldp, N * ldp)
    dqkv = torch.empty_like(qkv)
    dp = torch.empty(B * heads * N * ldp, dtype=torch.float32, device=dev)
    gemm(dout, qkv, dp, M=N, N=N, K=dh, lda=C_, ldb=tok, ldc=ldp, batch=(B, heads), stride_a=(N * C_, dh), stride_b=(N * tok, dh), stride_c=sP,
         b_off=2 * C_)
    dpm = dropout_bwd(dp, mk, p_drop)
    ds = dpm if T == torch.float32 else torch.empty(B * heads * N * ldp, dtype=T, device=dev)
    call("evp_softmax_rows_bwd", ptr(probs), ptr(dpm), ptr(ds), dt(probs), B * heads * N, N, ldp, stream_ptr())
    gemm(dropped, dout, dqkv, M=N, N=dh, K=N, trans_a=True, trans_b=True, lda=ldp, ldb=C_, ldc=tok, batch=(B, heads), stride_a=sP,
         stride_b=(N * C_, dh), stride_c=(N * tok, dh), c_off=2 * C_)
    gemm(ds, qkv, dqkv, M=N, N=dh, K=N, trans_b=True, lda=ldp, ldb=tok, ldc=tok, batch=(B, heads), stride_a=sP, stride_b=(N * tok, dh),
         stride_c=(N * tok, dh), b_off=C_, alpha=float(dh) ** -0.5)
    gemm(ds, qkv, dqkv, M=N, N=dh, K=N, trans_a=True, trans_b=True, lda=ldp, ldb=tok, ldc=tok, batch=(B, heads), stride_a=sP,
         stride_b=(N * tok, dh), stride_c=(N * tok, dh), c_off=C_, alpha=float(dh) ** -0.5)
    return dqkv


def mask_from_noise(noise, mask_ratio):
    """vit.py:75-103 on an explicit noise tensor -> (ids_keep int64, mask f32, ids_restore int64)."""
    B, L = noise.shape
    keep = int(L * (1 - mask_ratio))
    dev = noise.device
    ids_keep = torch.empty(B, keep, dtype=torch.int64, device=dev)
    mask = torch.empty(B, L, dtype=torch.float32, device=dev)
    ids_restore = torch.empty(B, L, dtype=torch.int64, device=dev)
    call("evp_mask_from_noise", ptr(_chk(noise, torch.float32)), B, L, keep, ptr(ids_keep), ptr(mask), ptr(ids_restore),
         stream_ptr())
    return ids_keep, mask, ids_restore


def density_noise(x, patch, sign):
    B, Cc, H, W = x.shape
    out = torch.empty(B, (H // patch) * (W // patch), dtype=torch.float32, device=x.device)
    call("evp_density_noise", ptr(_chk(x, torch.float32)), B, Cc, H, W, patch, float(sign), ptr(out), stream_ptr())
    return out


def add(a, b, c=None):
    out = torch.empty_like(a)
    call("evp_add_f32", ptr(_chk(a, torch.float32)), ptr(_chk(b, torch.float32)), ptr(c), a.numel(), ptr(out), stream_ptr())
    return out


# ----------------------------------------------------------------------------------------------------- deferred grads
class _DeferredGrads:
    """Weight / bias gradients do not feed the backward chain, only the optimizer. In bf16 mode they are therefore
    queued during backward and computed at its end by ONE grouped GEMM launch (thousands of 128x128 tiles: no split-K,
    no tail) and ONE grouped column-sum launch (csrc: evp_gemm_grouped_tn_bf16, evp_colsum_grouped). The autograd
    functions return None for a queued parameter; flush() -- an autograd end-of-backward callback -- writes the
    result straight into `param.grad` (allocating it, or accumulating into an existing one)."""

    def __init__(self):
        self.enabled = True
        self.hold = False               # keep the queue at the end of backward (see build_plan)
        self.w, self.b = [], []
        self.armed = False
        self._pin = {}
        self._capture_pins = []     # pinned tables owned by captured HIP graphs (never rewritten; see _stage)
        self.flat_buffers = []      # flat f32 buffers holding the gradients written by the last flush(es)
        self._flat_consumer = None  # weakref to the data-parallel reducer: without a live consumer the list must not grow
        self.join_streams = []      # side streams that ran part of the backward (split-batch step): flush() waits for them

    def track_flats(self):
        c = self._flat_consumer
        return c is not None and c() is not None

    def arm(self):
        if not self.armed:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self.flush)
                self.armed = True
            except RuntimeError:       # not inside a backward pass: the caller flushes explicitly
                pass

    def can_defer(self, param):
        return (self.enabled and _compute_dtype == torch.bfloat16 and isinstance(param, torch.Tensor) and param.is_leaf
                and param.requires_grad and param.dtype == torch.float32 and param.is_contiguous())

    def wgrad(self, param, dy, x, n_out, k_in, rows, bias_param=None):
        self.w.append(wgrad_plan.WgradProblem(param, dy, x, n_out, k_in, rows, bias_param))
        self.arm()

    def colsum(self, param, x2d):
        self.b.append((param, x2d))
        self.arm()

    def _stage(self, key, arr, dev):
        """numpy bytes -> pinned staging -> fresh device tensor (async H2D).
        Eager: one persistent pinned buffer per table key, guarded by an event so that it is not rewritten before the
        previous step's copy has run. Under HIP-graph capture: a NEW pinned buffer per table, owned by this object for
        the life of the process and never written again -- the graph's H2D node re-reads it at every replay, so it
        must not be shared with later eager steps or with other captures."""
        raw = torch.from_numpy(arr)
        n = raw.numel()
        if torch.cuda.is_current_stream_capturing():
            pin = torch.empty(max(n, 1), dtype=torch.uint8).pin_memory()
            pin[:n].copy_(raw)
            self._capture_pins.append(pin)
            d = torch.empty(n, dtype=torch.uint8, device=dev)
            d.copy_(pin[:n], non_blocking=True)
            return d
        ent = self._pin.get(key)
        if ent is None or ent[0].numel() < n:
            ent = [torch.empty(max(n, 1 << 16), dtype=torch.uint8).pin_memory(), None]
            self._pin[key] = ent
        pin, ev = ent
        if ev is not None:
            ev.synchronize()              # the previous step's H2D copy out of this pinned buffer must have run
        pin[:n].copy_(raw)
        d = torch.empty(n, dtype=torch.uint8, device=dev)
        d.copy_(pin[:n], non_blocking=True)
        ent[1] = torch.cuda.Event()
        ent[1].record()
        return d

    @staticmethod
    def _target(param):
        """(grad tensor to write, accumulate flag)"""
        if param.grad is None:
            param.grad = torch.empty_like(param, memory_format=torch.contiguous_format)
            return param.grad, 0
        if param.grad.dtype != torch.float32 or not param.grad.is_contiguous():
            raise _lib.EvpError("deferred gradients need contiguous float32 .grad tensors")
        return param.grad, 1

    def flush(self):
        """End-of-backward callback: launch everything that was queued (normal mode). While `hold` is set (the step
        executor capturing the forward+backward graph of the data-parallel path) the queue is kept for build_plan()."""
        self.armed = False
        if self.hold:
            return
        for s_ in self.join_streams:
            torch.cuda.current_stream().wait_stream(s_)
        if self.flat_buffers and not self.track_flats():
            self.flat_buffers = []          # leftovers of a reducer that is gone
        for st in self._build(n_chunks=1, static=False):
            st.run()

    def build_plan(self, n_chunks=4):
        """Data-parallel graph mode: turn the queue left by a captured backward into a list of re-runnable launch steps
        with STATIC device tables (the operands live in the graph's private pool, so their addresses repeat at every
        replay). Weight-gradient problems are cut into `n_chunks` launches, each writing its own flat gradient buffer, so
        the all-reduce of one chunk overlaps the next chunk's GEMMs (parallel.OverlappedPlan)."""
        self.armed = False
        return self._build(n_chunks=n_chunks, static=True)

    class _Step:
        def __init__(self, entry, pt, it, n_items, flats, zero, keep, post=()):
            self.entry, self.pt, self.it, self.n_items = entry, pt, it, n_items
            self.flats = flats          # flat gradient buffers complete once this step has run
            self.zero = zero            # buffers that accumulate with atomics: cleared before every run
            self.keep = keep            # operand tensors referenced by the tables
            self.post = list(post)      # split-K reductions: (workspace, out, n_slices, numel, accumulate)
            self.round = 0              # steps of one round touch disjoint gradients (may run concurrently); rounds are ordered

        def run(self):
            for z in self.zero:
                z.zero_()
            call(self.entry, self.pt.data_ptr(), self.it.data_ptr(), self.n_items, stream_ptr())
            for ws, out, ns, numel, acc in self.post:
                call("evp_sum_slices_f32", ws.data_ptr(), out.data_ptr(), ns, numel, acc, stream_ptr())

    def _build(self, n_chunks, static):
        w, b, self.w, self.b = [wgrad_plan.WgradProblem(*q) for q in self.w], self.b, [], []
        steps = []

        def table(key, arr, dev):
            if static:
                return torch.from_numpy(arr.copy()).to(dev)
            return self._stage(key, arr, dev)

        def alloc_fresh(params, dev, zeroed):
            """one flat buffer for the parameters of this launch that have no gradient yet; returns (flat | None, ids)"""
            fresh = [p_ for p_ in dict.fromkeys(params) if p_.grad is None]
            if not fresh:
                return None, set()
            sizes = [(p_.numel() + 63) // 64 * 64 for p_ in fresh]
            flat = (torch.zeros if zeroed else torch.empty)(sum(sizes), dtype=torch.float32, device=dev)
            o = 0
            for p_, n_ in zip(fresh, sizes):
                p_.grad = flat[o:o + p_.numel()].view_as(p_)
                o += n_
            if static or self.track_flats():    # only a reducer (or a plan being built) takes these; otherwise the
                self.flat_buffers.append(flat)  # parameters' .grad views are the only owners and zero_grad frees them
            return flat, {id(p_) for p_ in fresh}

        def target(param, fresh_ids):
            gt, acc = self._target(param)
            return gt, 0 if id(param) in fresh_ids else acc     # first write into the freshly allocated flat slice

        if w:
            dev = w[0].dy.device
            launches, listed = wgrad_plan.layout(w, n_chunks, _use_wgrad_g4, _wgrad_xcd_order)
            b += [(q.bias, q.dy) for q in listed]
            for ln in launches:
                flat, fresh_ids = alloc_fresh([m.q.param for m in ln.members] +
                                              [m.q.bias for m in ln.members if m.route.bias == "fused"], dev, zeroed=False)
                # per member: address and accumulate flag of its gradient (or workspace) and of its fused bias gradient
                dest, post = [], []
                for q, route in ln.members:
                    gt, acc = target(q.param, fresh_ids)
                    cs_ptr, cs_acc = 0, 0
                    if len(route.slices) > 1:
                        numel = q.n_out * q.k_in
                        ws = torch.empty(len(route.slices) * numel, dtype=torch.float32, device=dev)
                        post.append((ws, gt, len(route.slices), numel, acc))
                        gt, acc = ws, 0
                    elif route.bias == "fused":
                        bt, cs_acc = target(q.bias, fresh_ids)
                        cs_ptr = bt.data_ptr()
                    dest.append((gt.data_ptr(), acc, cs_ptr, cs_acc))
                addr = []
                for row in ln.rows:
                    q = ln.members[row.src].q
                    if ln.entry == wgrad_plan.G4:
                        _check_g4_problem(q.n_out, q.k_in, row.k)
                    c_ptr, acc, cs_ptr, cs_acc = dest[row.src]
                    addr.append((q.dy.data_ptr() + row.k0 * q.n_out * 2, q.x.data_ptr() + row.k0 * q.k_in * 2,
                                 c_ptr + max(row.ws_slice, 0) * q.n_out * q.k_in * 4, acc, cs_acc, cs_ptr))
                for name, column in zip(("A", "B", "C", "acc", "cacc", "colsum"), zip(*addr)):
                    ln.probs[name] = column
                pt = table(ln.tag + "p", ln.probs.view(np.uint8), dev)
                it = table(ln.tag + "i", ln.items.view(np.uint8).reshape(-1), dev)
                steps.append(self._Step(ln.entry, pt, it, int(ln.items.shape[0]), [flat] if flat is not None else [], [],
                                        [(m.q.dy, m.q.x) for m in ln.members], post))
                steps[-1].round = ln.round
        if b:
            dev = b[0][1].device
            probs = np.zeros(len(b), dtype=wgrad_plan.COLSUM_DT)
            # fresh bias gradients are slices of ONE flat buffer zeroed by one memset (they accumulate with atomics)
            flat, _ = alloc_fresh([param for param, _ in b], dev, zeroed=True)
            for i, (param, x2d) in enumerate(b):
                M, N = x2d.shape
                gt, acc = self._target(param)
                probs[i] = (x2d.data_ptr(), gt.data_ptr(), M, N, x2d.stride(0), dt(x2d), 0)
            items = wgrad_plan.colsum_items([x2d.shape for _, x2d in b])
            pt = table("bp", probs.view(np.uint8), dev)
            it = table("bi", items.view(np.uint8).reshape(-1), dev)
            st = self._Step(wgrad_plan.COLSUM, pt, it, int(items.shape[0]), [flat] if flat is not None else [],
                            [flat] if (static and flat is not None) else [], [x2d for _, x2d in b])
            # in a plan the short column-sum launch goes first: its all-reduce then hides under the first GEMM chunk
            if static:
                steps.insert(0, st)
            else:
                steps.append(st)
        return steps


def _check_g4_problem(M, N, K):
    """Host check of wgrad_plan.g4_ok before a G4 table is staged: on the device nothing checks it."""
    if not wgrad_plan.g4_ok(M, N, K):
        raise _lib.EvpError(f"G4 weight-gradient problem out of contract: M={M} N={N} K={K} ({wgrad_plan.G4_CONTRACT})")


_wgrad_xcd_order = os.environ.get("EVP_WGRAD_XCD", "1") != "0"
_use_wgrad_g4 = os.environ.get("EVP_WGRAD_G4", "1") != "0"


def set_wgrad_g4(flag):
    """A/B switch: long-K weight gradients with >= 256-wide outputs on the 256x256 G4 body (one wave per SIMD, 32x32x16; default)
    or on 128x128 tiles like the rest."""
    global _use_wgrad_g4
    _use_wgrad_g4 = bool(flag)


def set_wgrad_xcd_order(flag):
    """A/B switch: XCD-aware order of the grouped 256x256 weight-gradient items (default) or the plain problem-major list."""
    global _wgrad_xcd_order
    _wgrad_xcd_order = bool(flag)


_deferred = _DeferredGrads()


def set_deferred_grads(flag):
    """A/B switch: grouped end-of-backward weight/bias gradients (default) or one GEMM / column sum per layer."""
    _deferred.enabled = bool(flag)


def flush_deferred_grads():
    if _deferred.w or _deferred.b:
        _deferred.flush()


def hold_deferred_grads(flag):
    """While set, the end-of-backward callback leaves the queued gradient work in place (for build_deferred_plan)."""
    _deferred.hold = bool(flag)


def build_deferred_plan(n_chunks=4):
    return _deferred.build_plan(n_chunks)


def track_deferred_flat_buffers(consumer):
    """Called by the data-parallel reducer with itself: while that object is alive the flat gradient buffers of each flush
    are kept for take_deferred_flat_buffers(). Without a live consumer nothing is retained (the list would otherwise pin one
    set of gradient buffers per step). Pass None to switch tracking off."""
    import weakref
    _deferred._flat_consumer = weakref.ref(consumer) if consumer is not None else None
    if consumer is None:
        _deferred.flat_buffers = []


def take_deferred_flat_buffers():
    """Flat f32 buffers that hold the deferred gradients written since the last call (their parameters' .grad are
    views into them): the data-parallel reducer all-reduces these in place."""
    out, _deferred.flat_buffers = _deferred.flat_buffers, []
    return out


def _wgrad(dy, x, n_out, k_in, rows, param=None, shape=None, bias_param=None):
    """dW[n_out,k_in] = dy^T x (f32). Returns the gradient, or None when it was queued for the grouped launch
    (then flush() delivers it into param.grad). `bias_param`: the same Linear's bias, whose gradient sum_rows(dy) is
    then produced by the same grouped kernel (or the grouped column sums) -- only pass it when this call is queued
    (see _wgrad_bias)."""
    if param is not None and dy.dtype == torch.bfloat16 and n_out % 8 == 0 and k_in % 8 == 0 and _deferred.can_defer(param):
        _deferred.wgrad(param, dy, x, n_out, k_in, rows, bias_param)
        return None
    dw = torch.empty(n_out, k_in, dtype=torch.float32, device=dy.device)
    gemm(dy, x, dw, M=n_out, N=k_in, K=rows, trans_a=True, trans_b=True, lda=n_out, ldb=k_in)
    return dw if shape is None else dw.view(shape)


def _wgrad_bias(dy, x, n_out, k_in, rows, wparam, bparam, need_w, need_b, dy_f32=None, shape=None, dy_colsum=None):
    """(dW, db) of one Linear. When both can be deferred (bf16 mode, leaf parameters) the bias gradient is attached to the
    weight-gradient problem: the 256x256 grouped kernel sums dy's columns from the A fragments it holds anyway, so dy is
    not read a second time. Otherwise falls back to the separate paths (`dy_f32`: f32 version of dy for the exact sum)."""
    # only where dy exists in bf16 alone (qkv, fc1): proj / fc2 have the f32 residual-stream gradient, whose exact column
    # sum is kept (summing its bf16 copy moved those bias gradients by ~5e-3 of their max)
    fuse = (need_w and need_b and dy_f32 is None and dy.dtype == torch.bfloat16 and n_out % 8 == 0 and k_in % 8 == 0 and
            _deferred.can_defer(wparam) and _deferred.can_defer(bparam))
    if fuse:
        _deferred.wgrad(wparam, dy, x, n_out, k_in, rows, bparam)
        return None, None
    dw = _wgrad(dy, x, n_out, k_in, rows, wparam, shape) if need_w else None
    if need_b and dy_colsum is not None and _deferred.can_defer(bparam):
        _deferred.colsum(bparam, dy_colsum)       # per-block column sums left by the LayerNorm backward: a few rows to add
        return dw, None
    db = _bgrad(dy_f32 if dy_f32 is not None else dy, bparam) if need_b else None
    return dw, db


def _bgrad(x2d, param=None):
    """db[n] = sum_m x2d[m,n] (f32); None when queued (see _wgrad)."""
    if param is not None and x2d.shape[1] % 8 == 0 and _deferred.can_defer(param):
        _deferred.colsum(param, x2d)
        return None
    return colsum(x2d)


# ----------------------------------------------------------------------------------------------------- stochastic regularisers
class BlockDrop:
    """Stochastic regularisers of ONE call of a residual block (reference vit_block.py:241,252-253 / conv_block.py:35,43-49 /
    swin_block.py:257,270-271; timm `drop_path`, nn.Dropout): `u1`, `u2` = float32 [x.shape[0]] uniform draws for the two
    DropPath applications (None = off), keep_prob = 1 - drop_path; `drop` = elementwise dropout rate of the branch outputs and the
    MLP hidden (proj_drop / Mlp.drop), its masks drawn by evp_dropout_fwd from (seed, a per-use offset). `seed` is an int (tests:
    a given stream) or a 1-element int64 DEVICE tensor (draw_drop_seed): the kernel reads it at run time, so a replayed HIP graph --
    whose kernel arguments are frozen at capture -- draws new masks on every replay. A block called with rd=None takes the fused
    fast path (residual add inside the GEMM epilogue)."""

    def __init__(self, u1=None, u2=None, keep_prob=1.0, drop=0.0, seed=0, masks=None, attn_drop=0.0):
        self.u = (u1, u2)
        self.keep_prob = float(keep_prob)
        self.drop = float(drop)
        self.attn_drop = float(attn_drop)           # dropout on the attention probabilities (vit_block.py:127,138; swin_block.py:113,152)
        self.seed_dev = seed if torch.is_tensor(seed) else None
        self.seed = 0 if torch.is_tensor(seed) else int(seed)
        self.masks = masks            # optional explicit uint8 masks {"proj": .., "hidden": .., "fc2": ..} (tests: given-mask parity)
        self._n = 0

    def next_offset(self, numel):
        o = self._n
        self._n += (numel + 3) // 4
        return o


def dropout_fwd(x, rd, key):
    """-> (x * keep / (1 - p), mask uint8) for a contiguous tensor; the mask is rd.masks[key] when given."""
    out = torch.empty_like(x)
    n = x.numel()
    if rd.masks is not None and key in rd.masks:
        mask = _chk(rd.masks[key]).view(-1)
        call("evp_dropout_apply", ptr(_chk(x)), dt(x), ptr(mask), ptr(out), n, 1.0 / (1.0 - rd.drop), stream_ptr())
        return out, mask
    mask = torch.empty(n, dtype=torch.uint8, device=x.device)
    call("evp_dropout_fwd", ptr(_chk(x)), dt(x), ptr(out), ptr(mask), n, rd.drop, rd.seed, ptr(rd.seed_dev), rd.next_offset(n), stream_ptr())
    return out, mask


def dropout_bwd(g, mask, p):
    out = torch.empty_like(g)
    call("evp_dropout_apply", ptr(_chk(g)), dt(g), ptr(mask), ptr(out), g.numel(), 1.0 / (1.0 - p), stream_ptr())
    return out


def rows_scale(x, u, keep_prob, rows_per_sample, res=None, want_out=True, want_lp=False):
    """(res + s_b * x, bf16(s_b * x)) with s_b = floor(keep_prob + u[b]) / keep_prob per sample b (evp_rows_scale_f32)."""
    M, D = x.shape
    out = torch.empty(M, D, dtype=torch.float32, device=x.device) if want_out else None
    lp = torch.empty(M, D, dtype=torch.bfloat16, device=x.device) if want_lp else None
    call("evp_rows_scale_f32", ptr(_chk(x, torch.float32)), ptr(u), float(keep_prob), ptr(res), M, D, int(rows_per_sample), ptr(out), ptr(lp),
         stream_ptr())
    return out, lp


def _branch_residual(a, w, bias, res, rd, which, rps, key):
    """Residual-stream output of one branch, a [M,K] and w [N,K]: res + drop_path(dropout(a . w^T + bias)). rd None: fused in the
    GEMM epilogue. `key`: the branch's dropout mask in rd.masks; None for a branch without dropout of its own."""
    (M, K), N = a.shape, w.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    if rd is None:
        gemm(a, w, out, M=M, N=N, K=K, bias=bias, residual=res)
        return out, None
    gemm(a, w, out, M=M, N=N, K=K, bias=bias)
    mk = None
    if key is not None and rd.drop > 0:
        out, mk = dropout_fwd(out, rd, key)
    y, _ = rows_scale(out, rd.u[which], rd.keep_prob, rps, res=res)
    return y, mk


def _branch_grad(g, rd, which, rps, mk, T, side, lp=None):
    """Gradient entering a residual branch whose output was added as res + drop_path(dropout(.)), g being the f32 gradient
    of the sum: -> (f32 for the exact bias column sum, operand of the GEMMs in dtype T, column-sum partials | None).
    `side`: g may carry the record of the LayerNorm backward that made it (_side_take); `lp`: its bf16 copy where the
    caller holds one."""
    side_lp, cs = _side_take(g) if side else (None, None)
    if rd is None:
        if lp is None:
            lp = side_lp if side_lp is not None else cast(g, T)
        return g, lp, cs
    # the branch sees s_b * g (DropPath) times the dropout mask of its output
    gs, gs_lp = rows_scale(g, rd.u[which], rd.keep_prob, rps, want_lp=T == torch.bfloat16 and mk is None)
    if mk is not None:
        gs = dropout_bwd(gs, mk, rd.drop)
    return gs, (gs_lp if gs_lp is not None else cast(gs, T)), None


def _linear_bwd(dy, x, wl, wparam, bparam, need_w, need_b, dy_f32=None, dy_colsum=None, act=ACT_NONE, aux=None):
    """Backward of a Linear (or 1x1 conv) inside a residual block, y [M,N] = x [M,K] . wl^T + bias with wl [N,K] = wparam in the
    compute dtype: -> (dW in wparam's shape, db, dx [M,K] in dy's dtype). The weight gradient, with the bias on the same problem
    (_wgrad_bias; dy_f32 / dy_colsum as there), is queued first -- the order of the deferred queue -- then dx = act'(dy . wl) is
    launched (`act`, `aux`: the GEMM epilogue's). LinearFn, LinearBNFn and _rows_linear_bwd are not on this: they take _wgrad and
    _bgrad, the bias apart from the weight-gradient problem, and moving them here would change the deferred queue."""
    (M, N), K = dy.shape, x.shape[1]
    dw, db = _wgrad_bias(dy, x, N, K, M, wparam, bparam, need_w, need_b, dy_f32=dy_f32, shape=tuple(wparam.shape), dy_colsum=dy_colsum)
    dx = torch.empty(M, K, dtype=dy.dtype, device=dy.device)
    gemm(dy, wl, dx, M=M, N=K, K=N, trans_b=True, ldb=K, act=act, aux=aux)
    return dw, db, dx


def _mlp_fwd(x1, n2w, n2b, eps, w1, f1b, w2, f2b, rd, rps):
    """MLP half of a residual block on the f32 stream x1 [M,D]: x1 + drop_path(dropout(fc2(dropout(GELU(fc1(LayerNorm(x1))))))), GELU
    in fc1's epilogue with the pre-activation kept. w1 [Hd,D], w2 [D,Hd]: the weights in the compute dtype.
    -> (x2, (mean2, rstd2, ln2, h_pre, h_act) for _mlp_bwd, (hidden mask, fc2 mask))."""
    M, Hd = x1.shape[0], w1.shape[0]
    ln2, mean2, rstd2 = layernorm_fwd(x1, n2w, n2b, eps, _compute_dtype)
    h_pre = torch.empty(M, Hd, dtype=_compute_dtype, device=x1.device)
    h_act = torch.empty(M, Hd, dtype=_compute_dtype, device=x1.device)
    gemm(ln2, w1, h_act, M=M, N=Hd, K=x1.shape[1], bias=f1b, act=ACT_GELU, aux=h_pre)
    mk_h = None
    if rd is not None and rd.drop > 0:
        h_act, mk_h = dropout_fwd(h_act, rd, "hidden")
    x2, mk_2 = _branch_residual(h_act, w2, f2b, x1, rd, 1, rps, "fc2")
    return x2, (mean2, rstd2, ln2, h_pre, h_act), (mk_h, mk_2)


def _mlp_bwd(g2, x1, n2w, saved, w1, w2, prm, nprm, need, rd, rps, masks):
    """Backward of _mlp_fwd for g2 [M,D] f32, the gradient of x2. prm = (fc1.weight, fc1.bias, fc2.weight, fc2.bias) and nprm =
    (norm2.weight, norm2.bias), the leaf Parameters that take deferred gradients; need = prm's needs_input_grad flags.
    -> (g1 f32 at x1, residual path included; its bf16 copy where the LayerNorm backward wrote one; `side`, for the caller's
    _branch_grad(g1, ...); (dn2w, dn2b, dw1, db1, dw2, db2))."""
    mean2, rstd2, ln2, h_pre, h_act = saved
    f1w, f1b, f2w, f2b = prm
    mk_h, mk_2 = masks
    T = ln2.dtype
    bf = T == torch.bfloat16
    # with the bf16 copy and column-sum partials of the incoming gradient, if the LayerNorm backward that made it (the block
    # above, when nothing sits in between) left them; bias gradients ride on the weight-gradient launch
    g2b, g2_lp, g2_cs = _branch_grad(g2, rd, 1, rps, mk_2, T, side=bf)
    dw2, db2, dh_pre = _linear_bwd(g2_lp, h_act, w2, f2w, f2b, need[2], need[3], dy_f32=g2b, dy_colsum=g2_cs, act=ACT_DGELU, aux=h_pre)
    if mk_h is not None:            # hidden dropout sits between GELU and fc2: its mask commutes with the GELU' product
        dh_pre = dropout_bwd(dh_pre, mk_h, rd.drop)
    dw1, db1, dln2 = _linear_bwd(dh_pre, ln2, w1, f1w, f1b, need[0], need[1])
    side = bf and rd is None
    g1, g1_lp, dn2w, dn2b = layernorm_bwd(dln2, x1, n2w, mean2, rstd2, gres=g2, want_lp=side, params=nprm, side=side)
    return g1, g1_lp, side, (dn2w, dn2b, dw1, db1, dw2, db2)


# ----------------------------------------------------------------------------------------------------- patch convolutions
# A Conv2d with kernel = stride = p evaluated only at the kept tokens is a GEMM on the gathered patch rows (gathering first is
# equivalent because every step is per token). PatchEmbedFn, PatchProjFn, PatchEmbedNHWCFn, StridedConvTokensFn and
# SwinFuseConvFn differ in how they gather and in what follows the GEMM; the gathers, the linear core and the embed tail are here.
def _gather_nchw(x, ids_keep, patch):
    """Patch rows of an NCHW f32 image at ids_keep (int64 [B,n_keep]; None: all L tokens in order), inner order (c,py,px) =
    Conv2d weight.view(D,-1): -> (cols [B*n_keep, C*p*p] in the compute dtype, L, n_keep)."""
    B, Cc, H, W = x.shape
    L = (H // patch) * (W // patch)
    n_keep = L if ids_keep is None else ids_keep.shape[1]
    cols = torch.empty(B * n_keep, Cc * patch * patch, dtype=_compute_dtype, device=x.device)
    call("evp_patchify", ptr(_chk(x.detach(), torch.float32)), ptr(ids_keep), B, Cc, H, W, patch, n_keep, ptr(cols), dt(cols),
         stream_ptr())
    return cols, L, n_keep


def _gather_nhwc(x, ids_keep, patch, H, W):
    """The same of a channels-last f32 token map [B, H*W, C]."""
    B, Cin = x.shape[0], x.shape[-1]
    L = (H // patch) * (W // patch)
    n_keep = L if ids_keep is None else ids_keep.shape[1]
    cols = torch.empty(B * n_keep, Cin * patch * patch, dtype=_compute_dtype, device=x.device)
    call("evp_patchify_nhwc", ptr(_chk(x.detach().contiguous(), torch.float32)), ptr(ids_keep), B, H, W, Cin, patch, n_keep,
         ptr(cols), dt(cols), stream_ptr())
    return cols, L, n_keep


def _scatter_nhwc(dcols, ids_keep, B, H, W, Cin, patch, n_keep):
    """Adjoint of _gather_nhwc: dx [B, H*W, C] f32, zero at dropped patches."""
    dx = torch.empty(B, H * W, Cin, dtype=torch.float32, device=dcols.device)
    call("evp_unpatchify_nhwc", ptr(dcols), dt(dcols), ptr(ids_keep), B, H, W, Cin, patch, n_keep, 0, ptr(dx), stream_ptr())
    return dx


def _rows_linear(cols, w, b):
    """-> (y [M,D] f32 = cols . w.view(D,Kc)^T + b, that weight view in the compute dtype)."""
    M, Kc = cols.shape
    D = w.shape[0]
    wl = lp_weight(w).view(D, Kc)
    y = torch.empty(M, D, dtype=torch.float32, device=cols.device)
    gemm(cols, wl, y, M=M, N=D, K=Kc, bias=b)
    return y, wl


def _rows_linear_bwd(dy, db_from, cols, prm, need, wl=None, dcols_dtype=None):
    """Backward of _rows_linear for prm = (w, b), need = their needs_input_grad flags: -> (dw, db, dcols). dW = dy^T cols, then
    db = column sums of `db_from` (dy itself, or the f32 gradient it was cast from) -- this order is the order of the deferred
    queue. With `wl`, also dcols [M,Kc] = dy . wl in `dcols_dtype` (default: dy's)."""
    M, D = dy.shape
    Kc = cols.shape[1]
    dw = _wgrad(dy, cols, D, Kc, M, prm[0], prm[0].shape) if need[0] else None
    db = _bgrad(db_from, prm[1]) if need[1] else None
    dcols = None
    if wl is not None:
        dcols = torch.empty(M, Kc, dtype=dcols_dtype or dy.dtype, device=dy.device)
        gemm(dy, wl, dcols, M=M, N=Kc, K=D, trans_b=True, ldb=Kc)
    return dw, db, dcols


def _embed_post(y, gamma, beta, pos, ids_keep, B, n_keep, L):
    """GELU(LayerNorm_{eps 1e-5}(y)) + pos[token id] on the gathered rows: -> (out [M,D] f32, mean, rstd)."""
    M, D = y.shape
    out = torch.empty(M, D, dtype=torch.float32, device=y.device)
    mean = torch.empty(M, dtype=torch.float32, device=y.device)
    rstd = torch.empty(M, dtype=torch.float32, device=y.device)
    pos2d = None if pos is None else _chk(pos.detach().view(L, D), torch.float32)
    call("evp_embed_post_fwd", ptr(y), ptr(gamma), ptr(beta), ptr(pos2d), ptr(ids_keep), B, n_keep, L, D, 1e-5, ptr(out),
         ptr(mean), ptr(rstd), stream_ptr())
    return out, mean, rstd


def _embed_post_bwd(g, y, gamma, beta, mean, rstd, dtype, params):
    """-> (dy [M,D] in `dtype`, dgamma, dbeta). `params` as in _norm_grads: PatchEmbedFn passes its (gamma, beta) leaf
    Parameters, so d gamma / d beta go to the deferred (grouped) column sums and come back None; PatchEmbedNHWCFn passes None and
    has them reduced in the kernel. Nothing records a reason for that difference; removing it changes the deferred queue."""
    M, D = y.shape
    g = _chk(g.contiguous(), torch.float32).view(M, D)
    dy = torch.empty(M, D, dtype=dtype, device=g.device)
    ws, dgamma, dbeta, finish = _norm_grads(params, D, M, g.device)
    call("evp_embed_post_bwd", ptr(g), ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), M, D, ptr(dy), dt(dy), ptr(dgamma),
         ptr(dbeta), ptr(ws), stream_ptr())
    finish()
    return dy, dgamma, dbeta


# ----------------------------------------------------------------------------------------------------- autograd
class ViTBlockFn(torch.autograd.Function):
    """Pre-LN transformer block (model/sub_module/vit_block.py:246-254) on a [B,N,D] f32 residual stream."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkvw, qkvb, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, heads, eps, want_attn, rd=None):
        B, N, D = x.shape
        M = B * N
        dh = D // heads
        T = _compute_dtype
        x2d = _chk(x.detach()).view(M, D)
        dev = x.device
        wq, wp, w1, w2 = lp_weight(qkvw), lp_weight(pw), lp_weight(f1w), lp_weight(f2w)
        ln1, mean1, rstd1 = layernorm_fwd(x2d, n1w, n1b, eps, T)
        qkv = torch.empty(M, 3 * D, dtype=T, device=dev)
        gemm(ln1, wq, qkv, M=M, N=3 * D, K=D, bias=qkvb)
        a_drop = rd is not None and rd.attn_drop > 0
        fused = fused_attention_ok(T, N, dh) and not a_drop
        ad_saved = None
        if a_drop:           # probabilities materialised, dropped, multiplied with V (the returned map is the dropped one, vit_block.py:138-143)
            stat, probs, mk_a, att = attention_dropout_fwd(qkv, B, N, heads, dh, rd)
            ad_saved = (probs, mk_a)
        elif fused:
            att, stat, probs = attention_fused_fwd(qkv, B, N, heads, dh, want_probs=want_attn)   # stat = log-sum-exp
        else:
            probs, att = attention_fwd(qkv, B, N, heads, dh)
            stat = probs
        x1, mk_p = _branch_residual(att, wp, pb, x2d, rd, 0, N, "proj")
        x2, mlp, mk_mlp = _mlp_fwd(x1, n2w, n2b, eps, w1, f1b, w2, f2b, rd, N)
        ctx.save_for_backward(x2d, n1w, n2w, mean1, rstd1, ln1, qkv, stat, att, x1, wq, wp, w1, w2, *mlp)
        ctx.dims = (B, N, D, heads, dh)
        ctx.fused = fused
        ctx.attn_drop = ad_saved
        ctx.rd, ctx.drop_masks = rd, (mk_p, mk_mlp)
        ctx.prm = (qkvw, qkvb, pw, pb, f1w, f1b, f2w, f2b)     # leaf parameters: targets of the deferred gradients
        ctx.nprm = (n1w, n1b, n2w, n2b)
        out = x2.view(B, N, D)
        if want_attn:
            attn = probs[..., :N]
            ctx.mark_non_differentiable(attn)
            return out, attn
        return out

    @staticmethod
    def backward(ctx, g2, *_):
        x2d, n1w, n2w, mean1, rstd1, ln1, qkv, stat, att, x1, wq, wp, w1, w2, *mlp = ctx.saved_tensors
        B, N, D, heads, dh = ctx.dims
        M = B * N
        T = qkv.dtype
        bf = T == torch.bfloat16
        g2 = _chk(g2.contiguous(), torch.float32).view(M, D)
        rd = ctx.rd
        mk_p, mk_mlp = ctx.drop_masks
        qkvw_, qkvb_, pw_, pb_ = ctx.prm[:4]
        need = ctx.needs_input_grad
        g1, g1_lp, side, mlp_grads = _mlp_bwd(g2, x1, n2w, mlp, w1, w2, ctx.prm[4:], ctx.nprm[2:], need[9:13], rd, N, mk_mlp)
        g1b, g1_lp, g1_cs = _branch_grad(g1, rd, 0, N, mk_p, T, side=side, lp=g1_lp)
        # attention
        dwp, dbp, datt = _linear_bwd(g1_lp, att, wp, pw_, pb_, need[5], need[6], dy_f32=g1b, dy_colsum=g1_cs)
        if ctx.attn_drop is not None:
            dqkv = attention_dropout_bwd(qkv, stat, ctx.attn_drop[0], ctx.attn_drop[1], datt, B, N, heads, dh, rd.attn_drop)
        elif ctx.fused:
            dqkv = attention_fused_bwd(qkv, att, datt, stat, B, N, heads, dh)
        else:
            dqkv = attention_bwd(qkv, stat, datt, B, N, heads, dh)
        dwq, dbq, dln1 = _linear_bwd(dqkv, ln1, wq, qkvw_, qkvb_, need[3], need[4])
        # the block below this one takes g0 as ITS incoming gradient: leave it the bf16 copy and the column sums
        g0, _, dn1w, dn1b = layernorm_bwd(dln1, x2d, n1w, mean1, rstd1, gres=g1, want_lp=bf, params=ctx.nprm[:2], side=bf)
        return (g0.view(B, N, D), dn1w, dn1b, dwq, dbq, dwp, dbp, *mlp_grads, None, None, None, None)


class PatchEmbedFn(torch.autograd.Function):
    """Conv2d(k=s=p) + LayerNorm(eps 1e-5) + GELU (vit_block.py:60-68), + pos_embed, keeping only ids_keep tokens
    (vit.py:110-115)."""

    @staticmethod
    def forward(ctx, x, ids_keep, w, b, gamma, beta, pos, patch):
        B = x.shape[0]
        cols, L, n_keep = _gather_nchw(x, ids_keep, patch)
        y, _ = _rows_linear(cols, w, b)
        out, mean, rstd = _embed_post(y, gamma, beta, pos, ids_keep, B, n_keep, L)
        ctx.save_for_backward(cols, y, gamma, beta, mean, rstd)
        ctx.prm = (w, b)
        ctx.nprm = (gamma, beta)        # leaf parameters: targets of the deferred (grouped) column sums
        return out.view(B, n_keep, -1)

    @staticmethod
    def backward(ctx, g):
        cols, y, gamma, beta, mean, rstd = ctx.saved_tensors
        dy, dgamma, dbeta = _embed_post_bwd(g, y, gamma, beta, mean, rstd, cols.dtype, ctx.nprm)
        dw, db, _ = _rows_linear_bwd(dy, dy, cols, ctx.prm, ctx.needs_input_grad[2:4])
        return None, None, dw, db, dgamma, dbeta, None, None


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dim of f32 tokens; up to three inputs are summed first (vit.py:125-128)."""

    @staticmethod
    def forward(ctx, x, x2, x3, gamma, beta, eps):
        shp = x.shape
        D = shp[-1]
        xs = [None if t is None else _chk(t.detach().contiguous(), torch.float32).view(-1, D) for t in (x, x2, x3)]
        y, mean, rstd = layernorm_fwd(xs[0], gamma, beta, eps, torch.float32, xs[1], xs[2])
        ctx.save_for_backward(gamma, mean, rstd, *[t for t in xs if t is not None])
        ctx.prm = (gamma, beta)
        ctx.n_in = sum(t is not None for t in xs)
        ctx.has = (x2 is not None, x3 is not None)
        return y.view(shp)

    @staticmethod
    def backward(ctx, g):
        gamma, mean, rstd, *xs = ctx.saved_tensors
        D = gamma.shape[0]
        x = xs[0]
        rest = xs[1:]
        x2 = rest.pop(0) if ctx.has[0] else None
        x3 = rest.pop(0) if ctx.has[1] else None
        g2d = _chk(g.contiguous(), torch.float32).view(-1, D)
        bf = _compute_dtype == torch.bfloat16
        dx, _, dgamma, dbeta = layernorm_bwd(g2d, x, gamma, mean, rstd, x2=x2, x3=x3, params=ctx.prm, want_lp=bf, side=bf)
        dx = dx.view(g.shape)
        return dx, (dx if ctx.has[0] else None), (dx if ctx.has[1] else None), dgamma, dbeta, None


def _head_fwd(xl, wl, b):
    """y = xl @ wl^T + b as float32 [M, _pad8(N)] for a weight [N, K] in xl's dtype: a width that is not a multiple of 8 runs with
    zero rows behind the weight and zeros behind the bias. -> (y, the weight as it ran); the caller cuts y[:, :N]."""
    M, K = xl.shape
    N = wl.shape[0]
    Np = _pad8(N)
    bias = b
    if Np != N:
        wp = torch.zeros(Np, K, dtype=wl.dtype, device=wl.device)
        wp[:N].copy_(wl)
        wl = wp
        if b is not None:
            bias = torch.zeros(Np, dtype=torch.float32, device=wl.device)
            bias[:N].copy_(b.detach())
    y = torch.empty(M, Np, dtype=torch.float32, device=xl.device)
    gemm(xl, wl, y, M=M, N=Np, K=K, bias=bias)
    return y, wl


def _head_bwd(g, xl, wl, N, pad_into, bias_sum, wparam, need_w, need_b, dx_dtype):
    """Backward of _head_fwd on what it saved. g: the [M, N] gradient; where the head ran padded, `pad_into(gp)` copies it into the
    zeroed float32 [M, _pad8(N)] buffer (the caller's copy kernel) and dw, db are cut back to N. `bias_sum(gp)`: the caller's column
    sum; `wparam`: the parameter _wgrad may queue dw on (whole-width heads only), or None. -> (dx [M, K] in dx_dtype or None without
    one, dw, db)."""
    (M, K), Np = xl.shape, wl.shape[0]
    if Np != N:
        gp = torch.zeros(M, Np, dtype=torch.float32, device=g.device)
        pad_into(gp)
    else:
        gp = _contig(g, torch.float32)
    gl = cast(gp, xl.dtype)
    cut = (lambda t: t[:N].contiguous()) if Np != N else (lambda t: t)
    dw = cut(_wgrad(gl, xl, Np, K, M, wparam)) if need_w else None
    db = cut(bias_sum(gp)) if need_b else None
    dx = None
    if dx_dtype is not None:
        dx = torch.empty(M, K, dtype=dx_dtype, device=g.device)
        gemm(gl, wl, dx, M=M, N=K, K=Np, trans_b=True, ldb=K)
    return dx, dw, db


class LinearFn(torch.autograd.Function):
    """nn.Linear on f32 tokens (f32 in / f32 out; operands rounded to the compute dtype for the MFMA). An output width
    that is not a multiple of 8 (a classification head with 10 or 101 classes) runs zero-padded to the next multiple --
    the kernels' vector accesses want 16-byte-aligned rows -- and is sliced back."""

    @staticmethod
    def forward(ctx, x, w, b):
        shp, N = x.shape, w.shape[0]
        x2d = _chk(x.detach().contiguous(), torch.float32).view(-1, shp[-1])
        xl = cast(x2d, _compute_dtype)
        y, wl = _head_fwd(xl, lp_weight(w), b)
        ctx.save_for_backward(xl, wl)
        ctx.needs_dx = x.requires_grad
        ctx.prm = (w, b)
        ctx.n_out = N
        if wl.shape[0] != N:
            y = y[:, :N]
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, g):
        xl, wl = ctx.saved_tensors
        M, K = xl.shape
        N = ctx.n_out
        g2d = _chk(g.contiguous(), torch.float32).view(M, N)
        # the whole-width head queues its gradients on the parameters; the padded one has slices to cut first
        wparam, bparam = ctx.prm if wl.shape[0] == N else (None, None)
        dx, dw, db = _head_bwd(g2d, xl, wl, N, lambda gp: gp[:, :N].copy_(g2d), lambda gp: _bgrad(gp, bparam), wparam,
                               ctx.needs_input_grad[1], ctx.needs_input_grad[2], torch.float32 if ctx.needs_dx else None)
        return (None if dx is None else dx.view(*g.shape[:-1], K)), dw, db


class UnshuffleFn(torch.autograd.Function):
    """Decoder input assembly (pr_rec_decoder.py:56-62): mask tokens, un-shuffle by ids_restore, + pos_embed."""

    @staticmethod
    def forward(ctx, emb, mask_token, pos, ids_restore):
        B, n_keep, D = emb.shape
        L = ids_restore.shape[1]
        out = torch.empty(B, L, D, dtype=torch.float32, device=emb.device)
        call("evp_unshuffle_fwd", ptr(_chk(emb.detach().contiguous(), torch.float32)), ptr(_chk(mask_token.detach())),
             ptr(_chk(pos.detach())), ptr(_chk(ids_restore)), B, n_keep, L, D, ptr(out), stream_ptr())
        ctx.save_for_backward(ids_restore)
        ctx.dims = (B, n_keep, L, D)
        ctx.mt_shape = tuple(mask_token.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (ids_restore,) = ctx.saved_tensors
        B, n_keep, L, D = ctx.dims
        g = _chk(g.contiguous(), torch.float32)
        demb = torch.empty(B, n_keep, D, dtype=torch.float32, device=g.device)
        dmt = torch.empty(D, dtype=torch.float32, device=g.device)
        nb = (B * L + 63) // 64
        ws = torch.empty(nb * D, dtype=torch.float32, device=g.device)
        call("evp_unshuffle_bwd", ptr(g), ptr(ids_restore), B, n_keep, L, D, ptr(demb), ptr(dmt), ptr(ws), stream_ptr())
        return demb, dmt.view(ctx.mt_shape), None, None


class RecLossFn(torch.autograd.Function):
    """PrHubModel.reconstruct_loss (pr_hub_model.py:125-141) fused with frame2emb; returns a 0-dim f32 tensor."""

    @staticmethod
    def forward(ctx, pred, target, mask, patch, norm_pix):
        B, L, P = pred.shape
        _, Cc, H, W = target.shape
        dev = pred.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dpred = torch.empty(B, L, P, dtype=torch.float32, device=dev)
        ws = torch.empty(2 * B * L + 4, dtype=torch.float32, device=dev)
        call("evp_rec_loss", ptr(_chk(pred.detach().contiguous(), torch.float32)),
             ptr(_chk(target.detach().contiguous(), torch.float32)), ptr(mask), B, Cc, H, W, patch, int(bool(norm_pix)),
             ptr(loss), ptr(dpred), ptr(ws), stream_ptr())
        ctx.save_for_backward(dpred)
        ctx.scaled = False
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        # upstream gradient is a device scalar (1, or 1/accum_iter): scale in place without a host sync. The saved gradient is
        # consumed by that: a second pass through the same forward (retain_graph=True) would return g * g' * dpred, so it is refused
        if ctx.scaled:
            raise _lib.EvpError("RecLossFn: backward ran twice through one forward; the saved gradient is scaled in place by the "
                                "upstream scalar and cannot be used again -- run the forward again")
        ctx.scaled = True
        call("evp_scale_f32", ptr(dpred), ptr(_chk(g.contiguous().view(1), torch.float32)), dpred.numel(), stream_ptr())
        return dpred, None, None, None, None


def vit_block(x, blk, heads, eps, want_attn=False, rd=None):
    return ViTBlockFn.apply(x, blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias,
                            blk.attn.proj.weight, blk.attn.proj.bias, blk.norm2.weight, blk.norm2.bias,
                            blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias,
                            heads, eps, want_attn, rd)


# ----------------------------------------------------------------------------------------------------- contrastive stage
def _pad8(n):
    return (n + 7) // 8 * 8


def _bn_ws(R, N, device):
    """Workspace of evp_batchnorm_fwd / _bwd on [R, N]: two partial rows per row block and two result rows."""
    return torch.empty((2 * call("evp_batchnorm_nblk", R) + 2) * N, dtype=torch.float32, device=device)


def _bn_train_fwd(y_pre, gamma, beta, running_mean, running_var, eps, momentum, relu):
    """BatchNorm on the batch statistics of the rows of y_pre [R, N] (+ ReLU), in y_pre's dtype; the running statistics are updated in
    place. -> (y, mean, invstd)."""
    R, N = y_pre.shape
    dev = y_pre.device
    y = torch.empty(R, N, dtype=y_pre.dtype, device=dev)
    mean, invstd = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
    ws = _bn_ws(R, N, dev)
    call("evp_batchnorm_fwd", ptr(y_pre), dt(y_pre), R, N, ptr(gamma), ptr(beta), float(eps), float(momentum), int(relu),
         ptr(y), ptr(mean), ptr(invstd), ptr(running_mean), ptr(running_var), ptr(ws), stream_ptr())
    return y, mean, invstd


def _bn_train_bwd(g, y_pre, y, gamma, mean, invstd, relu):
    """Backward of _bn_train_fwd for g [R, N] in y's dtype -> (dpre, dgamma, dbeta); the last two None without gamma."""
    R, N = y.shape
    dev = g.device
    dpre = torch.empty(R, N, dtype=y.dtype, device=dev)
    dgamma, dbeta = (torch.empty(N, dtype=torch.float32, device=dev) if gamma is not None else None for _ in range(2))
    ws = _bn_ws(R, N, dev)
    call("evp_batchnorm_bwd", ptr(g), ptr(y_pre), ptr(y), dt(y), R, N, ptr(gamma), ptr(mean), ptr(invstd), int(relu),
         ptr(dpre), ptr(dgamma), ptr(dbeta), ptr(ws), stream_ptr())
    return dpre, dgamma, dbeta


class LinearBNFn(torch.autograd.Function):
    """Linear(no bias) -> BatchNorm over the B*L token rows (training statistics) -> optional ReLU: one stage of the
    MoCo-v3 heads (mlp_head.py:4-24 applied as pr_hub_model.py:223-237). Hidden stages keep the compute dtype, the
    last stage (affine=False, no ReLU) returns f32 tokens. Running statistics are updated in place."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, eps, momentum, relu, last):
        B, L, K = x.shape
        R, N = B * L, w.shape[0]
        T = _compute_dtype
        dev = x.device
        xl = cast(_chk(x.detach().contiguous()).view(R, K), T)
        wl = lp_weight(w)
        ydt = torch.float32 if last else T
        y_pre = torch.empty(R, N, dtype=ydt, device=dev)
        gemm(xl, wl, y_pre, M=R, N=N, K=K)
        y, mean, invstd = _bn_train_fwd(y_pre, gamma, beta, running_mean, running_var, eps, momentum, relu)
        ctx.save_for_backward(xl, wl, y_pre, y, mean, invstd, gamma)
        ctx.cfg = (B, L, K, N, bool(relu), x.dtype, x.requires_grad)
        ctx.prm = (w,)
        return y.view(B, L, N)

    @staticmethod
    def backward(ctx, g):
        xl, wl, y_pre, y, mean, invstd, gamma = ctx.saved_tensors
        B, L, K, N, relu, xdt, need_dx = ctx.cfg
        R = B * L
        g2d = cast(_chk(g.contiguous()).view(R, N), y.dtype)
        dpre, dgamma, dbeta = _bn_train_bwd(g2d, y_pre, y, gamma, mean, invstd, relu)
        dl = cast(dpre, xl.dtype)
        dw = _wgrad(dl, xl, N, K, R, ctx.prm[0]) if ctx.needs_input_grad[1] else None
        dx = None
        if need_dx:
            dx = torch.empty(R, K, dtype=xdt if xdt == torch.float32 else xl.dtype, device=g.device)
            gemm(dl, wl, dx, M=R, N=K, K=N, trans_b=True, ldb=K)
            dx = dx.view(B, L, K)
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None


def linear_bn_tokens(x, lin, bn, relu):
    """One [Linear, BatchNorm2d(, ReLU)] stage of an nn.Sequential head on (B, L, C) tokens."""
    if bn is None:
        return LinearFn.apply(x, lin.weight, None)
    if not bn.training:
        raise NotImplementedError("the pre-training heads only run in training mode (batch statistics)")
    last = not relu
    out = LinearBNFn.apply(x, lin.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                           0.1 if bn.momentum is None else bn.momentum, relu, last)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return out


class L2NormFn(torch.autograd.Function):
    """F.normalize(x, dim=-1) on f32 tokens."""

    @staticmethod
    def forward(ctx, x):
        C_ = x.shape[-1]
        x2 = _chk(x.detach().contiguous(), torch.float32).view(-1, C_)
        y = torch.empty_like(x2)
        nrm = torch.empty(x2.shape[0], dtype=torch.float32, device=x.device)
        call("evp_l2norm_rows_fwd", ptr(x2), x2.shape[0], C_, ptr(y), ptr(nrm), stream_ptr())
        ctx.save_for_backward(y, nrm)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        y, nrm = ctx.saved_tensors
        g2 = _chk(g.contiguous(), torch.float32).view(y.shape)
        dx = torch.empty_like(y)
        call("evp_l2norm_rows_bwd", ptr(g2), ptr(y), ptr(nrm), y.shape[0], y.shape[1], ptr(dx), stream_ptr())
        return dx.view(g.shape)


class InfoNCEQueueFn(torch.autograd.Function):
    """Per-position InfoNCE of normalised q against the positive key and the (C,L,K) queue
    (pr_hub_model.py:150-160). q, k: normalised f32 (B,L,C)."""

    @staticmethod
    def forward(ctx, q, k, queue, T_):
        B, L, C_ = q.shape
        K = queue.shape[2]
        Kp = _pad8(K)
        R = B * L
        dev = q.device
        Tc = _compute_dtype
        q2, k2 = _chk(q.detach().contiguous(), torch.float32).view(R, C_), _chk(k.detach().contiguous(), torch.float32).view(R, C_)
        pos = torch.empty(R, dtype=torch.float32, device=dev)
        call("evp_rowdot_f32", ptr(q2), ptr(k2), R, C_, ptr(pos), stream_ptr())
        qw = queue.detach() if Kp == K else torch.nn.functional.pad(queue.detach(), (0, Kp - K))   # tiny test queues only
        ql, qul = cast(q2, Tc), cast(qw.contiguous(), Tc)
        if qul.data_ptr() == queue.data_ptr():
            # f32 mode with K % 8 == 0: cast()/contiguous() returned the live buffer, which _dequeue_and_enqueue overwrites
            # in place before backward reads it (the reference uses self.queue.clone().detach(), pr_hub_model.py:152)
            qul = qul.clone()
        neg = torch.empty(B, L, Kp, dtype=torch.float32, device=dev)
        # neg[b,l,:] = q[b,l,:] . queue[:,l,:]   ('blc,clk->blk'), batched over l
        gemm(ql, qul, neg, M=B, N=K, K=C_, trans_b=True, lda=L * C_, ldb=L * Kp, ldc=L * Kp, batch=(L, 1),
             stride_a=(C_, 0), stride_b=(Kp, 0), stride_c=(Kp, 0))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dpos = torch.empty(R, dtype=torch.float32, device=dev)
        dneg = torch.empty(B, L, Kp, dtype=torch.float32, device=dev)
        ws = torch.empty(R, dtype=torch.float32, device=dev)
        call("evp_infonce_queue", ptr(pos), ptr(neg), R, K, Kp, 1.0 / T_, ptr(loss), ptr(dpos), ptr(dneg), ptr(ws), stream_ptr())
        ctx.save_for_backward(q2, k2, qul, dpos, dneg)
        ctx.cfg = (B, L, C_, K, Kp)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        q2, k2, qul, dpos, dneg = ctx.saved_tensors
        B, L, C_, K, Kp = ctx.cfg
        R = B * L
        dev = g.device
        dq_pos = torch.empty(R, C_, dtype=torch.float32, device=dev)
        call("evp_scale_rows_f32", ptr(k2), ptr(dpos), None, R, C_, ptr(dq_pos), stream_ptr())
        dk = torch.empty(R, C_, dtype=torch.float32, device=dev)
        call("evp_scale_rows_f32", ptr(q2), ptr(dpos), None, R, C_, ptr(dk), stream_ptr())
        dq = torch.empty(R, C_, dtype=torch.float32, device=dev)
        dnl = cast(dneg, qul.dtype)
        # dq[b,l,:] = dpos*k + dneg[b,l,:] . queue[:,l,:]^T    ('blk,clk->blc')
        gemm(dnl, qul, dq, M=B, N=C_, K=K, lda=L * Kp, ldb=L * Kp, ldc=L * C_, batch=(L, 1), stride_a=(Kp, 0),
             stride_b=(Kp, 0), stride_c=(C_, 0), residual=dq_pos)
        gs = _chk(g.contiguous().view(1), torch.float32)
        call("evp_scale_f32", ptr(dq), ptr(gs), dq.numel(), stream_ptr())
        call("evp_scale_f32", ptr(dk), ptr(gs), dk.numel(), stream_ptr())
        return dq.view(B, L, C_), dk.view(B, L, C_), None, None


class InfoNCEInBatchFn(torch.autograd.Function):
    """MoCo-v3 in-batch InfoNCE (pr_hub_model.py:170-188): logits[n,l,m] = q[n,l,:].k_all[m,l,:] / T, label of row
    (n,l) = n + N*rank. k_all carries no gradient when it was all-gathered (as in the reference)."""

    @staticmethod
    def forward(ctx, q, k_all, T_, rank, k_has_grad):
        N, L, C_ = q.shape
        Mk = k_all.shape[0]
        Mp = _pad8(Mk)
        dev = q.device
        Tc = _compute_dtype
        q2 = _chk(q.detach().contiguous(), torch.float32)
        ka = _chk(k_all.detach().contiguous(), torch.float32)
        ql, kl = cast(q2, Tc), cast(ka, Tc)
        logits = torch.zeros(N, L, Mp, dtype=torch.float32, device=dev)
        gemm(ql, kl, logits, M=N, N=Mk, K=C_, lda=L * C_, ldb=L * C_, ldc=L * Mp, batch=(L, 1), stride_a=(C_, 0),
             stride_b=(C_, 0), stride_c=(Mp, 0), alpha=1.0 / T_)
        labels = (torch.arange(N, device=dev, dtype=torch.int64) + N * rank).unsqueeze(1).expand(N, L).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dlog = torch.empty(N, L, Mp, dtype=torch.float32, device=dev)
        ws = torch.empty(N * L, dtype=torch.float32, device=dev)
        call("evp_cross_entropy", ptr(logits), ptr(labels), N * L, Mk, Mp, ptr(loss), ptr(dlog), ptr(ws), stream_ptr())
        ctx.save_for_backward(ql, kl, dlog)
        ctx.cfg = (N, L, C_, Mk, Mp, T_, bool(k_has_grad))
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        ql, kl, dlog = ctx.saved_tensors
        N, L, C_, Mk, Mp, T_, k_has_grad = ctx.cfg
        dev = g.device
        dl = cast(dlog, ql.dtype)
        gs = _chk(g.contiguous().view(1), torch.float32)
        dq = torch.empty(N, L, C_, dtype=torch.float32, device=dev)
        gemm(dl, kl, dq, M=N, N=C_, K=Mk, trans_b=True, lda=L * Mp, ldb=L * C_, ldc=L * C_, batch=(L, 1), stride_a=(Mp, 0),
             stride_b=(C_, 0), stride_c=(C_, 0), alpha=1.0 / T_)
        call("evp_scale_f32", ptr(dq), ptr(gs), dq.numel(), stream_ptr())
        dk = None
        if k_has_grad:
            dk = torch.empty(Mk, L, C_, dtype=torch.float32, device=dev)
            gemm(dl, ql, dk, M=Mk, N=C_, K=N, trans_a=True, trans_b=True, lda=L * Mp, ldb=L * C_, ldc=L * C_, batch=(L, 1),
                 stride_a=(Mp, 0), stride_b=(C_, 0), stride_c=(C_, 0), alpha=1.0 / T_)
            call("evp_scale_f32", ptr(dk), ptr(gs), dk.numel(), stream_ptr())
        return dq, dk, None, None, None


def info_nce_queue(emb_h, clip_emb, queue, T_):
    """-> (loss, normalised keys (detached) for the enqueue)."""
    q = L2NormFn.apply(emb_h)
    k = L2NormFn.apply(clip_emb)
    return InfoNCEQueueFn.apply(q, k, queue, T_), k.detach()


def info_nce_inbatch(emb_h, clip_emb, T_, distributed=False, gather=None):
    """`gather` (engine.ForwardCollectives.gather): takes the all-gather's place under a captured data-parallel step."""
    q = L2NormFn.apply(emb_h)
    k = L2NormFn.apply(clip_emb)
    rank = 0
    if distributed:
        import torch.distributed as dist
        from .model.pretrain.pr_hub_model import concat_all_gather
        rank = dist.get_rank()
        # RCCL all-gather over xGMI; no gradient (reference pr_hub_model.py:176-182,248-259)
        k_all = concat_all_gather(k) if gather is None else gather(k.detach())
        return InfoNCEInBatchFn.apply(q, k_all, T_, rank, False)
    return InfoNCEInBatchFn.apply(q, k, T_, rank, True)


def enqueue_keys(queue, keys, ptr_):
    B, L, C_ = keys.shape
    call("evp_enqueue_keys", ptr(_chk(queue, torch.float32)), ptr(_chk(keys.contiguous(), torch.float32)), int(ptr_), B, L, C_,
         queue.shape[2], stream_ptr())


def enqueue_keys_dev(queue, keys, queue_ptr):
    """_dequeue_and_enqueue with the pointer kept on the device (queue_ptr: int64 [1] buffer): no host sync."""
    B, L, C_ = keys.shape
    call("evp_enqueue_keys_dev", ptr(_chk(queue, torch.float32)), ptr(_chk(keys.contiguous(), torch.float32)),
         ptr(_chk(queue_ptr, torch.int64)), B, L, C_, queue.shape[2], stream_ptr())


# ----------------------------------------------------------------------------------------------------- ConvViT stages
class PatchEmbedNHWCFn(torch.autograd.Function):
    """PatchEmbed (Conv2d k=s=p -> LayerNorm(eps 1e-5) -> GELU, vit_block.py:60-68) on a channels-last token map
    x (B, H*W, C) f32, optionally restricted to ids_keep and with a positional table: the conv is a GEMM on the
    gathered patch matrix (convvit.py:22-25,141,153). dx only where x requires a gradient."""

    @staticmethod
    def forward(ctx, x, ids_keep, w, b, gamma, beta, pos, patch, H, W):
        B, Cin = x.shape[0], x.shape[-1]
        cols, L, n_keep = _gather_nhwc(x, ids_keep, patch, H, W)
        y, wl = _rows_linear(cols, w, b)
        out, mean, rstd = _embed_post(y, gamma, beta, pos, ids_keep, B, n_keep, L)
        ctx.save_for_backward(cols, y, gamma, beta, mean, rstd, wl, ids_keep)
        ctx.geom = (B, H, W, Cin, patch, n_keep)
        ctx.need_dx = x.requires_grad
        ctx.prm = (w, b)
        return out.view(B, n_keep, -1)

    @staticmethod
    def backward(ctx, g):
        cols, y, gamma, beta, mean, rstd, wl, ids_keep = ctx.saved_tensors
        dy, dgamma, dbeta = _embed_post_bwd(g, y, gamma, beta, mean, rstd, cols.dtype, None)
        dw, db, dcols = _rows_linear_bwd(dy, dy, cols, ctx.prm, ctx.needs_input_grad[2:4], wl if ctx.need_dx else None)
        dx = _scatter_nhwc(dcols, ids_keep, *ctx.geom) if ctx.need_dx else None
        return dx, None, dw, db, dgamma, dbeta, None, None, None, None


class StridedConvTokensFn(torch.autograd.Function):
    """Conv2d(k=s=p) + bias on a channels-last map, evaluated only at the tokens in ids_keep (the multi-scale fusion
    convs stage1/2_output_decode followed by the gather, convvit.py:137-140,149-151). dx always."""

    @staticmethod
    def forward(ctx, x, ids_keep, w, b, patch, H, W):
        B, _, Cin = x.shape
        cols, _, n_keep = _gather_nhwc(x, ids_keep, patch, H, W)
        y, wl = _rows_linear(cols, w, b)
        ctx.save_for_backward(cols, wl, ids_keep)
        ctx.geom = (B, H, W, Cin, patch, n_keep)
        ctx.prm = (w, b)
        return y.view(B, n_keep, -1)

    @staticmethod
    def backward(ctx, g):
        cols, wl, ids_keep = ctx.saved_tensors
        g2d = _chk(g.contiguous(), torch.float32).view(cols.shape[0], -1)
        gl = cast(g2d, cols.dtype)
        dw, db, dcols = _rows_linear_bwd(gl, g2d, cols, ctx.prm, ctx.needs_input_grad[2:4], wl)
        return _scatter_nhwc(dcols, ids_keep, *ctx.geom), None, dw, db, None, None, None


class AddPosGatherFn(torch.autograd.Function):
    """x[b,j,:] + pos[ids[b,j],:] (pos is a frozen table)."""

    @staticmethod
    def forward(ctx, x, pos, ids):
        B, n, D = x.shape
        L = pos.shape[-2]
        out = torch.empty(B, n, D, dtype=torch.float32, device=x.device)
        call("evp_add_rows_gather_f32", ptr(_chk(x.detach().contiguous(), torch.float32)), ptr(_chk(pos.detach().view(L, D))),
             ptr(ids), B, n, L, D, ptr(out), stream_ptr())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, None


class ConvBlockFn(torch.autograd.Function):
    """ConvMAE-style block on a channels-last token map (conv_block.py:41-51):
    x = x + conv2(dw5x5(keep * conv1(LN(x)))); x = x + fc2(GELU(fc1(LN(x)))), 1x1 convs as GEMMs."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, c1w, c1b, aw, ab, c2w, c2b, n2w, n2b, f1w, f1b, f2w, f2b, mask, mask_scale, H, W, rd=None):
        B, HW, Cc = x.shape
        M = B * HW
        T = _compute_dtype
        dev = x.device
        x2d = _chk(x.detach().contiguous(), torch.float32).view(M, Cc)
        w1, w2, wf1, wf2 = (lp_weight(c1w).view(Cc, Cc), lp_weight(c2w).view(Cc, Cc), lp_weight(f1w).view(-1, Cc),
                            lp_weight(f2w).view(Cc, -1))
        ln1, mean1, rstd1 = layernorm_fwd(x2d, n1w, n1b, 1e-5, T)
        c1 = torch.empty(M, Cc, dtype=T, device=dev)
        gemm(ln1, w1, c1, M=M, N=Cc, K=Cc, bias=c1b)
        a = torch.empty(M, Cc, dtype=T, device=dev)
        awf = _chk(aw.detach().contiguous(), torch.float32)
        call("evp_dwconv5x5_fwd", ptr(c1), dt(c1), ptr(mask), int(mask_scale), ptr(awf), ptr(ab), B, H, W, Cc, ptr(a), stream_ptr())
        # (CMlp.drop sits after GELU and after fc2, conv_block.py:19-21; the conv branch has no dropout of its own)
        x1, _ = _branch_residual(a, w2, c2b, x2d, rd, 0, HW, None)
        x2, mlp, mk_mlp = _mlp_fwd(x1, n2w, n2b, 1e-5, wf1, f1b, wf2, f2b, rd, HW)
        ctx.rd, ctx.drop_masks = rd, mk_mlp
        ctx.save_for_backward(x2d, n1w, n2w, mean1, rstd1, ln1, c1, a, x1, w1, w2, wf1, wf2, awf, mask, *mlp)
        ctx.cfg = (B, H, W, Cc, int(mask_scale), tuple(aw.shape))
        ctx.prm = (c1w, c1b, c2w, c2b, f1w, f1b, f2w, f2b)
        ctx.nprm = (n1w, n1b, n2w, n2b)
        return x2.view(B, HW, Cc)

    @staticmethod
    def backward(ctx, g2):
        x2d, n1w, n2w, mean1, rstd1, ln1, c1, a, x1, w1, w2, wf1, wf2, awf, mask, *mlp = ctx.saved_tensors
        B, H, W, Cc, mask_scale, awshape = ctx.cfg
        c1w_, c1b_, c2w_, c2b_ = ctx.prm[:4]
        need = ctx.needs_input_grad
        M = B * H * W
        T = c1.dtype
        bf = T == torch.bfloat16
        dev = g2.device
        g2 = _chk(g2.contiguous(), torch.float32).view(M, Cc)
        rd = ctx.rd
        HW = H * W
        # as in ViTBlockFn: bf16 copy / column sums left by the LayerNorm backward of the block above, bias gradients on the
        # weight-gradient launch, LayerNorm dgamma / dbeta through the grouped column sums
        g1, g1_lp, side, mlp_grads = _mlp_bwd(g2, x1, n2w, mlp, wf1, wf2, ctx.prm[4:], ctx.nprm[2:], need[11:15], rd, HW, ctx.drop_masks)
        g1b, g1_lp, g1_cs = _branch_grad(g1, rd, 0, HW, None, T, side=side, lp=g1_lp)
        # conv branch
        dwc2, dbc2, da = _linear_bwd(g1_lp, a, w2, c2w_, c2b_, need[7], need[8], dy_f32=g1b, dy_colsum=g1_cs)
        dc1 = torch.empty(M, Cc, dtype=T, device=dev)
        daw = torch.empty(Cc, 25, dtype=torch.float32, device=dev)
        dab = torch.empty(Cc, dtype=torch.float32, device=dev)
        ns = call("evp_dwconv5x5_bwd_nslab", B, H, W)
        ws = torch.empty(ns * 26 * Cc, dtype=torch.float32, device=dev)
        call("evp_dwconv5x5_bwd", ptr(da), ptr(c1), dt(c1), ptr(mask), mask_scale, ptr(awf), B, H, W, Cc, ptr(dc1), ptr(daw), ptr(dab),
             ptr(ws), stream_ptr())
        dwc1, dbc1, dln1 = _linear_bwd(dc1, ln1, w1, c1w_, c1b_, need[3], need[4])
        g0, _, dn1w, dn1b = layernorm_bwd(dln1, x2d, n1w, mean1, rstd1, gres=g1, want_lp=bf, params=ctx.nprm[:2], side=bf)
        return (g0.view(B, HW, Cc), dn1w, dn1b, dwc1, dbc1, daw.view(awshape), dab, dwc2, dbc2, *mlp_grads, None, None, None, None, None)


def conv_block(x, blk, H, W, mask=None, mask_scale=1, rd=None):
    return ConvBlockFn.apply(x, blk.norm1.weight, blk.norm1.bias, blk.conv1.weight, blk.conv1.bias, blk.attn.weight, blk.attn.bias,
                             blk.conv2.weight, blk.conv2.bias, blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight,
                             blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias, mask, mask_scale, H, W, rd)


# ----------------------------------------------------------------------------------------------------- Swin (row a15)
def gather_rows(x, idx, n_in=None):
    """out[b,s,:] = idx[s] >= 0 ? x[b,idx[s],:] : 0 for f32 tokens [B,n_in,C]; idx int32 [n_out] shared by the batch."""
    B, n, C = x.shape
    n_out = idx.shape[0]
    out = torch.empty(B, n_out, C, dtype=torch.float32, device=x.device)
    call("evp_gather_rows_f32", ptr(_chk(x, torch.float32)), ptr(_chk(idx, torch.int32)), ptr(out), B, n, n_out, C, 0, stream_ptr())
    return out


class GatherRowsFn(torch.autograd.Function):
    """GroupingModule.group / merge and PatchMerging's regrouping (swin_block.py:454-466,193-201) as one row gather.
    `idx_bwd` is the index of the adjoint gather: the real entries of `idx_fwd` form a permutation, padding slots
    (which the reference fills with a copy of token 0 and later drops) receive and send no gradient."""

    @staticmethod
    def forward(ctx, x, idx_fwd, idx_bwd):
        ctx.save_for_backward(idx_bwd)
        return gather_rows(x.detach().contiguous(), idx_fwd)

    @staticmethod
    def backward(ctx, g):
        (idx_bwd,) = ctx.saved_tensors
        return gather_rows(g.contiguous(), idx_bwd), None, None


class PatchProjFn(torch.autograd.Function):
    """Conv2d(k=s=patch) of an NCHW f32 image evaluated only at the tokens `ids_keep` (int64 [B,n_keep]), returned as
    f32 tokens [B,n_keep,D] (swin_block.py:58-62 before its norm)."""

    @staticmethod
    def forward(ctx, x, ids_keep, w, b, patch):
        cols, _, n_keep = _gather_nchw(x, ids_keep, patch)
        y, _ = _rows_linear(cols, w, b)
        ctx.save_for_backward(cols)
        ctx.prm = (w, b)
        return y.view(x.shape[0], n_keep, -1)

    @staticmethod
    def backward(ctx, g):
        (cols,) = ctx.saved_tensors
        g2d = _chk(g.contiguous(), torch.float32).view(cols.shape[0], -1)
        gl = cast(g2d, cols.dtype)
        dw, db, _ = _rows_linear_bwd(gl, g2d, cols, ctx.prm, ctx.needs_input_grad[2:4])
        return None, None, dw, db, None


class SwinFuseConvFn(torch.autograd.Function):
    """swin.py:201-208: scatter the visible stage tokens into a zero R x R grid, Conv2d(k, stride k) down to the
    decoder grid, gather each sample's ids_keep cells -- formed directly as the [B*K, C*k*k] patch rows of the kept
    cells times weight.view(out, C*k*k). The gather and its adjoint work in f32."""

    @staticmethod
    def forward(ctx, x, w, b, tokmap, coords, ids_keep, ids_restore, R, k):
        B, n, C = x.shape
        K = ids_keep.shape[1]
        A = torch.empty(B * K, C * k * k, dtype=torch.float32, device=x.device)
        call("evp_swin_fuse_gather_f32", ptr(_chk(x.detach().contiguous(), torch.float32)), ptr(_chk(tokmap, torch.int32)),
             ptr(_chk(ids_keep, torch.int64)), ptr(A), B, n, K, C, R, k, stream_ptr())
        Al = cast(A, _compute_dtype)
        y, wl = _rows_linear(Al, w, b)
        ctx.save_for_backward(Al, wl, coords, ids_restore)
        ctx.dims = (B, n, K, C, R, k)
        ctx.prm = (w, b)
        return y.view(B, K, -1)

    @staticmethod
    def backward(ctx, g):
        Al, wl, coords, ids_restore = ctx.saved_tensors
        B, n, K, C, R, k = ctx.dims
        g2d = _chk(g.contiguous(), torch.float32).view(B * K, -1)
        gl = cast(g2d, Al.dtype)
        dw, db, dA = _rows_linear_bwd(gl, g2d, Al, ctx.prm, ctx.needs_input_grad[1:3], wl, torch.float32)
        dx = torch.empty(B, n, C, dtype=torch.float32, device=g.device)
        call("evp_swin_fuse_gather_bwd_f32", ptr(dA), ptr(coords), ptr(ids_restore), ptr(dx), B, n, K, C, R, k, stream_ptr())
        return dx, dw, db, None, None, None, None, None, None


class SwinBlockFn(torch.autograd.Function):
    """SwinTransformerBlock.forward (swin_block.py:260-273) on grouped tokens [Bg, N, D] (Bg = batch * n_groups):
    pre-LN, window attention with the gathered relative-position bias and the -100 group mask (:135-158), MLP."""

    @staticmethod
    def forward(ctx, x, table, rel, n1w, n1b, qkvw, qkvb, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, heads, eps, want_attn, rd=None):
        Bg, N, D = x.shape
        nG = rel.shape[0]
        M = Bg * N
        dh = D // heads
        if dh != 32:
            raise _lib.EvpError(f"window attention kernel is built for d_h=32 (got {dh})")
        T = _compute_dtype
        dev = x.device
        x2d = _chk(x.detach().contiguous(), torch.float32).view(M, D)
        wq, wp, w1, w2 = lp_weight(qkvw), lp_weight(pw), lp_weight(f1w), lp_weight(f2w)
        ln1, mean1, rstd1 = layernorm_fwd(x2d, n1w, n1b, eps, T)
        qkv = torch.empty(M, 3 * D, dtype=T, device=dev)
        gemm(ln1, wq, qkv, M=M, N=3 * D, K=D, bias=qkvb)
        att = torch.empty(M, D, dtype=T, device=dev)
        probs = torch.empty(Bg, heads, N, N, dtype=torch.float32, device=dev) if want_attn else None
        tab = _chk(table.detach(), torch.float32)
        R = tab.shape[0]
        scale = dh ** -0.5
        # bf16 mode: the MFMA kernels of the ViT attention with the gathered bias as an additive matrix per (group, head); the
        # f32 LDS kernels stay the parity path and serve the blocks that return their probabilities
        a_drop = rd is not None and rd.attn_drop > 0
        fused = _use_window_mfma and T == torch.bfloat16 and not want_attn and N <= 128 and not a_drop
        lse = addm = addmT = None
        keep, keep_scale = None, 1.0
        if a_drop:           # swin_block.py:113,152: the LDS kernels hold the probabilities and take the keep flags; the MFMA form never does
            keep, keep_scale = _attn_keep_mask(rd, (Bg, heads, N, N), dev), 1.0 / (1.0 - rd.attn_drop)
        if fused:
            NP = call("evp_window_attention_fused_np", N)
            addm = torch.empty(nG * heads * NP * NP, dtype=torch.float32, device=dev)
            addmT = torch.empty_like(addm)
            call("evp_window_bias_build", ptr(tab), ptr(_chk(rel, torch.int32)), nG, N, heads, R, ptr(addm), ptr(addmT), stream_ptr())
            lse = torch.empty(Bg * heads * N, dtype=torch.float32, device=dev)
            call("evp_window_attention_fused_fwd", ptr(qkv), ptr(addm), Bg, nG, N, heads, scale, ptr(att), ptr(lse), stream_ptr())
        else:
            call("evp_window_attention_fwd", ptr(qkv), ptr(tab), ptr(_chk(rel, torch.int32)), ptr(att), ptr(probs), Bg, nG, N, heads, R,
                 scale, dt(qkv), ptr(keep), keep_scale, stream_ptr())
        x1, mk_p = _branch_residual(att, wp, pb, x2d, rd, 0, N, "proj")
        x2, mlp, mk_mlp = _mlp_fwd(x1, n2w, n2b, eps, w1, f1b, w2, f2b, rd, N)
        ctx.rd, ctx.drop_masks = rd, (mk_p, mk_mlp)
        ctx.save_for_backward(x2d, n1w, n2w, mean1, rstd1, ln1, qkv, att, x1, wq, wp, w1, w2, tab, rel, *mlp)
        ctx.dims = (Bg, nG, N, D, heads, R, scale)
        ctx.prm = (qkvw, qkvb, pw, pb, f1w, f1b, f2w, f2b)
        ctx.nprm = (n1w, n1b, n2w, n2b)
        ctx.win = (lse, addm, addmT)          # plain tensors of this node (not inputs / outputs): kept on ctx
        ctx.keep = (keep, keep_scale)
        out = x2.view(Bg, N, D)
        if want_attn:
            ctx.mark_non_differentiable(probs)
            return out, probs
        return out

    @staticmethod
    def backward(ctx, g2, *_):
        x2d, n1w, n2w, mean1, rstd1, ln1, qkv, att, x1, wq, wp, w1, w2, tab, rel, *mlp = ctx.saved_tensors
        Bg, nG, N, D, heads, R, scale = ctx.dims
        M = Bg * N
        T = qkv.dtype
        dev = g2.device
        bf = T == torch.bfloat16
        g2 = _chk(g2.contiguous(), torch.float32).view(M, D)
        # as in ViTBlockFn: the LayerNorm backward that produced g2 (the block above, when no regrouping gather sits in between:
        # the single-group stages) may have left its bf16 copy and column sums; bias gradients ride on the weight-gradient launch
        rd = ctx.rd
        mk_p, mk_mlp = ctx.drop_masks
        qkvw_, qkvb_, pw_, pb_ = ctx.prm[:4]
        need = ctx.needs_input_grad
        g1, g1_lp, side, mlp_grads = _mlp_bwd(g2, x1, n2w, mlp, w1, w2, ctx.prm[4:], ctx.nprm[2:], need[11:15], rd, N, mk_mlp)
        g1b, g1_lp, g1_cs = _branch_grad(g1, rd, 0, N, mk_p, T, side=side, lp=g1_lp)
        dwp, dbp, datt = _linear_bwd(g1_lp, att, wp, pw_, pb_, need[7], need[8], dy_f32=g1b, dy_colsum=g1_cs)
        dqkv = torch.empty(M, 3 * D, dtype=T, device=dev)
        dtable = torch.empty(R, heads, dtype=torch.float32, device=dev)
        lse, addm, addmT = ctx.win
        if lse is not None:
            nchunk = call("evp_window_attention_fused_nchunk", Bg, nG, heads)
            dA = torch.empty(nchunk * addm.numel(), dtype=torch.float32, device=dev)
            call("evp_window_attention_fused_bwd", ptr(qkv), ptr(att), ptr(datt), ptr(lse), ptr(addm), ptr(addmT), Bg, nG, N, heads, scale,
                 ptr(dqkv), ptr(dA), stream_ptr())
            call("evp_window_bias_reduce", ptr(dA), ptr(rel), Bg, nG, N, heads, R, ptr(dtable), stream_ptr())
        else:
            call("evp_window_attention_bwd", ptr(qkv), ptr(tab), ptr(rel), ptr(att), ptr(datt), ptr(dqkv), ptr(dtable), Bg, nG, N, heads,
                 R, scale, dt(qkv), ptr(ctx.keep[0]), ctx.keep[1], stream_ptr())
        dwq, dbq, dln1 = _linear_bwd(dqkv, ln1, wq, qkvw_, qkvb_, need[5], need[6])
        g0, _, dn1w, dn1b = layernorm_bwd(dln1, x2d, n1w, mean1, rstd1, gres=g1, want_lp=bf, params=ctx.nprm[:2], side=bf)
        return (g0.view(Bg, N, D), dtable, None, dn1w, dn1b, dwq, dbq, dwp, dbp, *mlp_grads, None, None, None, None)


def _attn_keep_mask(rd, shape, dev):
    """uint8 keep flags for dropout on attention probabilities of `shape`: rd.masks["attn"] when given, else drawn by evp_dropout_fwd from
    rd's Philox stream (the same draw the ViT path makes in attention_dropout_fwd: flag e <- word e of the stream at rd's next offset)."""
    if rd.masks is not None and "attn" in rd.masks:
        m = _chk(rd.masks["attn"]).view(-1)
        if m.numel() != math.prod(shape) or m.dtype != torch.uint8:
            raise _lib.EvpError(f"attention keep mask: expected uint8 with {math.prod(shape)} elements, got {m.dtype} {tuple(m.shape)}")
        return m
    sub = BlockDrop(drop=rd.attn_drop, seed=rd.seed_dev if rd.seed_dev is not None else rd.seed)
    sub._n = rd.next_offset(math.prod(shape))
    return dropout_fwd(torch.ones(shape, dtype=torch.float32, device=dev), sub, "attn")[1]


def swin_block(x, blk, rel, eps, want_attn=False, rd=None):
    a = blk.attn
    return SwinBlockFn.apply(x, a.relative_position_bias_table, rel, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias,
                             a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias,
                             blk.mlp.fc2.weight, blk.mlp.fc2.bias, a.num_heads, eps, want_attn, rd)


class DropoutFn(torch.autograd.Function):
    """nn.Dropout on a float32 tensor (vit.py:114 / convvit.py:132 / swin.py:185 `pos_drop`): evp_dropout_fwd / evp_dropout_apply."""

    @staticmethod
    def forward(ctx, x, p, seed, mask=None):
        xc = _chk(x.detach().contiguous(), torch.float32)
        rd = BlockDrop(drop=p, seed=seed, masks=None if mask is None else {"x": mask})
        out, mk = dropout_fwd(xc, rd, "x")
        ctx.save_for_backward(mk)
        ctx.p = p
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        (mk,) = ctx.saved_tensors
        return dropout_bwd(_chk(g.contiguous(), torch.float32), mk, ctx.p).view(g.shape), None, None, None


def draw_block_drop(module, n_samples, device):
    """BlockDrop for one training-mode call of a residual block module carrying `drop_path_rate` / `drop_rate` attributes, or None
    when both are off (the fused fast path). The draws come from torch's default generator of the device (as timm's `drop_path`
    and nn.Dropout do), so torch.manual_seed reproduces a run; the per-element masks use the Philox stream keyed by a seed
    drawn from the same device generator (draw_drop_seed)."""
    dp = float(getattr(module, "drop_path_rate", 0.0) or 0.0)
    dr = float(getattr(module, "drop_rate", 0.0) or 0.0)
    da = float(getattr(module, "attn_drop_rate", 0.0) or 0.0)
    if not module.training or (dp <= 0.0 and dr <= 0.0 and da <= 0.0):
        return None
    u1 = u2 = None
    if dp > 0.0:
        u = torch.rand(2, n_samples, device=device)
        u1, u2 = u[0], u[1]
    seed = draw_drop_seed(device) if (dr > 0.0 or da > 0.0) else 0
    return BlockDrop(u1, u2, 1.0 - dp, dr, seed, attn_drop=da)


def draw_drop_seed(device):
    """Key of one dropout stream, drawn ON the device from torch's generator (no host read-back; under HIP-graph capture torch's
    generator advances per replay, so every replay of a captured step gets fresh keys -- ADVICE r3)."""
    return torch.randint(0, 2 ** 62, (1,), device=device, dtype=torch.int64)


class AddFn(torch.autograd.Function):
    """a + b on f32 tokens (the 4-way stage sum of swin.py:239 exceeds LayerNormFn's three fused inputs)."""

    @staticmethod
    def forward(ctx, a, b):
        return add(a.detach().contiguous(), b.detach().contiguous())

    @staticmethod
    def backward(ctx, g):
        return g, g


# ----------------------------------------------------------------------------------------------------- fine-tune (cls) head
class TokenMeanFn(torch.autograd.Function):
    """emb_h.mean(dim=1) over the tokens (ft_cls_hub_model.py:136) on f32 [B,N,D]."""

    @staticmethod
    def forward(ctx, x):
        B, N, D = x.shape
        out = torch.empty(B, D, dtype=torch.float32, device=x.device)
        call("evp_token_mean_fwd", ptr(_chk(x.detach().contiguous(), torch.float32)), B, N, D, ptr(out), stream_ptr())
        ctx.dims = (B, N, D)
        return out

    @staticmethod
    def backward(ctx, g):
        B, N, D = ctx.dims
        dx = torch.empty(B, N, D, dtype=torch.float32, device=g.device)
        call("evp_token_mean_bwd", ptr(_chk(g.contiguous(), torch.float32)), B, N, D, ptr(dx), stream_ptr())
        return dx


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss()(pred, label) (mean reduction; ft_cls_trainer.py:66) on f32 logits [B, n_cls]; smoothing > 0:
    timm's LabelSmoothingCrossEntropy(smoothing)(pred, label) (ft_cls_trainer.py:63-64)."""

    @staticmethod
    def forward(ctx, logits, labels, smoothing=0.0):
        B, Cn = logits.shape
        lg = _chk(logits.detach().contiguous(), torch.float32)
        loss = torch.empty(1, dtype=torch.float32, device=lg.device)
        dlog = torch.empty(B, Cn, dtype=torch.float32, device=lg.device)
        ws = torch.empty(B, dtype=torch.float32, device=lg.device)
        call("evp_cross_entropy_smooth", ptr(lg), ptr(_chk(labels.contiguous(), torch.int64)), B, Cn, Cn, float(smoothing), ptr(loss),
             ptr(dlog), ptr(ws), stream_ptr())
        ctx.save_for_backward(dlog)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dlog,) = ctx.saved_tensors
        out = dlog.clone()
        call("evp_scale_f32", ptr(out), ptr(_chk(g.contiguous().view(1), torch.float32)), out.numel(), stream_ptr())
        return out, None, None


def cls_metrics(pred, label, table, cursor):
    """The evaluation record of one batch on the device (evp_cls_metrics; reference ft_cls_trainer.py:152-164): with s = cursor[0],
    table[s] = {mean cross entropy, top-1 %, top-5 %} of f32 logits `pred` [R, n_cls] against int64 `label` [R], then cursor[0] = s + 1;
    a full table (s >= table.shape[0]) is left alone. `table` f32 [capacity, 3] and `cursor` int64 [1] live in device memory, so a
    captured graph fills slot after slot with no host round-trip. The rows are read in place through pred.stride(0): the padded head
    output of LinearFn is not copied."""
    for t in (pred, label, table, cursor):
        if not t.is_cuda:
            raise _lib.EvpError("cls_metrics: tensor is not in device memory; eventpretrain_amd has no CPU path")
    if pred.dim() != 2 or pred.dtype != torch.float32:
        raise _lib.EvpError(f"cls_metrics: logits must be float32 [R, n_cls] (got {pred.dtype} {tuple(pred.shape)})")
    R, n_cls = pred.shape
    pred = pred.detach()
    ld = pred.stride(0) if R > 1 else n_cls
    # in place only where every row, the last included, has ld floats behind it in the storage (a column slice of a padded matrix)
    room = pred.untyped_storage().nbytes() // 4 - pred.storage_offset()
    if pred.stride(1) != 1 or ld < n_cls or R * ld > room:
        pred, ld = pred.contiguous(), n_cls
    if tuple(label.shape) != (R,):
        raise _lib.EvpError(f"cls_metrics: expected {R} labels, got {tuple(label.shape)}")
    if table.dim() != 2 or table.shape[1] != 3 or cursor.numel() != 1:
        raise _lib.EvpError("cls_metrics: table must be float32 [capacity, 3] and cursor one int64")
    ws = torch.empty(_lib.CLS_METRICS_WS, dtype=torch.float32, device=pred.device) if R > _lib.CLS_METRICS_SINGLE_ROWS else None
    call("evp_cls_metrics", pred.data_ptr(), ptr(_chk(label, torch.int64)), R, n_cls, ld, ptr(_chk(cursor, torch.int64)),
         ptr(_chk(table, torch.float32)), table.shape[0], ptr(ws), stream_ptr())


# ----------------------------------------------------------------------------------------------------- dense-prediction heads
# csrc/dense.hip. A "map" is a token-major 2-D tensor [B*H*W, C] whose rows may be further apart than C (a channel slice of a wider
# buffer). `out=(buf, off)`: the op writes its C columns into buf[:, off:off+C] and returns that slice, so the reference's
# torch.cat(dim=1) becomes one buffer its producers fill (CatFn).
def _map(t, what="map"):
    """-> (tensor, leading dimension in elements) of a token-major map."""
    if not t.is_cuda:
        raise _lib.EvpError(f"{what} is not in device memory; eventpretrain_amd has no CPU path")
    if t.dim() != 2:
        raise _lib.EvpError(f"{what} must be a 2-D tensor (got shape {tuple(t.shape)})")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()           # a gradient that arrives channel-major (through the NCHW permute of a prediction)
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _slot(out, R, C, dtype, device):
    """-> (buffer, ld, column offset, the [R, C] view the caller returns) of an output given as None or (buf, off)."""
    if out is None:
        buf = torch.empty(R, C, dtype=dtype, device=device)
        return buf, C, 0, buf
    buf, off = out
    if buf.dim() != 2 or not buf.is_contiguous() or buf.shape[0] != R or off < 0 or off + C > buf.shape[1]:
        raise _lib.EvpError(f"output slot [{R}, {off}:{off + C}] does not fit a buffer of shape {tuple(buf.shape)}")
    return buf, buf.shape[1], off, buf[:, off:off + C]


def map_copy(x, dtype, out=None, scale=None, rows_per_sample=None):
    """Strided cast-copy of a map (evp_channel_scale), times scale[b, c] when given (float32 [B, C], rows_per_sample rows per b)."""
    x, ldi = _map(x)
    R, Cc = x.shape
    buf, ldo, off, view = _slot(out, R, Cc, dtype, x.device)
    Bn, P = (1, R) if scale is None else (R // rows_per_sample, rows_per_sample)
    call("evp_channel_scale", ptr(x), dt(x), ldi, ptr(scale), Bn, P, Cc, ptr(buf), dt(buf), ldo, off, stream_ptr())
    return view


def _contig(x, dtype):
    """A contiguous [R, C] copy of a map in `dtype`, or the map itself where it already is one."""
    if x.dtype == dtype and x.is_contiguous():
        return x
    return map_copy(x, dtype)


def colsum_ordered(x):
    x, ld = _map(x)
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    call("evp_colsum_ordered", ptr(x), dt(x), x.shape[0], x.shape[1], ld, ptr(out), stream_ptr())
    return out


def im2col3x3(x, B, H, W):
    x, ldi = _map(x)
    Cc = x.shape[1]
    cols = torch.empty(B * H * W, Cc * 9, dtype=_compute_dtype, device=x.device)
    call("evp_im2col3x3", ptr(x), dt(x), ldi, B, H, W, Cc, ptr(cols), dt(cols), Cc * 9, stream_ptr())
    return cols


class MapCopyFn(torch.autograd.Function):
    """A map in another element type and / or in its slice of a concat buffer; the gradient comes back in the input's type."""

    @staticmethod
    def forward(ctx, x, dtype, out):
        ctx.xdt = x.dtype
        return map_copy(x.detach(), dtype, out)

    @staticmethod
    def backward(ctx, g):
        return _contig(g, ctx.xdt), None, None


class CatFn(torch.autograd.Function):
    """torch.cat(maps, dim=1) where every map already IS its slice of `buf` (the ops' `out=(buf, off)`): nothing moves. Backward hands
    each producer its columns of the gradient, as a strided view."""

    @staticmethod
    def forward(ctx, holder, *views):
        (buf,), off = holder, 0
        for v in views:
            if v.data_ptr() != buf.data_ptr() + off * buf.element_size() or v.stride(0) != buf.stride(0) or v.dtype != buf.dtype:
                raise _lib.EvpError("CatFn: a map is not the slice of the buffer it stands for")
            off += v.shape[1]
        if off != buf.shape[1]:
            raise _lib.EvpError("CatFn: the maps do not fill the buffer")
        ctx.widths = [v.shape[1] for v in views]
        return buf.view(buf.shape)

    @staticmethod
    def backward(ctx, g):
        outs, off = [], 0
        for w in ctx.widths:
            outs.append(g[:, off:off + w])
            off += w
        return (None, *outs)


class ConvBNFn(torch.autograd.Function):
    """The reference's ConvModule (ft_dense_decoder.py:7-20) on a token-major map: Conv2d(kernel 1 or 3, stride 1, padding k // 2, with
    bias) -> BatchNorm2d -> ReLU. The convolution is a GEMM on the map's rows (k = 1) or on their 3x3 patch rows (evp_im2col3x3), the
    bias in its epilogue: it sits in front of the normalisation, so it moves running_mean and its gradient is the column sum of the
    pre-BN gradient (zero up to rounding in training mode). training: batch statistics over the B*H*W rows, running statistics updated
    in place; else evp_batchnorm_eval on the running statistics (no gradients for the BatchNorm affine parameters then)."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, B, H, W, eps, momentum, relu, training, out):
        T = _compute_dtype
        R, N, k = B * H * W, w.shape[0], w.shape[-1]
        if k not in (1, 3) or w.shape[-2] != k:
            raise NotImplementedError("ConvBNFn: kernel size 1 or 3")
        if training and R == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, N, H, W]}")
        dev = x.device
        xd = x.detach()
        a = _contig(xd, T) if k == 1 else im2col3x3(xd, B, H, W)
        K = a.shape[1]
        wl = lp_weight(w).view(N, K)
        y_pre = torch.empty(R, N, dtype=T, device=dev)
        gemm(a, wl, y_pre, M=R, N=N, K=K, bias=b)
        if training:
            y, mean, invstd = _bn_train_fwd(y_pre, gamma, beta, running_mean, running_var, eps, momentum, relu)
            ret = y if out is None else map_copy(y, T, out)
            ctx.save_for_backward(a, wl, y_pre, y, mean, invstd, gamma)
        else:
            buf, ldo, off, ret = _slot(out, R, N, T, dev)
            call("evp_batchnorm_eval", ptr(y_pre), dt(y_pre), N, R, N, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                 float(eps), int(relu), ptr(buf), dt(buf), ldo, off, stream_ptr())
            ctx.save_for_backward(a, wl, ret, running_var.clone(), gamma)
        ctx.cfg = (B, H, W, k, bool(relu), bool(training), float(eps), x.dtype, x.requires_grad)
        ctx.prm = (w, b)
        return ret

    @staticmethod
    def backward(ctx, g):
        B, H, W, k, relu, training, eps, xdt, need_dx = ctx.cfg
        w, b = ctx.prm
        R, N, dev = B * H * W, w.shape[0], g.device
        dgamma = dbeta = None
        if training:
            a, wl, y_pre, y, mean, invstd, gamma = ctx.saved_tensors
            dpre, dgamma, dbeta = _bn_train_bwd(_contig(g, y.dtype), y_pre, y, gamma, mean, invstd, relu)
        else:
            a, wl, y, rvar, gamma = ctx.saved_tensors
            gm, ldg = _map(g)
            ym, ldy = _map(y)
            dpre = torch.empty(R, N, dtype=y.dtype, device=dev)
            call("evp_batchnorm_eval_bwd", ptr(gm), dt(gm), ldg, ptr(ym), dt(ym), ldy, R, N, ptr(gamma), ptr(rvar), eps, int(relu),
                 ptr(dpre), dt(dpre), N, stream_ptr())
        K = a.shape[1]
        db = colsum_ordered(dpre) if (b is not None and ctx.needs_input_grad[2]) else None
        dw = _wgrad(dpre, a, N, K, R, w, shape=tuple(w.shape)) if ctx.needs_input_grad[1] else None
        dx = None
        if need_dx:
            if k == 1:
                dx = torch.empty(R, K, dtype=xdt, device=dev)
                gemm(dpre, wl, dx, M=R, N=K, K=N, trans_b=True, ldb=K)
            else:
                Cin = K // 9
                dcols = torch.empty(R, K, dtype=dpre.dtype, device=dev)
                gemm(dpre, wl, dcols, M=R, N=K, K=N, trans_b=True, ldb=K)
                dx = torch.empty(R, Cin, dtype=xdt, device=dev)
                call("evp_col2im3x3", ptr(dcols), dt(dcols), K, B, H, W, Cin, ptr(dx), dt(dx), Cin, 0, stream_ptr())
        return (dx, dw, db, dgamma, dbeta) + (None,) * 10


def conv_bn_map(x, conv, bn, B, H, W, relu=True, out=None):
    """One ConvModule on a map: the parameters and buffers of (nn.Conv2d, nn.BatchNorm2d), the module's training flag, and the
    num_batches_tracked count torch keeps."""
    if conv.stride != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding != (conv.kernel_size[0] // 2,) * 2:
        raise NotImplementedError("conv_bn_map: stride 1, dilation 1, padding k // 2 only")
    y = ConvBNFn.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, B, H, W, bn.eps,
                       0.1 if bn.momentum is None else bn.momentum, relu, bn.training, out)
    if bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return y


class AdaptivePoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d(s) on a map [B*H*W, C] -> [B*s*s, C] in the compute dtype."""

    @staticmethod
    def forward(ctx, x, B, H, W, s):
        xm, ldi = _map(x.detach())
        Cc = xm.shape[1]
        out = torch.empty(B * s * s, Cc, dtype=_compute_dtype, device=x.device)
        call("evp_adaptive_avgpool_fwd", ptr(xm), dt(xm), ldi, B, H, W, Cc, s, ptr(out), dt(out), Cc, 0, stream_ptr())
        ctx.cfg = (B, H, W, Cc, s, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        B, H, W, Cc, s, xdt = ctx.cfg
        gm, ldg = _map(g)
        dx = torch.empty(B * H * W, Cc, dtype=xdt, device=g.device)
        call("evp_adaptive_avgpool_bwd", ptr(gm), dt(gm), ldg, B, H, W, Cc, s, ptr(dx), dt(dx), Cc, 0, stream_ptr())
        return dx, None, None, None, None


class UpsampleBilinearFn(torch.autograd.Function):
    """F.interpolate(size=(H, W), mode="bilinear", align_corners=False) on a map [B*h*w, C] -> [B*H*W, C] (the input's element type,
    or the slot's)."""

    @staticmethod
    def forward(ctx, x, B, h, w, H, W, out):
        xm, ldi = _map(x.detach())
        Cc = xm.shape[1]
        buf, ldo, off, view = _slot(out, B * H * W, Cc, xm.dtype, x.device)
        call("evp_upsample_bilinear_fwd", ptr(xm), dt(xm), ldi, B, h, w, H, W, Cc, ptr(buf), dt(buf), ldo, off, stream_ptr())
        ctx.cfg = (B, h, w, H, W, Cc, x.dtype)
        return view

    @staticmethod
    def backward(ctx, g):
        B, h, w, H, W, Cc, xdt = ctx.cfg
        gm, ldg = _map(g)
        dx = torch.empty(B * h * w, Cc, dtype=xdt, device=g.device)
        call("evp_upsample_bilinear_bwd", ptr(gm), dt(gm), ldg, B, h, w, H, W, Cc, ptr(dx), dt(dx), Cc, 0, stream_ptr())
        return (dx,) + (None,) * 6


def resize_map(x, B, h, w, H, W, mode="bilinear", out=None):
    """The reference's resize() between two map sizes; at equal size the map itself."""
    if mode != "bilinear":
        raise NotImplementedError(f"sample_mode {mode!r}: only 'bilinear' (what both of the reference's entry scripts set)")
    if (h, w) == (H, W):
        return x if out is None else MapCopyFn.apply(x, _compute_dtype, out)
    return UpsampleBilinearFn.apply(x, B, h, w, H, W, out)


class ChannelDropoutFn(torch.autograd.Function):
    """nn.Dropout2d on a map: out[(b,p), c] = x[(b,p), c] * scale[b, c] with scale in {0, 1/(1-p)} (float32 [B, C]); the output is
    the compute-dtype operand of the classifier GEMM. The backward is the same kernel."""

    @staticmethod
    def forward(ctx, x, scale, rows_per_sample):
        ctx.save_for_backward(scale)
        ctx.cfg = (rows_per_sample, x.dtype)
        return map_copy(x.detach(), _compute_dtype, scale=_chk(scale, torch.float32), rows_per_sample=rows_per_sample)

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        rps, xdt = ctx.cfg
        return map_copy(g, xdt, scale=scale, rows_per_sample=rps), None, None


def draw_channel_scale(B, Cc, p, device, keep=None):
    """-> (scale float32 [B, C] in {0, 1/(1-p)}, keep mask uint8 [B*C]) of one Dropout2d call. The mask is `keep` when given, else
    drawn by evp_dropout_fwd from a key drawn on the device (draw_drop_seed): a replayed graph draws a new one."""
    ones = torch.ones(B * Cc, dtype=torch.float32, device=device)
    rd = BlockDrop(drop=p, seed=0 if keep is not None else draw_drop_seed(device),
                   masks=None if keep is None else {"c": keep.to(device=device, dtype=torch.uint8).contiguous().view(-1)})
    scale, mask = dropout_fwd(ones, rd, "c")
    return scale.view(B, Cc), mask


class DenseClsFn(torch.autograd.Function):
    """The heads' `conv_dense` (nn.Conv2d(channels, out_channels, 1); ft_dense_decoder.py:41,48) on a map -> float32 [B*H*W, out_channels].
    11 classes or 2 flow components run zero-padded to 8 columns (_head_fwd / _head_bwd, LinearFn's narrow heads); the bias gradient
    is an ordered sum and nothing is queued."""

    @staticmethod
    def forward(ctx, x, w, b):
        T = _compute_dtype
        xl = _contig(x.detach(), T)
        N = w.shape[0]
        y, wl = _head_fwd(xl, lp_weight(w).view(N, xl.shape[1]), b)
        ctx.save_for_backward(xl, wl)
        ctx.cfg = (N, x.dtype, x.requires_grad, tuple(w.shape))
        return y[:, :N]

    @staticmethod
    def backward(ctx, g):
        xl, wl = ctx.saved_tensors
        N, xdt, need_dx, wshape = ctx.cfg
        dx, dw, db = _head_bwd(g, xl, wl, N, lambda gp: map_copy(g, torch.float32, (gp, 0)), colsum_ordered, None,
                               ctx.needs_input_grad[1], ctx.needs_input_grad[2], xdt if need_dx else None)
        return dx, (None if dw is None else dw.view(wshape)), db


# ----------------------------------------------------------------------------------------------------- segmentation objective
# csrc/semseg.hip: cross entropy + Dice, and the evaluation's confusion table, from the LOW-RESOLUTION logits of a head. The logits of
# an output pixel are interpolated in registers (resize_map's bits); the label map is the only full-resolution operand.
_semseg_status = {}


def semseg_status(device):
    """int32 [1] in device memory: how many valid (not ignored) labels outside [0, num_classes) the segmentation kernels have met
    since the last semseg_check_labels. Such pixels enter no sum; the count is read where the host reads back anyway."""
    device = torch.device(device)
    key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _semseg_status:
        _semseg_status[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _semseg_status[key]


def semseg_check_labels(device):
    """One read-back: raise if a label outside [0, num_classes) that is not the ignore label was met; the count starts again."""
    st = semseg_status(device)
    n = int(st.item())
    if n:
        st.zero_()
        raise _lib.EvpError(f"segmentation labels: {n} pixels carry a label outside [0, num_classes) that is not the ignore label")


def _map_in_place(x):
    """float32 [R, C] -> (the map read where it lies, its leading dimension), or (a contiguous copy, C). In place only where every row,
    the last included, has ld floats behind it in the storage (a column slice of a padded matrix)."""
    m = x.detach()
    C = m.shape[1]
    ld = m.stride(0) if m.shape[0] > 1 else C
    room = m.untyped_storage().nbytes() // 4 - m.storage_offset()
    if m.stride(1) != 1 or ld < C or m.shape[0] * ld > room:
        m, ld = m.contiguous(), C
    return m, ld


def _semseg_operands(what, logits_map, B, h, w, label, ignore_label):
    """-> (map read in place or a contiguous copy, ld, C, H, W, label, ignore value, has_ignore) of a segmentation call."""
    for t in (logits_map, label):
        if not t.is_cuda:
            raise _lib.EvpError(f"{what}: tensor is not in device memory; eventpretrain_amd has no CPU path")
    if logits_map.dim() != 2 or logits_map.dtype != torch.float32 or logits_map.shape[0] != B * h * w:
        raise _lib.EvpError(f"{what}: logits must be a float32 map [B*h*w, C] = [{B * h * w}, C] (got {logits_map.dtype} {tuple(logits_map.shape)})")
    C = logits_map.shape[1]
    if not 2 <= C <= _lib.SEMSEG_MAX_CLASSES:
        raise _lib.EvpError(f"{what}: {C} classes (2 to {_lib.SEMSEG_MAX_CLASSES} are supported)")
    if label.dtype != torch.int64 or label.dim() != 4 or label.shape[0] != B or label.shape[1] != 1:
        raise _lib.EvpError(f"{what}: label must be int64 [B, 1, H, W] with B = {B} (got {label.dtype} {tuple(label.shape)})")
    H, W = int(label.shape[2]), int(label.shape[3])
    if ignore_label is not None and 0 <= int(ignore_label) < C:
        raise NotImplementedError(f"{what}: an ignore label inside [0, num_classes) (the reference then drops that class from the Dice sum)")
    m, ld = _map_in_place(logits_map)
    return m, ld, C, H, W, label.contiguous(), (0 if ignore_label is None else int(ignore_label)), int(ignore_label is not None)


def _semseg_workspace(P, device):
    return torch.empty(call("evp_semseg_nblk", P) * _lib.SEMSEG_WS_ROW, dtype=torch.int32, device=device)


class SemsegObjectiveFn(torch.autograd.Function):
    """SemsegLoss of the reference (nn.CrossEntropyLoss(ignore_index) and the batch-wide Dice loss, trainer/finetune_semseg/
    semseg_loss.py) applied to resize(logits, label size): (logits_map [B*h*w, C] float32, B, h, w, label int64 [B, 1, H, W],
    ignore_label or None) -> (ce, dice), 0-d float32, differentiable in the map. The resized logits are never stored: forward is a
    pixel pass and a finishing launch, backward one gather launch that writes the map's gradient (same leading dimension as the map,
    pad columns zero). The map is read in place through its leading dimension (DenseClsFn's column slice of a padded matrix).
    (h, w) == (H, W) is the reference's call form with logits already at label size: correct, but then every pixel is a map cell of
    its own and the backward launches one wave per pixel; it is not meant to be fast."""

    @staticmethod
    def forward(ctx, logits_map, B, h, w, label, ignore_label=None):
        m, ld, C, H, W, lab, ign, has = _semseg_operands("SemsegObjectiveFn", logits_map, B, h, w, label, ignore_label)
        dev = m.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        saved = torch.empty(_lib.SEMSEG_SAVED, dtype=torch.float32, device=dev)
        ws = _semseg_workspace(B * H * W, dev)
        call("evp_semseg_objective_fwd", m.data_ptr(), ld, B, h, w, H, W, C, ptr(lab), ign, has, ptr(out), ptr(saved),
             ptr(semseg_status(dev)), ptr(ws), stream_ptr())
        ctx.save_for_backward(m, lab, saved)
        ctx.cfg = (ld, B, h, w, H, W, C, ign, has)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_ce, g_dice):
        m, lab, saved = ctx.saved_tensors
        ld, B, h, w, H, W, C, ign, has = ctx.cfg
        grad = torch.empty(B * h * w, ld, dtype=torch.float32, device=m.device)
        call("evp_semseg_objective_bwd", m.data_ptr(), ld, B, h, w, H, W, C, ptr(lab), ign, has, ptr(saved),
             ptr(_chk(g_ce.contiguous().view(1), torch.float32)), ptr(_chk(g_dice.contiguous().view(1), torch.float32)), ptr(grad), ld,
             stream_ptr())
        return (grad[:, :C],) + (None,) * 5


def semseg_metrics(logits_map, B, h, w, label, ignore_label, table, cursor, confusion=None, argmax=None):
    """The evaluation record of one segmentation batch on the device (evp_semseg_metrics; reference ft_semseg_trainer.py:207-241):
    with s = cursor[0], table[s] = {ce + dice, mIoU, mAcc} of resize(logits, label size) against the labels, then cursor[0] = s + 1;
    a full table is left alone. `confusion` (int64 [C, C], rows = label, columns = argmax) and `argmax` (uint8 [B, H, W], every pixel)
    are filled when given. Arguments as SemsegObjectiveFn's; `table` float32 [capacity, 3] and `cursor` int64 [1] as cls_metrics'."""
    for t in (table, cursor, confusion, argmax):
        if t is not None and not t.is_cuda:
            raise _lib.EvpError("semseg_metrics: tensor is not in device memory; eventpretrain_amd has no CPU path")
    m, ld, C, H, W, lab, ign, has = _semseg_operands("semseg_metrics", logits_map, B, h, w, label, ignore_label)
    if table.dim() != 2 or table.shape[1] != 3 or cursor.numel() != 1:
        raise _lib.EvpError("semseg_metrics: table must be float32 [capacity, 3] and cursor one int64")
    if confusion is not None and (tuple(confusion.shape) != (C, C) or not confusion.is_contiguous()):
        raise _lib.EvpError(f"semseg_metrics: confusion must be a contiguous int64 [{C}, {C}] (got {tuple(confusion.shape)})")
    if argmax is not None and (tuple(argmax.shape) != (B, H, W) or not argmax.is_contiguous()):
        raise _lib.EvpError(f"semseg_metrics: argmax must be a contiguous uint8 [{B}, {H}, {W}] (got {tuple(argmax.shape)})")
    dev = m.device
    ws = _semseg_workspace(B * H * W, dev)
    cws = torch.empty(call("evp_semseg_nblk", B * H * W) * C * C, dtype=torch.int32, device=dev)
    call("evp_semseg_metrics", m.data_ptr(), ld, B, h, w, H, W, C, ptr(lab), ign, has, ptr(_chk(cursor, torch.int64)),
         ptr(_chk(table, torch.float32)), table.shape[0], None if confusion is None else ptr(_chk(confusion, torch.int64)),
         None if argmax is None else ptr(_chk(argmax, torch.uint8)), ptr(semseg_status(dev)), ptr(ws), ptr(cws), stream_ptr())


# ------------------------------------------------------------------------------------------------------ optical-flow objective
# csrc/flow.hip: the masked L1 loss, and the validation's end-point error and outlier share, from the LOW-RESOLUTION two-channel
# prediction of a head. A pixel's prediction is interpolated and scaled in registers (resize_flow); the labels are the only
# full-resolution operands.
def _flow_operands(what, flow_map, B, h, w, target, valid):
    """-> (map read in place or a contiguous copy, ld, H, W, target, valid) of a flow call."""
    for t in (flow_map, target, valid):
        if not t.is_cuda:
            raise _lib.EvpError(f"{what}: tensor is not in device memory; eventpretrain_amd has no CPU path")
    if flow_map.dim() != 2 or flow_map.dtype != torch.float32 or tuple(flow_map.shape) != (B * h * w, 2):
        raise _lib.EvpError(f"{what}: the prediction must be a float32 map [B*h*w, 2] = [{B * h * w}, 2] (got {flow_map.dtype} {tuple(flow_map.shape)})")
    if target.dtype != torch.float32 or target.dim() != 4 or target.shape[0] != B or target.shape[1] != 2:
        raise _lib.EvpError(f"{what}: target must be float32 [B, 2, H, W] with B = {B} (got {target.dtype} {tuple(target.shape)})")
    H, W = int(target.shape[2]), int(target.shape[3])
    if valid.dtype != torch.float32:
        valid = valid.float()
    if tuple(valid.shape) != (B, 1, H, W):
        raise _lib.EvpError(f"{what}: valid must be [B, 1, H, W] = [{B}, 1, {H}, {W}] (got {tuple(valid.shape)})")
    m, ld = _map_in_place(flow_map)
    return m, ld, H, W, target.contiguous(), valid.contiguous()


def _flow_workspace(P, device):
    return torch.empty(call("evp_flow_nblk", P) * _lib.FLOW_WS_ROW, dtype=torch.int32, device=device)


class FlowObjectiveFn(torch.autograd.Function):
    """FlowLoss of the reference (trainer/finetune_flow/flow_loss.py) applied to resize_flow(prediction, label size): (flow_map
    [B*h*w, 2] float32, B, h, w, target float32 [B, 2, H, W], valid [B, 1, H, W], max_flow) -> the mean of |p - t| over both
    components of the pixels with valid >= 0.5 and |t| < max_flow, 0-d float32, differentiable in the map; NaN with an all-zero
    gradient when no pixel is valid. The resized prediction is never stored: forward is a pixel pass and a finishing launch, backward
    one gather launch that writes the map's gradient (same leading dimension as the map, pad columns zero). The map is read in place
    through its leading dimension (DenseClsFn's column slice of a padded matrix)."""

    @staticmethod
    def forward(ctx, flow_map, B, h, w, target, valid, max_flow):
        m, ld, H, W, tgt, val = _flow_operands("FlowObjectiveFn", flow_map, B, h, w, target, valid)
        dev = m.device
        out = torch.empty(1, dtype=torch.float32, device=dev)
        saved = torch.empty(_lib.FLOW_SAVED, dtype=torch.float32, device=dev)
        ws = _flow_workspace(B * H * W, dev)
        call("evp_flow_objective_fwd", m.data_ptr(), ld, B, h, w, H, W, ptr(tgt), ptr(val), float(max_flow), ptr(out), ptr(saved), ptr(ws),
             stream_ptr())
        ctx.save_for_backward(m, tgt, val, saved)
        ctx.cfg = (ld, B, h, w, H, W, float(max_flow))
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        m, tgt, val, saved = ctx.saved_tensors
        ld, B, h, w, H, W, max_flow = ctx.cfg
        grad = torch.empty(B * h * w, ld, dtype=torch.float32, device=m.device)
        call("evp_flow_objective_bwd", m.data_ptr(), ld, B, h, w, H, W, ptr(tgt), ptr(val), max_flow, ptr(saved),
             ptr(_chk(g_loss.contiguous().view(1), torch.float32)), ptr(grad), ld, stream_ptr())
        return (grad[:, :2],) + (None,) * 6


def flow_metrics(flow_map, B, h, w, target, valid, max_flow, org, table, cursor):
    """The evaluation record of one flow batch on the device (evp_flow_metrics; reference ft_flow_trainer.py:191-231): with
    s = cursor[0], table[s] = {l1 (FlowObjectiveFn's bits), aee, outlier} of resize_flow(prediction, label size) over the sparse mask
    -- valid non-zero and an event in `org` (float32 [B, C, H, W], the unnormalised voxel grid) at the pixel -- then cursor[0] = s + 1;
    a full table is left alone. Arguments as FlowObjectiveFn's; `table` float32 [capacity, 3] and `cursor` int64 [1] as cls_metrics'."""
    for t in (org, table, cursor):
        if not t.is_cuda:
            raise _lib.EvpError("flow_metrics: tensor is not in device memory; eventpretrain_amd has no CPU path")
    m, ld, H, W, tgt, val = _flow_operands("flow_metrics", flow_map, B, h, w, target, valid)
    if org.dim() != 4 or org.shape[0] != B or tuple(org.shape[2:]) != (H, W):
        raise ValueError(f"flow_metrics: the event grid must be [B, C, H, W] at the label's size [{B}, C, {H}, {W}] (got {tuple(org.shape)})")
    if org.dtype != torch.float32:
        raise _lib.EvpError(f"flow_metrics: the event grid must be float32 (got {org.dtype})")
    if table.dim() != 2 or table.shape[1] != 3 or cursor.numel() != 1:
        raise _lib.EvpError("flow_metrics: table must be float32 [capacity, 3] and cursor one int64")
    ws = _flow_workspace(B * H * W, m.device)
    call("evp_flow_metrics", m.data_ptr(), ld, B, h, w, H, W, ptr(tgt), ptr(val), float(max_flow), ptr(org.contiguous()), int(org.shape[1]),
         ptr(_chk(cursor, torch.int64)), ptr(_chk(table, torch.float32)), table.shape[0], ptr(ws), stream_ptr())

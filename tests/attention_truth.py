"""Shared by the CPU and GPU tests that pin the attention CORES to float64 truth (tests/test_attention_truth_host.py,
tests/test_gpu_attention_truth.py): the cases, their references, the families of sub-blocks and the mutants the gates must reject.

The cores are the oracle's own formulation without the Linear layers around it (oracle/model_oracle.py::attention and
::window_attention -- the latter with the -100 on blocked pairs and the bias zeroed there), on a packed qkv tensor [B, N, 3, heads, d_h]
drawn in f32 and rounded to bf16 ONCE, so that truth and the kernels see the same numbers; every (batch, head) has its own data.
Three runs per case, as in tests/block_truth.py: truth T in float64, yardstick Y in f32 under torch.autocast("cpu", bfloat16), F in
plain f32. Gradients are those of (out * dout).sum(). Tensors (named "core:..." for block_truth.families):
  ViT core     out, lse, dqkv (and its q, k, v thirds dq, dk, dv), attn where probabilities are returned;
  window core  out, lse, dqkv (dq, dk, dv), dtable.
lse is the logsumexp of the run's own logits. Gates: block_truth.compare -- whole tensor, scale, and the sub-block families of
block_truth._core_families: one block per (batch, head) and one per (batch, head, 16-row strip) for out, dq, dk, dv; one per
(batch, head) for lse and attn; one per head column for dtable. FACTOR, FLOOR and MAX_EXCLUDED are block_truth's.

N = 1 has no scale to measure with (Y equals T; dq = dk = 0 in truth): it never goes through the gates, the GPU test asserts what is
exact there instead."""
import contextlib
import functools
import math
import zlib

import torch

import block_truth as bt

R_TABLE = 169           # 13 x 13 relative positions of a 7 x 7 window
BLOCKED = 0.4           # share of blocked pairs in a window case
LN2 = math.log(2.0)

VIT_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 197, 209, 223, 224)      # fused ViT core, at d_h 32 and 64
HEAD_MAP = ((4, 4, 32), (8, 2, 32), (16, 3, 32), (3, 4, 32), (4, 4, 64))               # (B, heads, d_h) at N = 33
WIN_N = (16, 17, 32, 33, 64, 65, 81, 96, 97, 113, 128)                                # windowed core: B = 2 per group, nG = 3, heads = 2
WIN_WALK = ((16, 16, 3, 24, 2, 2), (22, 24, 3, 17, 3, 1), (8, 32, 3, 98, 2, 2), (16, 16, 5, 33, 3, 2))   # nG, heads, B, N, per, nchunk
UNFUSED_N = (17, 225, 260)
WAVES_N = (17, 65, 129, 224)                                                           # one per NT of the fused ViT kernels


def vit_name(B, heads, N, dh, amp=0.8):
    return f"vit_B{B}_h{heads}_N{N}_d{dh}" + ("" if amp == 0.8 else f"_x{amp:g}")


def win_name(nG, heads, B, N):
    return f"win_g{nG}_h{heads}_B{B}_N{N}"


SPECS = {}
for _dh in (32, 64):
    for _N in VIT_N + UNFUSED_N:
        SPECS[vit_name(2, 2, _N, _dh)] = dict(kind="vit", B=2, heads=2, N=_N, dh=_dh, amp=0.8)
    SPECS[vit_name(2, 2, 197, _dh, 3.0)] = dict(kind="vit", B=2, heads=2, N=197, dh=_dh, amp=3.0)       # peaked rows: logits of order +-15
for _B, _h, _dh in HEAD_MAP:
    SPECS[vit_name(_B, _h, 33, _dh)] = dict(kind="vit", B=_B, heads=_h, N=33, dh=_dh, amp=0.8)
for _N in WIN_N + (1,):
    SPECS[win_name(3, 2, 2, _N)] = dict(kind="win", nG=3, heads=2, B=2, N=_N, dh=32, amp=1.0)
for _g, _h, _B, _N, _, _ in WIN_WALK:
    SPECS[win_name(_g, _h, _B, _N)] = dict(kind="win", nG=_g, heads=_h, B=_B, N=_N, dh=32, amp=1.0)

FUSED_VIT = [vit_name(2, 2, N, dh) for dh in (32, 64) for N in VIT_N if N > 1]
HEAD_MAP_CASES = [vit_name(B, h, 33, dh) for B, h, dh in HEAD_MAP]
PEAKED = [vit_name(2, 2, 197, dh, 3.0) for dh in (32, 64)]
WIN_EDGE = [win_name(3, 2, 2, N) for N in WIN_N]
WIN_WALK_CASES = [win_name(g, h, B, N) for g, h, B, N, _, _ in WIN_WALK]
UNFUSED = [vit_name(2, 2, N, dh) for dh in (32, 64) for N in UNFUSED_N]
WAVES = [vit_name(2, 2, N, dh) for dh in (32, 64) for N in WAVES_N]


# ------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=8)
def make_case(name):
    """-> dict(spec fields, qkv bf16 [B(g), N, 3, heads, d_h], dout bf16 [B(g), N, heads * d_h], and for a window case table f32
    [R, heads], rel int64 [nG, N, N], blocked bool [nG, N, N]; batch row bg belongs to group bg % nG). Seeded from the name."""
    s = SPECS[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    Bt = s["B"] * s.get("nG", 1)
    N, h, dh = s["N"], s["heads"], s["dh"]
    c = dict(s, name=name, Bt=Bt, scale=dh ** -0.5)
    c["qkv"] = (torch.randn(Bt, N, 3, h, dh, generator=g) * s["amp"]).bfloat16()
    c["dout"] = torch.randn(Bt, N, h * dh, generator=g).bfloat16()
    if s["kind"] == "win":
        nG = s["nG"]
        c["table"] = torch.randn(R_TABLE, h, generator=g) * 0.5
        c["rel"] = torch.randint(0, R_TABLE, (nG, N, N), generator=g)
        blocked = torch.rand(nG, N, N, generator=g) < BLOCKED
        blocked[:, torch.arange(N), torch.arange(N)] = False          # the diagonal stays open ...
        if nG > 2:
            blocked[-1] = True                                        # ... but for one padding group: every pair blocked
        c["blocked"] = blocked
    return c


def rel_i32(c):
    """rel as the kernels take it: int32, -1 on the blocked pairs."""
    return torch.where(c["blocked"], torch.full_like(c["rel"], -1), c["rel"]).to(torch.int32)


# ------------------------------------------------------------------------------------------------------------- references
def _logits(c, q, k, table):
    """The logits as the oracle forms them: (q @ k^T) * scale for the ViT core; (q * scale) @ k^T + table[rel] (zeroed where blocked)
    - 100 where blocked for the window core."""
    if c["kind"] == "vit":
        return (q @ k.transpose(-2, -1)) * c["scale"]
    nG, N, h = c["nG"], c["N"], c["heads"]
    att = (q * c["scale"]) @ k.transpose(-2, -1)
    blocked = c["blocked"]
    bias = table[c["rel"].masked_fill(blocked, 0).reshape(-1)].view(nG, N, N, h) * (~blocked).view(nG, N, N, 1).float()
    mask = torch.where(blocked, -100.0, 0.0).to(table.dtype)
    att = att.view(c["Bt"] // nG, nG, h, N, N) + bias.permute(0, 3, 1, 2).unsqueeze(0) + mask.view(1, nG, 1, N, N)
    return att.view(c["Bt"], h, N, N)


def split(c, out=None, lse=None, dqkv=None, attn=None, dtable=None):
    """The tensors of a core as the comparator takes them: out and the thirds of dqkv as [B, heads, N, d_h]."""
    Bt, N, h, dh = c["Bt"], c["N"], c["heads"], c["dh"]
    r = {}
    if out is not None:
        r["core:out"] = out.reshape(Bt, N, h, dh).permute(0, 2, 1, 3)
    if lse is not None:
        r["core:lse"] = lse.reshape(Bt, h, N)
    if dqkv is not None:
        d = dqkv.reshape(Bt, N, 3, h, dh)
        r["core:dqkv"] = d
        for i, t in enumerate(("core:dq", "core:dk", "core:dv")):
            r[t] = d[:, :, i].permute(0, 2, 1, 3)
    if attn is not None:
        r["core:attn"] = attn.reshape(Bt, h, N, N)
    if dtable is not None:
        r["core:dtable"] = dtable
    return {k: v.detach().double().contiguous() for k, v in r.items()}


def core(c, qkv, table=None):
    """The oracle's attention / window_attention between its two Linear layers, on qkv [B, N, 3, heads, d_h] (the host test holds it
    against those two functions). -> (out [B, N, heads * d_h], probabilities, logits)."""
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    s = _logits(c, q, k, table)
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(c["Bt"], c["N"], -1), p, s


def _run(name, mode):
    c = make_case(name)
    dt = torch.float64 if mode == "truth" else torch.float32
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if mode == "yardstick" else contextlib.nullcontext()
    qkv = c["qkv"].to(dt).requires_grad_(True)
    table = c["table"].detach().clone().to(dt).requires_grad_(True) if c["kind"] == "win" else None      # a copy: the case is shared
    with ctx:
        out, p, s = core(c, qkv, table)
    lse = torch.logsumexp(s.detach().to(dt), -1)
    (out.to(dt) * c["dout"].to(dt)).sum().backward()
    return split(c, out, lse, qkv.grad, attn=p if c["kind"] == "vit" else None, dtable=None if table is None else table.grad)


class Reference:
    def __init__(self, name):
        self.name = name
        self.T, self.Y, self.F = _run(name, "truth"), _run(name, "yardstick"), _run(name, "f32")
        self.tensors = list(self.T)

    def e_ref(self, t):
        return bt.rel_err(self.Y[t], self.T[t])


@functools.lru_cache(maxsize=4)
def reference(name):
    """Computed once and shared by the tests that follow each other on one case; nobody writes into it."""
    return Reference(name)


def gate(name, got):
    """`got`: the output of split(). -> (failures, (worst ratio, "tensor/gate"), table as text), block_truth.compare_all's."""
    return bt.compare_all(got, reference(name))


# ------------------------------------------------------------------------------------------------------------- kernel geometry
def vit_np(N):
    """Rows of the LDS images of the fused ViT kernels (16 * NT, NT = 2 / 4 / 8 / 14)."""
    return 32 if N <= 32 else 64 if N <= 64 else 128 if N <= 128 else 224


def win_np(N):
    return 32 if N <= 32 else 64 if N <= 64 else 96 if N <= 96 else 128


def win_chunks(Bg, nG, heads, target=512):
    """(nchunk, per) of the windowed backward's batch walk: the formula of win_chunks in csrc/attention_fused.hip."""
    B = Bg // nG
    nc = max(1, min(B, -(-target // (nG * heads))))
    per = -(-B // nc)
    return -(-B // per), per


# ------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {
    "a_pad_keys_unmasked": "keys N .. NP - 1 stay in the softmax with score 0",
    "b_last_key_tile_dropped": "the last key tile (key N - 1 at N = 16 k + 1) is skipped by the last query strip",
    "c_head_pair_exchanged": "the two heads of a d_h = 32 pair exchanged in out",
    "d_dk_dv_exchanged": "dK and dV exchanged",
    "e_dq_unscaled": "scale missing from dQ",
    "f_lse_base2": "lse in base 2",
    "g_bias_transposed_in_dkdv": "window: the bias read transposed in the dK / dV pass",
    "h_dtable_last_item_missing": "window: the last batch item missing from dtable",
    "i_dq_stale_item": "window: one item's dq taken from the previous item of its (group, head)",
}
VIT_MUTANTS = tuple(MUTANTS)[:6]
WIN_MUTANTS = tuple(MUTANTS)[6:]


def manual(name, mutant=None):
    """The core written out by hand in float64 -- forward, then the backward in the two passes of the kernels (dQ from the query side,
    dK / dV from the key side, both from P = exp(logits - lse)) -- with at most one defect. Without a defect it is truth (the host
    test checks that against autograd); the host test lays the yardstick's noise over a mutant before it asks the gates."""
    assert mutant is None or mutant in MUTANTS, mutant
    c = make_case(name)
    Bt, N, h, dh, sc = c["Bt"], c["N"], c["heads"], c["dh"], c["scale"]
    win = c["kind"] == "win"
    q, k, v = c["qkv"].double().permute(2, 0, 3, 1, 4)
    do = c["dout"].double().view(Bt, N, h, dh).permute(0, 2, 1, 3)
    table = c["table"].double() if win else None
    s = _logits(c, q, k, table)
    s_fwd = s
    if mutant == "b_last_key_tile_dropped":
        assert N % 16 == 1
        s_fwd = s.clone()
        s_fwd[:, :, N - 1 - (N - 1) % 16:, N - 1] = -math.inf
    lse = torch.logsumexp(s_fwd, -1)
    if mutant == "a_pad_keys_unmasked":
        NP = win_np(N) if win else vit_np(N)
        assert NP > N
        lse = torch.logaddexp(lse, torch.full_like(lse, math.log(NP - N)))
    p = torch.exp(s_fwd - lse.unsqueeze(-1))
    o = p @ v
    if mutant == "c_head_pair_exchanged":
        o = o[:, [1, 0] + list(range(2, h))]
    # backward, from the forward's own out and lse
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-2, -1) - delta)                       # d logits
    dq = sc * (ds @ k)
    p2, ds2 = p, ds
    if mutant == "g_bias_transposed_in_dkdv":
        nG = c["nG"]
        add = (s - (q * sc) @ k.transpose(-2, -1)).view(Bt // nG, nG, h, N, N)
        s2 = (s.view_as(add) - add + add.transpose(-2, -1)).reshape(Bt, h, N, N)
        p2 = torch.exp(s2 - lse.unsqueeze(-1))
        ds2 = p2 * (do @ v.transpose(-2, -1) - delta)
    dk, dv = sc * (ds2.transpose(-2, -1) @ q), p2.transpose(-2, -1) @ do
    if mutant == "d_dk_dv_exchanged":
        dk, dv = dv, dk
    if mutant == "e_dq_unscaled":
        dq = dq / sc
    if mutant == "i_dq_stale_item":
        dq = dq.clone()
        dq[c["nG"]:2 * c["nG"]] = dq[:c["nG"]].clone()                   # the second item of every group repeats the first
    dtable = None
    if win:
        nG = c["nG"]
        dA = ds.view(Bt // nG, nG, h, N, N)
        dA = (dA[:-1] if mutant == "h_dtable_last_item_missing" else dA).sum(0)                # [nG, h, N, N]
        open_ = ~c["blocked"]
        dtable = torch.zeros(R_TABLE, h, dtype=torch.float64)
        dtable.index_add_(0, c["rel"][open_], dA.permute(0, 2, 3, 1)[open_])
    lse_out = lse / LN2 if mutant == "f_lse_base2" else lse
    dqkv = torch.stack([t.permute(0, 2, 1, 3) for t in (dq, dk, dv)], 2)       # [Bt, N, 3, h, dh]
    return split(c, o.permute(0, 2, 1, 3), lse_out, dqkv, attn=None if win else p, dtable=dtable)


# ------------------------------------------------------------------------------------------------------------- on the device
# Shared by tests/test_gpu_attention_truth.py and its child processes (tests/attention_fused_worker.py). Every output of a kernel lies
# inside a larger NaN-filled buffer: a guard of at least one (batch, head) plane of that output (rounded up to 64 elements, which keeps
# the 16-byte alignment of the kernels' vector stores) in front of it and behind it.
class Guarded:
    def __init__(self, what, shape, dtype, plane):
        self.what, self.n, self.g = what, math.prod(shape), -(-max(plane, 1) // 64) * 64
        self.buf = torch.full((self.n + 2 * self.g,), math.nan, dtype=dtype, device="cuda")
        self.t = self.buf[self.g:self.g + self.n].view(shape)

    def check(self, inner=None):
        """Guards untouched, and every in-range element (of `inner`, where the kernel leaves part of the buffer unwritten) finite."""
        assert torch.isnan(self.buf[:self.g]).all(), f"{self.what}: written in front of the buffer"
        assert torch.isnan(self.buf[self.g + self.n:]).all(), f"{self.what}: written past the end of the buffer"
        assert torch.isfinite(self.t if inner is None else inner).all(), f"{self.what}: not finite (or not written)"


def run_fused_vit(name, want_probs):
    """evp_attention_fused_fwd (with or without probs) and evp_attention_fused_bwd on the forward's own bf16 out.
    -> (split() of the device tensors on the CPU, raw dict(out, lse, dqkv, probs) on the CPU)."""
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    c = make_case(name)
    B, N, h, dh = c["Bt"], c["N"], c["heads"], c["dh"]
    ldp = (N + 7) // 8 * 8
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    out = Guarded("out", (B, N, h * dh), torch.bfloat16, N * h * dh)
    lse = Guarded("lse", (B, h, N), torch.float32, N)
    probs = Guarded("probs", (B, h, N, ldp), torch.bfloat16, N * ldp) if want_probs else None
    dqkv = Guarded("dqkv", (B, N, 3, h, dh), torch.bfloat16, N * 3 * h * dh)
    call("evp_attention_fused_fwd", ptr(qkv), B, N, h, dh, c["scale"], ptr(out.t), ptr(lse.t), ptr(probs.t) if want_probs else None, ldp,
         stream_ptr())
    call("evp_attention_fused_bwd", ptr(qkv), ptr(out.t), ptr(dout), ptr(lse.t), B, N, h, dh, c["scale"], ptr(dqkv.t), stream_ptr())
    torch.cuda.synchronize()
    for gd in (out, lse, dqkv) + ((probs,) if want_probs else ()):
        gd.check()
    raw = dict(out=out.t.cpu(), lse=lse.t.cpu(), dqkv=dqkv.t.cpu(), probs=probs.t.cpu() if want_probs else None)
    if want_probs:
        assert (raw["probs"][..., N:] == 0).all(), "probs: pad columns N .. ldp not zero"
    return split(c, raw["out"], raw["lse"], raw["dqkv"], attn=raw["probs"][..., :N] if want_probs else None), raw


def gate_report(name, got, what):
    """Prints the worst ratio and the table, -> the failures."""
    fails, worst, table = gate(name, got)
    print(f"\n[{what}] worst e_hip / e_ref = {worst[0]:.2f} at {worst[1]} (bound {bt.FACTOR:g})\n{table}")
    return fails, worst

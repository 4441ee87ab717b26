"""The attention cores on the GPU -- the fused ViT kernels, the windowed MFMA chain and the unfused bf16 core, called through the C
ABI -- against the float64 run of the oracle's formulation (tests/attention_truth.py): at every edge of the tile dispatch, with the
head-pair renumbering on and off, with more than one batch item per workgroup of the windowed backward, and at the other wave counts.
The bound of every tensor and sub-block is FACTOR = 3 times the error of the same formulation under CPU autocast to bf16
(block_truth.compare); the host half (tests/test_attention_truth_host.py) shows what these gates accept and reject.

Every output lies in a NaN-filled buffer with a guard of at least one (batch, head) plane on both sides: the guards must stay NaN
and every in-range element must be finite. Every test hands its cases to one child process (tests/attention_fused_worker.py, which
says why; the runners of the windowed chain and of the unfused core are below). Each child prints, per case, the worst e_hip / e_ref with its tensor and gate; the docstrings record
the figures of an MI355X run."""
import os
import subprocess
import sys

import pytest
import torch

import attention_truth as at

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23


def _child(group, extra_env=None):
    """One fresh process of tests/attention_fused_worker.py on a group of cases (the worker's docstring says why these kernels are not
    launched in the suite's own process); its output is printed, a non-zero exit fails the test with it."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_fused_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("EVP_ATTN_FWD_WAVES", "EVP_ATTN_BWD_WAVES")}
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, worker, group], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, f"{group} {extra_env or ''}: exit {r.returncode}\n{r.stdout[-8000:]}\n{r.stderr[-4000:]}"
    assert "all gates hold" in r.stdout


def test_fused_vit_core_at_tile_edges():
    """evp_attention_fused_fwd / _bwd at B = 2, heads = 2 and every N next to a dispatch edge of NT (32 | 33, 64 | 65, 128 | 129), at
    both ends of a 16-row strip (15, 16, 17, ...) and of the supported range (223, 224), d_h = 32 and 64 (attention_truth.FUSED_VIT);
    forward with and without probs (pad columns N .. ldp zero), the backward on the forward's own bf16 out. One child process runs
    the 32 cases, each through all gates and guards.
    MI355X: worst ratio per case 0.69 .. 0.89 at d_h = 32 (0.89: N = 15, out / strip16) and 0.79 .. 0.98 at d_h = 64 (0.98: N = 209,
    dv / strip16), the same with and without probs; lse at 0.00 everywhere (the kernels keep the scores in f32)."""
    _child("edges")


def test_fused_vit_core_head_mapping():
    """head_of_block at N = 33: the pair renumbering is on at d_h = 32 with B * heads a multiple of 16 and heads even ((4, 4), (8, 2)),
    off with odd heads (16, 3), with B * heads = 12 (3, 4) and at d_h = 64 (4, 4). Every (batch, head) has its own data, and the
    per-(batch, head) family measures each one against its own truth.
    MI355X: 0.81 (4, 4), 0.77 (8, 2), 0.72 (16, 3), 0.74 (3, 4), 0.90 (4, 4 at d_h = 64)."""
    _child("heads")


def test_fused_vit_core_peaked_rows():
    """Inputs randn * 3: logits of order +-15, rows dominated by a few keys -- the max subtraction and lse.
    MI355X: 0.40 at d_h = 32, 0.39 at d_h = 64 (dq / strip16): the yardstick rounds logits of that size to bf16, the kernels do not."""
    _child("peaked")


def test_fused_vit_core_single_token_identities():
    """N = 1 at d_h = 32 and 64: out = v and dv = dout bit for bit, P = 1, lse = q.k * scale within f32 rounding, |dq| and |dk| under
    the summation-order bound derived in attention_fused_worker.single_token."""
    _child("single_token")


def _run_window(name):
    """bias_build -> fused_fwd -> fused_bwd -> bias_reduce. -> (split() of the outputs, raw tensors on the CPU, nchunk)."""
    from eventpretrain_amd._lib import call, ptr, stream_ptr
    c = at.make_case(name)
    Bg, nG, N, H, dh, R = c["Bt"], c["nG"], c["N"], c["heads"], c["dh"], at.R_TABLE
    qkv, dout, table, rel = c["qkv"].cuda(), c["dout"].cuda(), c["table"].cuda(), at.rel_i32(c).cuda()
    NP = call("evp_window_attention_fused_np", N)
    nchunk = call("evp_window_attention_fused_nchunk", Bg, nG, H)
    assert NP == at.win_np(N) and nchunk == at.win_chunks(Bg, nG, H)[0]
    addm = torch.full((nG, H, NP, NP), float("nan"), device="cuda")
    addmT = torch.full_like(addm, float("nan"))
    call("evp_window_bias_build", ptr(table), ptr(rel), nG, N, H, R, ptr(addm), ptr(addmT), stream_ptr())
    assert torch.isfinite(addm).all() and torch.equal(addm.transpose(2, 3), addmT)
    out = at.Guarded("out", (Bg, N, H * dh), torch.bfloat16, N * H * dh)
    lse = at.Guarded("lse", (Bg, H, N), torch.float32, N)
    dqkv = at.Guarded("dqkv", (Bg, N, 3, H, dh), torch.bfloat16, N * 3 * H * dh)
    dA = at.Guarded("dA", (nchunk, nG, H, NP, NP), torch.float32, NP * NP)
    dtab = at.Guarded("dtable", (R, H), torch.float32, H)
    dtab.t.fill_(7.0)                                     # overwritten, not accumulated
    call("evp_window_attention_fused_fwd", ptr(qkv), ptr(addm), Bg, nG, N, H, c["scale"], ptr(out.t), ptr(lse.t), stream_ptr())
    call("evp_window_attention_fused_bwd", ptr(qkv), ptr(out.t), ptr(dout), ptr(lse.t), ptr(addm), ptr(addmT), Bg, nG, N, H, c["scale"],
         ptr(dqkv.t), ptr(dA.t), stream_ptr())
    call("evp_window_bias_reduce", ptr(dA.t), ptr(rel), Bg, nG, N, H, R, ptr(dtab.t), stream_ptr())
    torch.cuda.synchronize()
    for gd in (out, lse, dqkv, dtab):
        gd.check()
    dA.check(inner=dA.t[..., :N, :N])                     # the N x N part of every plane is written
    raw = dict(out=out.t.cpu(), lse=lse.t.cpu(), dqkv=dqkv.t.cpu(), dtable=dtab.t.cpu())
    return at.split(c, raw["out"], raw["lse"], raw["dqkv"], dtable=raw["dtable"]), raw, nchunk


def test_window_mfma_chain_at_tile_edges():
    """The windowed chain at d_h = 32, R = 169, B = 2 per group, nG = 3 (the last group with every pair blocked), heads = 2, 40 % of
    the pairs blocked: N on both sides of NP = 32 | 64 | 96 | 128, NT = 6 with its half-used chunk of the backward (65, 81, 96).
    MI355X: 0.60 .. 0.77, and 1.33 at N = 17 (dq / strip16: the strip of one row)."""
    _child("win_edge")


def window_edge(name):
    got, _, nchunk = _run_window(name)
    assert nchunk == 2
    return at.gate_report(name, got, name)


def test_window_mfma_backward_batch_walk():
    """win_attn_bwd_mfma_kernel with more than one batch item per workgroup: LDS restaged between items, dacc carried across them,
    the early break on a ragged last chunk (B = 3, per = 2; B = 5, per = 3), one chunk only (per = 3 = B), and the 8-wave form
    (N = 98). per and nchunk of the table are checked against evp_window_attention_fused_nchunk.
    MI355X, in the order of the table: 1.09 (dq / head), 1.58 (dk / strip16, the one-row strip of N = 17), 0.76, 1.07; dtable 0.54, 0.72, 0.23, 0.44."""
    _child("win_walk")


def window_walk(nG, heads, B, N, per, nchunk):
    from eventpretrain_amd._lib import call
    name = at.win_name(nG, heads, B, N)
    assert call("evp_window_attention_fused_nchunk", B * nG, nG, heads) == nchunk
    assert at.win_chunks(B * nG, nG, heads) == (nchunk, per) and per > 1 and -(-B // per) == nchunk
    return at.gate_report(name, _run_window(name)[0], name)


def test_window_mfma_chain_single_token_identities():
    """N = 1 (attention_fused_worker.single_token has the derivation): out = v and dv = dout bit for bit, lse = q.k * scale + bias within f32
    rounding, |dq|, |dk| under the summation-order bound, and dtable[r, h] -- the sum over the batch items and open groups with
    rel = r of P * (dP - delta) -- under the sum of the same bounds without the scale and the bf16 roundings (dA is f32)."""
    _child("win_single_token")


def window_single_token():
    name = at.win_name(3, 2, 2, 1)
    c = at.make_case(name)
    _, raw, _ = _run_window(name)
    Bg, nG, h, dh = c["Bt"], c["nG"], c["heads"], c["dh"]
    q, k, v = c["qkv"].view(Bg, 3, h, dh).unbind(1)
    do = c["dout"].view(Bg, h, dh)
    assert torch.equal(raw["out"].view(Bg, h, dh), v)
    d = raw["dqkv"].view(Bg, 3, h, dh)
    assert torch.equal(d[:, 2], do)
    grp = torch.arange(Bg) % nG
    blocked, rel = c["blocked"].view(nG), c["rel"].view(nG)
    bias = torch.where(blocked.view(nG, 1), torch.tensor(-100.0, dtype=torch.float64), c["table"].double()[rel])[grp]      # [Bg, h]
    dot = (q.double() * k.double()).sum(-1) * c["scale"]
    # the f32 sum of d_h products, then at most six roundings at the logit's magnitude: scale * log2(e) and bias * log2(e) (constant
    # and product each), their fma, and the product with ln 2 and its constant
    tol = (dh + 2) * U23 * (q.double() * k.double()).abs().sum(-1) * c["scale"] + 6 * U23 * (bias.abs() + dot.abs())
    assert ((raw["lse"].view(Bg, h).double() - (dot + bias)).abs() <= tol).all()
    gam = 2 * (dh - 1) * U23 * (do.double() * v.double()).abs().sum(-1, keepdim=True)                                     # [Bg, h, 1]
    assert (d[:, 0].double().abs() <= 1.02 * c["scale"] * gam * k.double().abs()).all()
    assert (d[:, 1].double().abs() <= 1.02 * c["scale"] * gam * q.double().abs()).all()
    bound = torch.zeros(at.R_TABLE, h, dtype=torch.float64)
    opened = ~blocked[grp]
    bound.index_add_(0, rel[grp][opened], 1.02 * gam[opened, :, 0])
    assert (raw["dtable"].double().abs() <= bound).all()


def test_unfused_bf16_core_beyond_the_fused_range():
    """evp_attention_fwd / evp_attention_bwd in bf16 where they are what runs (N = 225, 260 > 224) and at N = 17: probs, out, dqkv.
    MI355X: 0.69 .. 0.81 at N = 225 and 260, 0.97 (d_h = 32) and 1.11 (d_h = 64, dk / strip16) at N = 17."""
    _child("unfused")


def unfused(name):
    from eventpretrain_amd._lib import EVP_BF16, call, ptr, stream_ptr
    c = at.make_case(name)
    B, N, h, dh = c["Bt"], c["N"], c["heads"], c["dh"]
    ldp = (N + 7) // 8 * 8
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    scores = torch.full((B * h * N * ldp,), float("nan"), device="cuda")
    dp = torch.full_like(scores, float("nan"))
    ds = torch.full((B * h * N * ldp,), float("nan"), dtype=torch.bfloat16, device="cuda")
    probs = at.Guarded("probs", (B, h, N, ldp), torch.bfloat16, N * ldp)
    out = at.Guarded("out", (B, N, h * dh), torch.bfloat16, N * h * dh)
    dqkv = at.Guarded("dqkv", (B, N, 3, h, dh), torch.bfloat16, N * 3 * h * dh)
    call("evp_attention_fwd", ptr(qkv), EVP_BF16, B, N, h, dh, c["scale"], ptr(scores), ptr(probs.t), ldp, ptr(out.t), stream_ptr())
    call("evp_attention_bwd", ptr(qkv), ptr(probs.t), ptr(dout), EVP_BF16, B, N, h, dh, c["scale"], ldp, ptr(dp), ptr(ds), ptr(dqkv.t),
         stream_ptr())
    torch.cuda.synchronize()
    for gd in (probs, out, dqkv):
        gd.check()
    p = probs.t.cpu()
    assert (p[..., N:] == 0).all()
    return at.gate_report(name, at.split(c, out.t.cpu(), None, dqkv.t.cpu(), attn=p[..., :N]), name)


WAVE_RUNS = (dict(EVP_ATTN_FWD_WAVES="8", EVP_ATTN_BWD_WAVES="4"), dict(EVP_ATTN_BWD_WAVES="16"))


def test_fused_vit_core_other_wave_counts():
    """The instantiations the defaults (4 waves forward, 8 backward) never launch: 8 forward with 4 backward, then 16 backward, each in
    a fresh child process (the wave counts are read once per process) that runs N = 17, 65, 129, 224 at both d_h through the same
    gates. The first child that exits non-zero ends the test with its output; the next one is not started.
    MI355X: both children 0.70 .. 0.92, case by case the figures of the default wave counts (the strips are computed alike)."""
    for extra in WAVE_RUNS:
        _child("waves", extra)

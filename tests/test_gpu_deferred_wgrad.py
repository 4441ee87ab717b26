"""The deferred bf16 weight / bias gradients on the device against float64:
  a. the grouped entries on their own: evp_gemm_grouped_tn_bf16 (128x128 tiles, K tail masked at kend), evp_sum_slices_f32,
     evp_colsum_grouped -- exact on small integers;
  b. the whole deferred engine (eager flush and build_deferred_plan steps, G4 and XCD order on / off) on the synthetic queues
     of tests/test_deferred_wgrad_host.py: integer data, so every .grad must be bit-equal to the float64 truth;
  c. real bf16 steps at bench shapes, each gradient pinned to its own queued operands (dY, X, partial rows) in float64."""
import numpy as np
import pytest
import torch

import deferred_plan as dp

pytestmark = pytest.mark.gpu


def _call(entry, pt, it, n):
    from eventpretrain_amd._lib import call, stream_ptr
    call(entry, pt.data_ptr(), it.data_ptr(), n, stream_ptr())


# ------------------------------------------------------------------------------------------------------ a. entries
def _grouped_128(specs, ints, gen, pad_items=True):
    probs = np.zeros(len(specs), dtype=dp.PDT)
    keep, items = [], []
    for i, (M, N, K, acc) in enumerate(specs):
        if ints:
            dy = torch.randint(-3, 4, (K, M), generator=gen, device="cuda").bfloat16()
            x = torch.randint(-3, 4, (K, N), generator=gen, device="cuda").bfloat16()
        else:
            dy = torch.randn(K, M, generator=gen, device="cuda").bfloat16()
            x = torch.randn(K, N, generator=gen, device="cuda").bfloat16()
        c = torch.full((M, N), 3.0, device="cuda")
        keep.append((dy, x, c, acc))
        probs[i] = (dy.data_ptr(), x.data_ptr(), c.data_ptr(), M, N, K, M, N, N, int(acc), 0, 0)
        for tn in range((N + 127) // 128):
            for tm in range((M + 127) // 128):
                items.append((i, tm, tn, 0))
                if pad_items and (tm + tn) % 3 == 0:
                    items.append((-1, 0, 0, 0))       # padding entries between live ones are skipped
    pt = torch.from_numpy(probs.view(np.uint8)).cuda()
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    _call(dp.T128, pt, it, len(items))
    torch.cuda.synchronize()
    return keep


# (M, N, K, accumulate): ragged M / N (multiples of 8 only), K below one 64-deep stage, between stages, one long K
SPECS_128 = [(136, 264, 16, False), (128, 128, 32, True), (200, 72, 48, False), (392, 520, 80, True), (256, 384, 6272, False),
             (72, 1032, 80, False), (520, 24, 6272, True)]


def test_grouped_tn128_exact_on_integers():
    """evp_gemm_grouped_tn_bf16: dW = dY^T X of several problems in one launch, exact on small integers (every partial sum is
    an integer below 2^24); K in {16, 32, 48, 80, 6272} pins down the K-tail masking at kend; accumulate on and off; padding
    items (prob = -1) interleaved."""
    gen = torch.Generator(device="cuda").manual_seed(21)
    for dy, x, c, acc in _grouped_128(SPECS_128, True, gen):
        ref = dy.double().t() @ x.double() + (3.0 if acc else 0.0)
        assert torch.equal(c.double(), ref), (tuple(c.shape), dy.shape[0], acc)


def test_grouped_tn128_random_within_f32_accumulation():
    """Random bf16 operands: f32 accumulation error bounded by a few ulps of sum |a||b| per element."""
    gen = torch.Generator(device="cuda").manual_seed(22)
    for dy, x, c, acc in _grouped_128(SPECS_128, False, gen):
        K = dy.shape[0]
        ref = dy.double().t() @ x.double() + (3.0 if acc else 0.0)
        scale = dy.double().abs().t() @ x.double().abs() + 3.0
        err = ((c.double() - ref).abs() / scale).max().item()
        assert err <= 4 * 2.0 ** -24 * max(1.0, (K / 16) ** 0.5), (tuple(c.shape), K, err)


def test_sum_slices_exact():
    """evp_sum_slices_f32: out (+)= sum over slices, integer data (exact), accumulate on and off, n_slices 1 .. 13."""
    from eventpretrain_amd._lib import call, stream_ptr
    gen = torch.Generator(device="cuda").manual_seed(23)
    for ns, numel in [(1, 4), (5, 1536 * 384), (13, 1028), (64, 4096)]:
        ws = torch.randint(-1000, 1000, (ns * numel,), generator=gen, device="cuda").float()
        for acc in (0, 1):
            out = torch.full((numel + 4,), 11.0, device="cuda")
            call("evp_sum_slices_f32", ws.data_ptr(), out.data_ptr(), ns, numel, acc, stream_ptr())
            torch.cuda.synchronize()
            ref = ws.view(ns, numel).double().sum(0) + (11.0 if acc else 0.0)
            assert torch.equal(out[:numel].double(), ref), (ns, numel, acc)
            assert torch.equal(out[numel:], torch.full((4,), 11.0, device="cuda"))     # nothing past numel


def test_colsum_grouped_exact():
    """evp_colsum_grouped: several bf16 / f32 problems in one launch, ld > N, N not a multiple of 128 (and not of 8 for a
    scalar tail), M not a multiple of 256; outputs accumulate (atomics) onto what they hold."""
    gen = torch.Generator(device="cuda").manual_seed(24)
    specs = [(300, 200, 208, torch.bfloat16), (513, 520, 520, torch.float32), (7, 12, 24, torch.float32),
             (1000, 1032, 1040, torch.bfloat16), (256, 128, 136, torch.bfloat16), (9, 2304, 2304, torch.float32)]
    probs = np.zeros(len(specs), dtype=dp.CDT)
    keep, items = [], []
    for i, (M, N, ld, dtp) in enumerate(specs):
        xs = torch.randint(-8, 9, (M, ld), generator=gen, device="cuda").to(dtp)
        out = torch.full((N + 8,), 2.0, device="cuda")
        keep.append((xs, out, N))
        probs[i] = (xs.data_ptr(), out.data_ptr(), M, N, ld, 0 if dtp == torch.float32 else 1, 0)
        for rs in range((M + 255) // 256):
            for cb in range((N + 127) // 128):
                items.append((i, cb, rs, 0))
    from eventpretrain_amd import _lib
    assert (_lib.EVP_F32, _lib.EVP_BF16) == (0, 1)
    perm = torch.randperm(len(items), generator=torch.Generator().manual_seed(1))
    items = [items[j] for j in perm]
    pt = torch.from_numpy(probs.view(np.uint8)).cuda()
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    _call(dp.COLSUM, pt, it, len(items))
    torch.cuda.synchronize()
    for xs, out, N in keep:
        ref = xs[:, :N].double().sum(0) + 2.0
        assert torch.equal(out[:N].double(), ref), (tuple(xs.shape), N)
        assert torch.equal(out[N:], torch.full((8,), 2.0, device="cuda"))


# ------------------------------------------------------------------------------------------------------ b. the engine
def _to_cuda(d):
    """The synthetic queue of a host case with every tensor (and parameter, and pre-existing .grad) on the device."""
    from eventpretrain_amd import ops
    pmap = {}

    def P(p_):
        if p_ is None:
            return None
        if id(p_) not in pmap:
            q = torch.nn.Parameter(p_.detach().cuda())
            if p_.grad is not None:
                q.grad = p_.grad.cuda()
            pmap[id(p_)] = q
        return pmap[id(p_)]
    g = ops._DeferredGrads()
    g.w = [(P(p_), dy.cuda(), x.cuda(), n, k, r, P(b)) for (p_, dy, x, n, k, r, b) in d.w]
    g.b = [(P(p_), x2d.cuda()) for p_, x2d in d.b]
    return g


@pytest.mark.parametrize("g4,xcd", [(True, True), (True, False), (False, True)])
def test_engine_bit_equal_on_integer_queues(g4, xcd):
    """Every synthetic queue (tests/test_deferred_wgrad_host.py NUMERIC_CASES, including the 39200-row ConvViT stage-2 problem
    that left a 32-row G4 slice before the planner fix) through eager flush() and through build_plan(n) steps for n = 1 .. 4:
    every .grad bit-equal to the float64 truth."""
    from eventpretrain_amd import ops
    from test_deferred_wgrad_host import NUMERIC_CASES, _queue_case, truth
    ops.set_wgrad_g4(g4)
    ops.set_wgrad_xcd_order(xcd)
    try:
        for case in NUMERIC_CASES:
            for mode in ("eager", 1, 2, 3, 4):
                d = _to_cuda(_queue_case(case, torch.Generator().manual_seed(NUMERIC_CASES.index(case))))
                ref = truth(d.w, d.b)
                if mode == "eager":
                    d.flush()
                else:
                    for st in d.build_plan(mode):
                        st.run()
                torch.cuda.synchronize()
                for p_, r in ref.values():
                    assert torch.equal(p_.grad.double(), r), (case, mode, tuple(p_.shape))
                del d, ref
    finally:
        ops.set_wgrad_g4(True)
        ops.set_wgrad_xcd_order(True)


# ------------------------------------------------------------------------------------------------------ c. real steps
def _snapshot_truth(w, b):
    """float64 truth of every queued parameter, computed on the device one contribution at a time (the float64 copy of a
    ConvViT stage-1 dY alone is 1.6 GB at B = 64)."""
    ref = {}

    def add(p_, f):
        v = f().reshape(p_.shape)
        if id(p_) in ref:
            ref[id(p_)][1].add_(v)
        else:
            base = p_.grad.double() if p_.grad is not None else torch.zeros(p_.shape, dtype=torch.float64, device="cuda")
            ref[id(p_)] = (p_, base.add_(v))
    for (p_, dy, x, n_out, k_in, rows, bias) in w:
        add(p_, lambda: _tn_f64(dy, x))
        if bias is not None:
            add(bias, lambda: dy.double().sum(0))
    for p_, x2d in b:
        add(p_, lambda: x2d.double().sum(0))
    return ref


def _tn_f64(dy, x, chunk=16384):
    out = None
    for k0 in range(0, dy.shape[0], chunk):
        v = dy[k0:k0 + chunk].double().t() @ x[k0:k0 + chunk].double()
        out = v if out is None else out.add_(v)
    return out


def _errors(g, r):
    """(relative error of the whole gradient, worst per-128x128-block error relative to that block's reference norm)"""
    g, r = g.double(), r.double()
    rel = ((g - r).norm() / r.norm().clamp_min(1e-300)).item()
    if r.dim() == 1:
        r2, g2 = r.view(1, -1), g.view(1, -1)
    else:
        r2, g2 = r.reshape(r.shape[0], -1), g.reshape(g.shape[0], -1)
    M, N = r2.shape
    Mp, Np = (M + 127) // 128 * 128, (N + 127) // 128 * 128
    pad = lambda t: torch.nn.functional.pad(t, (0, Np - N, 0, Mp - M))
    blk = lambda t: pad(t).view(Mp // 128, 128, Np // 128, 128).pow(2).sum((1, 3)).sqrt()
    rn, en = blk(r2), blk(g2 - r2)
    floor = 1e-6 * r2.norm() / max(1, rn.numel()) ** 0.5          # blocks of an all-but-zero reference
    worst = (en / torch.maximum(rn, floor)).max().item()
    return rel, worst


def _real_step(config, B, phase=None):
    from eventpretrain_amd import ops
    from eventpretrain_amd.model.pretrain import pr_hub_model as hub
    from eventpretrain_amd.testing import make_args
    import bench
    bb, size, ph, fac = bench.CONFIGS[config][1:5] if config in bench.CONFIGS else dp.EXTRA_CONFIGS[config]
    ph = phase or ph
    a = make_args(model_size=size, pr_phase=ph, backbone_type=bb, device="cuda", batch_size=B, use_queue=True, mask_ratio=0.5)
    torch.manual_seed(1234)
    m = getattr(hub, fac)(a, emb_frames_dim=512, queue_length=64, T=0.07).cuda().train()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 5, 224, 224, generator=g).cuda() * 0.5
    y = torch.randn(B, 1, 224, 224, generator=g).cuda()
    noise = torch.rand(B, m.backbone.num_patches, generator=g).cuda()
    ops.set_compute_dtype(torch.bfloat16)
    ops.hold_deferred_grads(True)
    try:
        loss = m(x, y, is_rec=True, noise=noise)[0]
        if ph == "rec+con":
            clip = torch.randn(B, 197, 512, generator=g).cuda()
            loss = loss + m(x, clip)[0]
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.hold_deferred_grads(False)
    q = ops._deferred
    w, b = list(q.w), list(q.b)
    assert w, "nothing was queued"
    ref = _snapshot_truth(w, b)
    names = {id(p_): n for n, p_ in m.named_parameters()}
    rounds = max(sum(1 for it in w if it[0] is p_) for p_, _ in ref.values())
    del w, b
    ops.flush_deferred_grads()
    torch.cuda.synchronize()
    out = []
    for p_, r in ref.values():
        out.append((names.get(id(p_), "?"),) + _errors(p_.grad, r))
    ops.set_compute_dtype(torch.float32)
    return out, rounds


REAL_CASES = [("vit_base_rec", 64, None), ("convvit_base_rec", 64, None), ("convvit_base_rec", 50, None), ("vit_small_rec", 8, "rec+con")]


@pytest.mark.parametrize("config,B,phase", REAL_CASES)
def test_real_step_gradients_match_their_own_operands(config, B, phase):
    """A real bf16 step at bench shapes with the queue held: the float64 truth of every deferred gradient is computed from the
    queued operands themselves (dY^T X, sum_rows dY, the LayerNorm backward's partial rows), then the queue is flushed. Gates
    per parameter: |g - ref| / |ref| <= 6e-6, and every 128x128 block within 1e-4 of that block's reference norm -- a
    dropped or doubled tile or K-slice moves a block by O(1) and the whole gradient by >= 1e-3.
    Measured on an MI355X (worst parameter): relative 5.9e-7 / 5.9e-7 / 5.2e-7 / 5.2e-7 and per-block 1.7e-5 / 2.5e-5 /
    1.9e-5 / 5.3e-6 for the four cases below; the whole-gradient gate is 10x the worst measured value.
    ViT-Base B=64: G4 + fused bias + LN partial rows; ConvViT-Base B=64: K-slices at stages 1 and 2; ConvViT-Base B=50:
    the folded 32-row tail; ViT-Small rec+con: two rounds per backbone parameter."""
    res, rounds = _real_step(config, B, phase)
    if phase == "rec+con":
        assert rounds >= 2
    worst_rel = max(res, key=lambda t: t[1])
    worst_blk = max(res, key=lambda t: t[2])
    print(f"{config} B={B} {phase or ''}: {len(res)} params, worst rel {worst_rel[1]:.2e} ({worst_rel[0]}), "
          f"worst block {worst_blk[2]:.2e} ({worst_blk[0]})")
    bad = [t for t in res if not (t[1] <= 6e-6 and t[2] <= 1e-4)]
    assert not bad, bad[:8]

"""The seams of the reconstruction step and the optimizer update against float64 truth (tests/pretrain_truth.py): evp_rec_loss,
evp_unshuffle_fwd / _bwd, evp_add_rows_gather_f32, evp_patchify, evp_density_noise, evp_mask_from_noise, the AdamW update and the
element-wise entries, each through the C ABI at the shapes where its paths part and, where ops.py / optim.py wrap it, through the
wrapper as well (the wrappers size the workspaces). Every output lies inside a NaN-filled buffer whose slack must stay untouched; an
output that a wrong kernel could add into instead of overwriting starts at 7.0. Each case runs in two versions: small integers
(equality) and random values (the gates). The host half (tests/test_pretrain_truth_host.py) shows what the gates accept and reject.

Each test prints its worst error over the bound per tensor; pretrain_truth's docstring records the figures of an MI355X run."""
import pytest
import torch

import pretrain_truth as pt
from test_gpu_contrast_truth import Canary, _api, _dev, _run

pytestmark = pytest.mark.gpu


def _seven(shape, dtype=torch.float32):
    """An output that must be overwritten, not added into: 7.0 inside, NaN slack."""
    return Canary(shape, dtype, init=torch.full(shape if isinstance(shape, tuple) else (shape,), 7.0))


# ---------------------------------------------------------------------------------------------------------------- evp_rec_loss
def _hip_rec(c):
    """evp_rec_loss with and without dpred. -> loss, per_row (the workspace), dpred."""
    call, dt, ptr, stream_ptr = _api()
    B, L, P, rows = c["B"], c["L"], c["P"], c["rows"]
    pred, target, mask = _dev(c["pred"]), _dev(c["target"]), _dev(c["mask"])
    out = []
    for grads in (True, False):
        loss, ws = _seven(1), Canary(rows + 1)
        dpred = Canary((B, L, P)) if grads else None
        call("evp_rec_loss", ptr(pred), ptr(target), ptr(mask), B, c["C"], c["H"], c["W"], c["p"], c["norm_pix"], ptr(loss.t),
             ptr(dpred.t) if grads else None, ptr(ws.t), stream_ptr())
        torch.cuda.synchronize()
        out.append(dict(loss=loss.take("loss").view(()), per_row=ws.take("workspace")[:rows]))
        if grads:
            out[0]["dpred"] = dpred.take("dpred")
    assert torch.equal(out[0]["loss"], out[1]["loss"]) and torch.equal(out[0]["per_row"], out[1]["per_row"]), "the dpred = NULL form differs"
    return out[0]


def _ops_rec(c, upstream=pt.UPSTREAM):
    from eventpretrain_amd import ops
    cp = c["pred"].cuda().requires_grad_(True)
    loss = ops.RecLossFn.apply(cp, c["target"].cuda(), _dev(c["mask"]), c["p"], bool(c["norm_pix"]))
    assert loss.dim() == 0
    (loss * upstream).backward()
    return dict(loss=loss.detach().cpu(), dpred=cp.grad.cpu())


@pytest.mark.parametrize("shape", pt.REC_SHAPES, ids=lambda s: "%dx%dx%dx%d_p%d" % s)
def test_rec_loss_against_float64(shape):
    """evp_rec_loss and RecLossFn (upstream gradient 0.25) with norm_pix 0 / 1 x no mask / half / all ones / a single one: the loss
    (1e-5 relative), the per-row losses in the workspace (f32 class), dpred (rtol 1e-4, atol 1e-7), dpred exactly 0 on unmasked rows;
    with integers and norm_pix = 0 the per-row losses and dpred are equal to the exact values, the loss too where P is a power of two.
    Truth: frame2emb in the order (py, px, c), unbiased variance, (var + 1e-6) ** 0.5, the masked or plain mean, float64 autograd."""
    reps = []
    for key in pt.rec_cases():
        if key[:5] == tuple(shape) and len(key) == 8:
            c = pt.rec_case(*key)
            reps.append(pt.check_rec(c, _hip_rec(c)))
            reps.append(pt.check_rec(c, _ops_rec(c), pt.UPSTREAM))
    assert len(reps) == 24
    _run(reps, "rec loss %dx%dx%dx%d/%d" % shape)


def test_rec_loss_constant_and_low_variance_patch():
    """norm_pix with a constant target patch (variance 0: the normalised target is exactly 0, the row loss mean(pred^2)) and a patch
    of variance 1e-6, where 1 / sqrt(var + 1e-6) and 1 / (sqrt(var) + 1e-6) differ by 40 %."""
    c = pt.rec_case(*pt.rec_cases()[-1])
    assert len(pt.rec_cases()[-1]) == 9
    got = _hip_rec(c)
    _run([pt.check_rec(c, got), pt.check_rec(c, _ops_rec(c), pt.UPSTREAM)], "rec loss, special patches")


def test_rec_loss_second_backward_is_refused():
    """RecLossFn scales its saved gradient in place by the upstream scalar; a second backward through the same forward used to return
    g * g' * dpred without a word. It is refused now, and the first pass's gradient stays what it was."""
    from eventpretrain_amd import ops
    from eventpretrain_amd._lib import EvpError
    c = pt.rec_case(2, 3, 8, 12, 4, 1, "half", "random")
    cp = c["pred"].cuda().requires_grad_(True)
    loss = ops.RecLossFn.apply(cp, c["target"].cuda(), c["mask"].cuda(), c["p"], True)
    (g1,) = torch.autograd.grad(loss * pt.UPSTREAM, cp, retain_graph=True)
    with pytest.raises(EvpError):
        torch.autograd.grad(loss * pt.UPSTREAM, cp)
    torch.cuda.synchronize()
    _run([pt.check_rec(c, dict(loss=loss.detach().cpu(), dpred=g1.cpu()), pt.UPSTREAM)], "rec loss, first of two backward passes")
    # a fresh forward gives the same gradient again
    assert torch.equal(_ops_rec(c)["dpred"], g1.cpu())


# ---------------------------------------------------------------------------------------------------------------- unshuffle, gathers
def _hip_unshuffle(c, null_form=False):
    call, dt, ptr, stream_ptr = _api()
    B, L, n_keep, D = c["B"], c["L"], c["n_keep"], c["D"]
    emb, mt, pos, ids, g = (_dev(c[k]) for k in ("emb", "mask_token", "pos", "ids", "g"))
    out, demb = Canary((B, L, D)), Canary((B, n_keep, D))
    call("evp_unshuffle_fwd", ptr(emb), ptr(mt), ptr(pos), ptr(ids), B, n_keep, L, D, ptr(out.t), stream_ptr())
    if null_form:
        call("evp_unshuffle_bwd", ptr(g), ptr(ids), B, n_keep, L, D, ptr(demb.t), None, None, stream_ptr())
        torch.cuda.synchronize()
        return dict(out=out.take("out"), demb=demb.take("demb"))
    dmt, ws = _seven(D), Canary(pt.unsh_slabs(B, L) * D)
    call("evp_unshuffle_bwd", ptr(g), ptr(ids), B, n_keep, L, D, ptr(demb.t), ptr(dmt.t), ptr(ws.t), stream_ptr())
    torch.cuda.synchronize()
    ws.take("workspace")
    return dict(out=out.take("out"), demb=demb.take("demb"), dmask_token=dmt.take("dmask_token"))


def _ops_unshuffle(c):
    from eventpretrain_amd import ops
    B, L, D = c["B"], c["L"], c["D"]
    ce, cm = c["emb"].cuda().requires_grad_(True), c["mask_token"].view(1, 1, D).cuda().requires_grad_(True)
    o = ops.UnshuffleFn.apply(ce, cm, c["pos"].view(1, L, D).cuda(), c["ids"].cuda())
    o.backward(c["g"].cuda())
    assert cm.grad.shape == (1, 1, D)
    return dict(out=o.detach().cpu(), demb=ce.grad.cpu(), dmask_token=cm.grad.view(D).cpu())


@pytest.mark.parametrize("shape", pt.UNSH_SHAPES, ids=lambda s: "B%d_L%d_keep%d_D%d" % s)
def test_unshuffle_against_float64(shape):
    """evp_unshuffle_fwd / _bwd and UnshuffleFn, ids_restore a random permutation per sample: the forward and demb exact, dmask_token
    (slabs of 64 rows, then sum_partials' 16 fold groups over 64-column blocks) equal with integers, f32 class with random values,
    exactly 0 where n_keep = L."""
    reps = []
    for kind in ("int", "random"):
        c = pt.unsh_case(*shape, kind)
        reps.append(pt.check_unsh(c, _hip_unshuffle(c)))
        reps.append(pt.check_unsh(c, _ops_unshuffle(c)))
    _run(reps, "unshuffle B%d L%d keep%d D%d" % shape)


def test_unshuffle_bwd_without_mask_token_gradient():
    """dmask_token = NULL, workspace = NULL: the scatter alone."""
    c = pt.unsh_case(*pt.UNSH_NULL_SHAPE)
    _run([pt.check_unsh(c, _hip_unshuffle(c, null_form=True))], "unshuffle, dmask_token NULL")


@pytest.mark.parametrize("key", pt.GATHER_CASES, ids=lambda k: "B%d_n%d_L%d_D%d_ids%d" % k)
def test_add_rows_gather_exact(key):
    call, dt, ptr, stream_ptr = _api()
    reps = []
    for kind in ("int", "random"):
        c = pt.gather_case(*key, kind)
        x, table, ids, out = _dev(c["x"]), _dev(c["table"]), _dev(c["ids"]), Canary((c["B"], c["n"], c["D"]))
        call("evp_add_rows_gather_f32", ptr(x), ptr(table), ptr(ids), c["B"], c["n"], c["L"], c["D"], ptr(out.t), stream_ptr())
        torch.cuda.synchronize()
        rep = pt.Report("add_rows_gather " + kind)
        rep.exact("out", out.take("out"), c["T"])
        reps.append(rep)
    _run(reps, "add_rows_gather B%d n%d L%d D%d ids%d" % key)


@pytest.mark.parametrize("key", pt.PATCHIFY_CASES, ids=lambda k: "%dx%dx%dx%d_p%d_keep%d_ids%d" % k)
def test_patchify_exact(key):
    """evp_patchify of tokens.hip, float32 and bf16 output: cols[(b, j), c p p + py p + px] of token ids_keep[b, j] (or j)."""
    call, dt, ptr, stream_ptr = _api()
    c = pt.patchify_case(*key)
    rep = pt.Report("patchify")
    x, ids = _dev(c["x"]), _dev(c["ids"])
    for dtype in (torch.float32, torch.bfloat16):
        cols = Canary(tuple(c["T"].shape), dtype)
        call("evp_patchify", ptr(x), ptr(ids), c["B"], c["C"], c["H"], c["W"], c["p"], c["n_keep"], ptr(cols.t),
             dt(cols.t), stream_ptr())
        torch.cuda.synchronize()
        rep.exact(str(dtype), cols.take("cols"), c["T"].to(dtype).float())
    _run([rep], "patchify")


# ---------------------------------------------------------------------------------------------------------------- density, masks
@pytest.mark.parametrize("shape", pt.DENS_SHAPES, ids=lambda s: "%dx%dx%dx%d_p%d" % s)
def test_density_noise_against_float64(shape):
    """evp_density_noise and ops.density_noise, both signs: with integers equal to the exact integer sum divided once in float32,
    with random values at the f32 class."""
    from eventpretrain_amd import ops
    call, dt, ptr, stream_ptr = _api()
    reps = []
    for sign in (1, -1):
        for kind in ("int", "random"):
            c = pt.density_case(*shape, sign, kind)
            B, C, H, W, p = shape
            x = _dev(c["x"])
            out = Canary((B, (H // p) * (W // p)))
            call("evp_density_noise", ptr(x), B, C, H, W, p, float(sign), ptr(out.t), stream_ptr())
            torch.cuda.synchronize()
            reps.append(pt.check_density(c, out.take("noise")))
            reps.append(pt.check_density(c, ops.density_noise(x, p, float(sign)).cpu()))
    _run(reps, "density noise %dx%dx%dx%d/%d" % shape)


@pytest.mark.parametrize("c", pt.mask_cases(), ids=lambda c: "B%d_L%d_keep%d" % (c["B"], c["L"], c["len_keep"]))
def test_mask_from_noise_missing_edges(c):
    """L = 257 and 4096 (the largest the entry takes), len_keep = 0 with ids_keep = NULL, len_keep = L, and rows of +-0, +-Inf and NaN,
    against torch.argsort(stable=True): all three outputs equal."""
    from eventpretrain_amd import ops
    call, dt, ptr, stream_ptr = _api()
    B, L, keep = c["B"], c["L"], c["len_keep"]
    noise = _dev(c["noise"])
    ids_keep = Canary((B, keep), torch.int64, init=torch.full((B, keep), -3), fill=-7) if keep else None
    mask = Canary((B, L))
    restore = Canary((B, L), torch.int64, init=torch.full((B, L), -3), fill=-7)
    call("evp_mask_from_noise", ptr(noise), B, L, keep, ptr(ids_keep.t) if keep else None, ptr(mask.t), ptr(restore.t), stream_ptr())
    torch.cuda.synchronize()
    got = dict(mask=mask.take("mask"), ids_restore=restore.take("ids_restore"))
    if keep:
        got["ids_keep"] = ids_keep.take("ids_keep")
    reps = [pt.check_mask(c, got)]
    ratio = 1.0 - keep / L
    if int(L * (1 - ratio)) == keep:
        k, m, r = ops.mask_from_noise(noise, ratio)
        reps.append(pt.check_mask(c, dict(ids_keep=k.cpu(), mask=m.cpu(), ids_restore=r.cpu())))
    _run(reps, "mask B%d L%d keep%d" % (B, L, keep))


# ---------------------------------------------------------------------------------------------------------------- AdamW
def _fused(c):
    """-> (optimizer, parameters, the parameter without a gradient, {tensor: bf16 shadow})."""
    from eventpretrain_amd import ops
    from eventpretrain_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(p.clone().cuda()) for p in c["p0"]]
    frozen = torch.nn.Parameter(c["frozen"].clone().cuda())
    last = len(c["groups"]) - 1
    groups = [dict(params=[p for i, p in enumerate(ps) if c["group_of"][i] == gi] + ([frozen] if gi == last else []), **g)
              for gi, g in enumerate(c["groups"])]
    opt = FusedAdamW(groups, betas=pt.ADAM_BETAS, eps=pt.ADAM_EPS, grad_scale=c["grad_scale"])
    ops.set_compute_dtype(torch.bfloat16)
    try:
        sh = {i: ops.lp_weight(ps[i]) for i in c["shadows"]}
    finally:
        ops.set_compute_dtype(torch.float32)
    return opt, ps, frozen, sh


def _set_step(opt, ps, c, k):
    for gi, grp in enumerate(opt.param_groups):
        grp["lr"] = c["steps"][k][1][gi]
    for p, g in zip(ps, c["grads"][k]):
        p.grad = g.cuda()


def _state(opt, ps, sh):
    torch.cuda.synchronize()
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu(), sh[i].cpu() if i in sh else None)
            for i, p in enumerate(ps)]


def _adam_report(reps, what):
    worst = {}
    for rep in reps:
        for n, w in pt.worst_by_kind(rep).items():
            worst[n] = max(worst.get(n, 0.0), w)
    print(f"\n[{what}] worst error / bound: " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    fails = [f for rep in reps for f in rep.fails]
    assert not fails, "\n".join(fails)


def test_fused_adamw_against_float64():
    """FusedAdamW over tensors of 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3 and 2 CHUNK + 2 elements in two groups (wd 0.05
    at lr 0.1, wd 0 at lr 0.03), betas (0.9, 0.95), grad_scale 0.5, bf16 shadows on 5, CHUNK + 1 and CHUNK + 3, three steps with a
    changing lr, then load_state_dict with step = 100000 and one more step. After every step the parameters and exp_avg sit at the
    f32 class of torch.optim.AdamW in float64 (at |p| <= 1 and lr 0.1: 1e-4 of an update), exp_avg_sq within 2e-6 relative, each
    shadow equals its parameter in bf16, and the parameter without a gradient is untouched bit for bit and has no state."""
    c = pt.adam_case()
    opt, ps, frozen, sh = _fused(c)
    reps = []
    for k, (step, _) in enumerate(c["steps"]):
        if step == pt.ADAM_RESUME_STEP + 1:
            sd = opt.state_dict()
            for st in sd["state"].values():
                st["step"] = torch.tensor(float(pt.ADAM_RESUME_STEP))
            opt.load_state_dict(sd)
        _set_step(opt, ps, c, k)
        opt.step()
        assert opt._step == step
        reps.append(pt.check_adam(c, k, _state(opt, ps, sh)))
        assert torch.equal(frozen.detach().cpu(), c["frozen"]) and "exp_avg" not in opt.state.get(frozen, {})
    _adam_report(reps, "FusedAdamW")


def test_fused_adamw_parts_equal_one_launch():
    """The same two steps through build_parts / launch_part over three parts and through launch(): parameters, both moments and the
    shadows bit-identical."""
    c = pt.adam_case()
    a, pa, _, sha = _fused(c)
    b, pb, _, shb = _fused(c)
    for k in range(2):
        _set_step(a, pa, c, k)
        _set_step(b, pb, c, k)
        a.step()
        with torch.no_grad():
            assert b.refresh()
            assert b.build_parts([pb[0:3], pb[3:6]]) == 3
            for i in range(3):
                b.launch_part(i)
        for i, (x, y) in enumerate(zip(_state(a, pa, sha), _state(b, pb, shb))):
            for name, u, v in zip(("p", "exp_avg", "exp_avg_sq", "shadow"), x, y):
                assert (u is None and v is None) or torch.equal(u, v), (k, c["numel"][i], name)
    _adam_report([pt.check_adam(c, 1, _state(b, pb, shb), what="launch_part")], "launch_part")


def test_fused_adamw_recipe_lr_gates_the_moments():
    """The recipe's lr = 1e-3 (wd 0.05, grad_scale 1), five steps: at this lr the parameter gate resolves an update only to 1e-2, so
    the moments carry the check."""
    c = pt.adam_case(True)
    opt, ps, _, sh = _fused(c)
    reps = []
    for k in range(len(c["steps"])):
        _set_step(opt, ps, c, k)
        opt.step()
        reps.append(pt.check_adam(c, k, _state(opt, ps, sh)))
    _adam_report(reps, "FusedAdamW lr 1e-3")


def test_adamw_c_abi_without_device_hyper():
    """evp_adamw_multi with dev_hyper = NULL (the entry computes the bias corrections from `step`), the same tensors, gradients and
    steps, step 100001 given directly; parameters, moments and shadows inside NaN-slacked buffers."""
    call, dt, ptr, stream_ptr = _api()
    c = pt.adam_case()
    n = len(c["numel"])
    P = [Canary(x, init=p) for x, p in zip(c["numel"], c["p0"])]
    M = [Canary(x, init=torch.zeros(x)) for x in c["numel"]]
    V = [Canary(x, init=torch.zeros(x)) for x in c["numel"]]
    LP = {i: Canary(c["numel"][i], torch.bfloat16, init=c["p0"][i].bfloat16()) for i in c["shadows"]}
    table = lambda v, dtype=torch.int64: torch.tensor(v, dtype=dtype, device="cuda")        # noqa: E731
    chunk_t = [i for i, x in enumerate(c["numel"]) for _ in range(0, x, pt.CHUNK)]
    chunk_o = [o for x in c["numel"] for o in range(0, x, pt.CHUNK)]
    tabs = dict(p=table([x.t.data_ptr() for x in P]), m=table([x.t.data_ptr() for x in M]), v=table([x.t.data_ptr() for x in V]),
                lp=table([LP[i].t.data_ptr() if i in LP else 0 for i in range(n)]), numel=table(list(c["numel"])),
                wd=table([c["groups"][g]["weight_decay"] for g in c["group_of"]], torch.float32),
                ct=table(chunk_t, torch.int32), co=table(chunk_o))
    reps = []
    for k, (step, lrs) in enumerate(c["steps"]):
        grads = [g.cuda() for g in c["grads"][k]]
        tg, tl = table([g.data_ptr() for g in grads]), table([lrs[g] for g in c["group_of"]], torch.float32)
        call("evp_adamw_multi", ptr(tabs["p"]), ptr(tg), ptr(tabs["m"]), ptr(tabs["v"]), ptr(tabs["lp"]), ptr(tabs["numel"]), ptr(tabs["wd"]),
             ptr(tl), ptr(tabs["ct"]), ptr(tabs["co"]), len(chunk_t), pt.CHUNK, 1.0, pt.ADAM_BETAS[0], pt.ADAM_BETAS[1], pt.ADAM_EPS, step,
             c["grad_scale"], None, stream_ptr())
        torch.cuda.synchronize()
        got = [(P[i].take("p"), M[i].take("exp_avg"), V[i].take("exp_avg_sq"), LP[i].take("shadow").bfloat16() if i in LP else None)
               for i in range(n)]
        reps.append(pt.check_adam(c, k, got, what="evp_adamw_multi"))
    _adam_report(reps, "evp_adamw_multi, dev_hyper NULL")


# ---------------------------------------------------------------------------------------------------------------- element-wise
@pytest.mark.parametrize("n", pt.EW_SIZES)
def test_add_and_scale_exact(n):
    """evp_add_f32 with and without `c` (and ops.add) and evp_scale_f32: no vector body (n < 4), no tail, a tail, and 2048 x 1024 + 5
    elements, past ew_grid's cap of 2048 blocks. One rounding per sum or product: equal to the rounded float64 truth; a + b + c equal
    to (a + b) + c in float32."""
    from eventpretrain_amd import ops
    call, dt, ptr, stream_ptr = _api()
    reps = []
    for kind in ("int", "random"):
        c = pt.ew_case(n, kind)
        a, b, cc = _dev(c["a"]), _dev(c["b"]), _dev(c["c"])
        o2, o3, sc = Canary(n), Canary(n), Canary(n, init=c["a"])
        s = torch.tensor([pt.SCALE], dtype=torch.float32, device="cuda")
        call("evp_add_f32", ptr(a), ptr(b), None, n, ptr(o2.t), stream_ptr())
        call("evp_add_f32", ptr(a), ptr(b), ptr(cc), n, ptr(o3.t), stream_ptr())
        call("evp_scale_f32", ptr(sc.t), ptr(s), n, stream_ptr())
        torch.cuda.synchronize()
        reps.append(pt.check_ew(c, dict(add2=o2.take("a + b"), add3=o3.take("a + b + c"), scale=sc.take("scale"))))
        reps.append(pt.check_ew(c, dict(add2=ops.add(a, b).cpu(), add3=ops.add(a, b, cc).cpu())))
    _run(reps, f"add / scale n = {n}")


@pytest.mark.parametrize("n", pt.CAST_SIZES)
def test_cast_specials_and_rounding(n):
    """evp_cast and ops.cast both ways: NaN (compared as NaN, not by payload), +-Inf, -0, the ties 1 + 2^-8 (down to even) and
    1 + 3 * 2^-8 (up to even), 3.4e38 (rounds to Inf), in the vector body and in the scalar tail; equal to tensor.bfloat16() on the CPU."""
    from eventpretrain_amd import ops
    call, dt, ptr, stream_ptr = _api()
    c = pt.cast_case(n)
    x, xb = _dev(c["x"]), _dev(c["T"])
    down, up = _seven(n, torch.bfloat16), _seven(n)
    call("evp_cast", ptr(x), dt(x), ptr(down.t), dt(down.t), n, stream_ptr())
    call("evp_cast", ptr(xb), dt(xb), ptr(up.t), dt(up.t), n, stream_ptr())
    torch.cuda.synchronize()
    rep = pt.Report(f"cast n = {n}")
    pt.bits_equal(rep, "f32 -> bf16", down.t.cpu(), c["T"])
    pt.bits_equal(rep, "bf16 -> f32", up.t.cpu(), c["T"].float())
    down.take("f32 -> bf16", written=False)
    up.take("bf16 -> f32", written=False)
    pt.bits_equal(rep, "ops.cast f32 -> bf16", ops.cast(x, torch.bfloat16).cpu(), c["T"])
    pt.bits_equal(rep, "ops.cast bf16 -> f32", ops.cast(xb, torch.float32).cpu(), c["T"].float())
    _run([rep], f"cast n = {n}")


@pytest.mark.parametrize("shape", pt.TRANSPOSE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_transpose_exact(shape):
    call, dt, ptr, stream_ptr = _api()
    R, C = shape
    rep = pt.Report("transpose %dx%d" % shape)
    for dtype in (torch.float32, torch.bfloat16):
        m = pt.transpose_case(R, C).to(dtype)
        src, out = _dev(m), Canary((C, R), dtype)
        call("evp_transpose", ptr(src), ptr(out.t), dt(m), R, C, stream_ptr())
        torch.cuda.synchronize()
        rep.exact(str(dtype), out.take("out"), m.t().contiguous().float())
    _run([rep], "transpose %dx%d" % shape)

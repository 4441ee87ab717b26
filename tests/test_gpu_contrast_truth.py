"""The contrastive stage against float64 truth (tests/contrast_truth.py): part 1 -- BatchNorm, row normalisation, row dot / scale,
InfoNCE against a queue, cross entropy, the enqueue and the token mean, each through the C ABI at the shapes where its paths part,
every output inside a NaN- or sentinel-filled buffer whose slack must stay untouched; part 2 -- the two MoCo-v3 heads, the loss, the
enqueue and the backward as PrHubModel orders them, in f32 and bf16 mode, tensor by tensor. The host half
(tests/test_contrast_truth_host.py) shows what the gates accept and reject.

Each test prints its worst error over the bound per tensor; the docstrings record the figures of an MI355X run."""
import contextlib
import copy

import pytest
import torch

import contrast_truth as ct

pytestmark = pytest.mark.gpu

PAD = 64                 # elements of slack on either side: keeps the 16-byte alignment the vector forms ask for
SENTINEL = -7.25         # slack of buffers whose own content is data (the queue); the int64 pointer's slack holds -7


class Canary:
    """n elements inside a buffer of n + 2 * PAD, all NaN (or `init` inside, `fill` outside). take() asserts that the slack is as it
    was and, unless told otherwise, that no element inside kept its NaN."""

    def __init__(self, shape, dtype=torch.float32, init=None, fill=float("nan")):
        self.shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.fill = fill
        self.buf = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device="cuda")
        if init is not None:
            self.buf[PAD:PAD + self.n] = init.reshape(-1).to(dtype).cuda()
        self.t = self.buf[PAD:PAD + self.n].view(self.shape)
        assert self.t.data_ptr() % 16 == 0

    def take(self, name="", written=True):
        slack = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]]).cpu()
        same = torch.isnan(slack) if self.fill != self.fill else slack == self.fill
        assert bool(same.all()), f"{name}: wrote outside its output"
        out = self.t.cpu()
        if written and out.is_floating_point():
            assert not bool(torch.isnan(out).any()), f"{name}: left {int(torch.isnan(out).sum())} elements of its output unwritten"
        return out.float() if out.is_floating_point() else out


def _api():
    from eventpretrain_amd._lib import call, dt, ptr, stream_ptr
    return call, dt, ptr, stream_ptr


def _dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).cuda().contiguous()


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def _hip_bn(c):
    call, dt, ptr, stream_ptr = _api()
    R, C = c["R"], c["C"]
    io = torch.bfloat16 if c["io"] == "bf16" else torch.float32
    x, dy, gamma, beta = _dev(c["x"], io), _dev(c["dy"], io), _dev(c["gamma"]), _dev(c["beta"])
    assert x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
    y, dx = Canary((R, C), io), Canary((R, C), io)
    mean, invstd = Canary(C), Canary(C)
    rm = Canary(C, init=c["rm0"]) if c["running"] else None
    rv = Canary(C, init=c["rv0"]) if c["running"] else None
    dgamma, dbeta = (Canary(C), Canary(C)) if c["affine"] else (None, None)
    nb = call("evp_batchnorm_nblk", R)
    assert nb == (R + 63) // 64
    ws1, ws2 = Canary((2 * nb + 2) * C), Canary((2 * nb + 2) * C)
    t = lambda cn: None if cn is None else cn.t       # noqa: E731
    call("evp_batchnorm_fwd", ptr(x), dt(x), R, C, ptr(gamma), ptr(beta), ct.EPS, ct.MOMENTUM, int(c["relu"]), ptr(y.t), ptr(mean.t),
         ptr(invstd.t), ptr(t(rm)), ptr(t(rv)), ptr(ws1.t), stream_ptr())
    call("evp_batchnorm_bwd", ptr(dy), ptr(x), ptr(y.t), dt(x), R, C, ptr(gamma), ptr(mean.t), ptr(invstd.t), int(c["relu"]), ptr(dx.t),
         ptr(t(dgamma)), ptr(t(dbeta)), ptr(ws2.t), stream_ptr())
    torch.cuda.synchronize()
    ws1.take("fwd workspace", written=False)
    ws2.take("bwd workspace", written=False)
    got = dict(y=y.take("y"), mean=mean.take("mean"), invstd=invstd.take("invstd"), dx=dx.take("dx"))
    if c["running"]:
        got.update(running_mean=rm.take("running_mean"), running_var=rv.take("running_var"))
    if c["affine"]:
        got.update(dgamma=dgamma.take("dgamma"), dbeta=dbeta.take("dbeta"))
    return got


def _run(reports, what):
    worst = {}
    for rep in reports:
        for n, g, w in rep.rows:
            worst[n] = max(worst.get(n, 0.0), w)
    print(f"\n[{what}] worst error / bound: " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    fails = [f for rep in reports for f in rep.fails]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", ct.BN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm_f32_against_float64(shape):
    """evp_batchnorm_fwd / _bwd with f32 I/O: y, mean, invstd, both running statistics (momentum 0.1 from non-trivial starts, unbiased
    variance), dx, dgamma, dbeta against autograd of the oracle formula in float64; relu 0 / 1 x affine given / null x running
    statistics given / null (the two grid-stride shapes: two of the eight). Columns of standard deviation 0.05 to 2, one negative
    gain; with ReLU, dy is 0 where truth's pre-activation is within 1e-4 of 0, and in one configuration wherever y == 0.
    Bound: |got - T| <= 1e-5 * max(1, max|T|). Measured on an MI355X, worst error over the bound: dx 0.53 at 2 x 4 (a column's
    variance from two samples) and 0.016 elsewhere, mean 0.035 and dgamma 0.031 (135 x 261), y 0.024, dbeta 0.025, invstd 0.016,
    running statistics 0.010; the two grid-stride shapes 0.018 at most."""
    reps = []
    for key in ct.bn_cases("f32"):
        if key[:2] == tuple(shape):
            c = ct.bn_case(*key)
            reps.append(ct.check_bn(c, _hip_bn(c)))
    assert reps
    _run(reps, f"batchnorm f32 {shape[0]}x{shape[1]}")


@pytest.mark.parametrize("shape", [s for s in ct.BN_SHAPES if s not in ct.BN_GRID_STRIDE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm_bf16_io_against_float64(shape):
    """The same with bf16 x, dy, y, dx: truth in float64 from the ROUNDED inputs; mean, invstd, running statistics, dgamma, dbeta at the
    f32 class; y and dx carry one round-to-nearest store, |got - T| <= 2^-8 |T| + 1e-5 max|T| (2^-8 is bf16's unit roundoff, so a
    correct store reaches the bound to within the f32 term). The backward reads the forward's own bf16 y for the ReLU mask, as
    training does. Measured on an MI355X, worst error over the bound: y 0.991, dx 0.989 (the store's own half ulp), dgamma 0.046,
    mean 0.025, invstd 0.017, running statistics 0.011."""
    reps = []
    for key in ct.bn_cases("bf16"):
        if key[:2] == tuple(shape):
            c = ct.bn_case(*key)
            reps.append(ct.check_bn(c, _hip_bn(c)))
    assert reps
    _run(reps, f"batchnorm bf16 {shape[0]}x{shape[1]}")


def test_batchnorm_offset_columns_keep_the_f32_class():
    """Columns of mean 30 and unit variance, 1091 x 12 (18 slabs): Welford errs by about u * kappa ~ 2e-6 on the variance, a sum of
    squares by u * kappa^2 ~ 5e-5 (the host test shows that form failing this very gate at 6.5 x the bound). Offset 30, not lowered:
    torch-CPU float32 batch_norm reads 0.10 x the bound (y; 0.007 on invstd), the kernel on an MI355X 0.044 (dgamma; y 0.028,
    invstd 0.011, running_var 0.007)."""
    R, C = ct.BN_OFFSET_SHAPE
    c = ct.bn_case(R, C, 0, True, True, "f32", ct.BN_OFFSET)
    _run([ct.check_bn(c, _hip_bn(c))], f"batchnorm offset {ct.BN_OFFSET:g}")


# ---------------------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("shape", ct.SCALE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_kernels_against_float64(shape):
    """evp_l2norm_rows_fwd / _bwd (one all-zero row: the norm clamps at 1e-12 and its dx = dy / 1e-12 is compared relative to its own
    size), evp_rowdot_f32, evp_scale_rows_f32 with and without `add`; 16390 x 8 runs past rows_grid's 4096 blocks of 4 rows, 4100 x 257
    (scale only) past 4096 x 256 elements. Bound: the f32 class. Measured on an MI355X, worst error over the bound: rowdot 0.016
    (7 x 64), y 0.012 and dx 0.009 (16390 x 8), the zero row's dx 0.006, scale 0.005, scale + add 0.007."""
    call, dt, ptr, stream_ptr = _api()
    c = ct.row_case(*shape)
    R, C = c["R"], c["C"]
    x, dy, b, add, s = (_dev(c[k]) for k in ("x", "dy", "b", "add", "s"))
    got = {}
    sc, sca = Canary((R, C)), Canary((R, C))
    call("evp_scale_rows_f32", ptr(x), ptr(s), None, R, C, ptr(sc.t), stream_ptr())
    call("evp_scale_rows_f32", ptr(x), ptr(s), ptr(add), R, C, ptr(sca.t), stream_ptr())
    if tuple(shape) in ct.ROW_SHAPES:
        y, nrm, dx, rd = Canary((R, C)), Canary(R), Canary((R, C)), Canary(R)
        call("evp_l2norm_rows_fwd", ptr(x), R, C, ptr(y.t), ptr(nrm.t), stream_ptr())
        call("evp_l2norm_rows_bwd", ptr(dy), ptr(y.t), ptr(nrm.t), R, C, ptr(dx.t), stream_ptr())
        call("evp_rowdot_f32", ptr(x), ptr(b), R, C, ptr(rd.t), stream_ptr())
        torch.cuda.synchronize()
        got.update(y=y.take("y"), norm=nrm.take("norm"), dx=dx.take("dx"), rowdot=rd.take("rowdot"))
    torch.cuda.synchronize()
    got.update(scale=sc.take("scale"), scale_add=sca.take("scale_add"))
    _run([ct.check_rows(c, got)], f"rows {R}x{C}")


# ---------------------------------------------------------------------------------------------------------------- loss kernels
@pytest.mark.parametrize("shape", ct.NCE_SHAPES, ids=lambda s: "R%d_K%d_ld%d" % s)
def test_infonce_queue_against_float64(shape):
    """evp_infonce_queue at 1 / T = 1 / 0.07: the loss (1e-5 relative), the row losses in the workspace (f32 class), dpos and dneg
    (rtol 1e-4, atol 1e-7), columns [K, ldn) of dneg exactly 0 while those of neg hold NaN (never read); K below, at and above the
    256-thread stride, K = 65536, 1500 rows through mean_kernel; a row whose positive is the maximum and one where a negative is.
    With dpos / dneg null only the loss and the row losses are written. Measured on an MI355X, worst error over the bound: loss
    0.012, row losses 0.012, dpos 0.007, dneg 0.008; K = 65536: loss 0.010."""
    call, dt, ptr, stream_ptr = _api()
    c = ct.nce_case(*shape)
    R, K, ldn = shape
    pos, neg = _dev(c["pos"]), _dev(c["neg"])
    reps = []
    for grads in (True, False):
        loss, ws = Canary(1), Canary(R)
        dpos, dneg = (Canary(R), Canary((R, ldn))) if grads else (None, None)
        call("evp_infonce_queue", ptr(pos), ptr(neg), R, K, ldn, ct.INV_T, ptr(loss.t), ptr(dpos.t) if grads else None,
             ptr(dneg.t) if grads else None, ptr(ws.t), stream_ptr())
        torch.cuda.synchronize()
        got = dict(loss=loss.take("loss").view(()), row_loss=ws.take("row losses"))
        if grads:
            got.update(dpos=dpos.take("dpos"), dneg=dneg.take("dneg"))
        reps.append(ct.check_nce(c, got))
    _run(reps, "infonce R%d K%d ld%d" % shape)


@pytest.mark.parametrize("shape", ct.CE_SHAPES, ids=lambda s: "R%d_n%d_ld%d" % s)
def test_cross_entropy_padded_against_float64(shape):
    """evp_cross_entropy (smoothing 0) and evp_cross_entropy_smooth (0 and 0.1) with ld >= n_cls: logits of magnitude 1 / 0.07, padding
    columns of the logits NaN (never read), those of dlogits exactly 0, a label 0 and a label n_cls - 1, 1500 rows through mean_kernel.
    Truth: F.cross_entropy and the oracle's label_smoothing_ce in float64. Measured on an MI355X, worst error over the bound: loss
    0.021 and row losses 0.013 (1500 rows), dlogits 0.038 (6 x 10)."""
    call, dt, ptr, stream_ptr = _api()
    R, n_cls, ld = shape
    reps = []
    for entry, s in (("evp_cross_entropy", 0.0), ("evp_cross_entropy_smooth", 0.0), ("evp_cross_entropy_smooth", 0.1)):
        c = ct.ce_case(R, n_cls, ld, s)
        logits, labels = _dev(c["logits"]), _dev(c["labels"])
        loss, ws, dl = Canary(1), Canary(R), Canary((R, ld))
        args = (ptr(logits), ptr(labels), R, n_cls, ld) + ((float(s),) if entry.endswith("smooth") else ())
        call(entry, *args, ptr(loss.t), ptr(dl.t), ptr(ws.t), stream_ptr())
        torch.cuda.synchronize()
        reps.append(ct.check_ce(c, dict(loss=loss.take("loss").view(()), row_loss=ws.take("row losses"), dlogits=dl.take("dlogits"))))
    _run(reps, "cross entropy R%d n%d ld%d" % shape)


# ---------------------------------------------------------------------------------------------------------------- enqueue, token mean
def _hip_enqueue(c, start, host):
    """-> (queue after, pointer after or None). The queue is a view into a sentinel-filled buffer, and so is the pointer."""
    call, dt, ptr, stream_ptr = _api()
    B, L, C, K = c["B"], c["L"], c["C"], c["K"]
    q = Canary((C, L, K), init=c["queue"], fill=SENTINEL)
    keys = _dev(c["keys"])
    if host:
        call("evp_enqueue_keys", ptr(q.t), ptr(keys), int(start), B, L, C, K, stream_ptr())
        torch.cuda.synchronize()
        return q.take("queue"), None
    p = Canary(1, dtype=torch.int64, init=torch.tensor([start]), fill=-7)
    call("evp_enqueue_keys_dev", ptr(q.t), ptr(keys), ptr(p.t), B, L, C, K, stream_ptr())
    torch.cuda.synchronize()
    return q.take("queue"), int(p.take("pointer"))


@pytest.mark.parametrize("shape", ct.ENQ_SHAPES, ids=lambda s: "B%d_L%d_C%d_K%d" % s)
def test_enqueue_keys_dev_bit_exact(shape):
    """evp_enqueue_keys_dev equals the oracle's enqueue bit for bit, untouched slots and the advanced pointer included, from start
    positions 0, a middle slot and the last slot (the pointer wraps to 0): ragged 64 x 64 tiles (B = 5, 70; C = 64, 66), one element,
    and L = 65536, which takes the element-wise kernel. A start position of K - B + 1 or -1 (both kernels return on a pointer outside
    [0, K - B], contrast.hip) leaves the queue and the slack around it bit-identical."""
    c = ct.enq_case(*shape)
    reps = []
    for start in ct.enq_starts(c["B"], c["K"]):
        q, p = _hip_enqueue(c, start, host=False)
        reps.append(ct.check_enqueue(c, start, q, p))
    for bad in (c["K"] - c["B"] + 1, -1):
        q, _ = _hip_enqueue(c, bad, host=False)
        assert torch.equal(q, c["queue"]), f"start {bad}: the queue changed"
    _run(reps, "enqueue (device pointer) B%d L%d C%d K%d" % shape)


@pytest.mark.parametrize("shape", ct.ENQ_HOST_SHAPES, ids=lambda s: "B%d_L%d_C%d_K%d" % s)
def test_enqueue_keys_host_pointer_bit_exact(shape):
    """evp_enqueue_keys (the write position as an argument) at the same start positions."""
    c = ct.enq_case(*shape)
    for start in ct.enq_starts(c["B"], c["K"]):
        q, _ = _hip_enqueue(c, start, host=True)
        want, _ = ct.mo.enqueue(c["queue"], start, c["keys"])
        assert torch.equal(q, want), f"start {start}"


@pytest.mark.parametrize("shape", ct.MEAN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_token_mean_against_float64(shape):
    """evp_token_mean_fwd / _bwd: one column group, 65 groups (D = 260), a second block of groups (D = 1028). Bound: the f32 class.
    Measured on an MI355X, worst error over the bound: out 0.033 (N = 197), dx 0.000."""
    call, dt, ptr, stream_ptr = _api()
    c = ct.mean_case(*shape)
    B, N, D = shape
    out, dx = Canary((B, D)), Canary((B, N, D))
    call("evp_token_mean_fwd", ptr(_dev(c["x"])), B, N, D, ptr(out.t), stream_ptr())
    call("evp_token_mean_bwd", ptr(_dev(c["g"])), B, N, D, ptr(dx.t), stream_ptr())
    torch.cuda.synchronize()
    _run([ct.check_mean(c, dict(out=out.take("out"), dx=dx.take("dx")))], "token mean %dx%dx%d" % shape)


# ---------------------------------------------------------------------------------------------------------------- part 2
@contextlib.contextmanager
def _compute(dtype):
    from eventpretrain_amd import ops
    ops.set_compute_dtype(dtype)
    try:
        yield ops
    finally:
        ops.set_compute_dtype(torch.float32)


def _hip_stage(name, mode, T_, dtype):
    """The module tail on the device in the order of PrHubModel: heads, loss, enqueue (which overwrites the live queue), backward.
    -> ({tensor: CPU tensor}, the run's own normalised keys)."""
    from eventpretrain_amd._lib import EvpError
    from eventpretrain_amd.model.sub_module.mlp_head import run_mlp_2d
    c = ct.stage_case(name)
    heads = copy.deepcopy(c["heads"]).cuda().train()
    emb, clip = c["emb_h"].cuda().requires_grad_(True), c["clip_emb"].cuda().requires_grad_(True)
    queue, qptr = c["queue"].cuda().clone(), torch.tensor([c["ptr0"]], dtype=torch.int64, device="cuda")
    with _compute(dtype) as ops:
        h = run_mlp_2d(heads["emb_h_pred"], run_mlp_2d(heads["emb_h_proj"], emb))
        if mode == "queue":
            loss, k = ops.info_nce_queue(h, clip, queue, T_)
        else:
            loss, k = ops.info_nce_inbatch(h, clip, T_), ops.L2NormFn.apply(clip.detach())
        if c["enqueue"]:
            ops.enqueue_keys_dev(queue, k, qptr)
        else:
            with pytest.raises(EvpError):          # K % B != 0: refused on the host, nothing launched
                ops.enqueue_keys_dev(queue, k, qptr)
        (loss * ct.UPSTREAM).backward()
        ops.flush_deferred_grads()
        torch.cuda.synchronize()
    got = {"loss": loss, "act:h": h, "act:d_emb_h": emb.grad, "act:d_clip_emb": clip.grad}
    got.update({"grad:" + n: p.grad for n, p in heads.named_parameters()})
    got.update({"stat:" + n: b for n, b in heads.named_buffers() if n.endswith(("running_mean", "running_var"))})
    if c["enqueue"]:
        got.update(queue=queue, ptr=qptr)
    assert all(v is not None for v in got.values()), [n for n, v in got.items() if v is None]
    return {n: v.detach().cpu() if n == "ptr" else v.detach().float().cpu() for n, v in got.items()}, k.detach().float().cpu()


@pytest.mark.parametrize("name,mode,T_", ct.stage_runs())
def test_contrastive_tail_f32_against_float64_truth(name, mode, T_):
    """f32 mode: loss, the head output h, d emb_h, d clip_emb, every parameter gradient, the ten running statistics, each by its
    relative L2 error against mo.mlp_head x 2 + mo.info_nce_queue / mo.info_nce_inbatch in float64; bound per tensor max(3 x the error
    of the same oracle functions in float32 on the CPU, 1e-5). The queue after the enqueue equals mo.enqueue of the run's own keys bit
    for bit, sits at the f32 class of truth's, and the pointer is truth's. k40, k48 and k320 take the live-queue clone (the enqueue
    has overwritten the queue when the backward reads it), k36 and k35 the padded copy; K = 36 with B = 5 is refused by the enqueue
    (asserted), so k36 checks everything but the queue.
    Measured on an MI355X, worst e_hip / e_F over the tensors of a run: 1.23 to 1.35 in all twenty runs for every tensor but the
    loss; the loss, whose float32-oracle error is one draw of 6e-10 to 2e-7, reads up to 55.8 x it (k35 queue T = 0.07) and stays
    under the 1e-5 floor by a factor of 100."""
    got, keys = _hip_stage(name, mode, T_, torch.float32)
    fails, worst, table = ct.check_stage_f32(name, mode, T_, got, keys)
    print(f"\n[stage f32 {name} {mode} T={T_}] worst e_hip / e_F = {worst[0]:.2f} at {worst[1]} (bound max({ct.FACTOR:g} e_F, 1e-5))\n{table}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,mode,T_", ct.stage_runs())
def test_contrastive_tail_bf16_against_float64_truth(name, mode, T_):
    """bf16 mode, the mode the benchmark trains in: the same tensors through the three gates of block_truth.compare (whole tensor,
    16 x 64 / 128 x 128 sub-blocks, scale) against the same oracle functions under CPU autocast to bf16, FACTOR = 3. At T = 0.07 the
    yardstick's own error on d emb_h and the upstream gradients is 0.07 to 0.13, and it is the same at T = 1.0 (0.065 to 0.14: it
    does not come from the division by 0.07), so there the sub-block and scale gates carry the weight. The queue and the pointer as
    in f32 mode. The loss is measured against the yardstick's loss error pooled over the five cases (contrast_truth.loss_yardstick:
    3.3e-4 / 3.9e-5 for the queue at T = 0.07 / 1.0, 1.2e-3 / 1.1e-4 in-batch); against its own case's single draw (1.4e-6 to
    2.5e-3) the same HIP losses, 3e-5 to 9e-4 off truth, read 0.1 to 64 x.
    Measured on an MI355X, worst e_hip / e_ref over all tensors and gates (bound 3), T = 0.07 / 1.0, queue then in-batch:
    k40 1.12 / 1.23, 1.30 / 1.16; k48 1.51 / 1.38 (loss), 1.01 / 1.08; k36 1.55 / 1.48 (loss), 0.81 / 0.94; k35 0.99 / 1.09,
    0.87 / 0.92; k320 0.98 / 0.97, 1.03 / 0.94 -- d emb_h's 16 x 64 tiles or a weight gradient wherever the loss is not named."""
    got, keys = _hip_stage(name, mode, T_, torch.bfloat16)
    fails, worst, table = ct.check_stage_bf16(name, mode, T_, got, keys)
    print(f"\n[stage bf16 {name} {mode} T={T_}] worst e_hip / e_ref = {worst[0]:.2f} at {worst[1]} (bound {ct.FACTOR:g})\n{table}")
    assert not fails, "\n".join(fails)

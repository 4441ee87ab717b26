"""Shared by the CPU and GPU tests that pin the contrastive stage to float64 truth (tests/test_contrast_truth_host.py,
tests/test_gpu_contrast_truth.py): the cases, their float64 references, the gates, a float32 CPU restatement of every operation in
the kernels' own order, and the single mutations of that restatement which the gates have to reject.

Kernel -> the cases that reach it (part 1 = one kernel through the C ABI, part 2 = the module tail as the model runs it):
  evp_batchnorm_fwd / evp_batchnorm_bwd     BN_SHAPES x BN_CONFIGS in f32 and bf16 I/O, BN_OFFSET; every stage of part 2.
      2 x 4 smallest legal (row lanes 2, 3 of the vector combine empty); 60 x 264 one partial slab, vector form, second column block,
      C % 64 != 0; 135 x 261 scalar form across column 256, last slab of 7 rows; 129 / 130 / 131 x 8 last slab of 1 / 2 / 3 rows in
      the vector form; 1091 x 12 18 slabs > the 16 fold groups of bn_stats_finalize / bn_bwd_finalize; 4100 x 261 and 4100 x 1028
      the grid-stride tails of bn_apply / bn_bwd_apply (4096 x 256 elements, x 4 in the vector form); affine=False and null running
      statistics in BN_CONFIGS.
  evp_l2norm_rows_fwd / _bwd, evp_rowdot_f32   ROW_SHAPES (16390 x 8: rows_grid's cap of 4096 blocks x 4 rows); part 2.
  evp_scale_rows_f32                           ROW_SHAPES + 4100 x 257 (cap of 4096 x 256 elements), with and without `add`; part 2 (queue).
  evp_infonce_queue                            NCE_SHAPES (K below, at and above the 256-thread stride, padding columns, 1500 rows
                                               through mean_kernel); part 2 (queue): K = 36 / 35 padded, K = 40 / 48 / 320 not.
  evp_cross_entropy / _smooth                  CE_SHAPES x smoothing 0 / 0.1 (ld > n_cls with NaN padding); part 2 (in-batch: n_cls 5 or 6, ld 8).
  evp_enqueue_keys_dev / evp_enqueue_keys      ENQ_SHAPES x start positions (ragged 64 x 64 tiles, the element-wise fallback for
                                               L > 65535, the wrap of the pointer, the guard on a pointer outside [0, K - B]); part 2.
  evp_token_mean_fwd / _bwd                    MEAN_SHAPES.
  the live-queue clone of InfoNCEQueueFn       part 2, f32 mode, K % 8 == 0 (K = 40, 48, 320): the enqueue runs before backward.

Gates of part 1 (the project's f32 class, tests/test_gpu_ops.py, tests/test_gpu_finetune.py):
  f32_class   |got - T| <= 1e-5 * max(1, max|T|) elementwise;        rel_class  scalar losses to 1e-5 relative;
  grad_class  |got - T| <= 1e-7 + 1e-4 * |T| (dlogits-type);         bf16_store |got - T| <= 2^-8 * |T| + 1e-5 * max|T| (one RNE store).
Gates of part 2: f32 mode -- per-tensor relative L2 error <= max(FACTOR * that of the oracle's own float32 run, 1e-5); bf16 mode -- the
three gates of block_truth.compare against the oracle under CPU autocast to bf16, FACTOR = 3; the scalar loss alone is measured
against the yardstick's loss error pooled over the cases (loss_yardstick: one draw of a scalar's rounding error has no stable size).
The queue after the enqueue and the pointer are f32 / exact in both modes (the keys are normalised in f32 either way), so they take
the f32 class and equality."""
import contextlib
import functools
import itertools

import torch
import torch.nn.functional as F

import block_truth as bt
from eventpretrain_amd.testing import det_fill_module_
from oracle import model_oracle as mo

FACTOR = bt.FACTOR
F32_TOL, LOSS_RTOL, GRAD_RTOL, GRAD_ATOL, BF16_HALF_ULP_X2 = 1e-5, 1e-5, 1e-4, 1e-7, 2.0 ** -8
EPS, MOMENTUM = 1e-5, 0.1
INV_T = float(torch.tensor(1.0 / 0.07, dtype=torch.float32))      # what the C ABI's float argument holds
L2_EPS = 1e-12
NEAR_ZERO = 1e-4        # |pre-ReLU truth| below this: dy is made 0 there, so that an f32 sign flip of a value that is 0 +- rounding
                        # cannot move dx (a condition on the inputs)

BN_SHAPES = ((2, 4), (60, 264), (135, 261), (129, 8), (130, 8), (131, 8), (1091, 12), (4100, 261), (4100, 1028))
BN_GRID_STRIDE = ((4100, 261), (4100, 1028))
BN_CONFIGS = tuple(itertools.product((0, 1), (True, False), (True, False)))        # relu, affine, running statistics given
BN_CONFIGS_LARGE = ((1, True, True), (0, False, False))    # the grid-stride tails sit in the apply kernels, whose control flow no flag changes
BN_OFFSET_SHAPE, BN_OFFSET = (1091, 12), 30.0
ROW_SHAPES = ((1, 1), (5, 7), (7, 64), (9, 65), (6, 256), (16390, 8))
SCALE_SHAPES = ROW_SHAPES + ((4100, 257),)
NCE_SHAPES = ((1, 1, 1), (5, 40, 40), (5, 255, 256), (3, 256, 256), (4, 257, 264), (3, 65536, 65536), (1500, 8, 8))
CE_SHAPES = ((1, 1, 1), (6, 10, 16), (7, 256, 256), (5, 257, 264), (1500, 12, 16))
ENQ_SHAPES = ((5, 27, 64, 40), (70, 3, 66, 140), (1, 1, 1, 1), (2, 65536, 3, 4))      # B, L, C, K
ENQ_HOST_SHAPES = ENQ_SHAPES[:2]
MEAN_SHAPES = ((1, 1, 4), (3, 197, 260), (2, 50, 1028))
# part 2: B, L, D, MLP, K. K = 36 is no multiple of B = 5, which the enqueue's host check refuses (K % B == 0), so that case runs
# without the enqueue (and asserts the refusal); k35 is the same padded path with the enqueue. The in-batch form has no enqueue in
# the model; here it enqueues its own normalised keys all the same, so that every run checks the queue and the pointer.
STAGE = dict(
    k40=dict(B=5, L=27, D=64, MLP=264, K=40),       # K % 8 == 0: the live-buffer clone in f32; 135 rows = 3 slabs, last of 7
    k48=dict(B=6, L=10, D=64, MLP=264, K=48),       # one partial slab
    k36=dict(B=5, L=27, D=64, MLP=264, K=36, enqueue=False),      # K % 8 != 0: the padded path
    k35=dict(B=5, L=27, D=64, MLP=264, K=35),
    k320=dict(B=5, L=27, D=64, MLP=264, K=320),     # K above the 256 stride
)
STAGE_MODES = ("queue", "inbatch")
STAGE_T = (0.07, 1.0)
UPSTREAM = 0.25


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(round(float(k) * 1000))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _bf16(x):
    return x.bfloat16().float()


# ================================================================================================================ the gates
class Report:
    """Collects, per tensor, the worst error over its bound's scale (the figure the docstrings record) and the violated gates."""

    def __init__(self, what):
        self.what, self.rows, self.fails = what, [], []

    def _add(self, name, gate, err, bound):
        ok = bool(torch.all(err <= bound)) and bool(torch.isfinite(err).all())
        worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        self.rows.append((name, gate, worst))
        if not ok:
            self.fails.append(f"{self.what} {name}/{gate}: worst error {worst:.3g} x its bound")

    def f32_class(self, name, got, T):
        T = T.double()
        assert got.shape == T.shape, (name, tuple(got.shape), tuple(T.shape))
        self._add(name, "f32", (got.double() - T).abs(), torch.full_like(T, F32_TOL * max(1.0, float(T.abs().max()) if T.numel() else 0.0)))

    def rel_class(self, name, got, T):
        T = T.double().reshape(-1)
        self._add(name, "rel", (got.double().reshape(-1) - T).abs(), LOSS_RTOL * T.abs())

    def grad_class(self, name, got, T):
        T = T.double()
        assert got.shape == T.shape, (name, tuple(got.shape), tuple(T.shape))
        self._add(name, "grad", (got.double() - T).abs(), GRAD_ATOL + GRAD_RTOL * T.abs())

    def bf16_store(self, name, got, T):
        T = T.double()
        assert got.shape == T.shape, (name, tuple(got.shape), tuple(T.shape))
        self._add(name, "bf16", (got.double() - T).abs(), BF16_HALF_ULP_X2 * T.abs() + F32_TOL * float(T.abs().max()))

    def exact(self, name, got, T):
        if not (got.shape == T.shape and torch.equal(got, T.to(got.dtype))):
            self.fails.append(f"{self.what} {name}/exact: differs")
        self.rows.append((name, "exact", 0.0))

    def zero(self, name, got):
        if not bool((got == 0).all()):
            self.fails.append(f"{self.what} {name}/zero: padding not exactly 0")

    def text(self):
        return f"[{self.what}] " + "  ".join(f"{n} {g} {w:.3f}" for n, g, w in self.rows)


# ================================================================================================================ BatchNorm
@functools.lru_cache(maxsize=None)
def bn_case(R, C, relu, affine, running, io="f32", offset=0.0):
    """-> inputs (float32, already rounded to bf16 where io == "bf16") and truth T (float64, from those inputs)."""
    g = _gen(R, C, relu, affine, running, io == "bf16", offset)
    if offset:
        scale, shift = torch.ones(C), offset + 0.1 * torch.randn(C, generator=g)
    else:
        scale = torch.tensor((0.05, 0.5, 1.0, 2.0))[torch.arange(C) % 4]
        shift = scale * (torch.arange(C) % 5 - 2.0) * 0.5
    x = torch.randn(R, C, generator=g) * scale + shift
    dy = torch.randn(R, C, generator=g)
    gamma = (1.0 + 0.4 * torch.randn(C, generator=g)) if affine else None
    if affine:
        gamma[C // 2] = -0.7                       # a negative gain: y > 0 where y_pre < the mean
    beta = 0.3 * torch.randn(C, generator=g) if affine else None
    rm0 = torch.randn(C, generator=g) if running else None
    rv0 = (0.5 + torch.rand(C, generator=g)) if running else None
    if io == "bf16":
        x, dy = _bf16(x), _bf16(dy)
    xd = x.double()
    z = (xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + EPS)
    if affine:
        z = z * gamma.double() + beta.double()
    if relu:
        dy = torch.where(z.abs() < NEAR_ZERO, torch.zeros(()), dy)
        if not affine and not running:
            dy = torch.where(z <= 0, torch.zeros(()), dy)           # the dy of a ReLU'd consumer: exactly 0 where y == 0
    xr = xd.clone().requires_grad_(True)
    gr = gamma.double().clone().requires_grad_(True) if affine else None
    br = beta.double().clone().requires_grad_(True) if affine else None
    zero = torch.zeros(C, dtype=torch.float64)
    y, rm, rv = mo.batchnorm_tokens(xr[None], gr, br, rm0.double() if running else zero, rv0.double() if running else zero,
                                    eps=EPS, momentum=MOMENTUM)
    y = torch.relu(y[0]) if relu else y[0]
    (y * dy.double()).sum().backward()
    T = dict(y=y.detach(), mean=xd.mean(0), invstd=1.0 / torch.sqrt(xd.var(0, unbiased=False) + EPS), dx=xr.grad)
    if running:
        T.update(running_mean=rm.detach(), running_var=rv.detach())
    if affine:
        T.update(dgamma=gr.grad, dbeta=br.grad)
    return dict(R=R, C=C, relu=relu, affine=affine, running=running, io=io, x=x, dy=dy, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, T=T)


def bn_cases(io="f32"):
    out = []
    for R, C in BN_SHAPES:
        if (R, C) in BN_GRID_STRIDE and io == "bf16":
            continue
        for relu, affine, running in (BN_CONFIGS_LARGE if (R, C) in BN_GRID_STRIDE else BN_CONFIGS):
            out.append((R, C, relu, affine, running, io))
    return out


def check_bn(c, got, rep=None):
    """got: y, mean, invstd, dx (+ running_mean, running_var, dgamma, dbeta where the case has them), float32 on the CPU."""
    rep = rep or Report(f"bn {c['R']}x{c['C']} relu{c['relu']} affine{int(c['affine'])} run{int(c['running'])} {c['io']}")
    T = c["T"]
    assert sorted(got) == sorted(T), sorted(set(got) ^ set(T))
    for k in T:
        (rep.bf16_store if c["io"] == "bf16" and k in ("y", "dx") else rep.f32_class)(k, got[k], T[k])
    return rep


def _slabs(x, rows=64):
    """[R, C] -> ([ns, rows, C] zero-padded, valid [ns, rows])."""
    R, C = x.shape
    ns = (R + rows - 1) // rows
    p = torch.zeros(ns * rows, C, dtype=x.dtype)
    p[:R] = x
    v = torch.zeros(ns * rows, dtype=torch.bool)
    v[:R] = True
    return p.view(ns, rows, C), v.view(ns, rows)


def _welford(xs, valid, divide):
    """Sequential Welford over dim 1 of xs [ns, n, C] in float32, skipping invalid rows. -> n [ns, 1], mean, m2 [ns, C]."""
    ns, n_, C = xs.shape
    mean, m2, n = torch.zeros(ns, C), torch.zeros(ns, C), torch.zeros(ns, 1)
    for i in range(n_):
        ok = valid[:, i:i + 1]
        n1 = n + ok.float()
        v = xs[:, i]
        d = v - mean
        mean1 = mean + (d / n1.clamp_min(1.0) if divide else d * (1.0 / n1.clamp_min(1.0)))
        m21 = m2 + d * (v - mean1)
        mean, m2, n = torch.where(ok, mean1, mean), torch.where(ok, m21, m2), n1
    return n, mean, m2


def _chan(n, mu, q, nb, mb, qb, skip_empty=True):
    """Chan's update of (n, mu, q) by (nb, mb, qb), elementwise; nb == 0 leaves the triple alone."""
    tot = n + nb
    delta = mb - mu
    safe = tot.clamp_min(1.0)
    mu1 = mu + delta * nb / safe
    q1 = q + qb + delta * delta * n * nb / safe
    if not skip_empty:
        return tot, mu1, q1
    live = nb > 0
    return torch.where(live, tot, n), torch.where(live, mu1, mu), torch.where(live, q1, q)


def bn_fwd_restated(x, gamma, beta, relu, rm0, rv0, io="f32", mutant=None):
    """evp_batchnorm_fwd in float32 on the CPU in the kernels' order: per slab of 64 rows a Welford pass (C % 4 == 0: four row lanes
    of every 4th row each, met by Chan's update in float32; otherwise one pass), the slabs folded in double by 16 groups of every
    16th slab, the groups met in double; statistics cast to float32. -> y, mean, invstd, running_mean, running_var."""
    R, C = x.shape
    xs, valid = _slabs(x)
    ns = xs.shape[0]
    if C % 4 == 0:
        lanes = [_welford(xs[:, l::4], valid[:, l::4], divide=False) for l in range(4)]
        n, mu, q = lanes[0]
        for nb, mb, qb in lanes[1:]:
            if mutant == "empty_lane_counts_one":
                nb = nb.clamp_min(1.0)
            n, mu, q = _chan(n.expand_as(mu), mu, q, nb.expand_as(mu), mb, qb)
    else:
        n, mu, q = _welford(xs, valid, divide=True)
    cnt = valid.sum(1).double()
    if mutant == "last_slab_dropped" and ns > 1:
        ns, cnt, mu, q = ns - 1, cnt[:-1], mu[:-1], q[:-1]
    # finalize: 16 groups fold every 16th slab, then group 0 takes the others in turn
    gn, gm, gq = torch.zeros(16, 1, dtype=torch.float64), torch.zeros(16, C, dtype=torch.float64), torch.zeros(16, C, dtype=torch.float64)
    for k in range((ns + 15) // 16):
        idx = torch.arange(16) + 16 * k
        live = idx < ns
        idc = idx.clamp_max(ns - 1)
        nb = torch.where(live, cnt[idc], torch.zeros((), dtype=torch.float64)).view(16, 1)
        gn2, gm2, gq2 = _chan(gn.expand_as(gm), gm, gq, nb.expand_as(gm), mu[idc].double(), q[idc].double())
        gn, gm, gq = gn2[:, :1], gm2, gq2
    n, m, m2 = gn[0].expand(C), gm[0], gq[0]
    for i in range(1, 16):
        n, m, m2 = _chan(n, m, m2, gn[i].expand(C), gm[i], gq[i])
    var_b = (m2 / n).float()
    mean = m.float()
    invstd = 1.0 / (torch.sqrt(var_b) + EPS) if mutant == "eps_outside_sqrt" else 1.0 / torch.sqrt(var_b + EPS)
    rm = rv = None
    if rm0 is not None:
        var_u = (m2 / n).float() if mutant == "biased_running_var" else (m2 / torch.where(n > 1, n - 1, torch.ones_like(n))).float()
        if mutant == "momentum_on_wrong_term":
            rm, rv = MOMENTUM * rm0 + (1.0 - MOMENTUM) * mean, MOMENTUM * rv0 + (1.0 - MOMENTUM) * var_u
        else:
            rm, rv = (1.0 - MOMENTUM) * rm0 + MOMENTUM * mean, (1.0 - MOMENTUM) * rv0 + MOMENTUM * var_u
    y = (x - mean) * invstd
    if gamma is not None:
        y = y * gamma + beta
    if relu:
        y = y.clamp_min(0.0)
    return (_bf16(y) if io == "bf16" else y), mean, invstd, rm, rv


def bn_bwd_restated(dy, x, y, gamma, mean, invstd, relu, io="f32", mutant=None, y_pre_affine=None):
    """evp_batchnorm_bwd: per slab the sums of dy' and dy' * xhat (vector form: four row lanes, added pairwise), the slabs folded by
    16 groups in float32, dx = gamma * invstd * (dy' - sum_dy / R - xhat * sum_dy_xhat / R). -> dx, dgamma (sum dy' xhat), dbeta."""
    R, C = x.shape
    d = dy
    if relu:
        mask_src = x if mutant == "relu_mask_from_y_pre" else y               # y_pre is the kernel's INPUT x
        d = torch.where(mask_src > 0, dy, torch.zeros(()))
    xh = (x - mean) * invstd
    a, _ = _slabs(d)
    b, _ = _slabs(d * xh)
    ns = a.shape[0]

    def slab_sum(t):
        if C % 4 == 0:
            lane = []
            for l in range(4):
                s = torch.zeros(ns, C)
                for i in range(l, 64, 4):
                    s = s + t[:, i]
                lane.append(s)
            part = (lane[0] + lane[1]) + (lane[2] + lane[3])
        else:
            part = torch.zeros(ns, C)
            for i in range(64):
                part = part + t[:, i]
        grp = torch.zeros(16, C)
        for s in range(ns):
            grp[s % 16] = grp[s % 16] + part[s]
        tot = grp[0]
        for i in range(1, 16):
            tot = tot + grp[i]
        return tot
    s0, s1 = slab_sum(a), slab_sum(b)
    invR = 1.0 if mutant == "no_1_over_R_in_dx" else 1.0 / R
    g = gamma if gamma is not None else torch.ones(C)
    dx = g * invstd * (d - s0 * invR - xh * s1 * invR)
    if mutant == "dgamma_dbeta_swapped":
        s0, s1 = s1, s0
    return (_bf16(dx) if io == "bf16" else dx), s1, s0


def bn_restated(c, mutant=None):
    """The case through the restatement, as the GPU test runs it through the kernels: the backward gets the forward's own outputs."""
    y, mean, invstd, rm, rv = bn_fwd_restated(c["x"], c["gamma"], c["beta"], c["relu"], c["rm0"], c["rv0"], c["io"], mutant)
    dx, dgamma, dbeta = bn_bwd_restated(c["dy"], c["x"], y, c["gamma"], mean, invstd, c["relu"], c["io"], mutant)
    got = dict(y=y, mean=mean, invstd=invstd, dx=dx)
    if c["running"]:
        got.update(running_mean=rm, running_var=rv)
    if c["affine"]:
        got.update(dgamma=dgamma, dbeta=dbeta)
    return got


# ================================================================================================================ row kernels
@functools.lru_cache(maxsize=None)
def row_case(R, C):
    g = _gen(R, C, 7)
    x, dy, b, add = (torch.randn(R, C, generator=g) for _ in range(4))
    x = x * (0.5 + torch.arange(R).remainder(5).float().view(R, 1))           # norms that differ from row to row
    s = torch.randn(R, generator=g)
    zero_row = R // 2 if R >= 5 else None
    if zero_row is not None:
        x[zero_row] = 0.0
    xd, dyd = x.double(), dy.double()
    norm = xd.norm(dim=1).clamp_min(L2_EPS)
    y = xd / norm[:, None]
    dx = (dyd - y * (dyd * y).sum(1, keepdim=True)) / norm[:, None]           # the zero row: dy / 1e-12, as F.normalize's clamp gives
    T = dict(y=y, norm=norm, dx=dx, rowdot=(xd * b.double()).sum(1), scale=s.double()[:, None] * xd,
             scale_add=s.double()[:, None] * xd + add.double())
    return dict(R=R, C=C, x=x, dy=dy, b=b, add=add, s=s, zero_row=zero_row, T=T)


def check_rows(c, got, rep=None):
    """got: any of y, norm, dx, rowdot, scale, scale_add. The all-zero row of dx (1e12 times dy) is compared relative to its own size."""
    rep = rep or Report(f"rows {c['R']}x{c['C']}")
    T, z = c["T"], c["zero_row"]
    for k, v in got.items():
        if k == "dx" and z is not None:
            keep = torch.arange(c["R"]) != z
            rep.f32_class("dx", v[keep], T["dx"][keep])
            rep.f32_class("dx[zero row]", v[z] * L2_EPS, T["dx"][z] * L2_EPS)
        else:
            rep.f32_class(k, v, T[k])
    return rep


def _lane_sum(t):
    """sum over dim 1 as a wave does it: lane j takes every 64th column, the 64 partial sums are added."""
    R, C = t.shape
    p = torch.zeros(R, (C + 63) // 64 * 64)
    p[:, :C] = t
    acc = torch.zeros(R, 64)
    for k in range(p.shape[1] // 64):
        acc = acc + p[:, 64 * k:64 * k + 64]
    return acc.sum(1)


def l2norm_fwd_restated(x):
    nrm = torch.sqrt(_lane_sum(x * x)).clamp_min(torch.tensor(L2_EPS, dtype=torch.float32))
    return x * (1.0 / nrm)[:, None], nrm


def l2norm_bwd_restated(dy, y, nrm):
    return (dy - y * _lane_sum(dy * y)[:, None]) * (1.0 / nrm)[:, None]


def rows_restated(c):
    y, nrm = l2norm_fwd_restated(c["x"])
    return dict(y=y, norm=nrm, dx=l2norm_bwd_restated(c["dy"], y, nrm), rowdot=_lane_sum(c["x"] * c["b"]),
                scale=c["s"][:, None] * c["x"], scale_add=c["s"][:, None] * c["x"] + c["add"])


# ================================================================================================================ loss kernels
def _thread_sum(t):
    """sum over dim 1 as a 256-thread block does it: thread j takes every 256th column in turn, the partial sums are added."""
    R, n = t.shape
    p = torch.zeros(R, (n + 255) // 256 * 256)
    p[:, :n] = t
    acc = torch.zeros(R, 256)
    for k in range(p.shape[1] // 256):
        acc = acc + p[:, 256 * k:256 * k + 256]
    return acc.sum(1)


def mean_restated(v):
    """mean_kernel: 1024 threads walk the row losses, one block."""
    n = v.numel()
    p = torch.zeros((n + 1023) // 1024 * 1024)
    p[:n] = v
    return p.view(-1, 1024).sum(0).sum() / n


@functools.lru_cache(maxsize=None)
def nce_case(R, K, ldn):
    g = _gen(R, K, ldn, 11)
    pos = torch.rand(R, generator=g) * 1.6 - 0.8
    neg = torch.full((R, ldn), float("nan"))                  # the padding columns [K, ldn) are not read
    neg[:, :K] = torch.rand(R, K, generator=g) * 1.6 - 0.8
    if R > 1:
        pos[0] = 0.99                                         # the positive is the row's maximum
        pos[1], neg[1, K // 2] = -0.5, 0.97                   # a negative is
    else:
        pos[0], neg[0, 0] = 0.3, 0.35     # one row: a loss of order 1 (log(1 + e^-14) against a relative bound would measure logf, not the kernel)
    p = pos.double().clone().requires_grad_(True)
    n = neg[:, :K].double().clone().requires_grad_(True)
    rows = F.cross_entropy(torch.cat([p[:, None], n], 1) * INV_T, torch.zeros(R, dtype=torch.long), reduction="none")
    rows.mean().backward()
    dneg = torch.zeros(R, ldn, dtype=torch.float64)
    dneg[:, :K] = n.grad
    return dict(R=R, K=K, ldn=ldn, pos=pos, neg=neg, T=dict(loss=rows.mean().detach(), row_loss=rows.detach(), dpos=p.grad, dneg=dneg))


def check_nce(c, got, rep=None):
    """got: loss, row_loss (+ dpos, dneg unless the run passed null gradients)."""
    rep = rep or Report(f"infonce R{c['R']} K{c['K']} ld{c['ldn']}")
    T = c["T"]
    rep.rel_class("loss", got["loss"], T["loss"])
    rep.f32_class("row_loss", got["row_loss"], T["row_loss"])
    if "dneg" in got:
        rep.grad_class("dpos", got["dpos"], T["dpos"])
        rep.grad_class("dneg", got["dneg"], T["dneg"])
        rep.zero("dneg[:, K:]", got["dneg"][:, c["K"]:])
    return rep


def nce_restated(pos, neg, K, inv_T=INV_T, mutant=None):
    """infonce_queue_kernel + mean_kernel: per row the maximum, the sum of exponentials, the logarithm."""
    R, ldn = neg.shape
    n = ldn if mutant == "padding_in_softmax" else K
    lg = neg[:, :n] * inv_T
    p0 = pos * inv_T
    mx = torch.maximum(p0, lg.max(1).values)
    e = torch.exp(lg - mx[:, None])
    s = _thread_sum(e)
    if mutant != "no_positive_in_denominator":
        s = s + torch.exp(p0 - mx)
    rows = (torch.log(s) + mx) - p0
    sc = (1.0 if mutant == "one_over_T_once" else inv_T) / R
    dneg = torch.zeros(R, ldn)
    dneg[:, :n] = e * (1.0 / s)[:, None] * sc
    return dict(loss=mean_restated(rows), row_loss=rows, dpos=(torch.exp(p0 - mx) / s - 1.0) * sc, dneg=dneg)


@functools.lru_cache(maxsize=None)
def ce_case(R, n_cls, ld, smoothing):
    g = _gen(R, n_cls, ld, smoothing, 13)
    logits = torch.full((R, ld), float("nan"))                # padding: never read
    logits[:, :n_cls] = (torch.rand(R, n_cls, generator=g) * 2 - 1) * INV_T
    labels = torch.randint(0, n_cls, (R,), generator=g)
    labels[0] = 0
    labels[-1] = n_cls - 1
    lg = logits[:, :n_cls].double().clone().requires_grad_(True)
    loss = mo.label_smoothing_ce(lg, labels, smoothing) if smoothing else F.cross_entropy(lg, labels)
    rows = F.cross_entropy(lg.detach(), labels, label_smoothing=smoothing, reduction="none")
    loss.backward()
    dl = torch.zeros(R, ld, dtype=torch.float64)
    dl[:, :n_cls] = lg.grad
    return dict(R=R, n_cls=n_cls, ld=ld, smoothing=smoothing, logits=logits, labels=labels,
                T=dict(loss=loss.detach(), row_loss=rows, dlogits=dl))


def check_ce(c, got, rep=None):
    rep = rep or Report(f"ce R{c['R']} n{c['n_cls']} ld{c['ld']} s{c['smoothing']}")
    T = c["T"]
    rep.rel_class("loss", got["loss"], T["loss"])
    rep.f32_class("row_loss", got["row_loss"], T["row_loss"])
    rep.grad_class("dlogits", got["dlogits"], T["dlogits"])
    rep.zero("dlogits[:, n_cls:]", got["dlogits"][:, c["n_cls"]:])
    return rep


def ce_restated(logits, labels, n_cls, smoothing=0.0, mutant=None):
    """ce_rows_kernel + mean_kernel."""
    R, ld = logits.shape
    n = ld if mutant == "padding_in_softmax" else n_cls
    lr = logits[:, :n]
    mx = lr.max(1).values
    e = torch.exp(lr - mx[:, None])
    s = _thread_sum(e)
    lse = torch.log(s) + mx
    rows = lse - lr[torch.arange(R), labels]
    div = float(ld if mutant == "smoothing_over_ld" else n_cls)
    if smoothing > 0:
        rows = (1.0 - smoothing) * rows + smoothing * (lse - _thread_sum(lr) / div)
    onehot = F.one_hot(labels, n).float()
    dl = torch.zeros(R, ld)
    dl[:, :n] = (e * (1.0 / s)[:, None] - (onehot * (1.0 - smoothing) + smoothing / div)) * (1.0 / R)
    return dict(loss=mean_restated(rows), row_loss=rows, dlogits=dl)


# ================================================================================================================ enqueue, token mean
def enq_starts(B, K):
    """start positions: 0, a middle slot, the last slot (the pointer wraps to 0)."""
    return sorted({0, (K // B // 2) * B, K - B})


@functools.lru_cache(maxsize=None)
def enq_case(B, L, C, K):
    g = _gen(B, L, C, K, 17)
    return dict(B=B, L=L, C=C, K=K, queue=torch.randn(C, L, K, generator=g), keys=torch.randn(B, L, C, generator=g))


def enqueue_restated(queue, keys, ptr, mutant=None):
    """evp_enqueue_keys_dev: 64 x 64 tiles of (batch, channel) per token through a transposing buffer; element by element where
    L > 65535; nothing at all for a pointer outside [0, K - B]; then the pointer advances modulo K. -> (queue, pointer)."""
    B, L, C = keys.shape
    K = queue.shape[2]
    q = queue.clone()
    if 0 <= ptr <= K - B:
        if mutant == "enqueue_without_reversal":
            q[:, :, ptr:ptr + B] = keys.reshape(C, L, B)
        elif L <= 65535:
            for b0 in range(0, B, 64):
                for c0 in range(0, C, 64):
                    tile = keys[b0:b0 + 64, :, c0:c0 + 64]                  # [b, l, c]
                    q[c0:c0 + 64, :, ptr + b0:ptr + b0 + tile.shape[0]] = tile.permute(2, 1, 0)
        else:
            i = torch.arange(B * L * C)
            b, t = i % B, i // B
            l, c = t % L, t // L
            q.view(-1)[(c * L + l) * K + ptr + b] = keys.reshape(-1)[(b * L + l) * C + c]
    return q, (ptr + B if mutant == "pointer_without_modulo" else (ptr + B) % K)


def check_enqueue(c, start, got_queue, got_ptr, rep=None):
    rep = rep or Report(f"enqueue B{c['B']} L{c['L']} C{c['C']} K{c['K']} at {start}")
    want, ptr = mo.enqueue(c["queue"], start, c["keys"])
    rep.exact("queue", got_queue, want)
    rep.exact("ptr", torch.tensor(int(got_ptr)), torch.tensor(int(ptr)))
    return rep


@functools.lru_cache(maxsize=None)
def mean_case(B, N, D):
    g = _gen(B, N, D, 19)
    x, gy = torch.randn(B, N, D, generator=g) + 0.5, torch.randn(B, D, generator=g)
    return dict(B=B, N=N, D=D, x=x, g=gy, T=dict(out=x.double().mean(1), dx=(gy.double() / N)[:, None, :].expand(B, N, D).contiguous()))


def check_mean(c, got, rep=None):
    rep = rep or Report(f"token mean {c['B']}x{c['N']}x{c['D']}")
    for k in ("out", "dx"):
        rep.f32_class(k, got[k], c["T"][k])
    return rep


def token_mean_restated(x, g):
    B, N, D = x.shape
    s = torch.zeros(B, D)
    for n in range(N):
        s = s + x[:, n]
    return dict(out=s * (1.0 / N), dx=(g * (1.0 / N))[:, None, :].expand(B, N, D).contiguous())


# ================================================================================================================ part 2: the module tail
def _stage_seed(name):
    return 4000 + list(STAGE).index(name)


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """-> the two heads (CPU, closed-form weights, training mode), emb_h, clip_emb (B, L, D), the unit-normalised queue (D, L, K) and
    the start pointer. Deterministic; nobody writes into it (the GPU tests deep-copy the heads)."""
    from eventpretrain_amd.model.sub_module.mlp_head import _build_mlp_2d
    s = STAGE[name]
    g = torch.Generator().manual_seed(_stage_seed(name))
    proj, pred = _build_mlp_2d(3, s["D"], s["MLP"], s["D"]), _build_mlp_2d(2, s["D"], s["MLP"], s["D"])
    heads = torch.nn.ModuleDict(dict(emb_h_proj=proj, emb_h_pred=pred))
    det_fill_module_(heads)
    B, L, D, K = s["B"], s["L"], s["D"], s["K"]
    return dict(spec=s, heads=heads.train(), emb_h=torch.randn(B, L, D, generator=g), clip_emb=torch.randn(B, L, D, generator=g),
                queue=F.normalize(torch.randn(D, L, K, generator=g), dim=0), ptr0=K - B if name == "k40" else (B if K >= 2 * B else 0),
                enqueue=s.get("enqueue", True))


def stage_tensors(name):
    c = stage_case(name)
    t = ["loss", "act:h", "act:d_emb_h", "act:d_clip_emb"]
    t += ["grad:" + k for k, p in c["heads"].named_parameters()]
    t += ["stat:" + k for k, _ in c["heads"].named_buffers() if k.endswith(("running_mean", "running_var"))]
    return t + (["queue", "ptr"] if c["enqueue"] else [])


def _stage_oracle(name, mode, T_, how):
    """One run of the oracle functions: how = "truth" (float64), "f32", or "yardstick" (float32 under CPU autocast to bf16)."""
    c = stage_case(name)
    dt = torch.float64 if how == "truth" else torch.float32
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if how == "yardstick" else contextlib.nullcontext()
    sd = {k: v.detach().clone().to(dt) if v.is_floating_point() else v.detach().clone() for k, v in c["heads"].state_dict().items()}
    params = [k for k, _ in c["heads"].named_parameters()]
    for k in params:
        sd[k].requires_grad_(True)
    emb, clip = c["emb_h"].to(dt).clone().requires_grad_(True), c["clip_emb"].to(dt).clone().requires_grad_(True)
    queue0 = c["queue"].to(dt)
    res = {}
    with ctx:
        h, s1 = mo.mlp_head(sd, "emb_h_proj.", emb, 3)
        h, s2 = mo.mlp_head(sd, "emb_h_pred.", h, 2)
        if mode == "queue":
            loss, k = mo.info_nce_queue(h, clip, queue0, T_)
        else:
            loss, k = mo.info_nce_inbatch(h, clip, T_), F.normalize(clip, dim=-1)
        if c["enqueue"]:
            res["queue"], ptr = mo.enqueue(queue0, c["ptr0"], k.to(dt))
            res["ptr"] = torch.tensor([ptr])
    (loss.to(dt) * UPSTREAM).backward()
    res.update({"loss": loss, "act:h": h, "act:d_emb_h": emb.grad, "act:d_clip_emb": clip.grad})
    res.update({"grad:" + k: sd[k].grad for k in params})
    res.update({"stat:" + k: v for k, v in {**s1, **s2}.items()})
    return {k: v.detach().double() if k != "ptr" else v for k, v in res.items()}


class StageReference:
    def __init__(self, name, mode, T_):
        self.T, self.Y, self.F = (_stage_oracle(name, mode, T_, how) for how in ("truth", "yardstick", "f32"))
        self.tensors = stage_tensors(name)
        assert sorted(self.tensors) == sorted(self.T), sorted(set(self.tensors) ^ set(self.T))

    def e_ref(self, t):
        return bt.rel_err(self.Y[t], self.T[t])

    def e_f32(self, t):
        return bt.rel_err(self.F[t], self.T[t])


@functools.lru_cache(maxsize=None)
def stage_reference(name, mode, T_):
    """Computed once per process and shared; nobody writes into it."""
    return StageReference(name, mode, T_)


@functools.lru_cache(maxsize=None)
def loss_yardstick(mode, T_):
    """The yardstick's error on the LOSS, pooled: the RMS over the cases of STAGE of |Y - T| / |T| for this loss form and temperature.
    A tensor's relative L2 error is an RMS over its elements' errors; the loss has one element, and one draw of a near zero-mean
    rounding error has no stable size -- over the five cases the yardstick's own loss error spans 7e-6 to 6e-4 (queue, T = 0.07) and
    1.4e-6 to 2.4e-4 (in-batch, T = 1.0), so three times a single draw bounds nothing. Same oracle functions, same FACTOR."""
    e = [stage_reference(n, mode, T_).e_ref("loss") for n in STAGE]
    return (sum(x * x for x in e) / len(e)) ** 0.5


def stage_yardstick(name, mode, T_):
    """-> {tensor: the yardstick's value}, the loss placed at its pooled distance from truth (loss_yardstick)."""
    ref = stage_reference(name, mode, T_)
    Y = dict(ref.Y)
    Y["loss"] = ref.T["loss"] * (1.0 + loss_yardstick(mode, T_))
    return Y


def stage_runs():
    return [(n, m, t) for n in STAGE for m in STAGE_MODES for t in STAGE_T]


def _check_queue(ref, got, keys, c, rep):
    """The queue is f32 in both modes: bit-exact against mo.enqueue of the run's OWN normalised keys, f32 class against truth."""
    want, ptr = mo.enqueue(c["queue"], c["ptr0"], keys)
    rep.exact("queue (own keys)", got["queue"], want)
    rep.f32_class("queue", got["queue"], ref.T["queue"])
    rep.exact("ptr", got["ptr"].view(-1).long(), torch.tensor([ptr]))
    rep.exact("ptr (truth)", got["ptr"].view(-1).long(), ref.T["ptr"])


def check_stage_f32(name, mode, T_, got, keys=None):
    """Per-tensor relative L2 error against truth <= max(FACTOR * the float32 oracle's, 1e-5). -> (fails, worst (e_got / e_F, tensor), table)."""
    ref, c = stage_reference(name, mode, T_), stage_case(name)
    assert sorted(got) == sorted(ref.tensors), sorted(set(got) ^ set(ref.tensors))
    rep, worst, lines = Report(f"stage {name} {mode} T={T_} f32"), (0.0, ""), []
    for t in ref.tensors:
        if t in ("queue", "ptr"):
            continue
        g = got[t].detach().double().cpu()
        assert g.shape == ref.T[t].shape, (t, tuple(g.shape), tuple(ref.T[t].shape))
        e, ef = bt.rel_err(g, ref.T[t]), ref.e_f32(t)
        bound = max(FACTOR * ef, F32_TOL)
        worst = max(worst, (e / ef if ef > 0 else float("inf") if e > 0 else 0.0, t))
        lines.append(f"  {t:44s} e_hip {e:.2e}  e_F {ef:.2e}  bound {bound:.2e}")
        if not e <= bound:
            rep.fails.append(f"{rep.what} {t}: {e:.3e} > {bound:.3e} (the f32 oracle: {ef:.3e})")
    if c["enqueue"]:
        _check_queue(ref, got, keys, c, rep)
    return rep.fails, worst, "\n".join(lines)


def gate_bf16(name, mode, T_, got):
    """The three gates of block_truth.compare for the tensors of `got` (not the queue or the pointer) against stage_yardstick.
    -> (fails, worst (ratio, tensor/gate), table)."""
    ref, Y = stage_reference(name, mode, T_), stage_yardstick(name, mode, T_)
    fails, worst, lines = [], (0.0, ""), []
    for t, g in got.items():
        rows, f = bt.compare(t, g, ref.T[t], Y[t])
        fails += f
        for gate, val, bound, ratio in rows:
            worst = max(worst, (ratio, f"{t}/{gate}"))
        lines.append(f"  {t:44s} e_ref {bt.rel_err(Y[t], ref.T[t]):.2e}  " + "  ".join(f"{gate} {ratio:.2f}" for gate, _, _, ratio in rows))
    return fails, worst, "\n".join(lines)


def check_stage_bf16(name, mode, T_, got, keys=None):
    """gate_bf16 on every tensor, the queue and the pointer as in f32 mode. -> (fails, worst (ratio, tensor/gate), table)."""
    ref, c = stage_reference(name, mode, T_), stage_case(name)
    assert sorted(got) == sorted(ref.tensors), sorted(set(got) ^ set(ref.tensors))
    fails, worst, table = gate_bf16(name, mode, T_, {t: got[t] for t in ref.tensors if t not in ("queue", "ptr")})
    if c["enqueue"]:
        rep = Report(f"stage {name} {mode} T={T_} bf16")
        _check_queue(ref, got, keys, c, rep)
        fails = fails + rep.fails
    return fails, worst, table


def _linear_bn_fwd(x2, w, bn, relu, mutant):
    y_pre = x2 @ w.t()
    y, mean, invstd, rm, rv = bn_fwd_restated(y_pre, bn.weight.detach() if bn.affine else None, bn.bias.detach() if bn.affine else None,
                                              relu, bn.running_mean, bn.running_var, mutant=mutant)
    return y, (x2, w, y_pre, y, mean, invstd, bn, relu), (rm, rv)


def _linear_bn_bwd(g, saved, mutant):
    x2, w, y_pre, y, mean, invstd, bn, relu = saved
    dpre, dgamma, dbeta = bn_bwd_restated(g, y_pre, y, bn.weight.detach() if bn.affine else None, mean, invstd, relu, mutant=mutant)
    return dpre @ w, dpre.t() @ x2, dgamma, dbeta


def stage_restated(name, mode, T_, mutant=None):
    """The module tail in float32 on the CPU in the order of ops.py: Linear -> BatchNorm (-> ReLU) five times, row normalisation,
    the queue or in-batch InfoNCE, the enqueue, then the backward by hand. -> ({tensor: value}, the normalised keys)."""
    c = stage_case(name)
    s = c["spec"]
    B, L, D, K = s["B"], s["L"], s["D"], s["K"]
    R = B * L
    stages = []
    for head in ("emb_h_proj", "emb_h_pred"):
        mods = list(c["heads"][head])
        for i, m in enumerate(mods):
            if isinstance(m, torch.nn.Linear):
                relu = i + 2 < len(mods) and isinstance(mods[i + 2], torch.nn.ReLU)
                stages.append((f"{head}.{i}", m.weight.detach(), mods[i + 1], f"{head}.{i + 1}", relu))
    got, saved = {}, []
    x = c["emb_h"].reshape(R, D)
    for key, w, bn, bn_key, relu in stages:
        x, sv, (rm, rv) = _linear_bn_fwd(x, w, bn, relu, mutant)
        saved.append(sv)
        got[f"stat:{bn_key}.running_mean"], got[f"stat:{bn_key}.running_var"] = rm, rv
    h = x
    got["act:h"] = h.view(B, L, D)
    q, qn = l2norm_fwd_restated(h)
    k, kn = l2norm_fwd_restated(c["clip_emb"].reshape(R, D))
    queue_after, ptr = enqueue_restated(c["queue"], k.view(B, L, D), c["ptr0"], mutant) if c["enqueue"] else (c["queue"], c["ptr0"])
    q3, k3 = q.view(B, L, D), k.view(B, L, D)
    if mode == "queue":
        Kp = (K + 7) // 8 * 8
        neg = torch.zeros(R, Kp)
        neg[:, :K] = torch.einsum("blc,clk->blk", q3, c["queue"]).reshape(R, K)
        r = nce_restated(_lane_sum(q * k), neg, K, 1.0 / T_, mutant)
        qb = queue_after if mutant == "backward_reads_queue_after_enqueue" else c["queue"]
        dq = r["dpos"][:, None] * k + torch.einsum("blk,clk->blc", r["dneg"].view(B, L, Kp)[:, :, :K], qb).reshape(R, D)
        dk = r["dpos"][:, None] * q
    else:
        Mp = (B + 7) // 8 * 8
        logits = torch.zeros(R, Mp)
        logits[:, :B] = (torch.einsum("nlc,mlc->nlm", q3, k3) * (1.0 / T_)).reshape(R, B)
        labels = torch.arange(B).view(B, 1).expand(B, L).reshape(R)
        r = ce_restated(logits, labels, B, 0.0, mutant)
        dl = r["dlogits"].view(B, L, Mp)[:, :, :B]
        dq = (torch.einsum("nlm,mlc->nlc", dl, k3) * (1.0 / T_)).reshape(R, D)
        dk = (torch.einsum("nlm,nlc->mlc", dl, q3) * (1.0 / T_)).reshape(R, D)
    got["loss"] = r["loss"]
    g = l2norm_bwd_restated(dq * UPSTREAM, q, qn)
    got["act:d_clip_emb"] = l2norm_bwd_restated(dk * UPSTREAM, k, kn).view(B, L, D)
    for (key, w, bn, bn_key, relu), sv in zip(reversed(stages), reversed(saved)):
        g, dw, dgamma, dbeta = _linear_bn_bwd(g, sv, mutant)
        got[f"grad:{key}.weight"] = dw
        if bn.affine:
            got[f"grad:{bn_key}.weight"], got[f"grad:{bn_key}.bias"] = dgamma, dbeta
    got["act:d_emb_h"] = g.view(B, L, D)
    if c["enqueue"]:
        got["queue"], got["ptr"] = queue_after, torch.tensor([ptr])
    return got, k.view(B, L, D)


# ================================================================================================================ the mutants
# name -> what it is; every one must fail at least one gate of parts 1 and 2 (tests/test_contrast_truth_host.py)
MUTANTS = {
    "last_slab_dropped": "the last slab is missing from the BatchNorm statistics",
    "empty_lane_counts_one": "a row lane of the vector Welford combine that saw no row counts as one row",
    "biased_running_var": "the running variance takes the biased batch variance",
    "momentum_on_wrong_term": "momentum weighs the old running value instead of the batch value",
    "relu_mask_from_y_pre": "the ReLU mask of the BatchNorm backward is taken from the input y_pre, not the output y",
    "no_1_over_R_in_dx": "1 / R is missing from the mean terms of dx",
    "dgamma_dbeta_swapped": "dgamma and dbeta change places",
    "eps_outside_sqrt": "1 / (sqrt(var) + eps)",
    "no_positive_in_denominator": "InfoNCE without the positive in the softmax denominator",
    "one_over_T_once": "1 / T applied once instead of twice in the InfoNCE gradient",
    "padding_in_softmax": "the padding columns count in the softmax",
    "smoothing_over_ld": "the smoothing term is divided by ld instead of n_cls",
    "enqueue_without_reversal": "(B, L, C) written as (C, L, B) without reversing the dims",
    "pointer_without_modulo": "the pointer advances without the modulo",
    "backward_reads_queue_after_enqueue": "the backward reads the queue the enqueue has overwritten",
}

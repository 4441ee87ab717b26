"""Shared by the CPU and GPU tests of the deferred weight / bias gradients (eventpretrain_amd/wgrad_plan.py lays the launches
out, ops._DeferredGrads binds them): a float64 interpreter of the grouped launch tables they build (byte layout and entry names
taken from the planner; contracts and tile geometry stated here), and the per-layer problem lists of the benchmarked models.

The interpreter follows the C ABI (include/evtpretrain.h) of the four entries a plan step launches:
  evp_gemm_grouped_tn_bf16 / evp_gemm_grouped_tn_g4_bf16: C[m][n] (+)= sum_k A[k][m] B[k][n] per 128 / 256 output tile,
      `acc` = accumulate; G4 only: colsum[m] (+)= sum_k A[k][m] from the tile_n == 0 tiles, `cacc` = accumulate;
      items with prob < 0 are skipped;
  evp_sum_slices_f32: out[i] (+)= sum_s ws[s * numel + i];
  evp_colsum_grouped: out[n] += sum_m x[m, n] per (128-column block, 256-row slab), always accumulating.
Pointers are mapped back to the operands they came from (queued tensors, gradient buffers, split-K workspaces); every read
and write is bounds-checked against its tensor, every entry's contract is asserted (G4: K % 32 == 0, K >= 96, M, N >= 256,
N % 8 == 0), every output tile / column block must be produced exactly once per launch, and the K-slices of each queued
contribution must partition its rows exactly. `numeric=False` runs the same checks without arithmetic (fast sweeps over
full-size problem lists whose operands are never allocated)."""
import bisect

import numpy as np
import torch

from eventpretrain_amd import _lib
from eventpretrain_amd.wgrad_plan import COLSUM, G4, T128, COLSUM_DT as CDT, PROBLEM_DT as PDT

TILE = {G4: 256, T128: 128}


class FakeOperand:
    """Stand-in for a queued bf16 / f32 operand that is never allocated (sweeps at full size): the planner reads only its
    shape, stride, dtype, device and address. Addresses are far apart and above any real CPU allocation."""
    _next = 1 << 52

    def __init__(self, rows, cols, dtype=torch.bfloat16):
        self.shape = (rows, cols)
        self.dtype = dtype
        self.device = torch.device("cpu")
        self._ptr = FakeOperand._next
        FakeOperand._next += 1 << 38

    def data_ptr(self):
        return self._ptr

    def stride(self, d=None):
        s = (self.shape[1], 1)
        return s if d is None else s[d]

    def element_size(self):
        return 2 if self.dtype == torch.bfloat16 else 4

    def numel(self):
        return self.shape[0] * self.shape[1]


class PlanError(AssertionError):
    pass


def _check(cond, *msg):
    if not cond:
        raise PlanError(" ".join(str(m) for m in msg))


class _Region:
    def __init__(self, base, nbytes, obj, kind):
        self.base, self.nbytes, self.obj, self.kind = base, nbytes, obj, kind


class Interpreter:
    """Runs a list of ops._DeferredGrads._Step on the host. `queue_w` / `queue_b`: the queue the plan was built from (copies of
    _DeferredGrads.w / .b taken before build_plan / flush), `fresh`: ids of the parameters that had no .grad before the plan
    was built (their gradient memory starts as garbage: NaN here, so that a first contribution that accumulates shows)."""

    def __init__(self, queue_w, queue_b, fresh, numeric=True):
        self.numeric = numeric
        self.queue_w, self.queue_b = list(queue_w), list(queue_b)
        self.fresh = set(fresh)
        self.regions = []
        self.shadow = {}            # storage base -> float64 array (numeric mode)
        self.valid = {}             # param id -> False while its gradient memory is garbage (checked in both modes)
        self.cache = {}
        self.slices = {}            # id(dy) -> list of (k0, K, id(x) at k0)
        self.ws_written = {}        # (ws base, slice) -> count
        self.fused_bias = {}        # id(bias) -> count of fused column sums
        self.listed_bias = {}       # (id(param), id(x2d)) -> count in column-sum lists
        self.writers = {}           # round -> {step index: set of param ids written}
        self._ops = {}
        self._index = {}
        self._by_grad = None
        for item in self.queue_w:
            for t in (item[1], item[2]):
                self._add_operand(t)
        for _, x2d in self.queue_b:
            self._add_operand(x2d)

    # ---------------------------------------------------------------- memory
    def _add_operand(self, t):
        if id(t) in self._ops:
            return
        self._ops[id(t)] = t
        nbytes = t.numel() * t.element_size() if isinstance(t, FakeOperand) else t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()
        self.regions.append(_Region(t.data_ptr(), nbytes, t, "operand"))

    def add_output(self, t, garbage):
        """f32 gradient / workspace storage (views share their storage's shadow)."""
        st = t.untyped_storage()
        base = st.data_ptr()
        if base in self.shadow:
            return
        if self.numeric:
            cur = torch.empty(st.nbytes() // 4, dtype=torch.float32)
            cur.untyped_storage().copy_(st)
            sh = cur.double().numpy().copy()
            if garbage:
                sh[:] = np.nan
            self.shadow[base] = sh
        else:
            self.shadow[base] = None
        self.regions.append(_Region(base, st.nbytes(), st, "output"))

    def resolve(self, ptr, kind):
        idx = self._index.get(kind)
        if idx is None or idx[2] != len(self.regions):
            rs = sorted((r for r in self.regions if r.kind == kind), key=lambda r: r.base)
            idx = self._index[kind] = ([r.base for r in rs], rs, len(self.regions))
        i = bisect.bisect_right(idx[0], ptr) - 1
        if i >= 0:
            r = idx[1][i]
            if ptr < r.base + max(r.nbytes, 1):
                return r, ptr - r.base
        raise PlanError(f"pointer {ptr:#x} is not inside any known {kind}")

    def _read(self, ptr, rows, ld, cols):
        """float64 [rows, cols] view of a bf16 / f32 operand at ptr with leading dimension ld (elements)."""
        r, off = self.resolve(ptr, "operand")
        t = r.obj
        es = t.element_size()
        _check(off % es == 0, "misaligned operand pointer")
        e0 = off // es
        _check(rows >= 1 and cols >= 1 and ld >= cols, "bad operand shape", rows, cols, ld)
        _check(e0 + (rows - 1) * ld + cols <= t.numel(), "operand read out of bounds:", e0, rows, ld, cols, t.numel())
        if not self.numeric:
            return None
        a = self.cache.get(id(t))
        if a is None:
            a = t.detach().reshape(-1).float().numpy().astype(np.float64)
            self.cache[id(t)] = a
        return np.lib.stride_tricks.as_strided(a[e0:], shape=(rows, cols), strides=(ld * 8, 8))

    def _out(self, ptr, rows, ld, cols):
        r, off = self.resolve(ptr, "output")
        _check(off % 4 == 0, "misaligned output pointer")
        e0 = off // 4
        _check(e0 + (rows - 1) * ld + cols <= r.nbytes // 4, "output write out of bounds")
        return r, e0

    def _param_of(self, ptr):
        if self._by_grad is None:
            self._by_grad = {}
            for p_ in list(q[0] for q in self.queue_w) + [q[6] for q in self.queue_w if q[6] is not None] + [q[0] for q in self.queue_b]:
                if p_.grad is not None:
                    self._by_grad[p_.grad.data_ptr()] = p_
        return self._by_grad.get(ptr)

    def _note_write(self, p_, acc, step_i, rnd):
        if p_ is None:
            return
        if acc:
            _check(self.valid.get(id(p_), id(p_) not in self.fresh), "accumulate into a gradient that was never written (first "
                   "contribution must write, acc = 0)", tuple(p_.shape))
        self.valid[id(p_)] = True
        self.writers.setdefault(rnd, {}).setdefault(step_i, set()).add(id(p_))

    # ---------------------------------------------------------------- entries
    def _gemm(self, entry, pt, it, n_items, step_i, rnd):
        T = TILE[entry]
        probs = pt.numpy().view(PDT)
        items = it.numpy().view(np.int32).reshape(-1, 4)
        _check(items.shape[0] == n_items, "item count")
        count = [np.zeros(((p["M"] + T - 1) // T, (p["N"] + T - 1) // T), np.int64) for p in probs]
        vals = {}
        for i, p in enumerate(probs):
            M, N, K = int(p["M"]), int(p["N"]), int(p["K"])
            _check(M > 0 and N > 0 and K > 0, "empty problem")
            _check(p["lda"] % 8 == 0 and p["ldb"] % 8 == 0 and p["lda"] >= M and p["ldb"] >= N and p["ldc"] >= N, "leading dims", p)
            if entry == G4:
                _check(K % 32 == 0 and K >= 96, "G4 K contract (K % 32 == 0, K >= 96) violated: K =", K)
                _check(M >= 256 and N >= 256 and N % 8 == 0, "G4 M / N contract violated:", M, N)
            else:
                _check(int(p["colsum"]) == 0, "the 128x128 entry has no fused column sums")
            A = self._read(int(p["A"]), K, int(p["lda"]), M)
            B = self._read(int(p["B"]), K, int(p["ldb"]), N)
            ra, oa = self.resolve(int(p["A"]), "operand")
            rb, ob = self.resolve(int(p["B"]), "operand")
            k0a, k0b = oa // (2 * int(p["lda"])), ob // (2 * int(p["ldb"]))
            _check(oa % (2 * int(p["lda"])) == 0 and ob % (2 * int(p["ldb"])) == 0 and k0a == k0b, "A / B slices disagree")
            self.slices.setdefault(id(ra.obj), []).append((k0a, K, id(rb.obj)))
            if self.numeric:
                vals[i] = (A, B)
        self._count(items[items[:, 0] >= 0], count, entry)
        for i, p in enumerate(probs):
            _check((count[i] == 1).all(), f"{entry}: problem {i} tiles not produced exactly once "
                   f"(missing {(count[i] == 0).sum()}, repeated {(count[i] > 1).sum()})")
        for i, p in enumerate(probs):
            M, N, K, ldc = int(p["M"]), int(p["N"]), int(p["K"]), int(p["ldc"])
            r, e0 = self._out(int(p["C"]), M, ldc, N)
            gp = self._param_of(int(p["C"]))
            if gp is None:      # a split-K workspace slice
                _check(not p["acc"], "workspace slices are written, not accumulated")
                self.ws_written[(r.base, e0)] = self.ws_written.get((r.base, e0), 0) + 1
            else:
                _check(M * N == gp.numel() and ldc == N, "problem does not cover its whole gradient")
            self._note_write(gp, int(p["acc"]), step_i, rnd)
            if int(p["colsum"]):
                bp = self._param_of(int(p["colsum"]))
                _check(bp is not None and bp.numel() == M, "fused column sum does not land on a bias gradient")
                rc, ec = self._out(int(p["colsum"]), 1, M, M)
                self._note_write(bp, int(p["cacc"]), step_i, rnd)
                self.fused_bias[id(bp)] = self.fused_bias.get(id(bp), 0) + 1
            if self.numeric:          # tile by tile, as the items list them
                A, B = vals[i]
                c = self.shadow[r.base][e0:e0 + (M - 1) * ldc + N]
                c = np.lib.stride_tricks.as_strided(c, shape=(M, N), strides=(ldc * 8, 8))
                for _, tm, tn, _ in items[items[:, 0] == i]:
                    ms, ns_ = slice(tm * T, min(M, tm * T + T)), slice(tn * T, min(N, tn * T + T))
                    v = A[:, ms].T @ B[:, ns_]
                    c[ms, ns_] = c[ms, ns_] + v if p["acc"] else v
                    if int(p["colsum"]) and tn == 0:
                        cs = self.shadow[rc.base][ec:ec + M]
                        s = A[:, ms].sum(0)
                        cs[ms] = cs[ms] + s if p["cacc"] else s

    @staticmethod
    def _count(items, count, what):
        """count[prob][a, b] += 1 for every item (prob, a, b, pad), each item checked to lie inside its problem's grid"""
        _check(((items[:, 0] >= 0) & (items[:, 0] < len(count))).all(), what, "item names a missing problem")
        dims = np.array([c.shape for c in count], dtype=np.int64).reshape(-1, 2)
        d = dims[items[:, 0]]
        _check(((items[:, 1] >= 0) & (items[:, 1] < d[:, 0]) & (items[:, 2] >= 0) & (items[:, 2] < d[:, 1])).all(),
               what, "item outside its problem's grid")
        base = np.concatenate([[0], np.cumsum(dims[:, 0] * dims[:, 1])])
        flat = np.bincount(base[items[:, 0]] + items[:, 1].astype(np.int64) * d[:, 1] + items[:, 2], minlength=int(base[-1]))
        for i, c in enumerate(count):
            c += flat[base[i]:base[i + 1]].reshape(c.shape)

    def _sum_slices(self, ws, out, ns, numel, acc, step_i, rnd):
        _check(numel % 4 == 0 and ns >= 1, "evp_sum_slices_f32 contract")
        rw, ew = self._out(ws.data_ptr(), 1, ns * numel, ns * numel)
        for s in range(ns):
            _check(self.ws_written.pop((rw.base, ew + s * numel), 0) == 1, "workspace slice", s, "of", ns, "not written exactly once")
        ro, eo = self._out(out.data_ptr(), 1, numel, numel)
        gp = self._param_of(out.data_ptr())
        _check(gp is not None and gp.numel() == numel, "slice sum does not land on a gradient")
        self._note_write(gp, acc, step_i, rnd)
        if self.numeric:
            tot = self.shadow[rw.base][ew:ew + ns * numel].reshape(ns, numel).sum(0)
            o = self.shadow[ro.base][eo:eo + numel]
            o[...] = o + tot if acc else tot

    def _colsum(self, pt, it, n_items, step_i, rnd):
        probs = pt.numpy().view(CDT)
        items = it.numpy().view(np.int32).reshape(-1, 4)
        _check(items.shape[0] == n_items, "item count")
        count = [np.zeros(((int(p["N"]) + 127) // 128, (int(p["M"]) + 255) // 256), np.int64) for p in probs]
        self._count(items, count, "column-sum")
        for i, p in enumerate(probs):
            _check((count[i] == 1).all(), f"column-sum problem {i}: blocks not produced exactly once")
            M, N, ld = int(p["M"]), int(p["N"]), int(p["ld"])
            X = self._read(int(p["x"]), M, ld, N)
            rx, _ = self.resolve(int(p["x"]), "operand")
            _check(int(p["dtype"]) == (_lib.EVP_F32 if rx.obj.dtype == torch.float32 else _lib.EVP_BF16), "column-sum dtype code")
            ro, eo = self._out(int(p["out"]), 1, N, N)
            gp = self._param_of(int(p["out"]))
            _check(gp is not None and gp.numel() == N, "column sum does not land on a gradient")
            self._note_write(gp, 1, step_i, rnd)        # atomics: always accumulate (fresh outputs are zeroed)
            key = (id(gp), id(rx.obj))
            self.listed_bias[key] = self.listed_bias.get(key, 0) + 1
            if self.numeric:
                o = self.shadow[ro.base][eo:eo + N]
                for _, cb, rs, _ in items[items[:, 0] == i]:
                    cols = slice(cb * 128, min(N, cb * 128 + 128))
                    o[cols] += X[rs * 256:min(M, rs * 256 + 256), cols].sum(0)

    # ---------------------------------------------------------------- driver
    def run(self, steps):
        for p_ in {id(q[0]): q[0] for q in self.queue_w}.values():
            self.add_output(p_.grad, garbage=False)
        for q in self.queue_w:
            if q[6] is not None:
                self.add_output(q[6].grad, garbage=False)
        for p_, _ in self.queue_b:
            self.add_output(p_.grad, garbage=False)
        for st in steps:
            for f in st.flats:
                # GEMM flats come from torch.empty: garbage until written. The column-sum flat is zeroed (and re-zeroed by the step)
                self.add_output(f, garbage=st.entry != COLSUM)
            for ws, out, *_ in st.post:
                self.add_output(ws, garbage=True)
        for p_ in self.fresh_objects():
            self.valid[id(p_)] = False
        for i, st in enumerate(steps):
            rnd = getattr(st, "round", 0)
            for z in st.zero:
                if self.numeric:
                    self.shadow[z.untyped_storage().data_ptr()][:] = 0.0
            if st.entry == COLSUM:
                for z in st.flats:          # fresh outputs of the column sums are zeroed
                    for p_ in self.fresh_objects():
                        if p_.grad.untyped_storage().data_ptr() == z.untyped_storage().data_ptr():
                            self.valid[id(p_)] = True
                self._colsum(st.pt, st.it, st.n_items, i, rnd)
            else:
                _check(st.entry in TILE, "unknown entry", st.entry)
                self._gemm(st.entry, st.pt, st.it, st.n_items, i, rnd)
                for ws, out, ns, numel, acc in st.post:
                    self._sum_slices(ws, out, ns, numel, acc, i, rnd)
        self._final_checks()

    def fresh_objects(self):
        out = {}
        for q in self.queue_w:
            for p_ in (q[0], q[6]):
                if p_ is not None and id(p_) in self.fresh:
                    out[id(p_)] = p_
        for p_, _ in self.queue_b:
            if id(p_) in self.fresh:
                out[id(p_)] = p_
        return out.values()

    def _final_checks(self):
        _check(not self.ws_written, "workspace slices written but never reduced")
        # every queued contribution: its K-slices partition [0, rows) exactly, with the matching x rows
        for (param, dy, x, n_out, k_in, rows, bias) in self.queue_w:
            sl = sorted(self.slices.pop(id(dy), []))
            _check(sl, "a queued contribution was never computed", n_out, k_in, rows)
            k = 0
            for k0, K, xid in sl:
                _check(xid == id(x), "slice reads the wrong x")
                _check(k0 == k, f"K-slices of a {n_out}x{k_in} problem (rows {rows}) leave a gap or overlap at row {k} (slice at {k0})")
                k = k0 + K
            _check(k == rows, f"K-slices of a {n_out}x{k_in} problem cover {k} of {rows} rows")
        # every bias: produced exactly once per queued occurrence, fused or listed, never both
        expect_fused_or_listed = {}
        for q in self.queue_w:
            if q[6] is not None:
                expect_fused_or_listed.setdefault(id(q[6]), []).append(id(q[1]))
        for bid, dys in expect_fused_or_listed.items():
            fused = self.fused_bias.pop(bid, 0)
            listed = sum(self.listed_bias.pop((bid, d), 0) for d in dys)
            _check(fused + listed == len(dys), "bias produced", fused, "+", listed, "times for", len(dys), "contributions")
        for p_, x2d in self.queue_b:
            _check(self.listed_bias.pop((id(p_), id(x2d)), 0) == 1, "a queued column sum was not produced exactly once")
        _check(not self.fused_bias and not any(self.listed_bias.values()), "unexpected bias outputs")
        # steps of one round may run concurrently: they must write disjoint gradients
        for rnd, per_step in self.writers.items():
            seen = set()
            for s_ids in per_step.values():
                _check(not (seen & s_ids), f"two steps of round {rnd} write the same gradient")
                seen |= s_ids

    def grad(self, p_):
        st = p_.grad.untyped_storage()
        e0 = (p_.grad.data_ptr() - st.data_ptr()) // 4
        return torch.from_numpy(self.shadow[st.data_ptr()][e0:e0 + p_.numel()].copy()).view(p_.shape)


def snapshot_queue(d):
    """(w, b, fresh ids) of a _DeferredGrads queue before build_plan() / flush() consumes it."""
    fresh = set()
    for q in d.w:
        for p_ in (q[0], q[6]):
            if p_ is not None and p_.grad is None:
                fresh.add(id(p_))
    for p_, _ in d.b:
        if p_.grad is None:
            fresh.add(id(p_))
    return list(d.w), list(d.b), fresh


def interpret_plan(d, n_chunks, numeric=True, mutate=None):
    """Build the plan of `d`'s queue and run it through the interpreter. `mutate(steps)` may alter the tables first."""
    w, b, fresh = snapshot_queue(d)
    steps = d.build_plan(n_chunks)
    if mutate is not None:
        mutate(steps)
    it = Interpreter(w, b, fresh, numeric=numeric)
    it.run(steps)
    return it, steps


# -------------------------------------------------------------------- per-layer problem lists of the benchmarked models
def _layers(model):
    """(qualified name, module) of every Linear / pointwise-or-patch Conv2d whose weight gradient is a GEMM (depthwise
    convolutions have their own kernel)."""
    out = []
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.Linear) or (isinstance(m, torch.nn.Conv2d) and m.groups == 1):
            out.append((name, m))
    return out


def _rows_per_sample(model, name, phase, swin_geom):
    """Tokens per sample that layer `name` sees in the step (the row count of its dY and X) from the model's own geometry."""
    bb = model.backbone
    kind = type(bb).__name__
    masked = phase in ("rec", "rec+con")
    if name.startswith("pretrain_rec_decoder."):
        dec = model.pretrain_rec_decoder
        keep = int(dec.num_patches * (1 - bb.mask_ratio))
        return keep if name.endswith("patch_embed") else dec.num_patches
    if not name.startswith("backbone."):
        return 1                                        # contrastive heads: one row per sample
    sub = name[len("backbone."):]
    if kind == "ViT":
        L = bb.patch_embed.num_patches
        return int(L * (1 - bb.mask_ratio)) if masked else L
    if kind == "ConvViT":
        s1, s2 = bb.sizes[1], bb.sizes[2]
        L = bb.num_patches
        keep = int(L * (1 - bb.mask_ratio)) if masked else L
        if sub.startswith(("patch_embed1", "conv_block1")):
            return s1 * s1
        if sub.startswith(("patch_embed2", "conv_block2")):
            return s2 * s2
        return keep
    if kind == "SwinTransformer":
        if sub.startswith("patch_embed"):
            return swin_geom[0][1]
        if sub.startswith("swin_block."):
            parts = sub.split(".")
            i = int(parts[1])
            if parts[2] == "downsample":
                return swin_geom[i + 1][1]
            j = int(parts[3])
            mods = swin_geom[i][2]
            _, mode, gs, ng = mods[j % len(mods)]
            return gs * ng
        return swin_geom[-1][1]                         # stage*_output_decode: tokens of the last stage
    raise AssertionError(kind)


FUSED_FIRST = ("attn.qkv", "mlp.fc1", "conv1")        # the first Linear of each residual branch queues its bias with its weight


def model_queue(model, phase, B, d, make=None):
    """Fill the _DeferredGrads `d` with the weight / bias problems of one bf16 backward of `model` at batch B, the way the
    autograd functions queue them: the first Linear of a residual branch (qkv, fc1, conv1) with its bias fused, the second
    (proj, fc2, conv2) with its bias as a column sum of the LayerNorm backward's partial rows, LayerNorm weights / biases as
    partial-row column sums, every other layer with its bias as a column sum of dY. `make(rows, cols, dtype)` makes an
    operand (default: FakeOperand). Returns the parameters in queue order."""
    make = make or (lambda r, c, dt: FakeOperand(r, c, dt))
    swin_geom = None
    if type(model.backbone).__name__ == "SwinTransformer":
        from eventpretrain_amd.model.backbone.swin import StaticPatternPlan
        keep = int(model.backbone.num_patches * (1 - model.backbone.mask_ratio))
        swin_geom = StaticPatternPlan(model.backbone, "cpu", keep, slack=1.25).geom
    params = []
    for name, m in _layers(model):
        w = m.weight
        if not w.requires_grad:
            continue
        n_out, k_in = w.shape[0], w[0].numel()
        if n_out % 8 or k_in % 8:
            continue
        rows = B * _rows_per_sample(model, name, phase, swin_geom)
        dy, x = make(rows, n_out, torch.bfloat16), make(rows, k_in, torch.bfloat16)
        bias = m.bias if m.bias is not None and m.bias.requires_grad else None
        if bias is not None and name.endswith(FUSED_FIRST):
            d.w.append((w, dy, x, n_out, k_in, rows, bias))
        else:
            d.w.append((w, dy, x, n_out, k_in, rows, None))
            if bias is not None:
                part = name.endswith(("attn.proj", "mlp.fc2", "conv2"))
                d.b.append((bias, make(rows // 256 + 1, n_out, torch.float32) if part else dy))
        params += [w] + ([bias] if bias is not None else [])
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.LayerNorm) and m.weight.requires_grad:
            part = make(B * 4 + 1, m.weight.numel(), torch.float32)
            d.b.append((m.weight, part))
            d.b.append((m.bias, part))
            params += [m.weight, m.bias]
    return params


_MODELS = {}
# beside bench.py's six configurations: the small models (and the plumbing-size ViT-Tiny of BASELINE.json config 1)
EXTRA_CONFIGS = {"convvit_small_rec": ("convvit", "small", "rec", "pretrain_hub_model_small_patch16"),
                 "vit_small_rec": ("vit", "small", "rec", "pretrain_hub_model_small_patch16"),
                 "vit_tiny_rec": ("vit", "tiny", "rec", "pretrain_hub_model_tiny_patch16_64")}


def bench_model(config):
    """The model of one bench.py configuration, instantiated on the CPU (cached; its parameters never hold gradients here)."""
    if config not in _MODELS:
        import bench
        from eventpretrain_amd.model.pretrain import pr_hub_model as hub
        from eventpretrain_amd.testing import make_args
        if config in bench.CONFIGS:
            _, bb, size, phase, fac, _, _, _ = bench.CONFIGS[config]
        else:
            bb, size, phase, fac = EXTRA_CONFIGS[config]
        a = make_args(model_size=size, pr_phase=phase, backbone_type=bb, device="cpu", batch_size=2, use_queue=True,
                      mask_ratio=0.5 if phase == "rec" else 0.0)
        torch.manual_seed(0)
        m = getattr(hub, fac)(a, emb_frames_dim=512, queue_length=8, T=0.07)
        if phase == "adj":
            for k, v in m.backbone.named_parameters():
                if "norm_layer" not in k:
                    v.requires_grad = False
        _MODELS[config] = (m, phase)
    return _MODELS[config]

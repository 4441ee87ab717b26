"""Host-side launch trace of the residual-block autograd Functions (ViTBlockFn, ConvBlockFn, SwinBlockFn), no GPU: the Functions run
forward and backward on CPU tensors while every way ops.py reaches the device is replaced by a recorder. What is traced is what a
refactor of ops.py must keep: which kernel entries are called in which order, with which scalar arguments, on operands of which
shape and dtype, and which buffer feeds which launch; and what is queued for the deferred weight-gradient / column-sum launches.
No value is computed, so the traced code must not branch on tensor contents (it does not).

    python tests/launch_trace.py --write              regenerate tests/golden/block_launch_trace.json from this tree
    python tests/launch_trace.py --root DIR --write   ... importing eventpretrain_amd from another tree (DIR/eventpretrain_amd)
    python tests/launch_trace.py                      compare this tree with the golden file

One record per kernel entry: [entry, arg, ...] with scalars as they are and a tensor operand as [name, shape, dtype]. An operand is
named at its first appearance, by storage address and byte offset (inputs and parameters by the names the case gives them, the
rest t0, t1, ... in order of appearance); every tensor seen stays alive until the trace ends, so an address names one buffer. The
order of allocations therefore does not enter the trace. A gemm record is the call bound against ops.gemm's signature, arguments
that equal their default left out, so an omitted default and the same value passed explicitly give the same record. A flush of the
deferred queue is one record: ["deferred_flush", [wgrad ...], [colsum ...]], a weight gradient as [parameter shape, dy, x, n_out, k_in,
rows, bias-parameter shape | None] and a column sum as [parameter shape, operand].

Another autograd Function joins the trace as one more entry in CASES (and, for a new kind, a runner in RUNNERS)."""
import argparse
import difflib
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "block_launch_trace.json")

def _win_nchunk(Bg, nG, heads, target=512):
    """win_chunks of csrc/attention_fused.hip (tests/test_gpu_attention_truth.py holds this formula against the library's answer)."""
    B = Bg // nG
    per = -(-B // max(1, min(B, -(-target // (nG * heads)))))
    return -(-B // per)


# answers of the count queries (the entries that launch nothing and return a size): fixed here, the library is never loaded
COUNT_QUERIES = {
    "evp_layernorm_bwd_nblk": lambda M: 3,
    "evp_colsum_nblk": lambda M: 2,
    "evp_attention_fused_supported": lambda code, N, dh: int(code == 1 and N <= 224 and dh in (32, 64)),
    "evp_window_attention_fused_np": lambda N: 32 if N <= 32 else 64 if N <= 64 else 96 if N <= 96 else 128,
    "evp_window_attention_fused_nchunk": lambda Bg, nG, heads: _win_nchunk(Bg, nG, heads),
    "evp_dwconv5x5_bwd_nslab": lambda B, H, W: 5,
}
_STREAM = object()


class _Operand:
    """What the replaced ops.ptr hands to the replaced ops.call in place of a device address."""

    def __init__(self, t):
        self.t = t


class Recorder:
    def __init__(self):
        self.records, self._names, self._alive, self._n_given = [], {}, [], 0

    def name(self, t, given=None):
        key = (t.untyped_storage().data_ptr(), t.storage_offset() * t.element_size())
        if key not in self._names:
            self._names[key] = given or f"t{len(self._alive) - self._n_given}"
            self._n_given += given is not None
            self._alive.append(t)
        return self._names[key]

    def operand(self, t):
        return None if t is None else [self.name(t), list(t.shape), str(t.dtype).replace("torch.", "")]

    def arg(self, a):
        if isinstance(a, _Operand):
            return self.operand(a.t)
        if torch.is_tensor(a):
            return self.operand(a)
        if isinstance(a, (tuple, list)):
            return [self.arg(v) for v in a]
        return a


def trace(ops, body, switches=None, bf16=False):
    """Run body(ops, rec) with the device replaced by a Recorder -> its records. `switches`: module-level A/B flags of ops.py by
    attribute name, plus "deferred". Everything that was replaced or set is restored afterwards."""
    rec = Recorder()
    d = ops._deferred
    flags = ("_use_grad_side", "_use_fused_attention", "_use_window_mfma", "_use_wgrad_g4", "_wgrad_xcd_order", "_compute_dtype")
    saved = {k: getattr(ops, k) for k in ("call", "ptr", "stream_ptr", "_chk", "gemm") + flags}
    saved_d = (d.enabled, d.hold, d.__dict__.get("flush"))
    gemm_sig = inspect.signature(ops.gemm)

    def call(name, *args):
        rec.records.append([name] + [rec.arg(a) for a in args if a is not _STREAM])
        return COUNT_QUERIES[name](*args) if name in COUNT_QUERIES else 0

    def chk(t, dtype=None):
        assert t.is_contiguous() and (dtype is None or t.dtype == dtype), (t.shape, t.dtype, dtype)
        return t

    def gemm(*args, **kw):
        b = gemm_sig.bind(*args, **kw)
        b.apply_defaults()
        r = ["gemm"]
        for k, v in b.arguments.items():
            default = gemm_sig.parameters[k].default
            if default is inspect.Parameter.empty or torch.is_tensor(v) or v != default:
                r.append([k, rec.arg(v)])
        rec.records.append(r)
        return b.arguments["out"]

    def flush():
        d.armed = False
        w = [[list(q.param.shape), rec.name(q.dy), rec.name(q.x), q.n_out, q.k_in, q.rows, None if q.bias is None else list(q.bias.shape)]
             for q in d.w]
        b = [[list(p.shape), rec.name(x2d)] for p, x2d in d.b]
        d.w, d.b = [], []
        rec.records.append(["deferred_flush", w, b])

    try:
        ops.call, ops.ptr, ops.stream_ptr, ops._chk, ops.gemm = call, lambda t: None if t is None else _Operand(t), lambda: _STREAM, chk, gemm
        d.flush, d.hold, d.w, d.b, d.armed = flush, False, [], [], False
        for k in flags[:-1]:
            setattr(ops, k, True)
        d.enabled = True
        for k, v in (switches or {}).items():
            if k == "deferred":
                d.enabled = v
            else:
                assert k in flags, k
                setattr(ops, k, v)
        ops._compute_dtype = torch.bfloat16 if bf16 else torch.float32
        body(ops, rec)
        ops.flush_deferred_grads()
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        d.enabled, d.hold = saved_d[:2]
        if saved_d[2] is None:
            d.__dict__.pop("flush", None)
        else:
            d.flush = saved_d[2]
        d.w, d.b, d.armed = [], [], False
    return rec.records


# --------------------------------------------------------------------------------------------------------------- the cases
B, D, HEADS, HID, N, HW = 2, 64, 2, 256, 16, 4          # the smallest widths the gates allow: d_h = 32, 16 tokens / a 4 x 4 map


def _params(rec, tag, shapes, frozen=(), nonleaf=()):
    """name -> tensor, registered with the recorder as tag + name. Leaf Parameters; `frozen` without gradient, `nonleaf` the
    output of an operation on a Parameter (can_defer is false for it)."""
    out = {}
    for k, shape in shapes.items():
        p = torch.nn.Parameter(torch.zeros(shape), requires_grad=k not in frozen)
        out[k] = p * 1.0 if k in nonleaf else p
        rec.name(out[k], tag + k)
    return out


def _drop(ops, rec, kind, n_samples, rows, with_proj=True):
    """rd of a case: None, drop-path only ("path"), + dropout 0.25 from a seed ("seed") or from given masks ("masks"), or dropout on
    the attention probabilities ("attn")."""
    if kind is None:
        return None
    u1, u2 = torch.zeros(n_samples), torch.zeros(n_samples)
    rec.name(u1, "u1"), rec.name(u2, "u2")
    if kind == "path":
        return ops.BlockDrop(u1, u2, keep_prob=0.9)
    if kind == "attn":
        return ops.BlockDrop(u1, u2, keep_prob=0.9, seed=7, attn_drop=0.25)
    masks = None
    if kind == "masks":
        masks = {k: torch.ones(rows * w, dtype=torch.uint8) for k, w in (("proj", D), ("hidden", HID), ("fc2", D)) if with_proj or k != "proj"}
        for k, m in masks.items():
            rec.name(m, "mask." + k)
    return ops.BlockDrop(u1, u2, keep_prob=0.9, drop=0.25, seed=7, masks=masks)


def _finish(x, y):
    y = y[0] if isinstance(y, tuple) else y
    y.sum().backward()
    assert x.grad is not None


_ATTN_SHAPES = {"norm1.weight": (D,), "norm1.bias": (D,), "qkv.weight": (3 * D, D), "qkv.bias": (3 * D,), "proj.weight": (D, D),
                "proj.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,), "fc1.weight": (HID, D), "fc1.bias": (HID,),
                "fc2.weight": (D, HID), "fc2.bias": (D,)}


def run_vit(ops, rec, rd=None, want_attn=False, blocks=1, frozen=(), nonleaf=()):
    x = torch.zeros(B, N, D, requires_grad=True)
    rec.name(x, "x")
    t = x
    for i in range(blocks):
        p = _params(rec, f"b{i}." if blocks > 1 else "", _ATTN_SHAPES, frozen, nonleaf)
        t = ops.ViTBlockFn.apply(t, *p.values(), HEADS, 1e-6, want_attn, _drop(ops, rec, rd, B, B * N))
    _finish(x, t)


def run_conv(ops, rec, rd=None, keep_map=False):
    shapes = {"norm1.weight": (D,), "norm1.bias": (D,), "conv1.weight": (D, D, 1, 1), "conv1.bias": (D,), "attn.weight": (D, 1, 5, 5),
              "attn.bias": (D,), "conv2.weight": (D, D, 1, 1), "conv2.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,),
              "fc1.weight": (HID, D, 1, 1), "fc1.bias": (HID,), "fc2.weight": (D, HID, 1, 1), "fc2.bias": (D,)}
    x = torch.zeros(B, HW * HW, D, requires_grad=True)
    rec.name(x, "x")
    p = _params(rec, "", shapes)
    mask = None
    if keep_map:
        mask = torch.zeros(B, (HW // 2) * (HW // 2))
        rec.name(mask, "keep_map")
    y = ops.ConvBlockFn.apply(x, *p.values(), mask, 2 if keep_map else 1, HW, HW, _drop(ops, rec, rd, B, B * HW * HW, with_proj=False))
    _finish(x, y)


def run_swin(ops, rec, rd=None, groups=1, want_attn=False):
    Bg, R = B * groups, (2 * HW - 1) ** 2
    x = torch.zeros(Bg, N, D, requires_grad=True)
    rec.name(x, "x")
    table = torch.nn.Parameter(torch.zeros(R, HEADS))
    rel = torch.zeros(groups, N, N, dtype=torch.int32)
    rec.name(table, "table"), rec.name(rel, "rel")
    p = _params(rec, "", _ATTN_SHAPES)
    y = ops.SwinBlockFn.apply(x, table, rel, *p.values(), HEADS, 1e-5, want_attn, _drop(ops, rec, rd, Bg, Bg * N))
    _finish(x, y)


RUNNERS = {"vit": run_vit, "conv": run_conv, "swin": run_swin}


def _cases():
    """name -> (runner, bf16, switches, runner keywords)."""
    c = {}
    both = (("f32", False), ("bf16", True))
    for tag, bf in both:
        for rd in (None, "path", "seed", "masks", "attn"):
            c[f"vit_{tag}_rd_{rd or 'none'}"] = ("vit", bf, {}, dict(rd=rd))
        c[f"vit_{tag}_want_attn"] = ("vit", bf, {}, dict(want_attn=True))
        for rd in (None, "seed"):
            for keep_map in (True, False):
                c[f"conv_{tag}_rd_{rd or 'none'}_{'keep_map' if keep_map else 'no_map'}"] = ("conv", bf, {}, dict(rd=rd, keep_map=keep_map))
            for groups in (1, 2):
                c[f"swin_{tag}_rd_{rd or 'none'}_groups{groups}"] = ("swin", bf, {}, dict(rd=rd, groups=groups))
        c[f"swin_{tag}_want_attn"] = ("swin", bf, {}, dict(want_attn=True, groups=2))
        c[f"swin_{tag}_attn_drop"] = ("swin", bf, {}, dict(rd="attn", groups=2))
    c["vit_bf16_unfused_attention"] = ("vit", True, {"_use_fused_attention": False}, {})
    c["vit_bf16_undeferred"] = ("vit", True, {"deferred": False}, {})
    for side in (True, False):
        for deferred in (True, False):
            sw = {"_use_grad_side": side, "deferred": deferred}
            tag = f"side_{'on' if side else 'off'}_deferred_{'on' if deferred else 'off'}"
            c[f"vit_bf16_stacked_{tag}"] = ("vit", True, sw, dict(blocks=2))
            c[f"vit_bf16_stacked_frozen_{tag}"] = ("vit", True, sw, dict(blocks=2, frozen=("qkv.weight", "proj.bias", "fc2.bias")))
    c["vit_bf16_nonleaf_fc1_weight"] = ("vit", True, {}, dict(nonleaf=("fc1.weight",)))
    c["conv_bf16_undeferred"] = ("conv", True, {"deferred": False}, dict(keep_map=True))
    c["swin_bf16_window_lds"] = ("swin", True, {"_use_window_mfma": False}, dict(groups=2))
    return c


CASES = _cases()


def run_case(ops, name):
    kind, bf16, switches, kw = CASES[name]
    return trace(ops, lambda o, rec: RUNNERS[kind](o, rec, **kw), switches, bf16)


def lines(records):
    return [json.dumps(r, separators=(",", ":")) for r in records]


def dumps(traces):
    """The golden file's text: one record per line."""
    body = ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join(lines(v)) + "\n]" for k, v in traces.items())
    return "{\n" + body + "\n}\n"


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def diff(want, got, name):
    return "\n".join(difflib.unified_diff(lines(want), lines(got), f"golden/{name}", f"this tree/{name}", lineterm="", n=2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="write the golden file instead of comparing with it")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="tree to import eventpretrain_amd from (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from eventpretrain_amd import ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == os.path.abspath(a.root), ops.__file__
    traces = {name: run_case(ops, name) for name in CASES}
    if a.write:
        with open(GOLDEN, "w") as f:
            f.write(dumps(traces))
        print(f"wrote {len(traces)} cases, {sum(map(len, traces.values()))} records to {GOLDEN}")
        return 0
    golden = load_golden()
    bad = [n for n in CASES if json.loads(json.dumps(traces[n])) != golden.get(n)]
    for n in bad:
        print(diff(golden.get(n, []), traces[n], n))
    print(f"{len(CASES) - len(bad)} of {len(CASES)} cases equal the golden file")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

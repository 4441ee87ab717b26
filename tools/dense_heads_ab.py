#!/usr/bin/env python3
"""Timing record of the dense-prediction heads: decode_head (UPerNet) + auxiliary_head (FCN) of eventpretrain_amd.model.finetune_dense
(csrc/dense.hip + the GEMM), forward + backward, bf16, inside a captured graph, for ViT-Small / ViT-Base maps (four [B, 384 | 768, 14,
14]) at batch 2 and 8; each configuration in a process of its own, `--rounds` times; per process: warm-up, capture, then events around
each of `--replays` replays; the record is the median with min - max. A record, not a gate.

The other side of the intended A/B -- the same two heads from plain torch.nn modules under torch.autocast("cuda", bfloat16) -- is not
here: its process (torch.nn modules only, none of this project's kernels) ended with a segmentation fault on the MI355X, the cause was
not found, and it was taken out; a comparison has to wait for that.

    python tools/dense_heads_ab.py [--rounds 2] [--replays 60] > profiles/dense_heads_ab.txt

The weight gradients of the hip side run as the plain per-layer GEMMs here (ops.set_deferred_grads(False)): the grouped launch a whole
training step defers them to belongs to engine.GraphedStep, not to the heads."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(impl, size, batch, replays):
    import torch
    from eventpretrain_amd import ops
    from eventpretrain_amd.testing import det_normalish, make_args
    cin, n_cls = {"small": 384, "base": 768}[size], 11
    dev = "cuda"
    xs = [det_normalish(f"ab.x{i}", (batch, 196, cin)).to(dev).requires_grad_(True) for i in range(4)]
    w1, w2 = (det_normalish(f"ab.w{i}", (batch, n_cls, 14, 14)).to(dev) for i in range(2))
    if impl == "hip":
        from eventpretrain_amd.model.finetune_dense import ft_dense_decoder as dec
        a = make_args(sample_mode="bilinear")
        heads = torch.nn.ModuleList([dec.__dict__["finetune_decode_head_" + size](a, out_channels=n_cls),
                                     dec.__dict__["finetune_auxiliary_head_" + size](a, out_channels=n_cls)]).to(dev).train()
        ops.set_compute_dtype(torch.bfloat16)
        ops.set_deferred_grads(False)

        def run():
            maps = [t.reshape(batch, 14, 14, cin).permute(0, 3, 1, 2) for t in xs]
            d, x = heads[0](maps), heads[1](maps)
            ((d * w1).sum() + 0.4 * (x * w2).sum()).backward()
    else:
        raise SystemExit("only --impl hip exists (see the module docstring)")

    def zero():
        for p in list(heads.parameters()) + xs:
            p.grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
            zero()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    print(json.dumps(dict(impl=impl, size=size, batch=batch, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times),
                          replays=replays)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=("hip",))
    ap.add_argument("--size", default="small")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--replays", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.impl:
        return child(a.impl, a.size, a.batch, a.replays)
    print("# dense heads: decode_head + auxiliary_head, forward + backward, bf16, captured graph; ms per replay, median (min - max)")
    for size in ("small", "base"):
        for batch in (2, 8):
            for r in range(a.rounds):
                for impl in ("hip",):
                    cmd = [sys.executable, os.path.abspath(__file__), "--impl", impl, "--size", size, "--batch", str(batch), "--replays", str(a.replays)]
                    try:
                        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
                    except subprocess.TimeoutExpired:
                        print(f"{size} B={batch} round {r} {impl}: no result within {a.child_timeout} s; stopping", flush=True)
                        return 1
                    if out.returncode != 0:
                        print(f"{size} B={batch} round {r} {impl}: exit {out.returncode}; stopping\n{out.stderr[-1500:]}", flush=True)
                        return 1
                    d = json.loads(out.stdout.strip().splitlines()[-1])
                    print(f"{size:5s} B={batch} round {r} {impl:5s} {d['median_ms']:.3f} ({d['min_ms']:.3f} - {d['max_ms']:.3f}) ms over {d['replays']} replays",
                          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

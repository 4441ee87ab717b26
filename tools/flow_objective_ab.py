#!/usr/bin/env python3
"""Timing record of the optical-flow objective (csrc/flow.hip through ops.FlowObjectiveFn): both heads' masked L1 loss from their
low-resolution predictions, forward + backward, as one captured graph, against the same objective written in plain torch ops on
ops.resize_map (the resize kernel of the dense heads, then the two scale factors, the mask, abs and mean as torch ops, autograd).
Shape: B = 2, 14 x 14 -> 260 x 346 (MVSEC); the maps are column slices of matrices padded to 8 columns, as DenseClsFn hands them out.
One process per line: warm-up, capture, then events around each of `--replays` replays; median (min - max).

    python tools/flow_objective_ab.py [--replays 60] [--out profiles/flow_objective_ab.txt]

The fused figure is written (and flushed) first; the torch process runs after it. If a process does not end cleanly that is written
down, its line is left out and nothing is run again. The fused process also records which of the library's entries one step of the
objective calls (eager, uncaptured): each evp_flow_objective_fwd is two launches (pixel pass, finish), each evp_flow_objective_bwd one."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = dict(mvsec=dict(B=2, ld=8, h=14, w=14, H=260, W=346, max_flow=400.0))
WEIGHTS = (1.0, 0.4)          # decode_loss_weight, aux_loss_weight


def child(impl, shape, replays):
    import torch
    from eventpretrain_amd import ops
    from eventpretrain_amd.testing import det_normalish, det_uniform
    s = SHAPES[shape]
    B, ld, h, w, H, W, max_flow = (s[k] for k in ("B", "ld", "h", "w", "H", "W", "max_flow"))
    dev = "cuda"
    bufs = [torch.zeros(B * h * w, ld, device=dev) for _ in range(2)]
    for i, b in enumerate(bufs):
        b[:, :2] = (det_normalish(f"ab.flow.{i}", (B * h * w, 2)) * 10.0).to(dev)
    maps = [b[:, :2].requires_grad_(True) for b in bufs]
    target = (det_normalish("ab.flow.target", (B, 2, H, W)) * 200.0).to(dev)
    valid = (det_uniform("ab.flow.valid", (B, 1, H, W), 0.0, 1.0) >= 0.3).float().to(dev)
    calls = []
    if impl == "fused":
        def loss_of(m):
            return ops.FlowObjectiveFn.apply(m, B, h, w, target, valid, max_flow)
    else:
        factors = torch.tensor([W / w, H / h], device=dev)
        # the mask and its count depend on the labels alone: made once, outside the timed graph (boolean indexing cannot be captured)
        mask = ((valid >= 0.5) & (target.pow(2).sum(1, keepdim=True).sqrt() < max_flow)).float()
        inv = 1.0 / (2.0 * mask.sum())

        def loss_of(m):
            p = (ops.resize_map(m, B, h, w, H, W) * factors).view(B, H, W, 2).permute(0, 3, 1, 2)
            return ((p - target).abs() * mask).sum() * inv

    def run():
        total = WEIGHTS[0] * loss_of(maps[0]) + WEIGHTS[1] * loss_of(maps[1])
        total.backward()
        return total

    def zero():
        for m in maps:
            m.grad = None

    if impl == "fused":           # which entries one eager step calls
        real = ops.call
        ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        run()
        zero()
        ops.call = real
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
        total = run()
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
    launching = [c for c in calls if c != "evp_flow_nblk"]
    print(json.dumps(dict(impl=impl, shape=shape, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), replays=replays,
                          loss=total.item(), entries=launching,
                          launches=sum(2 if c == "evp_flow_objective_fwd" else 1 for c in launching))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=("fused", "torch"))
    ap.add_argument("--shape", default="mvsec")
    ap.add_argument("--replays", type=int, default=60)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_objective_ab.txt"))
    a = ap.parse_args()
    if a.impl:
        return child(a.impl, a.shape, a.replays)
    out = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        os.fsync(out.fileno())
    say("# flow objective, both heads, forward + backward, float32, one captured graph; ms per replay, median (min - max)")
    medians = {}
    for impl in ("fused", "torch"):
        for shape, s in SHAPES.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--impl", impl, "--shape", shape, "--replays", str(a.replays)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                say(f"{shape} {impl}: no result within {a.child_timeout} s; line left out, nothing is run again")
                return 1
            if res.returncode != 0:
                say(f"{shape} {impl}: the process ended with exit status {res.returncode}; line left out, nothing is run again")
                sys.stderr.write(res.stderr[-1500:])
                return 1
            d = json.loads(res.stdout.strip().splitlines()[-1])
            medians[(impl, shape)] = d["median_ms"]
            say(f"{shape:5s} B={s['B']} {s['h']}x{s['w']} -> {s['H']}x{s['W']}  {impl:5s} {d['median_ms']:.4f} ({d['min_ms']:.4f} - {d['max_ms']:.4f}) ms "
                f"over {d['replays']} replays, loss {d['loss']:.6f}")
            if impl == "fused":
                say(f"{shape:5s} fused: library entries of one step {d['entries']}: {d['launches']} launches for two heads")
    for shape in SHAPES:
        say(f"{shape:5s} torch / fused = {medians[('torch', shape)] / medians[('fused', shape)]:.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

#!/usr/bin/env python3
"""Timing record of the segmentation objective (csrc/semseg.hip through ops.SemsegObjectiveFn): both heads' cross entropy + Dice from
their low-resolution logits, forward + backward, as one captured graph, against the same objective written in plain torch ops on the
device (F.interpolate to the label size, F.cross_entropy, softmax / one-hot Dice, autograd). Shapes: B = 2, 11 classes, 14 x 14 ->
440 x 640 (DSEC) and 6 classes -> 200 x 346 (DDD17); the maps are column slices of matrices padded to 16 / 8 columns, as DenseClsFn
hands them out. One process per line: warm-up, capture, then events around each of `--replays` replays; median (min - max).

    python tools/semseg_objective_ab.py [--replays 60] [--out profiles/semseg_objective_ab.txt]

The fused figures of every shape are written (and flushed) first; the torch processes run after them. If a torch process does not end
cleanly that is written down, its line is left out and nothing is run again. The fused process also records which of the library's
entries one step of the objective calls (eager, uncaptured): each evp_semseg_objective_fwd is two launches (pixel pass, finish), each
evp_semseg_objective_bwd one."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = dict(dsec=dict(B=2, C=11, ld=16, h=14, w=14, H=440, W=640), ddd17=dict(B=2, C=6, ld=8, h=14, w=14, H=200, W=346))
WEIGHTS = (1.0, 0.4)          # decode_loss_weight, aux_loss_weight


def child(impl, shape, replays):
    import torch
    import torch.nn.functional as F
    from eventpretrain_amd.testing import det_normalish, det_uniform
    s = SHAPES[shape]
    B, C, ld, h, w, H, W = (s[k] for k in ("B", "C", "ld", "h", "w", "H", "W"))
    dev = "cuda"
    bufs = [torch.zeros(B * h * w, ld, device=dev) for _ in range(2)]
    for i, b in enumerate(bufs):
        b[:, :C] = (det_normalish(f"ab.semseg.{i}", (B * h * w, C)) * 3.0).to(dev)
    maps = [b[:, :C].requires_grad_(True) for b in bufs]
    label = (det_uniform("ab.semseg.label", (B, 1, H, W), 0.0, 1.0) * C).floor().clamp(0, C - 1).long()
    label[det_uniform("ab.semseg.ignore", (B, 1, H, W), 0.0, 1.0) < 0.2] = 255
    label = label.to(dev)
    calls = []
    if impl == "fused":
        from eventpretrain_amd import ops

        def loss_of(m):
            ce, dice = ops.SemsegObjectiveFn.apply(m, B, h, w, label, 255)
            return ce + dice
    else:
        def loss_of(m):
            z = F.interpolate(m.view(B, h, w, C).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
            ce = F.cross_entropy(z, label[:, 0], ignore_index=255)
            valid = label != 255
            hot = torch.zeros_like(z).scatter_(1, label * valid, 1.0) * valid
            p = torch.softmax(z, 1) * valid
            num = 2.0 * (p * hot).flatten(2).sum((0, 2)) + 1.0
            den = (p * p + hot * hot).flatten(2).sum((0, 2)) + 1.0
            return ce + (1.0 - num / den).mean()

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
    launching = [c for c in calls if c != "evp_semseg_nblk"]
    print(json.dumps(dict(impl=impl, shape=shape, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), replays=replays,
                          loss=total.item(), entries=launching,
                          launches=sum(2 if c == "evp_semseg_objective_fwd" else 1 for c in launching))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=("fused", "torch"))
    ap.add_argument("--shape", default="dsec")
    ap.add_argument("--replays", type=int, default=60)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semseg_objective_ab.txt"))
    a = ap.parse_args()
    if a.impl:
        return child(a.impl, a.shape, a.replays)
    out = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        os.fsync(out.fileno())
    say("# segmentation objective, both heads, forward + backward, float32, one captured graph; ms per replay, median (min - max)")
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
            say(f"{shape:5s} B={s['B']} C={s['C']} {s['h']}x{s['w']} -> {s['H']}x{s['W']}  {impl:5s} {d['median_ms']:.4f} ({d['min_ms']:.4f} - {d['max_ms']:.4f}) ms "
                f"over {d['replays']} replays, loss {d['loss']:.6f}")
            if impl == "fused":
                say(f"{shape:5s} fused: library entries of one step {d['entries']}: {d['launches']} launches for two heads")
    for shape in SHAPES:
        say(f"{shape:5s} torch / fused = {medians[('torch', shape)] / medians[('fused', shape)]:.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

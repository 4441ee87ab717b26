#!/usr/bin/env python3
"""Writes tests/golden/mvsec_gt_flow.npz: MVSEC's flow label as the REFERENCE's own FinetuneMVSECSeqDataset.gen_correspond_gt_flow
(dataset/finetune_flow/ft_mvsec_dataset.py:121-188) computes it, called on a bare instance (no files are opened) with the slice its
__getitem__ takes (:264-272), for the cases of tests/mvsec_flow_truth.py (13 x 17 frames, F in {1 direct, 1 two-hop, 2, 2 at the edge
t2 == ts[left + 1], 3, 4, 6}, float32 and float64 frames). Per case: the label, the slice (left, right), and the hops the reference's
prop_flow was called with -- which frame, in the order of the calls, and the scale_factor it was handed -- or, in the direct branch,
pre_dt / gt_dt as the formula gives it. The inputs are mvsec_flow_truth.case_inputs' deterministic fills and are not stored.

Two modules the reference imports at the top of that file are not needed to run the function and may be missing where this runs: h5py
(never called: the instance is bare) and cv2, of which only remap(src, map_x, map_y, INTER_NEAREST) is called. Both get in-memory
stand-ins. THE STAND-IN FOR remap STATES OpenCV's NEAREST RULE AS READ FROM ITS SOURCE -- cvRound (half to even) of each coordinate,
constant border 0 -- and has not been compared with a real cv2: the fixture pins the reference's arithmetic, order of reads, masks,
promotions and branch test, not that rule. Where a real cv2 imports, it is used instead and the output says so.

Asserted below: every propagated case meets a zero in one plane only (both ways), pixels that leave the frame on the first hop and
(three hops and more) on a later one, and (every case but F2_real, whose scales are what real timestamps leave) ties of both parities.
Data only: nothing of the reference is copied.

    EVP_REFERENCE=/path/to/reference python tools/gen_mvsec_flow_golden.py"""
import importlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from oracle import gen_golden  # noqa: E402
import mvsec_flow_truth as truth  # noqa: E402


def _remap_nearest(src, map_x, map_y, interpolation):
    assert interpolation == 0 and src.ndim == 2 and map_x.dtype == np.float32 and map_y.dtype == np.float32
    ix, iy = np.rint(map_x), np.rint(map_y)                 # cvRound: half to even
    ok = (ix >= 0) & (ix < src.shape[1]) & (iy >= 0) & (iy < src.shape[0])
    out = np.zeros(map_x.shape, src.dtype)                  # BORDER_CONSTANT, value 0
    out[ok] = src[iy[ok].astype(np.int64), ix[ok].astype(np.int64)]
    return out


def _standins():
    """-> "cv2" | "stand-in": which remap the fixture is made with."""
    used = "cv2"
    try:
        importlib.import_module("cv2")
    except ImportError:
        sys.modules["cv2"] = types.SimpleNamespace(remap=_remap_nearest, INTER_NEAREST=0)
        used = "stand-in"
    for name in ("h5py", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)      # imported at the top of the reference's file, never called here
    return used


def main():
    gen_golden._ref()
    remap = _standins()
    from dataset.finetune_flow.ft_mvsec_dataset import FinetuneMVSECSeqDataset
    ds = FinetuneMVSECSeqDataset.__new__(FinetuneMVSECSeqDataset)
    arrays = {"cases": np.array(truth.CASES), "remap": np.array(remap)}
    for name in truth.CASES:
        frames, ts, t1, t2 = truth.case_inputs(name)
        left, right = truth.flow_slice(ts, t1, t2)
        assert left <= right and left < len(ts) and right < len(ts)
        flows, flows_ts = frames[left:right].copy(), ts[left:right + 1]      # (the direct branch scales flows[0] in place)
        calls = []
        inner = FinetuneMVSECSeqDataset.prop_flow

        def recorded(x_flow, y_flow, *rest, scale_factor=1.0, _flows=flows):
            if rest[4:]:
                scale_factor, rest = rest[4], rest[:4]
            which = [i for i in range(len(_flows)) if np.shares_memory(_flows[i][0], x_flow) and np.shares_memory(_flows[i][1], y_flow)]
            assert len(which) == 1
            calls.append((left + which[0], np.float64(scale_factor)))
            return inner(ds, x_flow, y_flow, *rest, scale_factor)
        ds.prop_flow = recorded
        out = ds.gen_correspond_gt_flow(flows, flows_ts, t1, t2)
        if calls:
            assert out.dtype == np.float32
            hop_frames, hop_scales, n_hops = [c[0] for c in calls], [c[1] for c in calls], len(calls)
            stats = {}
            truth.label(frames, ts, t1, t2, stats=stats)
            exact = truth.case_times(name.split(".")[0])[3] is not None      # (F2_real: both scales as real timestamps leave them, no tie)
            need = ["zero_x_only", "zero_y_only", "left_first"] + (["tie_even", "tie_odd"] if exact else []) + (["left_later"] if n_hops >= 3 else [])
            assert all(stats.get(k, 0) > 0 for k in need), (name, stats)
        else:
            assert out.dtype == frames.dtype
            hop_frames, hop_scales, n_hops = [left], [(t2 - t1) / (flows_ts[1] - flows_ts[0])], 0
            stats = {}
        arrays[f"{name}|label"] = out
        arrays[f"{name}|slice"] = np.array([left, right], np.int64)
        arrays[f"{name}|hop_frames"] = np.array(hop_frames, np.int64)
        arrays[f"{name}|hop_scales"] = np.array(hop_scales, np.float64)
        arrays[f"{name}|n_hops"] = np.array(n_hops, np.int64)
        print(f"{name:<20s} slice [{left}, {right})  n_hops {n_hops}  scales {[float(s) for s in hop_scales]}  {stats}")
    print(f"remap: {remap}")
    gen_golden.save("mvsec_gt_flow", **arrays)


if __name__ == "__main__":
    main()

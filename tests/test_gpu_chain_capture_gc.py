"""CapturedChain keeps the cyclic garbage collector out of its graph capture. torch.cuda.graph no longer collects on entry, and a dead
reference cycle that owns GPU resources -- a loader whose pack raised is held by its own traceback, with its pinned slots, streams and
captured graph -- released by a collection that happens to start INSIDE the capture aborts the process. The chain therefore collects
before it captures and suspends the collector until the capture has ended. Checked here without any dead cycle at hand: what the
collector's state is while the chain's launches are being captured, and that it is restored."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_collector_is_off_inside_the_capture_and_restored_after(monkeypatch):
    from eventpretrain_amd.dataset.pretrain import gpu_input_pipeline as gip
    from eventpretrain_amd.dataset.finetune_dense.gpu_dense_loader import GpuDenseLoader
    from eventpretrain_amd.testing import make_args
    seen, collected = [], []
    inner = gip.CapturedChain._launches

    def watched(self):
        seen.append((bool(torch.cuda.is_current_stream_capturing()), gc.isenabled()))
        return inner(self)
    monkeypatch.setattr(gip.CapturedChain, "_launches", watched)
    monkeypatch.setattr(gip.gc, "collect", lambda *a: collected.append(bool(torch.cuda.is_current_stream_capturing())) or 0)
    a = make_args(phase="finetune_flow", crop_min=0.8, input_size=32, num_bins=5, fix_events_num=500, val_fix_events_num=500, device="cuda")
    assert gc.isenabled()
    loader = GpuDenseLoader(a, [], 2, 1, True, "flow", (20, 30), seed=1)
    assert loader.chain is not None and gc.isenabled()
    assert seen == [(False, True), (True, False)]              # the warm-up, then the capture
    assert collected == [False]                                 # one collection, before the capture began
    gc.disable()
    try:                                                        # a caller that runs with the collector off keeps it off
        GpuDenseLoader(a, [], 2, 1, True, "flow", (20, 30), seed=1)
        assert not gc.isenabled()
    finally:
        gc.enable()

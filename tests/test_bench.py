"""bench.py's plain run and its --dump-outputs files (the writer on the host; a plain run end to end on the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ["loss.npy", "weights_checksums.npy", "weights_sample.npy"]


def test_dump_outputs_writes_the_loss_and_a_fixed_sample_of_every_parameter(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(100, 80), torch.nn.Linear(80, 3))
    loss = torch.tensor(1.25)
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), loss, m)
    assert sorted(os.listdir(tmp_path / "a")) == DUMPED
    for name in DUMPED:       # the sample positions depend on nothing but the parameter shapes
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
    lo, sample, sums = (np.load(tmp_path / "a" / n) for n in ("loss.npy", "weights_sample.npy", "weights_checksums.npy"))
    assert lo.dtype == np.float64 and lo.tolist() == [1.25]
    params = [p.detach() for p in m.parameters()]
    assert sample.dtype == np.float32 and sample.shape == (bench.DUMP_SAMPLE + 80 + 240 + 3,)
    assert np.isin(sample[:bench.DUMP_SAMPLE], params[0].numpy().ravel()).all()      # sampled elements of the 8000-element weight
    assert np.array_equal(sample[bench.DUMP_SAMPLE:], torch.cat([p.reshape(-1) for p in params[1:]]).numpy())   # small ones whole
    want = np.array([[p.double().sum().item(), p.double().abs().sum().item(), (p.double() ** 2).sum().item()] for p in params])
    assert sums.dtype == np.float64 and np.allclose(sums, want, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_what_they_computed(tmp_path):
    """A plain run prints the headline line only (nothing that --full adds), `steps` timed steps, and --dump-outputs writes what
    the last of them computed; two runs with the same arguments start from the same inputs and agree."""
    lines = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8",
                            "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / tag)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["value"] == pytest.approx(8 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("ms_per_step_median", "roofline", "voxel", "loader_chain", "end_to_end", "cpu_baseline"):
        assert k not in d, k
    for tag, line in zip(("a", "b"), lines):
        assert sorted(os.listdir(tmp_path / tag)) == DUMPED
        assert sum(os.path.getsize(tmp_path / tag / n) for n in DUMPED) <= 64 << 20
        lo = np.load(tmp_path / tag / "loss.npy")
        assert lo.dtype == np.float64 and lo[0] == line["final_loss"]
    la, lb = (np.load(tmp_path / t / "loss.npy")[0] for t in ("a", "b"))
    assert lb == pytest.approx(la, rel=1e-3)
    wa, wb = (np.load(tmp_path / t / "weights_sample.npy") for t in ("a", "b"))
    assert wa.dtype == np.float32 and wa.shape == wb.shape and np.isfinite(wa).all()
    # the step's float-atomic reductions differ run to run in the last bits; an AdamW step (lr = 1e-3 * 8 / 256) moves a weight by about
    # lr at most, so a near-zero gradient whose sign flips between the runs parts the two by a few lr over the 3 steps
    assert np.allclose(wa, wb, rtol=1e-3, atol=5e-4)

"""The two forms of K1 (csrc/voxel.hip) share one row visit, one slab schedule and one flush. Pinned here: the plain form with float64
cells (algo 3) on every golden case, both column orders -- an instantiation no other test runs -- and the fused form WITHOUT decisions
(nothing erased, nothing added, no view) against the plain form on the same rows: equal bit for bit with float64 cells, where both sum
the same float32 addends into float64 and round once, and within 2e-5 with float32 cells (each within 1e-5 of the oracle).

Shapes (tools/voxel_digest.py builds them): bins 5 at 100 x 224 and 100 x 222 with max_window 3000 -- two y-tiles with float64 cells,
one with float32, the float4 and the scalar flush; a clip with two stamps swapped across regions (repair pass), one of 3400 rows (rows
behind the bitmap, list search with an empty list), an empty one; 3 clips and 8 (the two block -> clip maps); a 20 x 24 grid with
500-row clips at bins 2 (one workgroup, two jobs) and bins 6 (even count: the other pairing of the slabs); sensor 100 x 224 scaled by
(0.5, 0.5) into 50 x 112."""
import numpy as np
import pytest

from conftest import load_golden
from helpers import jl

pytestmark = pytest.mark.gpu

K1_TOL = 1e-5                    # the project's K1 bound against the oracle's sequential float32 sum


def test_plain_form_float64_cells_on_every_golden_case():
    from oracle.voxel_oracle import voxel_grid
    from tools.voxel_digest import run_plain
    d = load_golden("voxel")
    assert np.array_equal(run_plain([d["kat_events"]], 5, (4, 4), 3)[0], d["kat_grid"])
    orders = set()
    for c in jl(d["cases"]):
        ev, size = d[c["tag"] + "_events"], (c["H"], c["W"])
        want = voxel_grid(ev, c["bins"], size, c["is_txyp"])
        orders.add(bool(c["is_txyp"]))
        for t in (0, 1, 5):
            kw = dict(is_txyp=c["is_txyp"], tile_rows=min(t, c["H"]))
            g = run_plain([ev], c["bins"], size, 3, **kw)[0]
            err_fix, err_orc = float(np.abs(g - d[c["tag"] + "_grid"]).max()), float(np.abs(g - want).max())
            print(f"{c['tag']} tile_rows {t}: |f64 cells - fixture| {err_fix:.3e}, |f64 cells - oracle| {err_orc:.3e}")
            assert err_fix <= K1_TOL and err_orc <= K1_TOL, (c["tag"], t, err_fix, err_orc)
            assert np.array_equal(g, run_plain([ev], c["bins"], size, 3, **kw)[0]), (c["tag"], t)
    assert orders == {False, True}          # both column orders are among the cases


def _shapes():
    from tools.voxel_digest import shapes
    return shapes()


@pytest.mark.parametrize("index", range(7), ids=["100x224-3clips", "100x224-8clips", "100x222-3clips", "100x222-8clips", "20x24-bins2",
                                                 "20x24-bins6", "scaled-50x112"])
def test_fused_form_without_decisions_equals_the_plain_form(index):
    from tools.voxel_digest import run_fused, run_plain
    tag, clips, bins, size, scale, max_window = _shapes()[index]
    for algo in (3, 0):
        fused = run_fused(clips, bins, size, algo, max_window, scale or (1.0, 1.0))
        plain = run_plain(clips, bins, size, algo, scale=scale)
        diff = float(np.abs(fused - plain).max())
        print(f"{tag} algo {algo}: max |fused - plain| {diff:.3e}")
        if algo == 3:
            assert np.array_equal(fused, plain), (tag, int((fused != plain).sum()), diff)
        else:
            assert diff <= 2 * K1_TOL, (tag, diff)
        for i, ev in enumerate(clips):
            assert (float(np.abs(fused[i]).max()) == 0.0) == (ev.shape[0] == 0), (tag, i)
            assert (float(np.abs(plain[i]).max()) == 0.0) == (ev.shape[0] == 0), (tag, i)

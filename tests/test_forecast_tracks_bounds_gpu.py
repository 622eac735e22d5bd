"""GPU: WHERE the forecast-track kernels write -- mcd_forecast_assemble and mcd_denormalize_poses under the instrument of
tests/test_buffer_bounds_gpu.py: every device buffer the wrappers allocate (the three outputs and the list workspace; the output
rows) lies between guard bands with a poisoned interior, the inputs are passed between bands of NaNs / all-ones integers and of
finite random bits, and after the call (a) no guard byte changed, (b) no output element was left unwritten, (c) / (d) every output
equals the call outside the region bit for bit.  Shapes: the partial-workgroup ones of tests/test_forecast_tracks_gpu.py."""
import numpy as np
import pytest
import torch

import forecast_ref as FR
import test_buffer_bounds_gpu as BB
from dataset_spec import stress_rows
from test_buffer_bounds_gpu import DEV, run

pytestmark = pytest.mark.gpu

# the audit at the end of tests/test_buffer_bounds_gpu.py lists the entries exercised between guard bands; the two new ones are
# exercised HERE with that module's `run`, so this module adds them when it is imported (tests/test_error_maps_bounds_gpu.py)
NEW_ENTRIES = ["mcd_forecast_assemble", "mcd_denormalize_poses"]
BB.COVERED += [e for e in NEW_ENTRIES if e not in BB.COVERED]


@pytest.mark.parametrize("Tx", [1, 3, 12])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_forecast_assemble(N, Tx):
    """cells -2 .. n_cells + 1: a store through a cell outside the output would land in a guard band; max_cover 6 at N = 257 leaves
    cells whose list is full (a claim past the list's end would land in the next cell's words, or behind the workspace)"""
    from mocodad_amd.engine import forecast_assemble
    rng = np.random.default_rng(100 * N + Tx)
    poses = torch.from_numpy(rng.normal(size=(N, 2, Tx, 17)).astype(np.float32))
    n_cells = max(2, N * Tx // 5)
    cell = torch.from_numpy(rng.integers(-2, n_cells + 2, size=(N, Tx)).astype(np.int32))
    max_cover = 6 if N == 257 else 32

    def call(T, poses, cell):
        pose, count, spread = forecast_assemble(poses, cell, n_cells, method="median", spread_method="median", max_cover=max_cover)
        return {"pose": pose, "count": count, "spread": spread}

    r = run("mcd_forecast_assemble", call, {"poses": poses, "cell": cell})
    want = FR.assemble(poses.numpy(), cell.numpy(), n_cells, "median", "median", max_cover)
    assert np.array_equal(r["count"].cpu().numpy(), want[1])
    assert np.array_equal(FR.bits(r["pose"].cpu().numpy()), FR.bits(want[0]))
    assert np.array_equal(FR.bits(r["spread"].cpu().numpy()), FR.bits(want[2]))
    if N == 257:
        assert (want[1] > max_cover).any()


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_denormalize_poses(n, scaled):
    from mocodad_amd.engine import denormalize_poses
    rng = np.random.default_rng(400 + n)
    raw = torch.from_numpy(stress_rows(n, seed=40 + n))
    norm = torch.from_numpy(rng.normal(size=(n, 34)).astype(np.float32))
    count = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32))
    center, scale = (rng.normal(0, 0.2, 34), rng.uniform(0.5, 2.0, 34)) if scaled else (None, None)
    r = run("mcd_denormalize_poses", lambda T, norm, raw, count: {"out": denormalize_poses(norm, raw, (640, 360), center, scale, count)},
            {"norm": norm, "raw": raw, "count": count})
    want = FR.denormalize(norm.numpy(), raw.numpy(), (640, 360), center, scale, count.numpy())
    assert np.array_equal(FR.bits(r["out"].cpu().numpy()), FR.bits(want))


def test_the_new_entries_were_exercised_here():
    """What the audit's list is told above is true: each new entry saw guarded allocations under `run` in this module."""
    for e in NEW_ENTRIES:
        assert e in BB.ALLOC and BB.ALLOC[e], (e, sorted(BB.ALLOC))

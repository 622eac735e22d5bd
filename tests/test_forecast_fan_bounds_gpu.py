"""GPU: WHERE the forecast-fan kernels write -- mcd_forecast_fan under the instrument of tests/test_buffer_bounds_gpu.py: every
device buffer engine.forecast_fan allocates (the five outputs and the list workspace) lies between guard bands with a poisoned
interior, the inputs (poses_all, cell, observed, trans) are passed between bands of NaNs / all-ones integers and of finite random
bits, and after the call (a) no guard byte changed, (b) no output element was left unwritten, (c) / (d) every output equals the call
outside the region bit for bit.  Shapes: the partial-workgroup ones of tests/test_forecast_tracks_bounds_gpu.py (1, 5, 257 windows x 1,
3, 12 forecast frames; 256 pairs per claim workgroup), 3 samples, cells -2 .. n_cells + 1, and at 257 windows a max_cover of 6 that
leaves cells whose list is full; a case whose lists reach 1024 values (two joints per LDS group, the largest key stride)."""
import numpy as np
import pytest
import torch

import forecast_fan_ref as FF
import forecast_ref as FR
import forecast_tta_ref as TR
import test_buffer_bounds_gpu as BB
from mocodad_amd.utils.transforms import affine_table
from test_buffer_bounds_gpu import run

pytestmark = pytest.mark.gpu

# the audit at the end of tests/test_buffer_bounds_gpu.py lists the entries exercised between guard bands; the new one is exercised
# HERE with that module's `run`, so this module adds it when it is imported (tests/test_forecast_tracks_bounds_gpu.py)
NEW_ENTRIES = ["mcd_forecast_fan"]
BB.COVERED += [e for e in NEW_ENTRIES if e not in BB.COVERED]
NAMES = ("quant", "mean", "std", "rank", "count")
LEVELS = (0.0, 0.25, 0.5, 1.0)


def _check(r, want):
    for name, w in zip(NAMES, want):
        g = r[name].cpu().numpy()
        assert np.array_equal(g, w) if name == "count" else np.array_equal(FR.bits(g), FR.bits(w)), name


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "transforms"])
@pytest.mark.parametrize("Tx", [1, 3, 12])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_forecast_fan(N, Tx, tta):
    """cells -2 .. n_cells + 1: a store through a cell outside the output would land in a guard band; max_cover 6 at N = 257 leaves
    cells whose list is full (a claim past the list's end would land in the next cell's words, or behind the workspace)"""
    from mocodad_amd.engine import forecast_fan
    rng = np.random.default_rng(100 * N + Tx)
    S = 3
    poses_all = torch.from_numpy(rng.normal(size=(N, S, 2, Tx, 17)).astype(np.float32))
    n_cells = max(2, N * Tx // 5)
    cell = torch.from_numpy(rng.integers(-2, n_cells + 2, size=(N, Tx)).astype(np.int32))
    observed = torch.from_numpy(rng.normal(size=(n_cells, 2, 17)).astype(np.float32))
    max_cover = 6 if N == 257 else (64 if tta else 32)
    inputs = {"poses_all": poses_all, "cell": cell, "observed": observed}
    inv = None
    if tta:
        inputs["trans"] = torch.from_numpy(rng.integers(0, 5, N).astype(np.int32))
        inv = TR.inverse_table(affine_table(5).numpy())

    def call(T, poses_all, cell, observed, trans=None):
        out = forecast_fan(poses_all, cell, n_cells, levels=LEVELS, observed=observed, max_cover=max_cover, trans=trans, inv_affine=inv)
        return dict(zip(NAMES, out))

    r = run("mcd_forecast_fan", call, inputs)
    want = FF.fan(poses_all.numpy(), cell.numpy(), n_cells, LEVELS, observed.numpy(), max_cover,
                  inputs["trans"].numpy() if tta else None, inv)
    _check(r, want)
    if N == 257:
        assert (want[4] > max_cover).any()


def test_forecast_fan_at_the_largest_list():
    """32 pairs x 32 samples = 1024 values on a cell, 33 x 32 on the next (NaN), without observed rows (no rank buffer)"""
    from mocodad_amd.engine import forecast_fan
    rng = np.random.default_rng(9)
    N, S, Tx, n_cells = 23, 32, 3, 3
    poses_all = torch.from_numpy(rng.normal(size=(N, S, 2, Tx, 17)).astype(np.float32))
    flat = np.full(N * Tx, -1, np.int32)
    flat[:32], flat[32:65], flat[65:] = 0, 1, n_cells
    cell = torch.from_numpy(rng.permutation(flat).reshape(N, Tx))

    def call(T, poses_all, cell):
        out = forecast_fan(poses_all, cell, n_cells, levels=LEVELS, max_cover=32)
        assert out[3] is None
        return {k: v for k, v in zip(NAMES, out) if v is not None}

    r = run("mcd_forecast_fan", call, {"poses_all": poses_all, "cell": cell})
    want = FF.fan(poses_all.numpy(), cell.numpy(), n_cells, LEVELS, None, 32)
    assert want[4].tolist() == [32, 33, 0]
    for name in ("quant", "mean", "std"):
        assert np.array_equal(FR.bits(r[name].cpu().numpy()), FR.bits(want[NAMES.index(name)])), name
    assert np.array_equal(r["count"].cpu().numpy(), want[4])


def test_the_new_entry_was_exercised_here():
    """What the audit's list is told above is true: the new entry saw guarded allocations under `run` in this module."""
    for e in NEW_ENTRIES:
        assert e in BB.ALLOC and BB.ALLOC[e], (e, sorted(BB.ALLOC))

"""GPU: WHERE the kernels of the forecasts from every transform write -- mcd_stream_forecast_group_tta, mcd_stream_forecast_flush_tta
and mcd_forecast_assemble_view under the instrument of tests/test_buffer_bounds_gpu.py: every device buffer the Python layer
allocates (the forecast ring with its transform axis and the observed ring, the per-sample losses and poses of the scoring call, the
five outputs of every tick and of every close; the three outputs and the list workspace of the dataset call) lies between guard
bands with a poisoned interior, and after the calls (a) no guard byte changed, (b) no output element was left unwritten, (c) every
output equals the call outside the region bit for bit.  Shapes: 1, 5 and 65 emitting tracks x 5 transforms -- one store wave per
window of every transform (325 workgroups at 65) and 35 workgroups of raw rows behind them with a partial last one; one `push`, one
`push_many` group of three ticks whose LAST tick emits no window, one more tick without a window on its own, then `close_all`."""
import numpy as np
import pytest
import torch

import forecast_ref as FR
import forecast_tta_ref as TR
import test_buffer_bounds_gpu as BB
from test_buffer_bounds_gpu import run

pytestmark = pytest.mark.gpu

# the audit at the end of tests/test_buffer_bounds_gpu.py lists the entries exercised between guard bands; the three new ones are
# exercised HERE with that module's `run`, so this module adds them when it is imported (tests/test_stream_forecast_bounds_gpu.py)
NEW_ENTRIES = ["mcd_stream_forecast_group_tta", "mcd_stream_forecast_flush_tta", "mcd_forecast_assemble_view"]
BB.COVERED += [e for e in NEW_ENTRIES if e not in BB.COVERED]
FIELDS = ("expected", "expected_norm", "observed", "count", "spread")
NT = 5


@pytest.fixture(scope="module")
def stream_env(tmp_path_factory):
    from dataset_spec import load_dataset_golden
    from test_stream_many_gpu import _model
    g = load_dataset_golden()
    return g, _model(tmp_path_factory.mktemp("forecast_tta_bounds"), g)[0]


def _replay(g, model, n):
    from mocodad_amd.stream import ForecastCfg, PoseStream
    from test_stream_many_gpu import SEG_LEN, VID_RES
    st = PoseStream(model, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=n + 2, ring_len=SEG_LEN + 2,
                    forecasts=ForecastCfg("median", "median", "all"))
    assert st.num_transform == NT
    keys = [(1, 1 + i // 16, i) for i in range(n)]
    rng = np.random.default_rng(7)
    rows = lambda k: rng.uniform(20, 300, (k, 34)).astype(np.float32)
    res = [st.push(keys, [f + 1] * n, rows(n)) for f in range(SEG_LEN - 1)]           # no window yet: the raw rows only
    res.append(st.push(keys, [SEG_LEN] * n, rows(n)))                                   # one push: n windows x 5 transforms
    late, later = (9, 9, 1), (9, 9, 2)
    res += st.push_many([(keys, [SEG_LEN + 1] * n, rows(n)), (keys, [SEG_LEN + 2] * n, rows(n)),
                         ([late], [1], rows(1))])                                       # one group; its final tick emits no window
    res.append(st.push([later], [1], rows(1)))                                          # a tick of its own without a window
    assert [len(t.final) for t in res] == [0] * (SEG_LEN - 1) + [n, n, n, 0, 0]
    out = {}
    for i, t in enumerate(res):
        assert len(t.forecast) == len(t.final)
        out[f"scores{i}"], out[f"final{i}"] = t.scores, t.final.values
        for name in FIELDS:
            out[f"{name}{i}"] = getattr(t.forecast, name)
    tails = st.close_all()
    assert len(tails) == n * (SEG_LEN - 1) == len(tails.forecast)
    out["tails"] = tails.values
    for name in FIELDS:
        out[f"tail_{name}"] = getattr(tails.forecast, name)
    out.update(ring=st.ring, frame_scores_ring=st.rings.frame_scores_ring, forecast_tta_ring=st.rings.forecast_tta_ring,
               observed_ring=st.rings.observed_ring)
    return out


@pytest.mark.parametrize("n", [1, 5, 65])
def test_stream_replay_with_forecasts_of_every_transform(stream_env, n):
    from test_stream_many_gpu import SEG_LEN
    g, model = stream_env
    r = run("mcd_stream_forecast_group_tta + forecast_flush_tta", lambda T: _replay(g, model, n), None, [model.scorer()],
            partial=["ring", "frame_scores_ring", "forecast_tta_ring", "observed_ring"])
    ring = r["forecast_tta_ring"]
    assert tuple(ring.shape) == (n + 2, SEG_LEN + 2, NT, 3, 34) and bool((ring[:n] != 0).any(-1).any(-1).any(1).all()), "every transform stored"
    assert bool((r["observed_ring"][:n] != 0).any(-1).all()), "every position of every live slot took a raw row"
    # rows 0 .. 2 of every track come with its three windows, rows 3 .. 7 with the close (tails are track-major)
    counts = torch.cat([torch.stack([r[f"count{i}"] for i in range(SEG_LEN - 1, SEG_LEN + 2)]), r["tail_count"].view(n, SEG_LEN - 1).T])
    assert counts[:, 0].tolist() == [NT * c for c in (0, 0, 0, 1, 2, 3, 2, 1)] and bool((counts == counts[:, :1]).all())


@pytest.mark.parametrize("Tx", [1, 3, 12])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_forecast_assemble_view(N, Tx):
    """cells -2 .. n_cells + 1 and transforms -1 .. 5 of a table of 5: a store through a cell outside the output, or a read of a
    table row that is not there, would touch a guard band; max_cover 6 at N = 257 leaves cells whose list is full"""
    from mocodad_amd.engine import forecast_assemble
    from mocodad_amd.utils.transforms import inverse_affine_table
    rng = np.random.default_rng(100 * N + Tx)
    poses = torch.from_numpy(rng.normal(size=(N, 2, Tx, 17)).astype(np.float32))
    n_cells = max(2, N * Tx // 9)
    cell = torch.from_numpy(rng.integers(-2, n_cells + 2, size=(N, Tx)).astype(np.int32))
    trans = torch.from_numpy(rng.integers(-1, 6, size=N).astype(np.int32))
    inv = inverse_affine_table(5)
    max_cover = 6 if N == 257 else 64

    def call(T, poses, cell, trans, inv):
        pose, count, spread = forecast_assemble(poses, cell, n_cells, method="median", spread_method="median", max_cover=max_cover,
                                                trans=trans, inv_affine=inv)
        return {"pose": pose, "count": count, "spread": spread}

    r = run("mcd_forecast_assemble_view", call, {"poses": poses, "cell": cell, "trans": trans, "inv": inv})
    want = TR.assemble(poses.numpy(), cell.numpy(), trans.numpy(), inv.numpy(), n_cells, "median", "median", max_cover)
    assert np.array_equal(r["count"].cpu().numpy(), want[1])
    assert np.array_equal(FR.bits(r["pose"].cpu().numpy()), FR.bits(want[0]))
    assert np.array_equal(FR.bits(r["spread"].cpu().numpy()), FR.bits(want[2]))
    if N == 257:
        assert (want[1] > max_cover).any()
    if N > 1:
        assert ((trans < 0) | (trans > 4)).any()


def test_the_new_entries_were_exercised_here():
    """What the audit's list is told above is true: each new entry saw guarded allocations under `run` in this module."""
    ran = " ".join(BB.ALLOC)
    for e in NEW_ENTRIES:
        assert e.replace("mcd_stream_", "").replace("mcd_", "") in ran, (e, sorted(BB.ALLOC))

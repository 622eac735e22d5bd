"""GPU: WHERE the forecast kernels of a live stream write -- mcd_stream_forecast_group and mcd_stream_forecast_flush under the
instrument of tests/test_buffer_bounds_gpu.py: every device buffer the Python layer allocates (the forecast and observed rings, the
per-sample losses and poses the scoring call now returns, the five outputs of every tick and of every close) lies between guard
bands with a poisoned interior, and after the calls (a) no guard byte changed, (b) no output element was left unwritten, (c) every
output equals the call outside the region bit for bit.  Shapes: 1, 5 and 65 emitting tracks -- one wave per window and per final row,
so 65 is also 65 workgroups and, in the store launch, 35 workgroups of raw rows with a partial last one (65 * 34 = 2210 = 34 * 64 +
34 elements); one `push`, one `push_many` group of three ticks whose LAST tick emits no window (a new track's first row), one more
tick without a window on its own, then the close of everything."""
import numpy as np
import pytest
import torch

import test_buffer_bounds_gpu as BB
from test_buffer_bounds_gpu import run

pytestmark = pytest.mark.gpu

# tests/test_buffer_bounds_gpu.py ends with an audit: every declaration of include/mocodad_hip.h that writes a caller's buffer must
# be in its list of entries exercised between guard bands.  The two forecast entries are exercised HERE, with that module's own
# `run`, so this module adds them to that list when it is imported -- at collection, before any test runs.
NEW_ENTRIES = ["mcd_stream_forecast_group", "mcd_stream_forecast_flush"]
BB.COVERED += [e for e in NEW_ENTRIES if e not in BB.COVERED]
FIELDS = ("expected", "expected_norm", "observed", "count", "spread")


@pytest.fixture(scope="module")
def stream_env(tmp_path_factory):
    from dataset_spec import load_dataset_golden
    from test_stream_many_gpu import _model
    g = load_dataset_golden()
    return g, _model(tmp_path_factory.mktemp("forecast_bounds"), g)[0]


def _replay(g, model, n):
    from mocodad_amd.stream import ForecastCfg, PoseStream
    from test_stream_many_gpu import SEG_LEN, VID_RES
    st = PoseStream(model, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=n + 2, ring_len=SEG_LEN + 2,
                    forecasts=ForecastCfg("median", "median"))
    keys = [(1, 1 + i // 16, i) for i in range(n)]
    rng = np.random.default_rng(7)
    rows = lambda k: rng.uniform(20, 300, (k, 34)).astype(np.float32)
    res = [st.push(keys, [f + 1] * n, rows(n)) for f in range(SEG_LEN - 1)]           # no window yet: the raw rows only
    res.append(st.push(keys, [SEG_LEN] * n, rows(n)))                                   # one push: n windows
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
    out.update(ring=st.ring, frame_scores_ring=st.rings.frame_scores_ring, forecast_ring=st.rings.forecast_ring,
               observed_ring=st.rings.observed_ring)
    return out


@pytest.mark.parametrize("n", [1, 5, 65])
def test_stream_replay_with_forecasts(stream_env, n):
    from test_stream_many_gpu import SEG_LEN
    g, model = stream_env
    r = run("mcd_stream_forecast_group + forecast_flush", lambda T: _replay(g, model, n), None, [model.scorer()],
            partial=["ring", "frame_scores_ring", "forecast_ring", "observed_ring"])
    assert tuple(r["forecast_ring"].shape) == (n + 2, SEG_LEN + 2, 3, 34) and bool((r["forecast_ring"][:n] != 0).any())
    assert bool((r["observed_ring"][:n] != 0).any(-1).all()), "every position of every live slot took a raw row"
    # rows 0 .. 2 of every track come with its three windows, rows 3 .. 7 with the close (tails are track-major)
    counts = torch.cat([torch.stack([r[f"count{i}"] for i in range(SEG_LEN - 1, SEG_LEN + 2)]), r["tail_count"].view(n, SEG_LEN - 1).T])
    assert counts[:, 0].tolist() == [0, 0, 0, 1, 2, 3, 2, 1] and bool((counts == counts[:, :1]).all())


def test_the_new_entries_were_exercised_here():
    """What the audit's list is told above is true: each new entry saw guarded allocations under `run` in this module."""
    ran = " ".join(BB.ALLOC)
    for e in NEW_ENTRIES:
        assert e.replace("mcd_stream_", "") in ran, (e, sorted(BB.ALLOC))

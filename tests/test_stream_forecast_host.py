"""CPU: the forecast ring of a live stream (PoseStream(forecasts=...)) where no GPU is needed.

1. mcd_stream_forecast_group / mcd_stream_forecast_flush reject every argument error before any device call (there is no GPU here: a
   launch would not come back as the code asserted), and a call without rows is MCD_OK.  Pointers that a rejected call never reads
   are the dummy address P, as in tests/test_call_errors_host.py.
2. stream.forecast_cover -- the definition as code -- against a brute-force enumeration of a track's windows.
3. The NumPy model of the ring (tests/stream_forecast_ref.py: cell (r % L, j), validity by arithmetic, descending j), driven tick by
   tick and in groups, a slot reused after a close, against forecast_ref.assemble over the same track's windows + denormalize: bit
   for bit."""
import ctypes as C

import numpy as np
import pytest

import forecast_ref
from dataset_spec import stress_rows
from mocodad_amd import _lib
from mocodad_amd.stream import ForecastCfg, forecast_cover
from stream_forecast_ref import RingModel

P = C.c_void_p(0x1000)        # non-null, never dereferenced
INF = float("inf")
OK, EINVAL = 0, -1


def score_cfg(S=2, seg_len=6, corrupt=(3, 4, 5), n_cond=None):
    c = _lib.ScoreCfg()
    c.n_windows, c.n_samples, c.noise_steps, c.seg_len, c.loss_fn = 3, S, 4, seg_len, 0
    c.n_corrupt = len(corrupt)
    c.n_cond = seg_len - len(corrupt) if n_cond is None else n_cond
    cond = [t for t in range(seg_len) if t not in corrupt]
    for i, t in enumerate(cond[:c.n_cond]):
        c.cond_idx[i] = t
    for i, t in enumerate(corrupt):
        c.corrupt_idx[i] = t
    return c


def state(n_slots=4, ring_len=12, seg_len=6, nt=2):
    return _lib.StreamState(ring=0x1000, frame_scores=0x1000, n_slots=n_slots, ring_len=ring_len, seg_len=seg_len, num_transform=nt)


def fstate(forecast=0x1000, observed=0x1000, n_corrupt=3):
    return _lib.StreamForecastState(forecast=forecast, observed=observed, n_corrupt=n_corrupt)


def _ref(x):
    return C.byref(x) if x is not None else None


def group(L, s="default", fs="default", raw=P, desc=P, n=2, loss=P, poses=P, win=P, n_windows=1, cfg="default", aggr=1, method=2,
          spread=1, w=640.0, h=360.0, center=None, scale=None, outs=(P, P, P, P, P)):
    s, fs, cfg = (state() if s == "default" else s), (fstate() if fs == "default" else fs), (score_cfg() if cfg == "default" else cfg)
    return L.mcd_stream_forecast_group(_ref(s), _ref(fs), raw, desc, n, loss, poses, win, n_windows, _ref(cfg), aggr, method, spread,
                                       w, h, center, scale, *outs, None)


def flush(L, s="default", fs="default", win=P, n=1, cfg="default", method=2, spread=1, w=640.0, h=360.0, center=None, scale=None,
          outs=(P, P, P, P, P)):
    s, fs, cfg = (state() if s == "default" else s), (fstate() if fs == "default" else fs), (score_cfg() if cfg == "default" else cfg)
    return L.mcd_stream_forecast_flush(_ref(s), _ref(fs), win, n, _ref(cfg), method, spread, w, h, center, scale, *outs, None)


def _outs_without(i):
    return tuple(None if k == i else P for k in range(5))


# case -> (call, a piece of mcd_last_error())
CASES = {
    # ---- null pointers
    "group: null state": (lambda L: group(L, s=None), "null stream state"),
    "group: null forecast state": (lambda L: group(L, fs=None), "null stream forecast state"),
    "group: null forecast ring": (lambda L: group(L, fs=fstate(forecast=None)), "null stream forecast state"),
    "group: null observed ring": (lambda L: group(L, fs=fstate(observed=None)), "null stream forecast state"),
    "group: null cfg": (lambda L: group(L, cfg=None), "null argument"),
    "group: null raw": (lambda L: group(L, raw=None), "null argument"),
    "group: null desc": (lambda L: group(L, desc=None), "null argument"),
    "group: null loss_all": (lambda L: group(L, loss=None), "null argument"),
    "group: null poses_all": (lambda L: group(L, poses=None), "null argument"),
    "group: null win": (lambda L: group(L, win=None), "null argument"),
    **{f"group: null output {i}": (lambda L, i=i: group(L, outs=_outs_without(i)), "null argument") for i in range(5)},
    "flush: null state": (lambda L: flush(L, s=None), "null stream state"),
    "flush: null forecast state": (lambda L: flush(L, fs=None), "null stream forecast state"),
    "flush: null cfg": (lambda L: flush(L, cfg=None), "null argument"),
    "flush: null win": (lambda L: flush(L, win=None), "null argument"),
    **{f"flush: null output {i}": (lambda L, i=i: flush(L, outs=_outs_without(i)), "null argument") for i in range(5)},
    # ---- n_corrupt outside 1 .. 32, or not the cfg's
    "group: n_corrupt 0": (lambda L: group(L, fs=fstate(n_corrupt=0)), "1 <= n_corrupt <= 32"),
    "group: n_corrupt 33": (lambda L: group(L, fs=fstate(n_corrupt=33)), "1 <= n_corrupt <= 32"),
    "group: n_corrupt not the cfg's": (lambda L: group(L, fs=fstate(n_corrupt=2)), "cfg->n_corrupt is not"),
    "flush: n_corrupt 0": (lambda L: flush(L, fs=fstate(n_corrupt=0)), "1 <= n_corrupt <= 32"),
    "flush: n_corrupt 33": (lambda L: flush(L, fs=fstate(n_corrupt=33)), "1 <= n_corrupt <= 32"),
    "flush: n_corrupt not the cfg's": (lambda L: flush(L, fs=fstate(n_corrupt=2)), "cfg->n_corrupt is not"),
    # ---- a seg_len that is not the state's
    "group: seg_len not the state's": (lambda L: group(L, cfg=score_cfg(seg_len=8, corrupt=(5, 6, 7))), "cfg->seg_len is not"),
    "flush: seg_len not the state's": (lambda L: flush(L, cfg=score_cfg(seg_len=8, corrupt=(5, 6, 7))), "cfg->seg_len is not"),
    # ---- frame lists the cell rule cannot take
    "group: frame lists do not partition": (lambda L: group(L, cfg=score_cfg(n_cond=2)), "do not partition"),
    "group: corrupt_idx descending": (lambda L: group(L, cfg=score_cfg(corrupt=(5, 4, 3))), "corrupt_idx must ascend"),
    "group: corrupt_idx outside the window": (lambda L: group(L, cfg=score_cfg(corrupt=(4, 5, 6))), "corrupt_idx must ascend"),
    "flush: corrupt_idx repeated": (lambda L: flush(L, cfg=score_cfg(corrupt=(3, 3, 5))), "corrupt_idx must ascend"),
    # ---- an unknown method / spread
    "group: method 3": (lambda L: group(L, method=3), "method must be"),
    "group: method -1": (lambda L: group(L, method=-1), "method must be"),
    "group: spread unique": (lambda L: group(L, spread=0), "spread_method must be"),
    "flush: method 3": (lambda L: flush(L, method=3), "method must be"),
    "flush: spread 3": (lambda L: flush(L, spread=3), "spread_method must be"),
    # ---- an aggregation other than best / worst
    **{f"group: aggregation {name}": (lambda L, a=a: group(L, aggr=a), "MCD_AGGR_BEST or MCD_AGGR_WORST")
       for name, a in _lib.AGGR.items() if name not in ("best", "worst")},
    "group: aggregation 8": (lambda L: group(L, aggr=8), "MCD_AGGR_BEST or MCD_AGGR_WORST"),
    # ---- negative counts, counts a group cannot hold
    "group: n -1": (lambda L: group(L, n=-1, n_windows=0), "0 <= n_windows <= n"),
    "group: n_windows -1": (lambda L: group(L, n_windows=-1), "0 <= n_windows <= n"),
    "group: n_windows > n": (lambda L: group(L, n=1, n_windows=2), "0 <= n_windows <= n"),
    "group: n = 29": (lambda L: group(L, n=29), "more rows than"),                   # (state(): 4 * (12 - 6 + 1) = 28)
    "group: n_samples 0": (lambda L: group(L, cfg=score_cfg(S=0)), "n_samples >= 1"),
    "flush: n -1": (lambda L: flush(L, n=-1), "0 <= n <= n_slots"),
    "flush: n > n_slots": (lambda L: flush(L, n=5), "0 <= n <= n_slots"),
    # ---- the pixel box
    "group: vid_w inf": (lambda L: group(L, w=INF), "vid_res must be finite"),
    "group: center without scale": (lambda L: group(L, center=P), "both given or both NULL"),
    "flush: vid_h inf": (lambda L: flush(L, h=INF), "vid_res must be finite"),
    "flush: scale without center": (lambda L: flush(L, scale=P), "both given or both NULL"),
}


def test_the_exports_are_bound():
    L = _lib.lib()
    for name in ("mcd_stream_forecast_group", "mcd_stream_forecast_flush"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.ABI_VERSION == 15 and int(L.mcd_abi_version()) == 15


@pytest.mark.parametrize("name", list(CASES))
def test_rejected_before_any_device_call(name):
    L = _lib.lib()
    fn, text = CASES[name]
    assert int(fn(L)) == EINVAL
    assert text in L.mcd_last_error().decode()


def test_a_call_without_rows_is_ok_without_a_device_call():
    L = _lib.lib()
    assert group(L, n=0, n_windows=0) == OK
    assert group(L, raw=None, desc=None, n=0, loss=None, poses=None, win=None, n_windows=0, outs=(None,) * 5) == OK
    assert group(L, n=0, n_windows=0, aggr=2, method=0, spread=2) == OK
    assert flush(L, n=0) == OK and flush(L, win=None, n=0, outs=(None,) * 5) == OK
    assert flush(L, s=state(ring_len=4, seg_len=1), cfg=score_cfg(seg_len=1, corrupt=(0,)), fs=fstate(n_corrupt=1), n=3) == OK   # no pending row


# ---------------------------------------------------------------------------------------------------------------------- forecast_cover
SHAPES = [(6, [3, 4, 5]), (6, [2, 3]), (6, [0]), (6, [5]), (4, [1, 3])]


def brute_cover(cidx, T, r, n_rows):
    """Every window of a track of n_rows rows (end rows T - 1 .. n_rows - 1, ascending) that holds row r at a corrupt frame."""
    out = []
    for e in range(T - 1, n_rows):
        for j, c in enumerate(cidx):
            if e - T + 1 + c == r:
                out.append((e, j))
    return out


@pytest.mark.parametrize("T, cidx", SHAPES)
def test_forecast_cover_against_a_brute_force_enumeration(T, cidx):
    seen_counts = set()
    for n_rows in range(T, 2 * T + 2):
        pairs = set()
        for r in range(n_rows):
            at_close = forecast_cover(cidx, T, r, n_rows - 1)
            assert at_close == brute_cover(cidx, T, r, n_rows)                        # the windows that exist, in window order
            assert [e for e, _ in at_close] == sorted(e for e, _ in at_close) and len(set(at_close)) == len(at_close)
            assert [j for _, j in at_close] == sorted((j for _, j in at_close), reverse=True)      # ascending window = descending j
            if r + T - 1 <= n_rows - 1:                                               # final before the close: with window r + T - 1
                final = forecast_cover(cidx, T, r, r + T - 1)
                assert final == at_close == brute_cover(cidx, T, r, r + 3 * T)          # no later window covers the row
                assert len(final) == sum(c <= r for c in cidx)
                seen_counts.add(len(final))
            else:                                                                     # pending at the close
                assert len(at_close) == sum(c <= r and r + T - 1 - c <= n_rows - 1 for c in cidx)
            assert not pairs & set(at_close)
            pairs |= set(at_close)
        assert len(pairs) == (n_rows - T + 1) * len(cidx)                             # every (window, corrupt frame) pair exactly once
    assert max(seen_counts) == len(cidx)


def test_forecast_cfg_defaults_are_the_drivers():
    assert (ForecastCfg().method, ForecastCfg().spread) == ("median", "mean")


# ---------------------------------------------------------------------------------------------------------------------- the ring model
VID_RES = (640, 360)


def _track(n_rows, Tx, seed):
    rng = np.random.default_rng(seed)
    raw = stress_rows(n_rows, seed=seed)
    poses = rng.standard_normal((max(n_rows, 1), 2, Tx, 17)).astype(np.float32)       # window ending at row e: poses[e]
    if n_rows > 7:
        poses[7] = 0                                                                  # a window without a passing sample
    return raw, poses


def _offline(raw, poses, T, cidx, method, spread, center, scale):
    """forecast_ref.assemble over the track's windows (cell = the track row), then denormalize."""
    n_rows = len(raw)
    ends = np.arange(T - 1, n_rows)
    cell = np.asarray([[e - T + 1 + c for c in cidx] for e in ends], np.int64).reshape(len(ends), len(cidx))
    norm, count, spr = forecast_ref.assemble(poses[ends], cell, n_rows, method, spread)
    return forecast_ref.denormalize(norm, raw, VID_RES, center, scale, count=count), norm, count, spr


@pytest.mark.parametrize("T, cidx", SHAPES)
@pytest.mark.parametrize("extra, ticks", [(0, 1), (3, 1), (3, 4)])
@pytest.mark.parametrize("method, spread", [("median", "mean"), ("mean", "median"), ("unique", "mean")])
def test_ring_model_equals_assemble_over_the_tracks_windows(T, cidx, extra, ticks, method, spread):
    """Two tracks after each other in ONE slot of a ring that is never cleared (the second reuses it after the close), rows pushed in
    groups of `ticks` ticks (all rows and windows of a group stored before any of its final rows is read, as the two launches do)."""
    L = T + extra
    assert ticks <= L - T + 1
    rng = np.random.default_rng(3)
    center, scale = rng.standard_normal(34), rng.uniform(0.5, 2.0, 34)
    ring = RingModel(1, L, T, cidx, method, spread, VID_RES, center, scale)
    compared = 0
    for seed, n_rows in ((1, 2 * T + 1 + L), (2, T), (4, T + 1)):
        raw, poses = _track(n_rows, len(cidx), seed)
        want = _offline(raw, poses, T, cidx, method, spread, center, scale)
        got = {}
        for r0 in range(0, n_rows, ticks):
            rows = range(r0, min(r0 + ticks, n_rows))
            for r in rows:
                ring.store_row(0, r, raw[r])
                if r >= T - 1:
                    ring.store_window(0, r, poses[r])
            for r in rows:
                if r >= T - 1:
                    got[r - T + 1] = ring.final(0, r)
        for i, res in enumerate(ring.flush(0, n_rows - 1)):
            got[n_rows - T + 1 + i] = res
        assert sorted(got) == list(range(n_rows))
        for r in range(n_rows):
            e, nrm, obs, cnt, spr = got[r]
            assert cnt == want[2][r] == len(forecast_cover(cidx, T, r, n_rows - 1))
            assert np.array_equal(forecast_ref.bits(nrm), forecast_ref.bits(want[1][r])), (seed, r)
            assert np.array_equal(forecast_ref.bits(e), forecast_ref.bits(want[0][r])), (seed, r)
            assert np.array_equal(forecast_ref.bits(spr), forecast_ref.bits(want[3][r])) and np.array_equal(obs, raw[r])
            if cnt == 0:
                assert not e.any() and not nrm.any() and spr == 0
            compared += 1
    assert compared == 2 * T + 1 + L + T + T + 1

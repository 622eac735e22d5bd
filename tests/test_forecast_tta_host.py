"""CPU: forecasts from every test-time transform (mcd_forecast_assemble_view, mcd_stream_forecast_group_tta / _flush_tta,
ForecastCfg(transforms='all')) where no GPU is needed.

1. utils.transforms.inverse_affine_table: the identity's row in every bit, A^-1 A within a few float64 ulp of the identity for the
   shipped rows and for a row with shear and translation, a singular map refused; it is the restatement's table.
2. The three exports reject every argument error before any device call (no GPU here: a launch would not return the code asserted);
   trans = NULL is mcd_forecast_assemble; calls without rows are MCD_OK.
3. The ring model of the stream (forecast_tta_ref.TtaRingModel: the transform axis, validity, the order transform -> window),
   driven tick by tick and in groups, a slot reused after a close, against forecast_tta_ref.assemble over the track's windows of
   every transform in the dataset's transform-major order: bit for bit.
4. The refusals of the Python layer that need no device."""
import ctypes as C

import numpy as np
import pytest

import forecast_ref as FR
import forecast_tta_ref as TR
from dataset_spec import stress_rows
from mocodad_amd import _lib
from mocodad_amd.utils.transforms import affine_table, inverse_affine_rows, inverse_affine_table
from test_stream_forecast_host import EINVAL, INF, OK, P, _outs_without, _ref, score_cfg, state

SHEAR = [1.25, 0.5, -0.75, -0.25, 0.8, 2.0]          # shear, anisotropic scale and a translation


# ---------------------------------------------------------------------------------------------------------------------- the table
def test_identity_row_is_exact_and_zeros_are_positive():
    t = inverse_affine_table(5)
    assert t.dtype.is_floating_point and t.element_size() == 8 and tuple(t.shape) == (5, 6)
    assert t[0].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert not np.signbit(t.numpy()[t.numpy() == 0]).any()
    assert tuple(inverse_affine_table(1).shape) == (1, 6)


def test_inverse_times_forward_is_the_identity_to_a_few_ulp():
    rows = np.concatenate([affine_table(5).numpy().astype(np.float64), np.asarray([SHEAR])])
    inv = inverse_affine_rows(rows).numpy()
    assert np.array_equal(inv, TR.inverse_table(rows))                  # the restatement computes the same table
    assert np.array_equal(inverse_affine_table(5).numpy(), TR.inverse_table(affine_table(5).numpy()))
    for a, i in zip(rows, inv):
        A = np.array([[a[0], a[1], a[2]], [a[3], a[4], a[5]], [0, 0, 1]])
        I = np.array([[i[0], i[1], i[2]], [i[3], i[4], i[5]], [0, 0, 1]])
        # entries are O(1) sums of two or three O(1) products of correctly rounded quotients: a few ulp of 1 (8 eps, with room)
        assert np.abs(I @ A - np.eye(3)).max() <= 8 * np.finfo(np.float64).eps


def test_a_singular_map_is_refused():
    with pytest.raises(ValueError, match="singular"):
        inverse_affine_rows([[1.0, 2.0, 0.0, 2.0, 4.0, 0.0]])
    with pytest.raises(ValueError, match="singular"):
        inverse_affine_rows([[1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0]])


def test_map_back_inverts_the_forward_map():
    rng = np.random.default_rng(0)
    rows = np.concatenate([affine_table(5).numpy().astype(np.float64), np.asarray([SHEAR])])
    p = rng.standard_normal((6, 2, 3, 17)).astype(np.float32)
    fwd = np.stack([np.stack([a[0] * q[0] + a[1] * q[1] + a[2], a[3] * q[0] + a[4] * q[1] + a[5]]) for a, q in zip(rows, p.astype(np.float64))])
    back = TR.map_back(fwd.astype(np.float32), np.arange(6), TR.inverse_table(rows))
    assert np.abs(back - p).max() < 1e-5
    z = np.array([-0.0, np.nan], np.float32)
    q = np.zeros((1, 2, 1, 17), np.float32)
    q[0, 0, 0, :2], q[0, 1, 0, :2] = z, z[::-1]
    assert np.array_equal(TR.map_back(q, [0], TR.inverse_table(rows)).view(np.uint32), q.view(np.uint32))      # identity: the bits


# ---------------------------------------------------------------------------------------------------------------------- argument errors
def view(L, poses=P, cell=P, trans=P, inv=P, nt=5, n=4, Tx=3, n_cells=8, method=2, spread=1, cover=64, ws=P, outs=(P, P, P)):
    return L.mcd_forecast_assemble_view(poses, cell, trans, inv, nt, n, Tx, n_cells, method, spread, cover, ws, *outs, None)


def tstate(forecast=0x1000, observed=0x1000, n_corrupt=3, nt=2):
    return _lib.StreamForecastTtaState(forecast=forecast, observed=observed, n_corrupt=n_corrupt, num_transform=nt)


def group(L, s="default", fs="default", raw=P, desc=P, n=2, loss=P, poses=P, win=P, n_windows=1, cfg="default", aggr=1, method=2,
          spread=1, w=640.0, h=360.0, center=None, scale=None, inv=P, outs=(P, P, P, P, P)):
    s, fs, cfg = (state() if s == "default" else s), (tstate() if fs == "default" else fs), (score_cfg() if cfg == "default" else cfg)
    return L.mcd_stream_forecast_group_tta(_ref(s), _ref(fs), raw, desc, n, loss, poses, win, n_windows, _ref(cfg), aggr, method, spread,
                                           w, h, center, scale, inv, *outs, None)


def flush(L, s="default", fs="default", win=P, n=1, cfg="default", method=2, spread=1, w=640.0, h=360.0, center=None, scale=None, inv=P,
          outs=(P, P, P, P, P)):
    s, fs, cfg = (state() if s == "default" else s), (tstate() if fs == "default" else fs), (score_cfg() if cfg == "default" else cfg)
    return L.mcd_stream_forecast_flush_tta(_ref(s), _ref(fs), win, n, _ref(cfg), method, spread, w, h, center, scale, inv, *outs, None)


def _three_without(i):
    return tuple(None if k == i else P for k in range(3))


CASES = {
    # ---- mcd_forecast_assemble_view: the existing entry's errors ...
    "view: n -1": (lambda L: view(L, n=-1), "n, n_cells >= 0"),
    "view: n_cells -1": (lambda L: view(L, n_cells=-1), "n, n_cells >= 0"),
    "view: Tx 0": (lambda L: view(L, Tx=0), "1 <= n_corrupt <= 32"),
    "view: Tx 33": (lambda L: view(L, Tx=33), "1 <= n_corrupt <= 32"),
    "view: max_cover 0": (lambda L: view(L, cover=0), "1 <= max_cover <= 64"),
    "view: max_cover 65": (lambda L: view(L, cover=65), "1 <= max_cover <= 64"),
    "view: method 3": (lambda L: view(L, method=3), "method must be"),
    "view: spread unique": (lambda L: view(L, spread=0), "spread_method must be"),
    "view: n x Tx beyond 2^31": (lambda L: view(L, n=2**31 // 3 + 1), "exceeds 2^31 - 1"),
    "view: null poses": (lambda L: view(L, poses=None), "null argument"),
    "view: null cell": (lambda L: view(L, cell=None), "null argument"),
    "view: null workspace": (lambda L: view(L, ws=None), "null argument"),
    **{f"view: null output {i}": (lambda L, i=i: view(L, outs=_three_without(i)), "null argument") for i in range(3)},
    # ---- ... and the new ones
    "view: trans without inv_affine": (lambda L: view(L, inv=None), "trans needs inv_affine"),
    "view: n_transform 0": (lambda L: view(L, nt=0), "n_transform >= 1"),
    "view: n_transform -1": (lambda L: view(L, nt=-1), "n_transform >= 1"),
    # ---- trans = NULL is mcd_forecast_assemble, with its limit on max_cover and its errors
    "view, trans NULL: max_cover 33": (lambda L: view(L, trans=None, cover=33), "1 <= max_cover <= 32"),
    "view, trans NULL: null poses": (lambda L: view(L, trans=None, inv=None, cover=32, poses=None), "null argument"),
    # ---- the stream entries: the state
    "group: null state": (lambda L: group(L, s=None), "null stream state"),
    "group: null forecast state": (lambda L: group(L, fs=None), "null stream forecast state"),
    "group: null forecast ring": (lambda L: group(L, fs=tstate(forecast=None)), "null stream forecast state"),
    "group: null observed ring": (lambda L: group(L, fs=tstate(observed=None)), "null stream forecast state"),
    "group: num_transform not the state's": (lambda L: group(L, fs=tstate(nt=3)), "num_transform is not the stream state's"),
    "group: n_corrupt 0": (lambda L: group(L, fs=tstate(n_corrupt=0)), "1 <= n_corrupt <= 32"),
    "group: n_corrupt 33": (lambda L: group(L, fs=tstate(n_corrupt=33)), "1 <= n_corrupt <= 32"),
    "group: 22 transforms x 3 frames": (lambda L: group(L, s=state(nt=22), fs=tstate(nt=22)), "exceeds 64"),
    "group: 3 transforms x 22 frames": (lambda L: group(L, s=state(nt=3, seg_len=24, ring_len=24), fs=tstate(nt=3, n_corrupt=22)), "exceeds 64"),
    "group: n_corrupt not the cfg's": (lambda L: group(L, fs=tstate(n_corrupt=2)), "cfg->n_corrupt is not"),
    "group: null inv_affine": (lambda L: group(L, inv=None), "null inv_affine"),
    "flush: null state": (lambda L: flush(L, s=None), "null stream state"),
    "flush: null forecast state": (lambda L: flush(L, fs=None), "null stream forecast state"),
    "flush: num_transform not the state's": (lambda L: flush(L, fs=tstate(nt=1)), "num_transform is not the stream state's"),
    "flush: n_corrupt 33": (lambda L: flush(L, fs=tstate(n_corrupt=33)), "1 <= n_corrupt <= 32"),
    "flush: 22 transforms x 3 frames": (lambda L: flush(L, s=state(nt=22), fs=tstate(nt=22)), "exceeds 64"),
    "flush: n_corrupt not the cfg's": (lambda L: flush(L, fs=tstate(n_corrupt=2)), "cfg->n_corrupt is not"),
    "flush: null inv_affine": (lambda L: flush(L, inv=None), "null inv_affine"),
    # ---- the stream entries: everything the existing pair refuses
    "group: null cfg": (lambda L: group(L, cfg=None), "null argument"),
    "group: null raw": (lambda L: group(L, raw=None), "null argument"),
    "group: null desc": (lambda L: group(L, desc=None), "null argument"),
    "group: null loss_all": (lambda L: group(L, loss=None), "null argument"),
    "group: null poses_all": (lambda L: group(L, poses=None), "null argument"),
    "group: null win": (lambda L: group(L, win=None), "null argument"),
    **{f"group: null output {i}": (lambda L, i=i: group(L, outs=_outs_without(i)), "null argument") for i in range(5)},
    "flush: null cfg": (lambda L: flush(L, cfg=None), "null argument"),
    "flush: null win": (lambda L: flush(L, win=None), "null argument"),
    **{f"flush: null output {i}": (lambda L, i=i: flush(L, outs=_outs_without(i)), "null argument") for i in range(5)},
    "group: seg_len not the state's": (lambda L: group(L, cfg=score_cfg(seg_len=8, corrupt=(5, 6, 7))), "cfg->seg_len is not"),
    "flush: seg_len not the state's": (lambda L: flush(L, cfg=score_cfg(seg_len=8, corrupt=(5, 6, 7))), "cfg->seg_len is not"),
    "group: frame lists do not partition": (lambda L: group(L, cfg=score_cfg(n_cond=2)), "do not partition"),
    "group: corrupt_idx descending": (lambda L: group(L, cfg=score_cfg(corrupt=(5, 4, 3))), "corrupt_idx must ascend"),
    "flush: corrupt_idx repeated": (lambda L: flush(L, cfg=score_cfg(corrupt=(3, 3, 5))), "corrupt_idx must ascend"),
    "group: method 3": (lambda L: group(L, method=3), "method must be"),
    "group: spread unique": (lambda L: group(L, spread=0), "spread_method must be"),
    "flush: method -1": (lambda L: flush(L, method=-1), "method must be"),
    "flush: spread 3": (lambda L: flush(L, spread=3), "spread_method must be"),
    **{f"group: aggregation {name}": (lambda L, a=a: group(L, aggr=a), "MCD_AGGR_BEST or MCD_AGGR_WORST")
       for name, a in _lib.AGGR.items() if name not in ("best", "worst")},
    "group: n -1": (lambda L: group(L, n=-1, n_windows=0), "0 <= n_windows <= n"),
    "group: n_windows > n": (lambda L: group(L, n=1, n_windows=2), "0 <= n_windows <= n"),
    "group: n = 29": (lambda L: group(L, n=29), "more rows than"),
    "group: n_samples 0": (lambda L: group(L, cfg=score_cfg(S=0)), "n_samples >= 1"),
    "flush: n -1": (lambda L: flush(L, n=-1), "0 <= n <= n_slots"),
    "flush: n > n_slots": (lambda L: flush(L, n=5), "0 <= n <= n_slots"),
    "group: vid_w inf": (lambda L: group(L, w=INF), "vid_res must be finite"),
    "group: center without scale": (lambda L: group(L, center=P), "both given or both NULL"),
    "flush: vid_h inf": (lambda L: flush(L, h=INF), "vid_res must be finite"),
}


def test_the_exports_are_bound():
    L = _lib.lib()
    for name in ("mcd_forecast_assemble_view", "mcd_stream_forecast_group_tta", "mcd_stream_forecast_flush_tta"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.ABI_VERSION == 15 and int(L.mcd_abi_version()) == 15
    assert C.sizeof(_lib.StreamForecastTtaState) == 24 and C.sizeof(_lib.StreamForecastState) == 24      # the old state is untouched


@pytest.mark.parametrize("name", list(CASES))
def test_rejected_before_any_device_call(name):
    L = _lib.lib()
    fn, text = CASES[name]
    assert int(fn(L)) == EINVAL
    assert text in L.mcd_last_error().decode()


def test_calls_without_rows_are_ok_without_a_device_call():
    L = _lib.lib()
    assert view(L, n_cells=0) == OK and view(L, n_cells=0, poses=None, cell=None, ws=None, outs=(None,) * 3) == OK
    assert view(L, trans=None, inv=None, nt=0, n_cells=0, cover=32) == OK            # trans = NULL is accepted: the existing entry
    assert group(L, n=0, n_windows=0) == OK
    assert group(L, raw=None, desc=None, n=0, loss=None, poses=None, win=None, n_windows=0, outs=(None,) * 5) == OK
    assert group(L, s=state(nt=5), fs=tstate(nt=5, n_corrupt=3), n=0, n_windows=0, aggr=2, method=0, spread=2) == OK
    assert group(L, s=state(nt=2, seg_len=32, ring_len=32), fs=tstate(nt=2, n_corrupt=32), cfg=score_cfg(seg_len=32, corrupt=tuple(range(32))),
                 n=0, n_windows=0) == OK                                              # 64 forecasts on a row: the limit itself
    assert flush(L, n=0) == OK and flush(L, win=None, n=0, outs=(None,) * 5) == OK


# ---------------------------------------------------------------------------------------------------------------------- the ring model
VID_RES = (640, 360)
SHAPES = [(6, [3, 4, 5]), (6, [2, 3]), (6, [0]), (4, [1, 3])]
TABLES = {"shipped5": lambda: TR.inverse_table(affine_table(5).numpy()),
          "identity+shear": lambda: TR.inverse_table([[1, 0, 0, 0, 1, 0], SHEAR])}


def _track(n_rows, nt, Tx, seed):
    rng = np.random.default_rng(seed)
    poses = rng.standard_normal((nt, max(n_rows, 1), 2, Tx, 17)).astype(np.float32)      # [t, e]: the window ending at row e under t
    if n_rows > 7:
        poses[:, 7] = 0                                                                  # a window without a passing sample: mapped zeros
    return stress_rows(n_rows, seed=seed), poses


def _offline(raw, poses, T, cidx, inv, method, spread, center, scale):
    """forecast_tta_ref.assemble over the track's windows in the dataset's order -- transform-major, then window --, cell = the row."""
    n_rows, nt = len(raw), poses.shape[0]
    ends = np.arange(T - 1, n_rows)
    cell = np.asarray([[e - T + 1 + c for c in cidx] for e in ends], np.int64).reshape(len(ends), len(cidx))
    norm, count, spr = TR.assemble(poses[:, ends].reshape(nt * len(ends), 2, len(cidx), 17), np.tile(cell, (nt, 1)),
                                   np.repeat(np.arange(nt), len(ends)), inv, n_rows, method, spread, 64)
    return FR.denormalize(norm, raw, VID_RES, center, scale, count=count), norm, count, spr


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("T, cidx", SHAPES)
@pytest.mark.parametrize("extra, ticks", [(0, 1), (3, 1), (3, 4)])
@pytest.mark.parametrize("method, spread", [("median", "mean"), ("mean", "median"), ("unique", "mean")])
def test_ring_model_equals_assemble_over_every_transforms_windows(T, cidx, extra, ticks, method, spread, table):
    """Three tracks after each other in ONE slot of a ring that is never cleared, rows pushed in groups of `ticks` ticks (all rows
    and windows of a group stored before any of its final rows is read, as the two launches do)."""
    from mocodad_amd.stream import forecast_cover
    L = T + extra
    inv = TABLES[table]()
    nt = len(inv)
    rng = np.random.default_rng(3)
    center, scale = rng.standard_normal(34), rng.uniform(0.5, 2.0, 34)
    ring = TR.TtaRingModel(1, L, T, cidx, inv, method, spread, VID_RES, center, scale)
    assert ring.fc.shape == (1, L, nt, len(cidx), 34)
    for seed, n_rows in ((1, 2 * T + 1 + L), (2, T), (4, T + 1)):
        raw, poses = _track(n_rows, nt, len(cidx), seed)
        want = _offline(raw, poses, T, cidx, inv, method, spread, center, scale)
        got = {}
        for r0 in range(0, n_rows, ticks):
            rows = range(r0, min(r0 + ticks, n_rows))
            for r in rows:
                ring.store_row(0, r, raw[r])
                for t in range(nt) if r >= T - 1 else ():
                    ring.store_window(0, r, t, poses[t, r])
            for r in rows:
                if r >= T - 1:
                    got[r - T + 1] = ring.final(0, r)
        for i, res in enumerate(ring.flush(0, n_rows - 1)):
            got[n_rows - T + 1 + i] = res
        assert sorted(got) == list(range(n_rows))
        for r in range(n_rows):
            e, nrm, obs, cnt, spr = got[r]
            assert cnt == want[2][r] == nt * len(forecast_cover(cidx, T, r, n_rows - 1))
            assert np.array_equal(FR.bits(nrm), FR.bits(want[1][r])), (seed, r)
            assert np.array_equal(FR.bits(e), FR.bits(want[0][r])), (seed, r)
            assert np.array_equal(FR.bits(spr), FR.bits(want[3][r])) and np.array_equal(obs, raw[r])


def test_the_wide_restatement_is_forecast_refs_below_its_limit():
    """forecast_tta_ref restates forecast_ref.assemble's loops for lists of 33 .. 64 pairs; where both apply they agree in every bit."""
    rng = np.random.default_rng(5)
    poses = rng.standard_normal((40, 2, 3, 17)).astype(np.float32)
    cell = rng.integers(-1, 9, (40, 3))
    for method, spread in (("median", "median"), ("mean", "mean"), ("unique", "median")):
        a = FR.assemble(poses, cell, 8, method, spread, 32)
        b = TR._assemble_wide(poses, cell.astype(np.int64), 8, method, spread, 64)
        assert a[1].max() <= 32 and all(np.array_equal(FR.bits(x) if x.dtype != np.int32 else x, FR.bits(y) if y.dtype != np.int32 else y)
                                        for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------- the Python layer
def test_forecast_cfg_and_helpers_refuse_by_name():
    from mocodad_amd.stream import ForecastCfg
    from mocodad_amd.utils.eval_utils import forecast_cells_aligned, forecast_cells_dense, forecast_max_cover, forecast_track_rows
    assert ForecastCfg().transforms == "identity" and ForecastCfg("mean", "median", "all").transforms == "all"
    assert forecast_max_cover(5, 3) == 3 and forecast_max_cover(5, 3, "all") == 15 and forecast_max_cover(5, 12, "all") == 60
    assert forecast_max_cover(2, 32, "all") == 64
    with pytest.raises(ValueError, match="5 \\* 13 = 65"):
        forecast_max_cover(5, 13, "all")
    for fn in (lambda: forecast_max_cover(5, 3, "every"), lambda: forecast_cells_dense([0], [[1]], [0], 4, transforms="both"),
               lambda: forecast_cells_aligned([0], [[1]], [0], transforms=None),
               lambda: forecast_track_rows(np.zeros((1, 2, 1, 17)), [0], [[0]], None, meta=np.zeros((1, 4)), frames=np.ones((1, 2)), transforms="x")):
        with pytest.raises(ValueError, match="transforms must be one of"):
            fn()
    # the cells of the other transforms: -1 by default, the row of their forecast frame under 'all'
    base, mf, trans = np.array([0, 34, 0, 34]), np.array([[3, 4, 5]] * 4), np.array([0, 0, 1, 1])
    assert forecast_cells_aligned(base, mf, trans).tolist() == [[3, 4, 5], [4, 5, 6], [-1] * 3, [-1] * 3]
    assert forecast_cells_aligned(base, mf, trans, transforms="all").tolist() == [[3, 4, 5], [4, 5, 6], [3, 4, 5], [4, 5, 6]]
    assert forecast_cells_dense([0, 1], [[1, 2], [2, 9]], [0, 3], 4).tolist() == [[0, 1], [-1, -1]]
    assert forecast_cells_dense([0, 1], [[1, 2], [2, 9]], [0, 3], 4, transforms="all").tolist() == [[0, 1], [5, -1]]


def test_engine_refuses_before_the_device():
    import torch
    from mocodad_amd.engine import forecast_assemble
    poses, cell = torch.zeros(4, 2, 3, 17), torch.zeros(4, 3, dtype=torch.int32)
    inv = inverse_affine_table(5)
    for kw, text in ((dict(trans=torch.zeros(4, dtype=torch.int32)), "go together"), (dict(inv_affine=inv), "go together"),
                     (dict(trans=torch.zeros(3, dtype=torch.int32), inv_affine=inv), "trans must be an integer"),
                     (dict(trans=torch.zeros(4), inv_affine=inv), "trans must be an integer"),
                     (dict(trans=torch.zeros(4, dtype=torch.int32), inv_affine=inv[:, :5]), "inv_affine must be"),
                     (dict(trans=torch.zeros(4, dtype=torch.int32), inv_affine=inv, max_cover=65), "max_cover must be in 1 .. 64"),
                     (dict(max_cover=33), "max_cover must be in 1 .. 32")):
        with pytest.raises(ValueError, match=text):
            forecast_assemble(poses, cell, 8, **kw)


def test_driver_refusals_come_before_any_gpu_call(tmp_path):
    """eval_MoCoDAD.py --forecast-transforms all with 5 transforms x 13 forecast frames (65 > 64), and the option without
    --forecast-tracks: refused by name; there is no GPU here, so a refusal behind a device call would not be reached."""
    import os
    import subprocess
    import sys
    import yaml
    from dataset_spec import ROOT
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(seg_len=16, conditioning_indices=[0, 1, 2], exp_dir=str(tmp_path / "exp"))
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    base = [sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", str(p), "--synthetic", "2", "--random-init"]
    r = subprocess.run(base + ["--forecast-tracks", str(tmp_path / "f.npz"), "--forecast-transforms", "all"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--forecast-transforms all" in r.stderr and "5 * 13 = 65" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--forecast-transforms", "all"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "goes with --forecast-tracks" in r.stderr, r.stderr[-2000:]

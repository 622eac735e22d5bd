"""GPU: forecast tracks -- mcd_forecast_assemble and mcd_denormalize_poses against the float64 restatement of
tests/forecast_ref.py BIT FOR BIT (NaN payloads aside), the round trip denormalize(normalize(raw)) on the dataset fixture under a
bound the test computes from the roundings involved, forecast_track_rows on the pose model and on the latent model in pose space,
and eval_MoCoDAD.py --forecast-tracks on synthetic clips and on the dataset fixture.

Shapes: N in {1, 5, 257} windows x Tx in {1, 3, 12} forecast frames (the claim launch runs 256 pairs per workgroup: one partial
workgroup up to thirteen), cells drawn so that some are empty, some hold more pairs than max_cover, and some pairs name a cell
outside the output."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import forecast_ref as FR
from dataset_spec import DATASET, ROOT, bbox_centre, load_dataset_golden, normalise, stress_rows
from helpers import golden_weights, make_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG_LEN = 6
VID_RES = (640, 360)


def _assemble(poses, cell, n_cells, **kw):
    from mocodad_amd.engine import forecast_assemble
    return tuple(t.cpu().numpy() for t in forecast_assemble(poses, cell, n_cells, device=DEV, **kw))


def _same(got, want, what):
    for name, g, w in zip(("pose", "count", "spread"), got, want):
        if name == "count":
            assert np.array_equal(g, w), (what, name)
        else:
            bad = np.flatnonzero((FR.bits(g) != FR.bits(w)).reshape(len(g), -1).any(1))
            assert not len(bad), (what, name, bad[:5].tolist(), g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("Tx", [1, 3, 12])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_assemble_bits(N, Tx):
    rng = np.random.default_rng(100 * N + Tx)
    poses = (rng.normal(size=(N, 2, Tx, 17)) * rng.choice([0.01, 1.0, 5.0], size=(N, 1, 1, 1))).astype(np.float32)
    n_cells = max(2, N * Tx // 5) + 1
    cell = rng.integers(-2, n_cells + 2, size=(N, Tx)).astype(np.int32)          # -2, -1, n_cells, n_cells + 1: ignored
    cell[cell == n_cells - 1] = n_cells                                          # ... and the last cell stays empty
    tp, tc = torch.from_numpy(poses), torch.from_numpy(cell)
    for method in FR.METHODS:
        for sm in FR.SPREADS:
            for max_cover in ((6, 32) if N == 257 else (32,)):
                got = _assemble(tp, tc, n_cells, method=method, spread_method=sm, max_cover=max_cover)
                want = FR.assemble(poses, cell, n_cells, method, sm, max_cover)
                _same(got, want, (method, sm, max_cover))
                assert want[1][-1] == 0 and not got[0][-1].any() and got[2][-1] == 0
                if N == 257 and max_cover == 6:
                    assert (want[1] > 6).any() and np.isnan(want[0][want[1] > 6]).all()


def test_assemble_cover_edges_duplicates_and_a_nan():
    """max_cover = 4: cell 0 holds exactly 4 pairs, cell 1 holds 5 (NaN, count 5), cell 2 is named twice by ONE window (two
    forecast frames on one cell: both count, in frame order), cell 3 holds a window with one NaN element among finite ones (that
    feature and the spread are NaN, the other 33 features are not), cell 4 is empty."""
    rng = np.random.default_rng(7)
    poses = rng.normal(size=(12, 2, 2, 17)).astype(np.float32)
    poses[10, 1, 0, 5] = np.nan
    cell = np.full((12, 2), -1, np.int32)
    cell[[0, 3, 5, 7], 0] = 0
    cell[[1, 2, 4, 6, 8], 1] = 1
    cell[9] = 2
    cell[2, 0] = 2
    cell[[10, 11], 0] = 3
    cell[0, 1] = 3
    for method in FR.METHODS:
        for sm in FR.SPREADS:
            got = _assemble(torch.from_numpy(poses), torch.from_numpy(cell), 5, method=method, spread_method=sm, max_cover=4)
            _same(got, FR.assemble(poses, cell, 5, method, sm, 4), (method, sm))
            pose, count, spread = got
            assert count.tolist() == [4, 5, 3, 3, 0]
            assert np.isfinite(pose[0]).all() and np.isnan(pose[1]).all() and np.isnan(spread[1]) and not pose[4].any() and spread[4] == 0
            assert np.isnan(spread[3]) and np.isfinite(np.delete(pose[3], 11)).all()
            assert np.isnan(pose[3, 11]) == (method != "unique")            # (unique takes window 0's frame 1, which is finite)
            if method == "unique":
                assert np.array_equal(pose[2], poses[2, :, 0].T.reshape(34))


def test_assemble_does_not_depend_on_claim_order():
    """600 windows x 3 forecast frames = 1800 pairs in 8 workgroups of the claim launch; 8 cells take 25 .. 32 pairs each from
    all over the batch (the other pairs are ignored), max_cover = 32: twice, identical bits, equal to the restatement."""
    rng = np.random.default_rng(11)
    poses = rng.normal(size=(600, 2, 3, 17)).astype(np.float32)
    cell = np.full(1800, -1, np.int32)
    picks = rng.permutation(1800)
    lo = 0
    for c in range(8):
        k = 25 + c
        cell[picks[lo:lo + k]] = c
        lo += k
    cell = cell.reshape(600, 3)
    assert len({int(p) // 256 for p in picks[:25]}) > 4, "a cell's pairs come from several workgroups"
    tp, tc = torch.from_numpy(poses).to(DEV), torch.from_numpy(cell).to(DEV)
    for method, sm in (("median", "median"), ("mean", "mean")):
        a = _assemble(tp, tc, 8, method=method, spread_method=sm, max_cover=32)
        b = _assemble(tp, tc, 8, method=method, spread_method=sm, max_cover=32)
        assert a[1].tolist() == list(range(25, 33))
        _same(a, b, "second run")
        _same(a, FR.assemble(poses, cell, 8, method, sm, 32), (method, sm))


def test_assemble_empty_calls_and_caller_buffers():
    from mocodad_amd.engine import forecast_assemble
    pose, count, spread = forecast_assemble(torch.zeros(0, 2, 3, 17), torch.zeros(0, 3, dtype=torch.int32), 4, device=DEV)
    assert not pose.any() and not count.any() and not spread.any() and tuple(pose.shape) == (4, 34)
    pose, count, spread = forecast_assemble(torch.zeros(2, 2, 3, 17), torch.zeros(2, 3, dtype=torch.int32), 0, device=DEV)
    assert tuple(pose.shape) == (0, 34) and tuple(count.shape) == (0,)
    rng = np.random.default_rng(2)
    poses, cell = rng.normal(size=(5, 2, 3, 17)).astype(np.float32), rng.integers(0, 4, (5, 3)).astype(np.int32)
    out = (torch.full((4, 34), 9.0, device=DEV), torch.full((4,), 9, device=DEV, dtype=torch.int32), torch.full((4,), 9.0, device=DEV))
    ws = torch.full((4 * 32,), -5, device=DEV, dtype=torch.int32)
    res = forecast_assemble(torch.from_numpy(poses), torch.from_numpy(cell), 4, device=DEV, out=out, workspace=ws)
    assert all(a is b for a, b in zip(res, out))
    _same(tuple(t.cpu().numpy() for t in res), FR.assemble(poses, cell, 4), "caller buffers")


# ---------------------------------------------------------------- mcd_denormalize_poses
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_denormalize_bits(n, scaled):
    """stress rows: missing joints, all-zero frames, zero-width / zero-height boxes, boxes clipped at the border; count = 0 rows"""
    from mocodad_amd.engine import denormalize_poses
    rng = np.random.default_rng(300 + n)
    raw = stress_rows(n, seed=n)
    center, scale = (rng.normal(0, 0.2, 34), rng.uniform(0.05, 1.5, 34)) if scaled else (None, None)
    norm = np.where(rng.random((n, 34)) < 0.5, normalise(raw, VID_RES, center, scale), rng.normal(size=(n, 34))).astype(np.float32)
    count = rng.integers(0, 3, n).astype(np.int32)
    for cnt in (None, count):
        got = denormalize_poses(torch.from_numpy(norm), raw, VID_RES, center, scale, None if cnt is None else torch.from_numpy(cnt),
                                device=DEV).cpu().numpy()
        want = FR.denormalize(norm, raw, VID_RES, center, scale, cnt)
        bad = np.flatnonzero((FR.bits(got) != FR.bits(want)).any(1))
        assert not len(bad), (bad[:5].tolist(), raw[bad[0]].tolist(), got[bad[0]], want[bad[0]])
    if n > 1:
        L, R, T, B = FR.box_sides(raw, VID_RES)
        assert (R == L).any() and (B == T).any() and (raw == 0).any() and (count == 0).any()


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_round_trip_on_the_dataset_fixture(scaled):
    """denormalize(normalize(raw)) against raw.  With u = 2^-24 the forward kernel rounds d = x - c (error u |d|), v = d / s (u |v|, s
    pixels per unit), and under the scaler v - center_k (u |v - center_k|) and t = that / scale_k (u |t|, scale_k s pixels per unit);
    the inverse runs in float64 and rounds once (u |x|):
        |back - x| <= u (s (|v| + |v - center_k| + |t scale_k|) + |d| + |x|)          without the scaler: u (s |v| + |d| + |x|)
    Elements compared: joints that are not missing (x != 0) on a non-degenerate side (s != 0) whose normalised value is not exactly
    0 -- the scaler, like the reference's, treats an exact 0 as missing and leaves it unscaled, so such a joint cannot come back."""
    from mocodad_amd.data import trajectories as T
    from mocodad_amd.engine import denormalize_poses, normalize_poses
    g = load_dataset_golden()
    raw = T.load_raw(DATASET, "test", SEG_LEN).poses
    center, scale = (g["train_center"].astype(np.float64), g["train_scale"].astype(np.float64)) if scaled else (None, None)
    norm = normalize_poses(raw, VID_RES, center, scale, device=DEV).permute(0, 2, 1).reshape(-1, 34).contiguous()
    back = denormalize_poses(norm, raw, VID_RES, center, scale).cpu().numpy().astype(np.float64)
    L, R, T_, B = FR.box_sides(raw, VID_RES)
    s, c = np.zeros(raw.shape), np.zeros(raw.shape)
    s[:, 0::2], s[:, 1::2] = (R - L)[:, None], (B - T_)[:, None]
    c[:, 0::2], c[:, 1::2] = ((L + R) / 2)[:, None], ((T_ + B) / 2)[:, None]
    x = raw.astype(np.float64)
    d = np.abs((raw - c.astype(np.float32)).astype(np.float32).astype(np.float64))
    v = bbox_centre(raw, VID_RES).astype(np.float64)
    t = norm.cpu().numpy().astype(np.float64)
    u = 2.0 ** -24
    if scaled:
        bound = u * (s * (np.abs(v) + np.abs(v - center) + np.abs(t * scale)) + d + np.abs(x))
    else:
        bound = u * (s * np.abs(v) + d + np.abs(x))
    ok = (raw != 0) & (s != 0) & (t != 0)
    ratio = (np.abs(back - x)[ok] / bound[ok]).max()
    print(f"round trip ({'scaled' if scaled else 'plain'}): {ok.sum()} elements, max |back - x| {np.abs(back - x)[ok].max():.3e} px, "
          f"max error / bound {ratio:.3f}")
    assert ok.sum() > 1000 and ratio <= 1.0


# ---------------------------------------------------------------- the module surface
def _tracks(seg_len=6, nt=2):
    from mocodad_amd.data.windows import TrajectoryWindows
    rng = np.random.default_rng(21)
    trajs = {(1, 1, p): (3 + p, (rng.normal(size=(n, 2, 17)) * 0.3).astype(np.float32)) for p, n in ((0, 13), (2, 9), (5, 6))}
    return TrajectoryWindows(trajs, seg_len, nt).to(DEV)          # 8 + 4 + 1 windows x 2 transforms


def _check_module(m, tw, aggr, **fw):
    from mocodad_amd.engine import forecast_assemble
    from mocodad_amd.utils.eval_utils import forecast_track_rows
    batch = tw.batch(0, len(tw))
    with torch.no_grad():
        loss, poses = m.forward(batch, aggr_strategy=aggr, return_="all", window_offset=0, **fw)[:2]
    N, Tx = len(tw), m.n_frames_corrupt
    assert tuple(poses.shape) == (N, 2, Tx, 17) and torch.isfinite(poses).all()
    mf = m.map_frames(None, N).cpu().numpy()
    ref = lambda p, c, n, **kw: FR.assemble(p.cpu().numpy(), c.numpy(), n, **kw)
    for method, sm in (("unique", "mean"), ("mean", "median"), ("median", "mean")):
        got = forecast_track_rows(poses, tw.trans.numpy(), mf, forecast_assemble, windows=tw, method=method, spread_method=sm)
        want = forecast_track_rows(poses, tw.trans.numpy(), mf, ref, windows=tw, method=method, spread_method=sm)
        _same(tuple(t.cpu().numpy() for t in got[:3]), want[:3], (aggr, method, sm))
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        pose, count = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert count.max() == Tx and pose.shape == (13 + 9 + 6, 34)
        if method == "unique":      # every row: the slice of the lowest-index covering window's forecast, bit for bit
            first = {}
            for i in range(N // 2):
                for k in range(Tx):
                    first.setdefault(int(tw.base[i]) // 34 + int(mf[i, k]), (i, k))
            assert sorted(first) == np.flatnonzero(count).tolist()
            p = poses.cpu().numpy()
            for r, (i, k) in first.items():
                assert np.array_equal(pose[r].view(np.uint32), p[i, :, k].T.reshape(34).view(np.uint32)), r


@pytest.mark.parametrize("aggr", ["best", "median_pose"])
def test_pose_model_forecast_track_rows(aggr):
    from mocodad_amd.models.mocodad import MoCoDAD
    sd, cfg = golden_weights("inject")
    m = MoCoDAD(make_args(cfg, noise_steps=3, n_generated_samples=3, model_return_value="loss", aggregation_strategy="best")).to(DEV)
    m.load_state_dict(sd)
    assert cfg["seg_len"] == 6 and m.n_frames_corrupt == 3
    _check_module(m, _tracks(), aggr)


def test_latent_model_in_pose_space_forecast_track_rows():
    from test_latent_forecast_gpu import diffusion_module
    m, sd = diffusion_module()
    m.load_decoder(sd)
    try:
        _check_module(m, _tracks(), "best", space="pose")
    finally:
        m._decoder_sd = m._decoder = None


# ---------------------------------------------------------------- the driver
def _run_driver(cfg_path, out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", cfg_path, "--forecast-tracks", str(out), *extra],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "AUC:" in r.stdout and "forecast tracks:" in r.stdout, r.stdout[-2000:]
    return r.stdout, np.load(out)


def _track_checks(z, n_cond, Tx, max_cover=None):
    """max_cover None: a tail forecast (a row is forecast by at most Tx windows, the leading n_cond rows of a track by none)"""
    rows, frames, count = z["rows"], z["frames"], z["count"]
    R = len(rows)
    assert R > 0 and rows.shape == (R, 3) and frames.shape == (R,) and count.shape == (R,) and z["spread"].shape == (R,)
    assert z["expected_norm"].shape == (R, 34) and z["expected_norm"].dtype == np.float32 and list(z["joint_names"])[0] == "nose"
    assert 0 < count.max() <= (max_cover or Tx) and np.isfinite(z["expected_norm"]).all() and np.isfinite(z["spread"]).all()
    start = np.flatnonzero(np.r_[True, (rows[1:] != rows[:-1]).any(1)])
    for s in start if max_cover is None else ():
        assert not count[s:s + n_cond].any() and count[s + n_cond] == 1, "the leading n_cond rows of a track have no forecast"
    assert not z["expected_norm"][count == 0].any()
    return start


@pytest.mark.parametrize("config", ["hr_avenue_test.yaml", "ubnormal_latent_pose_test.yaml"], ids=["pose", "latent_pose"])
def test_driver_on_synthetic_clips(tmp_path, config):
    with open(os.path.join(ROOT, "configs", config)) as f:
        cfg = yaml.safe_load(f)
    cfg.update(noise_steps=4, n_generated_samples=2, exp_dir=str(tmp_path / "exp"))
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    stdout, z = _run_driver(str(p), tmp_path / "f.npz", "--synthetic", "4", "--random-init", "--device-windows", "--frames-per-clip", "40",
                            "--forecast-method", "mean")
    assert "expected_norm only" in stdout and "observed" not in z.files and "expected" not in z.files
    _track_checks(z, 3, 3)
    assert str(z["method"]) == "mean"


@pytest.mark.parametrize("draw", ["host", "device"])
def test_driver_under_random_imp(tmp_path, draw):
    """3 of 6 frames condition, another set per window: every window still forecasts 3 rows, a row is forecast by up to seg_len
    windows, and the rows follow each window's own set (MoCoDAD.map_frames of the masks the driver draws and passes on)."""
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(noise_steps=4, n_generated_samples=2, exp_dir=str(tmp_path / "exp"), conditioning_strategy="random_imp", conditioning_indices=3)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    stdout, z = _run_driver(str(p), tmp_path / "f.npz", "--synthetic", "2", "--random-init", "--device-windows", "--frames-per-clip", "30",
                            *(["--device-masks"] if draw == "device" else []))
    _track_checks(z, 3, 3, max_cover=6)
    n_windows = int(stdout.split("windows:")[1].split()[0])
    assert z["count"].sum() == n_windows // 5 * 3 and z["count"].max() > 3
    start = np.flatnonzero(np.r_[True, (z["rows"][1:] != z["rows"][:-1]).any(1)])
    assert any(z["count"][s:s + 3].any() for s in start), "some leading row of a track is forecast: the sets are not the tail"


def test_driver_on_the_dataset_fixture(tmp_path):
    from mocodad_amd.data import trajectories as T
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    from test_dataset_gpu import _driver_config, _write_scaler
    g = load_dataset_golden()
    cfg_path = _driver_config(tmp_path, g)
    args = load_config(cfg_path)
    _write_scaler(args.ckpt_dir, g["train_center"], g["train_scale"])
    torch.manual_seed(123)
    torch.save({"state_dict": MoCoDAD(args).state_dict()}, os.path.join(args.ckpt_dir, args.load_ckpt))
    stdout, z = _run_driver(cfg_path, tmp_path / "f.npz")
    assert "expected_norm only" not in stdout
    raw = T.load_raw(DATASET, "test", SEG_LEN)
    start = _track_checks(z, 3, 3)
    assert np.array_equal(z["observed"], raw.poses) and np.array_equal(z["frames"], raw.frames)
    assert np.array_equal(start, raw.offsets[:-1]) and [tuple(r) for r in z["rows"][start]] == raw.keys
    want = FR.denormalize(z["expected_norm"], raw.poses, VID_RES, g["train_center"], g["train_scale"], z["count"])
    assert np.array_equal(FR.bits(z["expected"]), FR.bits(want))
    assert (np.diff(z["frames"])[np.diff(z["frames"]) > 0] > 1).any(), "the CSV gaps reach the frame ids"

"""Host: forecast tracks without a GPU.

  - tests/forecast_ref.py, the float64 restatement the kernels are held to, against the REFERENCE's compute_fig_matrix +
    extract_single_pose through tests/golden/forecast_tracks.npz (tests/golden/gen_forecast_golden.py): within 1 fp32 ulp of the
    reference value rounded to fp32 -- both compute in float64 and round once; they differ in the order of NumPy's pairwise sums
    along a contiguous axis, which can move a float64 result by an ulp of ITS precision and so, rarely, the fp32 rounding by one;
  - reference_std_score against the reference's std_score, bit for bit (the same float64 operations);
  - the cell builders (dense, trajectory-aligned, the transform filter, per-window 'random_imp' frames) and forecast_track_rows
    on both of its sources;
  - the wrappers' and the driver's refusals, all of which come before anything touches a device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import forecast_ref as FR
from conftest import load_golden
from mocodad_amd.utils.eval_utils import forecast_cells_aligned, forecast_cells_dense, forecast_track_rows, reference_std_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("forecast_tracks.npz")


def _person(g, p):
    pos, fp, nf = g[f"p{p}_pos"], g[f"p{p}_frames_pos"], int(g[f"p{p}_n_frames"])
    return pos, fp, nf, forecast_cells_dense(np.zeros(len(pos), np.int64), fp, np.zeros(len(pos), np.int64), nf)


def test_restatement_against_the_reference(golden):
    g = golden
    assert int(g["n_persons"]) == 9
    covers = set()
    for p in range(9):
        pos, fp, nf, cell = _person(g, p)
        want_count = np.bincount(fp.reshape(-1) - 1, minlength=nf)
        covers |= set(want_count.tolist())
        for method in FR.METHODS:
            for sm in FR.SPREADS:
                pose, count, spread = FR.assemble(pos, cell, nf, method, sm, max_cover=32)
                assert np.array_equal(count, want_count)
                ref_pose, ref_std = g[f"p{p}_single_{method}"].astype(np.float32), g[f"p{p}_std_{sm}"].astype(np.float32)
                d_pose, d_std = FR.ulp_distance(pose, ref_pose).max(), FR.ulp_distance(spread, ref_std).max()
                print(f"person {p} {method}/{sm}: pose {d_pose} ulp, spread {d_std} ulp")
                assert d_pose <= 1 and d_std <= 1, (p, method, sm)
                assert not pose[count == 0].any() and not spread[count == 0].any()
    assert covers >= set(range(13)), "cover counts 0, 1, 2, 3 and every even and odd count up to 12"


def test_reference_std_score(golden):
    g = golden
    for p in range(9):
        for sm in FR.SPREADS:
            assert np.array_equal(reference_std_score(g[f"p{p}_std_{sm}"]), g[f"p{p}_score_{sm}"]), (p, sm)
    assert np.array_equal(reference_std_score(np.full(4, 0.25)), np.zeros(4))          # a constant vector: scale 1


def test_cell_builders():
    frames = np.array([[3, 4], [4, 5], [9, 10], [0, 11]])
    cell = forecast_cells_dense([0, 0, 1, 1], frames, [0, 0, 0, 0], 10)
    assert cell.dtype == np.int32 and cell.tolist() == [[2, 3], [3, 4], [18, 19], [-1, -1]]       # frames 0 and 11 fall outside 1 .. 10
    assert forecast_cells_dense([0, 0, -1, 1], frames, [0, 1, 0, 2], 10).tolist() == [[2, 3], [-1, -1], [-1, -1], [-1, -1]]
    base = np.array([0, 34, 68, 340]) * 1
    mf = np.array([[3, 5], [3, 5], [0, 1], [4, 5]])        # per-window frames ('random_imp')
    assert forecast_cells_aligned(base, mf, [0, 0, 0, 0]).tolist() == [[3, 5], [4, 6], [2, 3], [14, 15]]
    assert forecast_cells_aligned(base, mf, [0, 3, 0, 1]).tolist() == [[3, 5], [-1, -1], [2, 3], [-1, -1]]


def _ref_assemble(poses, cell, n_cells, **kw):
    return FR.assemble(poses.numpy(), cell.numpy(), n_cells, **kw)


@pytest.mark.parametrize("random_imp", [False, True], ids=["tail", "random_imp"])
def test_forecast_track_rows_on_both_sources(random_imp):
    """Two persons (8 and 7 rows, the second with a gap in its frame ids), seg_len 5, 2 transforms: the trajectory-aligned cells
    of a TrajectoryWindows and the (scene, clip, person, frame id) rows built from meta / frames number the same rows; UNIQUE is
    the lowest-index covering window's forecast; windows of transform 1 contribute nothing."""
    from mocodad_amd.data.windows import TrajectoryWindows
    rng = np.random.default_rng(3)
    trajs = {(1, 2, 0): (5, rng.normal(size=(8, 2, 17)).astype(np.float32)), (1, 2, 3): (1, rng.normal(size=(7, 2, 17)).astype(np.float32))}
    tw = TrajectoryWindows(trajs, 5, 2)
    tw.frames[tw.meta[:, 2] == 3] += (tw.frames[tw.meta[:, 2] == 3] > 4).int() * 6        # ids 1 .. 4, then 11 .. 13
    N, Tx = len(tw), 3
    assert N == 2 * (4 + 3)
    if random_imp:
        mf = np.stack([np.sort(rng.permutation(5)[:Tx]) for _ in range(N)])
    else:
        mf = np.tile(np.arange(2, 5), (N, 1))
    poses = torch.from_numpy(rng.normal(size=(N, 2, Tx, 17)).astype(np.float32))
    a = forecast_track_rows(poses, tw.trans.numpy(), mf, _ref_assemble, windows=tw, method="unique")
    b = forecast_track_rows(poses, tw.trans.numpy(), mf, _ref_assemble, meta=tw.meta.numpy(), frames=tw.frames.numpy(), method="unique")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    pose, count, spread, rows, fids = a
    assert pose.shape == (15, 34) and rows.tolist() == [[1, 2, 0]] * 8 + [[1, 2, 3]] * 7
    assert fids.tolist() == list(range(5, 13)) + [1, 2, 3, 4, 11, 12, 13]
    want_count = np.zeros(15, int)
    first = {}
    for i in range(N // 2):                                   # transform 0 only
        r0 = int(tw.base[i]) // 34
        for t in range(Tx):
            want_count[r0 + mf[i, t]] += 1
            first.setdefault(r0 + int(mf[i, t]), (i, t))
    assert np.array_equal(count, want_count) and count.max() <= (5 if random_imp else Tx)
    if not random_imp:
        assert not count[:2].any() and not count[8:10].any(), "the leading n_cond rows of a track have no forecast"
    for r, (i, t) in first.items():
        assert np.array_equal(pose[r], poses[i, :, t].numpy().T.reshape(34)), r
    with pytest.raises(ValueError, match="TrajectoryWindows or"):
        forecast_track_rows(poses, tw.trans.numpy(), mf, _ref_assemble)
    with pytest.raises(ValueError, match="per window"):
        forecast_track_rows(poses[:-1], tw.trans.numpy(), mf, _ref_assemble, windows=tw)


def test_restatement_edges():
    """k = max_cover is combined, k = max_cover + 1 is NaN with its true count; a NaN forecast stays in its cells; even-k median."""
    rng = np.random.default_rng(5)
    poses = rng.normal(size=(6, 2, 1, 17)).astype(np.float32)
    poses[4, 0, 0, 3] = np.nan
    cell = np.array([[0], [0], [1], [1], [2], [1]])
    pose, count, spread = FR.assemble(poses, cell, 4, "median", "median", max_cover=2)
    assert count.tolist() == [2, 3, 1, 0] and np.isnan(pose[1]).all() and np.isnan(spread[1])
    rows = poses.transpose(0, 2, 3, 1).reshape(6, 34).astype(np.float64)
    assert np.array_equal(pose[0], ((rows[0] + rows[1]) / 2).astype(np.float32)) and np.isfinite(spread[0])
    assert np.isnan(pose[2, 6]) and np.isnan(pose[2]).sum() == 1 and np.isnan(spread[2]) and not pose[3].any()


def test_denormalize_restatement_inverts_the_loader_spec():
    from dataset_spec import normalise, stress_rows
    raw = stress_rows(500, seed=2)
    rng = np.random.default_rng(8)
    center, scale = rng.normal(0, 0.2, 34), rng.uniform(0.05, 1.5, 34)
    norm = normalise(raw, (640, 360), center, scale)
    back = FR.denormalize(norm, raw, (640, 360), center, scale)
    ok = (raw != 0) & (norm != 0)
    assert ok.sum() > 5000 and np.abs(back - raw)[ok].max() < 1e-3
    assert not FR.denormalize(norm, raw, (640, 360), center, scale, count=np.zeros(500, int)).any()


def test_wrapper_argument_errors():
    from mocodad_amd.engine import denormalize_poses, forecast_assemble
    poses, cell = torch.zeros(4, 2, 3, 17), torch.zeros(4, 3, dtype=torch.int32)
    for kw, msg in ((dict(method="mode"), "method must be one of"), (dict(spread_method="unique"), "spread_method must be"),
                    (dict(max_cover=0), "max_cover must be in 1 .. 32"), (dict(max_cover=33), "max_cover must be in 1 .. 32")):
        with pytest.raises(ValueError, match=msg):
            forecast_assemble(poses, cell, 5, **kw)
    with pytest.raises(ValueError, match="n_cells must be >= 0"):
        forecast_assemble(poses, cell, -1)
    with pytest.raises(ValueError, match=r"poses must have shape \(N, 2, Tx, 17\)"):
        forecast_assemble(torch.zeros(4, 3, 2, 17), cell, 5)
    with pytest.raises(ValueError, match=r"poses must have shape \(N, 2, Tx, 17\)"):
        forecast_assemble(torch.zeros(4, 2, 33, 17), torch.zeros(4, 33, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="cell must be an integer"):
        forecast_assemble(poses, torch.zeros(4, 2, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="cell must be an integer"):
        forecast_assemble(poses, torch.zeros(4, 3), 5)
    with pytest.raises(ValueError, match="three buffers"):
        forecast_assemble(poses, cell, 5, device="cuda:0", out=(torch.zeros(5, 34),))
    with pytest.raises(ValueError, match=r"out\[0\] \(pose\) must be"):
        forecast_assemble(poses, cell, 5, device="cuda:0", out=(torch.zeros(5, 34), torch.zeros(5, dtype=torch.int32), torch.zeros(5)))
    with pytest.raises(ValueError, match="workspace must be"):
        forecast_assemble(poses, cell, 5, device="cuda:0", workspace=torch.zeros(5 * 32 - 1, dtype=torch.int32))
    norm, raw = torch.zeros(3, 34), np.ones((3, 34), np.float32)
    with pytest.raises(ValueError, match="go together"):
        denormalize_poses(norm, raw, (640, 360), center=np.zeros(34))
    with pytest.raises(ValueError, match=r"norm must be \(n, 34\)"):
        denormalize_poses(torch.zeros(3, 2, 17), raw, (640, 360))
    with pytest.raises(ValueError, match="raw pose rows must be"):
        denormalize_poses(norm, raw[:2], (640, 360))
    with pytest.raises(ValueError, match="NaN"):
        denormalize_poses(norm, np.full((3, 34), np.nan, np.float32), (640, 360))
    with pytest.raises(ValueError, match="count must be an integer"):
        denormalize_poses(norm, raw, (640, 360), count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="vid_res must be finite"):
        denormalize_poses(norm, raw, (float("inf"), 360))
    with pytest.raises(ValueError, match="center must hold 34"):
        denormalize_poses(norm, raw, (640, 360), center=np.zeros(33), scale=np.ones(34))
    with pytest.raises(ValueError, match="out must be"):
        denormalize_poses(norm, raw, (640, 360), device="cuda:0", out=torch.zeros(3, 2, 17))


def _refused(tmp_path, config, over, extra=(), env=None):
    with open(os.path.join(ROOT, "configs", config)) as f:
        cfg = yaml.safe_load(f)
    cfg.update(over)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    # no device is visible to the child: a refusal that came after a GPU call would fail differently
    e = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", **(env or {}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", str(p), "--synthetic", "2", "--random-init",
                        "--forecast-tracks", str(tmp_path / "f.npz"), *extra], capture_output=True, text=True, timeout=300, cwd=ROOT, env=e)
    assert r.returncode != 0 and not (tmp_path / "f.npz").exists()
    return r.stderr


@pytest.mark.parametrize("aggr,msg", [("mean", "selects none"), ("median", "selects none"), ("quantile:0.3", "selects none"),
                                      ("all", "one forecast per window"), ("random", "one forecast per window")])
def test_driver_refuses_aggregations_without_one_selected_pose(tmp_path, aggr, msg):
    err = _refused(tmp_path, "hr_avenue_test.yaml", dict(aggregation_strategy=aggr))
    assert "--forecast-tracks" in err and msg in err and repr(aggr) in err, err[-2000:]


def test_driver_refuses_more_than_one_process_and_the_latent_space(tmp_path):
    err = _refused(tmp_path, "hr_avenue_test.yaml", {}, env=dict(WORLD_SIZE="2"))
    assert "--forecast-tracks runs in one process" in err, err[-2000:]
    err = _refused(tmp_path, "ubnormal_latent_test.yaml", {})
    assert "--forecast-tracks needs the pose model, or the latent model with latent_score_space: 'pose'" in err, err[-2000:]
    err = _refused(tmp_path, "ubnormal_latent_pose_test.yaml", {}, extra=("--latent-score-space", "latent"))
    assert "--forecast-tracks needs the pose model" in err, err[-2000:]
    err = _refused(tmp_path, "hr_avenue_test.yaml", {}, extra=("--joint-scores", str(tmp_path / "j.npz")))
    assert "separate runs" in err, err[-2000:]

"""Dataset loader (mocodad_amd/data/trajectories.py) on the host: listing, parsing, the short-trajectory filter, window meta /
frame ids, the scaler pickle and the unsupported settings, against the fixture the reference's own pipeline made
(tests/golden/gen_dataset_golden.py).  The NumPy restatement of the per-frame normalisation (tests/dataset_spec.py) is pinned
to the reference's X_local bit for bit here; tests/test_dataset_gpu.py holds the kernel to it."""
import argparse
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from dataset_spec import DATASET, ROOT, bbox_centre, load_dataset_golden, normalise
from mocodad_amd.data import trajectories as T
from mocodad_amd.data.windows import TrajectoryWindows

SEG_LEN = 6
VID_RES = (640, 360)


def _windows_of(raw, seg_len=SEG_LEN, num_transform=1):
    buf = torch.zeros(raw.poses.shape[0] * 34)
    return TrajectoryWindows.from_buffer(buf, raw.offsets, raw.frames, raw.keys, seg_len, num_transform)


def _by_meta(meta):
    return {tuple(int(v) for v in m): i for i, m in enumerate(meta)}


def _rows_to_windows(rows, raw, seg_len=SEG_LEN):
    """(rows, 34) per-row values -> {meta: (seg_len, 34)} of every stride-1 window of the kept trajectories."""
    out = {}
    for i, key in enumerate(raw.keys):
        a, b = raw.offsets[i], raw.offsets[i + 1]
        for s in range(a, b - seg_len + 1):
            out[key + (int(raw.frames[s]),)] = rows[s:s + seg_len]
    return out


def test_listing_parsing_and_window_ids_match_the_reference():
    g = load_dataset_golden()
    raw = T.load_raw(DATASET, "test", SEG_LEN)
    assert raw.n_files == 22 and len(raw.keys) == 14            # one-row and shorter-than-seg_len CSVs are dropped
    assert raw.keys == sorted(raw.keys) and raw.poses.dtype == np.float32 and raw.frames.dtype == np.int32
    tw = _windows_of(raw)
    assert len(tw) == tw.n_samples == len(g["meta"])
    mine, ref = _by_meta(tw.meta.numpy()), _by_meta(g["meta"])
    assert mine.keys() == ref.keys()
    for k, i in mine.items():
        assert np.array_equal(tw.frames[i].numpy(), g["frames"][ref[k]]), k
    # the CSVs have gaps in their frame column: a window's frame ids are the rows' frame numbers, not first_frame + t
    assert (np.diff(g["frames"], axis=1) > 1).any()
    vraw = T.load_raw(DATASET, "validation", SEG_LEN)
    vtw = _windows_of(vraw)
    assert _by_meta(vtw.meta.numpy()).keys() == _by_meta(g["meta_val"]).keys()


def test_numpy_restatement_matches_the_reference_bit_for_bit():
    g = load_dataset_golden()
    assert int(np.__version__.split(".")[0]) >= 2, "the fixture and the spec follow NumPy >= 2 scalar promotion"
    raw = T.load_raw(DATASET, "test", SEG_LEN)
    for name, c, s in (("X_local", g["train_center"], g["train_scale"]), ("X_local_bbox", None, None)):
        wins = _rows_to_windows(normalise(raw.poses, VID_RES, c, s), raw)
        for k, i in _by_meta(g["meta"]).items():
            assert np.array_equal(wins[k].view(np.uint32), g[name][i].view(np.uint32)), (name, k)
    vraw = T.load_raw(DATASET, "validation", SEG_LEN)
    # the validation split fits its own scaler on the bbox rows (zeros masked): same statistics as the reference's fit
    center, scale = T.fit_validation_scaler(bbox_centre(vraw.poses, VID_RES))
    assert np.array_equal(center, g["val_center"].astype(np.float64)) and np.array_equal(scale, g["val_scale"])
    wins = _rows_to_windows(normalise(vraw.poses, VID_RES, center, scale), vraw)
    for k, i in _by_meta(g["meta_val"]).items():
        assert np.array_equal(wins[k].view(np.uint32), g["X_local_val"][i].view(np.uint32)), k


def test_fixture_holds_the_corner_cases():
    raw = T.load_raw(DATASET, "test", SEG_LEN)
    x, y = raw.poses[:, 0::2], raw.poses[:, 1::2]
    assert ((raw.poses == 0).all(1)).any()                                       # all-zero frame
    assert (((x == 0).all(1)) & ((y != 0).any(1))).any()                         # x all zero, y not
    assert ((raw.poses == 0).any(1) & (raw.poses != 0).any(1)).any()             # missing joints
    assert (x < 0).any() and (y > VID_RES[1] - 1).any()                          # clipped boxes
    nzx = np.where(x != 0, x, np.nan)[(x != 0).any(1)]
    assert (np.nanmax(nzx, 1) == np.nanmin(nzx, 1)).any()                        # zero-width box
    assert ((np.nanmin(nzx, 1) == np.float32(12.5)) & (np.nanmax(nzx, 1) == np.float32(21.5))).any()     # .5 ties
    b = bbox_centre(raw.poses, VID_RES)
    assert ((b[:, 0::2] == 0).all(1) & (b[:, 1::2] != 0).any(1)).any()           # zero width, non-zero height


def test_scaler_pickle_round_trips(tmp_path):
    from sklearn.preprocessing import RobustScaler
    g = load_dataset_golden()
    sc = RobustScaler(quantile_range=(10.0, 90.0))
    sc.center_, sc.scale_ = g["train_center"], g["train_scale"]
    with open(tmp_path / "local_robust.pickle", "wb") as f:
        pickle.dump(sc, f)
    c, s = T.load_scaler_stats(str(tmp_path))
    assert c.dtype == s.dtype == np.float64
    assert np.array_equal(c, g["train_center"].astype(np.float64)) and np.array_equal(s, g["train_scale"])
    with pytest.raises(FileNotFoundError, match="local_robust.pickle"):
        T.load_scaler_stats(str(tmp_path / "nowhere"))


def test_from_buffer_agrees_with_the_constructor_on_gapless_trajectories():
    rng = np.random.default_rng(0)
    trajs = {(1, 2, 3): (4, rng.random((9, 2, 17), dtype=np.float32)), (2, 1, 1): (1, rng.random((6, 2, 17), dtype=np.float32)),
             (2, 1, 2): (7, rng.random((4, 2, 17), dtype=np.float32))}
    a = TrajectoryWindows(trajs, seg_len=6, num_transform=3)
    keys = sorted(trajs)
    off = np.concatenate([[0], np.cumsum([trajs[k][1].shape[0] for k in keys])])
    fid = np.concatenate([trajs[k][0] + np.arange(trajs[k][1].shape[0]) for k in keys])
    buf = torch.from_numpy(np.concatenate([trajs[k][1].reshape(-1) for k in keys]))
    b = TrajectoryWindows.from_buffer(buf, off, fid, keys, seg_len=6, num_transform=3)
    for name in ("base", "trans", "meta", "frames"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.materialize(), b.materialize())
    with pytest.raises(ValueError, match="ascending"):
        TrajectoryWindows.from_buffer(buf, off, fid, keys[::-1], seg_len=6)


def test_bad_names_and_duplicates_name_the_file(tmp_path):
    row = "1," + ",".join(["1.5"] * 34) + "\n"
    root = tmp_path / "testing" / "trajectories"
    (root / "01-0002").mkdir(parents=True)
    (root / "01-0002" / "0003.csv").write_text(row)
    (root / "1-2").mkdir()
    (root / "1-2" / "3.csv").write_text(row)
    with pytest.raises(ValueError, match=r"duplicate.*\(1, 2, 3\)"):
        T.load_raw(str(tmp_path), "test", 1)
    (root / "1-2" / "3.csv").unlink()
    (root / "scene7").mkdir()
    (root / "scene7" / "1.csv").write_text(row)
    with pytest.raises(ValueError, match="scene7"):
        T.load_raw(str(tmp_path), "test", 1)
    (root / "scene7" / "1.csv").unlink()
    (root / "scene7").rmdir()
    raw = T.load_raw(str(tmp_path), "test", 1)
    assert raw.keys == [(1, 2, 3)] and raw.poses.shape == (1, 34) and raw.frames.tolist() == [1]
    dbg = T.list_trajectory_files(str(root), debug=True)
    assert [k for k, _ in dbg] == [(1, 2, 3)]


UNSUPPORTED = [({"split": "train"}, "training is out of scope"),
               ({"normalization_strategy": "zero_one"}, "only 'robust'"),
               ({"kp18_format": True}, "kp18_format"),
               ({"headless": True}, "headless"),
               ({"num_coords": 6}, "include_global")]


@pytest.mark.parametrize("over,msg", UNSUPPORTED, ids=[next(iter(o)) for o, _ in UNSUPPORTED])
def test_unsupported_settings_fail_fast(over, msg):
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(over)
    with pytest.raises(ValueError, match=msg):
        T.check_supported(argparse.Namespace(**cfg))


def test_driver_rejects_unsupported_settings_before_any_gpu_call(tmp_path):
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(split="train", data_dir=str(tmp_path / "nowhere"))
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", str(p)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "training is out of scope" in r.stderr, r.stderr[-2000:]


def test_loader_without_a_gpu_raises_the_device_error(tmp_path, monkeypatch):
    from sklearn.preprocessing import RobustScaler
    g = load_dataset_golden()
    sc = RobustScaler()
    sc.center_, sc.scale_ = g["train_center"], g["train_scale"]
    with open(tmp_path / "local_robust.pickle", "wb") as f:
        pickle.dump(sc, f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    args = argparse.Namespace(split="test", data_dir=DATASET, seg_len=SEG_LEN, vid_res=list(VID_RES), ckpt_dir=str(tmp_path),
                              num_transform=5, normalization_strategy="robust", num_coords=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.load_dataset(args, "cuda:0")

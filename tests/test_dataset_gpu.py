"""Dataset loader on the GPU: mcd_normalize_poses against the reference's X_local (bit for bit), against the NumPy restatement
on a 100 k-frame stress set, the dataset-built windows x the five test-time transforms, and eval_MoCoDAD.py on the fixture."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import load_golden
from dataset_spec import DATASET, ROOT, load_dataset_golden, normalise, stress_rows
from mocodad_amd.data import trajectories as T
from mocodad_amd.data.windows import TrajectoryWindows, WindowBatch

pytestmark = pytest.mark.gpu
SEG_LEN = 6
VID_RES = (640, 360)
DEV = "cuda:0"


def _by_meta(meta):
    return {tuple(int(v) for v in m): i for i, m in enumerate(meta)}


def _write_scaler(d, center, scale):
    from sklearn.preprocessing import RobustScaler
    sc = RobustScaler(quantile_range=(10.0, 90.0))
    sc.center_, sc.scale_ = center, scale
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "local_robust.pickle"), "wb") as f:
        pickle.dump(sc, f)


def _golden_windows(x_local):
    """reference (N, T, 34) -> (N, C, T, V) as its dataset reshapes it (utils/dataset.py:255,271)."""
    return torch.from_numpy(np.ascontiguousarray(x_local.reshape(*x_local.shape[:2], 17, 2).transpose(0, 3, 1, 2)))


@pytest.mark.parametrize("case", ["scaled", "bbox", "validation"])
def test_normalize_poses_matches_reference_x_local(case):
    from mocodad_amd.engine import normalize_poses
    g = load_dataset_golden()
    split, x_name, meta_name = ("validation", "X_local_val", "meta_val") if case == "validation" else ("test", "X_local", "meta")
    stats = {"scaled": (g["train_center"], g["train_scale"]), "bbox": (None, None),
             "validation": (g["val_center"], g["val_scale"])}[case]
    if case == "bbox":
        x_name = "X_local_bbox"
    raw = T.load_raw(DATASET, split, SEG_LEN)
    buf = normalize_poses(raw.poses, VID_RES, *stats, device=DEV)
    tw = TrajectoryWindows.from_buffer(buf.reshape(-1), raw.offsets, raw.frames, raw.keys, SEG_LEN, 1)
    wins = WindowBatch(tw.buffer, tw.base.to(DEV), None, None, SEG_LEN).materialize().cpu()
    ref = _golden_windows(g[x_name])
    mine, theirs = _by_meta(tw.meta.numpy()), _by_meta(g[meta_name])
    assert mine.keys() == theirs.keys()
    order = torch.tensor([mine[k] for k in theirs])
    assert torch.equal(wins[order], ref)


def test_normalize_poses_matches_numpy_spec_on_a_stress_set():
    from mocodad_amd.engine import normalize_poses
    raw = stress_rows(100_000, seed=5)
    rng = np.random.default_rng(6)
    center = rng.normal(0, 0.2, 34).astype(np.float32)            # a float32 fit's center_ / float64 scale_, like sklearn's
    scale = rng.uniform(0.05, 1.5, 34)
    for c, s in ((center, scale), (None, None)):
        got = normalize_poses(raw, VID_RES, c, s, device=DEV).cpu()
        want = torch.from_numpy(normalise(raw, VID_RES, c, s).reshape(-1, 17, 2).transpose(0, 2, 1).copy())
        bad = (got != want).reshape(len(raw), -1).any(1).nonzero().flatten()[:5].tolist()
        assert not bad, (c is None, bad, raw[bad[0]].tolist())
    with pytest.raises(ValueError, match="NaN"):
        bad_raw = raw[:4].copy()
        bad_raw[1, 3] = np.nan
        normalize_poses(bad_raw, VID_RES, device=DEV)


def test_dataset_windows_match_reference_windows_times_transforms(tmp_path):
    import argparse
    g = load_dataset_golden()
    _write_scaler(str(tmp_path), g["train_center"], g["train_scale"])
    args = argparse.Namespace(split="test", data_dir=DATASET, seg_len=SEG_LEN, vid_res=list(VID_RES), ckpt_dir=str(tmp_path),
                              num_transform=5, normalization_strategy="robust", num_coords=2, debug=False)
    tw, timing = T.load_dataset(args, DEV)
    assert set(timing) == {"parse", "normalise"}
    n = tw.n_samples
    assert len(tw) == 5 * n == 5 * len(g["meta"])
    mat = tw.materialize().cpu().numpy()
    tr = load_golden("transforms.npz")          # the reference's own affine matrices (utils/dataset_utils.py:255-310)
    ref = _golden_windows(g["X_local"]).numpy().astype(np.float64)
    theirs = _by_meta(g["meta"])
    trans, meta, frames = tw.trans.numpy(), tw.meta.numpy(), tw.frames.numpy()
    assert (trans == np.repeat(np.arange(5), n)).all()
    for t in range(5):
        m = tr[f"mat_{t}"].astype(np.float64)
        x, y = ref[:, 0], ref[:, 1]
        want = np.stack([m[0, 0] * x + m[0, 1] * y + m[0, 2], m[1, 0] * x + m[1, 1] * y + m[1, 2]], 1)
        for i in range(t * n, (t + 1) * n):
            j = theirs[tuple(int(v) for v in meta[i])]
            assert np.array_equal(frames[i], g["frames"][j])
            np.testing.assert_allclose(mat[i], want[j], atol=1e-6, rtol=0)
    assert (np.diff(frames, axis=1) > 1).any()      # the CSV gaps reach the frame ids


def _driver_config(tmp_path, g):
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(data_dir=DATASET, test_path=os.path.join(DATASET, "testing", "test_frame_mask"), exp_dir=str(tmp_path / "exp"),
               dataset_choice="HR-STC", dir_name="fixture", noise_steps=4, n_generated_samples=2, batch_size=256,
               seg_len=SEG_LEN, vid_res=list(VID_RES), num_transform=5, seed=11)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_eval_driver_scores_the_fixture_like_test_step_on_the_reference_windows(tmp_path):
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    g = load_dataset_golden()
    cfg_path = _driver_config(tmp_path, g)
    args = load_config(cfg_path)
    _write_scaler(args.ckpt_dir, g["train_center"], g["train_scale"])
    torch.manual_seed(123)
    m = MoCoDAD(args)
    torch.save({"state_dict": m.state_dict()}, os.path.join(args.ckpt_dir, args.load_ckpt))
    dump = tmp_path / "scores.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", cfg_path, "--dump-scores", str(dump)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "upload+normalise" in r.stdout and "AUC:" in r.stdout, r.stdout
    d = np.load(dump)
    assert np.isfinite(d["auc"])
    # the same windows built on the host from the reference's X_local, in the loader's order ((scene, clip, person), start),
    # fed to test_step with the same window ids
    order = np.lexsort(g["meta"].T[::-1])
    x = g["X_local"][order]                                    # (N, T, 34)
    n, nt = len(order), 5
    buf = torch.from_numpy(np.ascontiguousarray(x.reshape(n, SEG_LEN, 17, 2).transpose(0, 1, 3, 2))).reshape(-1).to(DEV)
    base = (torch.arange(n, dtype=torch.int64) * SEG_LEN * 34).repeat(nt)
    trans = torch.arange(nt, dtype=torch.int32).repeat_interleave(n)
    meta = torch.from_numpy(g["meta"][order]).repeat(nt, 1)
    frames = torch.from_numpy(g["frames"][order]).repeat(nt, 1)
    from mocodad_amd.utils.transforms import affine_table
    aff = affine_table(nt).to(DEV)
    m = MoCoDAD(args).to(DEV)
    m.load_state_dict(torch.load(os.path.join(args.ckpt_dir, args.load_ckpt), map_location="cpu", weights_only=False)["state_dict"])
    m.save_tensors = False
    m.on_test_epoch_start()
    bs = args.batch_size
    with torch.no_grad():
        for i, lo in enumerate(range(0, n * nt, bs)):
            hi = min(lo + bs, n * nt)
            m._calls = lo
            m.test_step([WindowBatch(buf, base[lo:hi], trans[lo:hi], aff, SEG_LEN), trans[lo:hi].long(), meta[lo:hi],
                         frames[lo:hi]], i)
    auc = m.on_test_epoch_end()
    assert np.array_equal(m.last_scores.view(np.uint32), d["scores"].view(np.uint32))
    assert auc == float(d["auc"])

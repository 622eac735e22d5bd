#!/usr/bin/env python3
"""Generate the pose-dataset fixture of the trajectory loader by IMPORTING the reference (aleflabo/MoCoDAD) on CPU.

    python tests/golden/gen_dataset_golden.py        (needs the reference checkout; MOCODAD_REFERENCE=<path>)

Writes, deterministically (running it twice gives identical bytes):
  tests/golden/dataset/{training,testing,validating}/trajectories/<scene>-<clip>/<person>.csv   a small pose tree in the
      reference's layout (frame, x1, y1, ..., x17, y17 per row) with the cases the normalisation has to get right:
      missing joints, an all-zero frame, a frame whose x values are all zero, boxes clipped at the image border, zero-width
      and zero-height boxes, a box side on an exact .5 rounding tie, negative coordinates, gaps in the frame column, a
      one-row CSV and a trajectory shorter than seg_len;
  tests/golden/dataset/testing/test_frame_mask/<scene>_<clip>.npy   a ground-truth mask per test clip;
  tests/golden/dataset_golden.npz   what the reference's data_of_combined_model (utils/get_robust_data.py:24-134) makes of it:
      the training split's RobustScaler (center_ / scale_; the run with split='train'), the test split's X_local, window meta and
      frame ids (scaled with that scaler, and once with normalize_pose=False = the bounding-box stage alone), the validation
      split's X_local with the scaler it fits itself, and the NumPy / scikit-learn versions they were made with.

Only DATA is written; no reference source text is stored.  The box arithmetic follows NumPy's scalar promotion rules, which
changed in NumPy 2 (NEP 50: the 0.1 margin is float32 arithmetic there, float64 under NumPy 1.x); the fixture records the
version it was made with and the loader follows NumPy >= 2."""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

REF = os.environ.get("MOCODAD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "dataset")
SEG_LEN = 6
VID_RES = (640, 360)

# split -> {(scene, clip): number of persons}
TREE = {
    "training": {(1, 1): 3, (2, 1): 3},
    "testing": {(1, 1): 4, (1, 2): 3, (2, 1): 3, (2, 2): 4},
    "validating": {(1, 3): 2, (2, 3): 2},
}


def _pose(rng, n):
    """(n, 34) float32 of one person walking: a skeleton of 17 joints around a drifting centre, 2-decimal coordinates."""
    W, H = VID_RES
    c = np.array([rng.uniform(60, W - 60), rng.uniform(60, H - 60)])
    size = rng.uniform(30, 90)
    off = rng.normal(0, 0.3, size=(17, 2)) * size
    vel = rng.normal(0, 1.5, size=2)
    rows = []
    for t in range(n):
        p = c + vel * t + off + rng.normal(0, 1.0, size=(17, 2))
        rows.append(p.reshape(-1))
    x = np.round(np.array(rows), 2).astype(np.float32)
    miss = rng.random((n, 17)) < 0.08                       # missing joints: both coordinates 0
    x.reshape(n, 17, 2)[miss] = 0.0
    return x


def _special_rows():
    """Rows that pin the corner cases of utils/data.py:11-43,165-186."""
    rows = {}
    z = np.zeros(34, np.float32)
    rows["all_zero"] = z.copy()
    r = z.copy(); r[1::2] = np.linspace(100, 160, 17); r[1] = 0.0             # every x 0, y not: box (0, 0, 0, 0)
    rows["x_all_zero"] = r
    r = np.zeros(34, np.float32)                                              # left / right / top / bottom on .5 ties:
    r[0::2] = np.linspace(12.5, 21.5, 17); r[1::2] = np.linspace(100.5, 109.5, 17)    # margin 0.1 * 10 = 1 -> 11.5, 22.5
    rows["tie"] = r
    r = np.zeros(34, np.float32); r[0::2] = 100.0; r[1::2] = np.linspace(50, 120, 17)  # zero-width box (margin 0.1 rounds away)
    rows["zero_width"] = r
    r = np.zeros(34, np.float32); r[0::2] = np.linspace(200, 260, 17); r[1::2] = 80.0  # zero-height box
    rows["zero_height"] = r
    r = np.zeros(34, np.float32); r[0::2] = np.linspace(-12.25, 40, 17); r[1::2] = np.linspace(300, 371.5, 17)
    rows["border"] = r                                                        # negative x, y beyond H - 1: clipped box
    r = np.zeros(34, np.float32); r[0::2] = np.linspace(600, 655, 17); r[1::2] = np.linspace(-5, 30, 17)
    r[4:10] = 0.0
    rows["border2"] = r
    return rows


def _write_csv(path, frames, x):
    with open(path, "w", newline="\n") as f:
        for fr, row in zip(frames, x):
            f.write(",".join([str(int(fr))] + [f"{float(v):.9g}" for v in row]) + "\n")


def write_tree():
    rng = np.random.default_rng(20261016)
    special = _special_rows()
    gts = {}
    for split, clips in TREE.items():
        for (scene, clip), n_persons in clips.items():
            folder = os.path.join(ROOT, split, "trajectories", f"{scene:02d}-{clip:04d}")
            os.makedirs(folder, exist_ok=True)
            last = 0
            for person in range(1, n_persons + 1):
                n = int(rng.integers(20, 31))
                steps = np.where(rng.random(n) < 0.12, rng.integers(2, 4, n), 1)      # gaps in the frame column
                frames = int(rng.integers(1, 8)) + np.concatenate([[0], np.cumsum(steps[1:])])
                x = _pose(rng, n)
                if split != "training":
                    for j, name in enumerate(special):
                        if (j + person + clip) % 3 == 0:
                            x[int(rng.integers(0, n))] = special[name]
                _write_csv(os.path.join(folder, f"{person:04d}.csv"), frames, x)
                last = max(last, int(frames[-1]))
            if split == "testing":
                # a one-row CSV and a trajectory shorter than seg_len: both dropped (utils/preprocessing.py:4-10)
                _write_csv(os.path.join(folder, f"{n_persons + 1:04d}.csv"), [3], _pose(rng, 1))
                _write_csv(os.path.join(folder, f"{n_persons + 2:04d}.csv"), np.arange(5, 5 + SEG_LEN - 2),
                           _pose(rng, SEG_LEN - 2))
                n_fr = last + 4
                gt = np.zeros(n_fr, np.int64)
                a = int(rng.integers(0, n_fr // 2))
                gt[a:a + n_fr // 3] = 1
                gts[(scene, clip)] = gt
    mdir = os.path.join(ROOT, "testing", "test_frame_mask")
    os.makedirs(mdir, exist_ok=True)
    for (scene, clip), gt in gts.items():
        np.save(os.path.join(mdir, f"{scene:02d}_{clip:04d}.npy"), gt)


def save_npz(path, **arrs):
    """np.savez_compressed with fixed zip timestamps (identical bytes on every run)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {os.path.relpath(path, HERE)}: {os.path.getsize(path) / 1024:.1f} KiB")


def _windows(local):
    X, (meta, segs) = local
    return np.asarray(X, np.float32), np.asarray(meta, np.int64).reshape(-1, 4), np.asarray(segs, np.int32).reshape(-1, SEG_LEN)


def main():
    import shutil
    import sklearn
    if os.path.isdir(ROOT):
        shutil.rmtree(ROOT)
    write_tree()
    sys.path.insert(0, REF)
    from utils.get_robust_data import data_of_combined_model, load_scaler
    common = dict(trajectories_path=ROOT, seg_len=SEG_LEN, seg_stride=1, vid_res=list(VID_RES), normalization_strategy="robust",
                  reconstruct_original_data=False, include_global=False, debug=False)
    out = {}
    with tempfile.TemporaryDirectory() as exp:
        data_of_combined_model(exp_dir=exp, split="train", normalize_pose=True, **common)
        sc = load_scaler(os.path.join(exp, "local_robust.pickle"))
        out["train_center"], out["train_scale"] = np.asarray(sc.center_), np.asarray(sc.scale_)
        _, local = data_of_combined_model(exp_dir=exp, split="test", normalize_pose=True, **common)
        out["X_local"], out["meta"], out["frames"] = _windows(local)
        _, local = data_of_combined_model(exp_dir=exp, split="test", normalize_pose=False, **common)
        out["X_local_bbox"], meta_b, _ = _windows(local)
        assert np.array_equal(meta_b, out["meta"])
        _, local = data_of_combined_model(exp_dir=exp, split="validation", normalize_pose=True, **common)
        out["X_local_val"], out["meta_val"], out["frames_val"] = _windows(local)
        sc = load_scaler(os.path.join(exp, "local_robust_val.pickle"))
        out["val_center"], out["val_scale"] = np.asarray(sc.center_), np.asarray(sc.scale_)
    out["seg_len"], out["vid_res"] = np.int64(SEG_LEN), np.asarray(VID_RES, np.int64)
    out["numpy_version"], out["sklearn_version"] = np.array(np.__version__), np.array(sklearn.__version__)
    save_npz(os.path.join(HERE, "dataset_golden.npz"), **out)


if __name__ == "__main__":
    main()

"""On-disk pose datasets -> a normalised trajectory buffer on the device (the reference's PoseDatasetRobust at test time:
utils/dataset.py:286-316 -> utils/get_robust_data.py:24-134).

The reference walks {data_dir}/{training|testing|validating}/trajectories/<folder>/<file>.csv, keeps the trajectories of at
least seg_len rows, then loops over every frame in Python to move the joints into bounding-box-centre coordinates
(utils/data.py:165-186) and applies the RobustScaler the training run pickled (utils/data.py:350-359).  Here the files are
parsed on the host (np.loadtxt, as the reference does), all kept rows cross PCIe once as one flat buffer, and the per-frame
normalisation is one HIP kernel (mcd_normalize_poses) writing the buffer TrajectoryWindows reads windows from.

Differences from the reference, none of which changes a window's values:
  - trajectories are ordered by (scene, clip, person) (the reference follows os.listdir, whose order is unspecified; scores
    are keyed by their metadata, so the AUC does not depend on it);
  - `debug: true` keeps the first 5 folders of the SORTED listing (the reference: the first 5 os.listdir returns);
  - a validation run that fits its own scaler (split 'validation', path without 'UBnormal', get_robust_data.py:122-125) does not
    write the reference's local_robust_val.pickle side file."""
import os
import pickle
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

N_FEATURES = 34          # x1, y1, ..., x17, y17
MAX_WORKERS = 16


def split_subfolder(split: str) -> str:
    """utils/get_robust_data.py:32-37."""
    if "train" in split:
        return "training"
    if "test" in split:
        return "testing"
    return "validating"


def trajectories_root(data_dir: str, split: str) -> str:
    return os.path.join(data_dir, split_subfolder(split), "trajectories")


def parse_trajectory_id(folder: str, file_name: str) -> Tuple[int, int, int]:
    """(scene, clip, person) of <folder>/<file_name> as the reference derives it (utils/data.py:229-232,
    utils/preprocessing.py:25-26: id = folder + '_' + file stem; scene, clip = ints of id.split('_')[0].split('-');
    person = int(id.split('_')[1]))."""
    tid = folder + "_" + file_name.split(".")[0]
    try:
        scene, clip = map(int, tid.split("_")[0].split("-"))
        person = int(tid.split("_")[1])
    except (ValueError, IndexError):
        raise ValueError(f"{os.path.join(folder, file_name)}: cannot derive (scene, clip, person) from the trajectory id "
                         f"{tid!r} (expected <scene>-<clip>/<person>.csv)") from None
    return scene, clip, person


def list_trajectory_files(root: str, debug: bool = False) -> List[Tuple[Tuple[int, int, int], str]]:
    """[((scene, clip, person), path)] of every file under root/<folder>/, sorted by key.  debug: the first 5 folders of the
    sorted listing only."""
    if not os.path.isdir(root):
        raise FileNotFoundError(f"trajectory directory {root} not found")
    folders = sorted(f for f in os.listdir(root) if os.path.isdir(os.path.join(root, f)))
    if debug:
        folders = folders[:5]
    seen: Dict[Tuple[int, int, int], str] = {}
    for folder in folders:
        for name in sorted(os.listdir(os.path.join(root, folder))):
            path = os.path.join(root, folder, name)
            key = parse_trajectory_id(folder, name)
            if key in seen:
                raise ValueError(f"{path}: duplicate trajectory (scene, clip, person) = {key}, already read from {seen[key]}")
            seen[key] = path
    return sorted((k, p) for k, p in seen.items())


def read_trajectory_csv(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(frames int32 (F,), poses float32 (F, 34)) exactly as utils/data.py:228-229 reads them."""
    t = np.loadtxt(path, dtype=np.float32, delimiter=",", ndmin=2)
    if t.shape[0] and t.shape[1] != 1 + N_FEATURES:
        raise ValueError(f"{path}: expected {1 + N_FEATURES} columns (frame, x1, y1, ..., x17, y17), got {t.shape[1]}")
    if not t.shape[0]:
        t = np.zeros((0, 1 + N_FEATURES), np.float32)
    return t[:, 0].astype(np.int32), np.ascontiguousarray(t[:, 1:])


@dataclass
class RawTrajectories:
    """The kept trajectories of a split, in (scene, clip, person) order: rows keys[i] are poses[offsets[i]:offsets[i+1]]."""
    keys: List[Tuple[int, int, int]]
    offsets: np.ndarray          # (n + 1,) int64 row offsets
    frames: np.ndarray           # (rows,) int32 frame column of the CSVs
    poses: np.ndarray            # (rows, 34) float32 columns 1..34
    n_files: int = 0
    timing: Dict[str, float] = field(default_factory=dict)


def load_raw(data_dir: str, split: str, seg_len: int, debug: bool = False) -> RawTrajectories:
    """Walk + parse (a thread pool of at most 16 workers) + drop the trajectories shorter than seg_len
    (utils/preprocessing.py:4-10 with the test-time stride 1)."""
    t0 = time.perf_counter()
    files = list_trajectory_files(trajectories_root(data_dir, split), debug=debug)
    workers = max(1, min(MAX_WORKERS, os.cpu_count() or 1, len(files)))
    with ThreadPoolExecutor(max_workers=workers) as ex:
        parsed = list(ex.map(lambda kp: read_trajectory_csv(kp[1]), files))
    keys, frames, poses = [], [], []
    for (key, _), (fr, po) in zip(files, parsed):
        if len(fr) < seg_len:
            continue
        keys.append(key)
        frames.append(fr)
        poses.append(po)
    offsets = np.zeros(len(keys) + 1, np.int64)
    offsets[1:] = np.cumsum([len(f) for f in frames])
    raw = RawTrajectories(keys, offsets,
                          np.concatenate(frames) if frames else np.zeros(0, np.int32),
                          np.concatenate(poses) if poses else np.zeros((0, N_FEATURES), np.float32), n_files=len(files))
    raw.timing["parse"] = time.perf_counter() - t0
    return raw


def load_scaler_stats(ckpt_dir: str) -> Tuple[np.ndarray, np.ndarray]:
    """center_ / scale_ of the RobustScaler the training run pickled to {ckpt_dir}/local_robust.pickle
    (utils/get_robust_data.py:116-127)."""
    path = os.path.join(ckpt_dir, "local_robust.pickle")
    if not os.path.exists(path):
        raise FileNotFoundError(f"robust scaler {path} not found (the training run writes it next to the checkpoint)")
    with open(path, "rb") as f:
        sc = pickle.load(f)
    center, scale = np.asarray(sc.center_, dtype=np.float64), np.asarray(sc.scale_, dtype=np.float64)
    if center.shape != (N_FEATURES,) or scale.shape != (N_FEATURES,):
        raise ValueError(f"{path}: expected a scaler over {N_FEATURES} features, got center_ {center.shape}, scale_ {scale.shape}")
    return center, scale


def fit_validation_scaler(bbox_rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """RobustScaler(quantile_range=(10, 90)) fitted on the bounding-box-normalised rows (rows, 34) with exact zeros masked as
    missing (utils/data.py:350-354)."""
    from sklearn.preprocessing import RobustScaler
    x = np.where(bbox_rows == 0.0, np.nan, bbox_rows)
    sc = RobustScaler(quantile_range=(10.0, 90.0)).fit(x)
    return np.asarray(sc.center_, dtype=np.float64), np.asarray(sc.scale_, dtype=np.float64)


def fits_own_scaler(split: str, data_dir: str) -> bool:
    """utils/get_robust_data.py:122: a validation run on a dataset other than UBnormal fits its own scaler."""
    return split == "validation" and "UBnormal" not in trajectories_root(data_dir, split)


def check_supported(args) -> None:
    """Settings the device loader does not cover fail here, before any file or GPU is touched."""
    g = lambda k, d=None: getattr(args, k, d)
    split = str(g("split", "test"))
    if "train" in split:
        raise ValueError(f"split: {split!r}: training is out of scope (this driver evaluates the 'test' / 'validation' split)")
    if g("normalization_strategy", "robust") != "robust":
        raise ValueError(f"normalization_strategy: {g('normalization_strategy')!r}: only 'robust' is supported (the reference "
                         "reads a different pipeline of pose JSON files otherwise, utils/dataset.py:313-314)")
    if g("kp18_format", False):
        raise ValueError("kp18_format: true is not supported (the loader produces the 17 COCO keypoints of the CSVs)")
    if g("headless", False):
        raise ValueError("headless: true is not supported (the loader produces all 17 keypoints)")
    if int(g("num_coords", 2)) != 2:
        raise ValueError(f"num_coords: {g('num_coords')}: only 2 is supported (6 = include_global, the global "
                         "bounding-box features, is not built)")


def load_dataset(args, device):
    """The test-time dataset of `args` (the reference's YAML keys) as a TrajectoryWindows on `device`: parse, upload the raw
    rows once, normalise them with mcd_normalize_poses into the trajectory buffer.  Returns (windows, timing) with timing =
    {'parse': s, 'normalise': s} (the second includes the upload and, for a self-fitted validation scaler, the fit).  The windows
    keep what takes a normalised row back to pixels: `.raw` (the RawTrajectories: row r of the buffer is raw.poses[r]), `.scaler`
    ((center, scale)) and `.vid_res`."""
    import torch
    from ..engine import normalize_poses
    from .windows import TrajectoryWindows

    check_supported(args)
    split = str(getattr(args, "split", "test"))
    seg_len = int(args.seg_len)
    raw = load_raw(args.data_dir, split, seg_len, debug=bool(getattr(args, "debug", False)))
    if not raw.keys:
        raise ValueError(f"no trajectory of at least seg_len = {seg_len} rows under {trajectories_root(args.data_dir, split)}")
    own = fits_own_scaler(split, args.data_dir)
    stats = None if own else load_scaler_stats(args.ckpt_dir)
    t0 = time.perf_counter()
    vid_res = tuple(getattr(args, "vid_res", (1080, 720)))
    if not torch.cuda.is_available():
        raise RuntimeError("mocodad_amd needs an MI355X (gfx950) GPU: the scoring path has no CPU fallback")
    dev = torch.device(device)
    if own:
        bbox = normalize_poses(raw.poses, vid_res, device=dev)
        rows = bbox.permute(0, 2, 1).reshape(-1, N_FEATURES).cpu().numpy()      # back to the interleaved feature order
        stats = fit_validation_scaler(rows)
        buf = normalize_poses(raw.poses, vid_res, *stats, device=dev, out=bbox)
    else:
        buf = normalize_poses(raw.poses, vid_res, *stats, device=dev)
    tw = TrajectoryWindows.from_buffer(buf.reshape(-1), raw.offsets, raw.frames, raw.keys, seg_len,
                                       int(getattr(args, "num_transform", 1)))
    # what takes a normalised row back to pixels (engine.denormalize_poses): row r of the buffer is raw.poses[r]
    tw.raw, tw.scaler, tw.vid_res = raw, stats, vid_res
    torch.cuda.synchronize(dev)
    raw.timing["normalise"] = time.perf_counter() - t0
    return tw, raw.timing

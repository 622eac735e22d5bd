#!/usr/bin/env python3
"""Load time of the dataset loader (mocodad_amd/data/trajectories.py) on a large synthetic pose tree.

    python tools/dataset_load_time.py [--clips 200] [--persons 8] [--rows 400] [--dir /tmp/mcd_load_tree]

Writes a tree in the reference's layout ({dir}/testing/trajectories/<scene>-<clip>/<person>.csv + a RobustScaler pickle),
then prints one JSON line: files, rows, windows, the parse time, the upload + normalise time of load_dataset, and the
mcd_normalize_poses kernel alone (device time of one launch over all rows, median of 10)."""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mocodad_amd.data import trajectories as T  # noqa: E402
from mocodad_amd.engine import normalize_poses  # noqa: E402


def write_tree(d, clips, persons, rows, seed=0):
    rng = np.random.default_rng(seed)
    for c in range(clips):
        folder = os.path.join(d, "testing", "trajectories", f"{c // 20 + 1:02d}-{c % 20 + 1:04d}")
        os.makedirs(folder, exist_ok=True)
        for p in range(1, persons + 1):
            x = rng.uniform(1, 630, (rows, 34)).astype(np.float32)
            x[rng.random((rows, 34)) < 0.05] = 0
            fr = np.arange(1, rows + 1, dtype=np.float32)[:, None]
            np.savetxt(os.path.join(folder, f"{p:04d}.csv"), np.hstack([fr, x]), fmt="%.3f", delimiter=",")
    from sklearn.preprocessing import RobustScaler
    sc = RobustScaler(quantile_range=(10.0, 90.0))
    sc.center_, sc.scale_ = np.zeros(34, np.float32), np.ones(34)
    os.makedirs(os.path.join(d, "ckpt"), exist_ok=True)
    with open(os.path.join(d, "ckpt", "local_robust.pickle"), "wb") as f:
        pickle.dump(sc, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--dir", default="/tmp/mcd_load_tree")
    a = ap.parse_args()
    t0 = time.perf_counter()
    write_tree(a.dir, a.clips, a.persons, a.rows)
    t_write = time.perf_counter() - t0
    args = argparse.Namespace(split="test", data_dir=a.dir, seg_len=6, vid_res=[640, 360], ckpt_dir=os.path.join(a.dir, "ckpt"),
                              num_transform=5, normalization_strategy="robust", num_coords=2, debug=False)
    torch.cuda.init()
    torch.zeros(1, device="cuda:0")
    tw, timing = T.load_dataset(args, "cuda:0")
    raw = T.load_raw(a.dir, "test", 6)
    dev_raw = torch.from_numpy(raw.poses).to("cuda:0")
    out = torch.empty(len(raw.poses), 2, 17, device="cuda:0")
    c, s = T.load_scaler_stats(args.ckpt_dir)
    ms = []
    for _ in range(11):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        normalize_poses(dev_raw, args.vid_res, c, s, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"files": raw.n_files, "rows": int(len(raw.poses)), "windows": len(tw), "write_s": round(t_write, 2),
                      "parse_s": round(timing["parse"], 3), "upload_normalise_s": round(timing["normalise"], 4),
                      "kernel_ms_median": round(float(np.median(ms[1:])), 4)}))


if __name__ == "__main__":
    main()

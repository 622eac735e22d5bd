"""Loader of the latentt_* fixtures (tests/golden/gen_latentt_golden.py): the latent model at 5 .. 12 corrupt frames -- 6 + 6 (S12),
12 + 12 through the integer form of conditioning_indices (S24, S24_hostile), 3 condition + 5 corrupt frames with 'E_unet' (S8U).
Test infrastructure; nothing under mocodad_amd/ imports it."""
import glob
import json
import os

import numpy as np
import torch

NAMES = ["S12", "S24", "S24_hostile", "S8U"]
AGGRS = ["best", "worst", "mean", "median", "quantile:0.3", "mean_pose", "median_pose"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def load(name: str):
    """-> (state_dict of float tensors, sorted [key, shape] list of the reference's full state_dict, YAML settings dict of this
    configuration, dict of recorded arrays).  Loaded once per session and shared: treat as read-only."""
    if name not in _cache:
        w = {}
        for p in sorted(glob.glob(os.path.join(GOLDEN, f"latentt_{name}_w[0-9].npz"))):
            d = np.load(p)
            w.update({k: d[k] for k in d.files})
        keys = json.loads(bytes(w.pop("__keys__")).decode())
        cfg = json.loads(bytes(w.pop("__cfg__")).decode())
        d = np.load(os.path.join(GOLDEN, f"latentt_{name}_io.npz"))
        io = {k: d[k] for k in d.files}
        _cache[name] = ({k: torch.from_numpy(v) for k, v in w.items()}, keys, cfg, io)
    return _cache[name]


def frame_lists(io):
    return [int(i) for i in io["cond_idx"]], [int(i) for i in io["corrupt_idx"]]


def batch_of(data: torch.Tensor):
    """The [data, transformation_idx, metadata, actual_frames] list MoCoDADlatent.forward takes."""
    B, T = data.shape[0], data.shape[2]
    return [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, T, dtype=torch.int32)]

"""Loader of the latentx_* fixtures (tests/golden/gen_latentx_golden.py): the latent model with the condition encoders the
shipped fixtures do not hold -- 'E_unet' (U, U_hostile), a runtime channel list (G), 7 condition frames (C7).  Test
infrastructure; nothing under mocodad_amd/ imports it."""
import glob
import json
import os

import numpy as np
import torch

NAMES = ["U", "U_hostile", "G", "C7"]
AGGRS = ["best", "worst", "mean", "median", "quantile:0.3", "mean_pose", "median_pose"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def load(name: str):
    """-> (state_dict of float tensors, sorted [key, shape] list of the reference's full state_dict, YAML settings dict of this
    configuration, dict of recorded arrays).  Loaded once per session and shared: treat as read-only."""
    if name not in _cache:
        w = {}
        for p in sorted(glob.glob(os.path.join(GOLDEN, f"latentx_{name}_w[0-9].npz"))):
            d = np.load(p)
            w.update({k: d[k] for k in d.files})
        keys = json.loads(bytes(w.pop("__keys__")).decode())
        cfg = json.loads(bytes(w.pop("__cfg__")).decode())
        d = np.load(os.path.join(GOLDEN, f"latentx_{name}_io.npz"))
        io = {k: d[k] for k in d.files}
        _cache[name] = ({k: torch.from_numpy(v) for k, v in w.items()}, keys, cfg, io)
    return _cache[name]


def frame_lists(io):
    return [int(i) for i in io["cond_idx"]], [int(i) for i in io["corrupt_idx"]]


def batch_of(data: torch.Tensor):
    """The [data, transformation_idx, metadata, actual_frames] list MoCoDADlatent.forward takes."""
    B, T = data.shape[0], data.shape[2]
    return [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, T, dtype=torch.int32)]

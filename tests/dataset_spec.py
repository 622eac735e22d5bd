"""NumPy restatement of the dataset loader's per-frame normalisation (the spec mcd_normalize_poses is tested against), and
helpers shared by tests/test_dataset_loader.py and tests/test_dataset_gpu.py.

Steps 3-4 of the reference's test-time pipeline (utils/data.py:11-43,165-186 then 350-359) under NumPy >= 2 scalar rules: the
box, its 0.1 margin and the clip in float32; sides rounded half-to-even to ints; (x - centre) and / size as float32
operations; RobustScaler.transform as float64 operations rounded to float32 after each; exact zeros (missing) stay 0."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATASET = os.path.join(ROOT, "tests", "golden", "dataset")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dataset_golden.npz")


def load_dataset_golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def bbox_centre(raw, vid_res):
    """(n, 34) float32 rows x1,y1,...,x17,y17 -> (n, 34) float32 bounding-box-centre coordinates."""
    raw = np.asarray(raw, np.float32)
    x, y = raw[:, 0::2], raw[:, 1::2]
    f32 = np.float32
    out = np.zeros_like(raw)
    ok = (x != 0).any(1) & (y != 0).any(1)
    sides = []
    for v, size in ((x, vid_res[0]), (y, vid_res[1])):
        nz = v != 0
        lo = np.where(nz, v, f32(np.inf)).min(1)
        hi = np.where(nz, v, f32(-np.inf)).max(1)
        lo, hi = np.where(ok, lo, f32(0)), np.where(ok, hi, f32(0))
        extra = f32(0.1) * ((hi - lo) + f32(1))
        top = f32(size) - f32(1)
        a = np.rint(np.minimum(np.maximum(lo - extra, f32(0)), top)).astype(np.int64)
        b = np.rint(np.minimum(np.maximum(hi + extra, f32(0)), top)).astype(np.int64)
        sides.append((a, b))
    for c, (v, (a, b)) in enumerate(zip((x, y), sides)):
        centre = ((a + b) / 2).astype(np.float32)[:, None]
        d = np.where(v == 0, centre, v) - centre                 # float32
        size = (b - a).astype(np.float32)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(size != 0, d / np.where(size != 0, size, f32(1)), f32(0))
        out[:, c::2] = np.where(ok[:, None], q, f32(0))
    return out


def robust_scale(rows, center, scale):
    """RobustScaler.transform of utils/data.py:350-359 on (n, 34) float32 rows: zeros are missing and stay 0."""
    rows = np.asarray(rows, np.float32)
    t = (rows.astype(np.float64) - np.asarray(center, np.float64)).astype(np.float32)
    t = (t.astype(np.float64) / np.asarray(scale, np.float64)).astype(np.float32)
    return np.where((rows != 0) & ~np.isnan(t), t, np.float32(0))


def normalise(raw, vid_res, center=None, scale=None):
    b = bbox_centre(raw, vid_res)
    return b if center is None else robust_scale(b, center, scale)


def stress_rows(n, seed=0, vid_res=(640, 360)):
    """(n, 34) float32 rows mixing missing joints, all-zero frames, x-only-zero frames, boxes clipped at (or beyond) the
    border, negative coordinates, half-integer ties and zero-width / zero-height boxes."""
    rng = np.random.default_rng(seed)
    W, H = vid_res
    c = np.stack([rng.uniform(-40, W + 40, n), rng.uniform(-40, H + 40, n)], 1)
    size = rng.uniform(0.5, 150, (n, 1, 1))
    p = c[:, None, :] + rng.normal(0, 0.4, (n, 17, 2)) * size
    kind = rng.integers(0, 10, n)
    p = np.where((kind == 1)[:, None, None], np.round(p * 2) / 2, p)             # half-integers
    p = np.where((kind == 2)[:, None, None], np.round(p), p)
    p[kind == 3, :, 0] = p[kind == 3, :1, 0]                                     # zero-width
    p[kind == 4, :, 1] = p[kind == 4, :1, 1]                                     # zero-height
    x = p.reshape(n, 34).astype(np.float32)
    miss = rng.random((n, 17)) < 0.15
    x.reshape(n, 17, 2)[miss] = 0
    x[kind == 5] = 0                                                             # all-zero frames
    x[kind == 6, 0::2] = 0                                                       # every x missing
    x[kind == 7, 1::2] = 0
    # exact .5 ties of a side: xmin = k + .5, xmax = xmin + 9 -> margin exactly 1
    t = np.flatnonzero(kind == 8)
    base = rng.integers(0, W - 20, len(t)) + np.float32(0.5)
    x[t, 0::2] = (base[:, None] + np.linspace(0, 9, 17)[None]).astype(np.float32)
    return x

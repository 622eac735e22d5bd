"""NumPy float64 restatement of mcd_forecast_assemble and mcd_denormalize_poses (include/mocodad_hip.h), with exactly the orders
the header states: what the kernels are held to bit for bit (tests/test_forecast_tracks_gpu.py), and what is itself held to the
reference's compute_fig_matrix + extract_single_pose (utils/eval_utils.py:13-24, 37-72) through tests/golden/forecast_tracks.npz
(tests/test_forecast_tracks_host.py).  Loops, no vectorised reductions: NumPy's own sums are pairwise along a contiguous axis."""
import numpy as np

METHODS = ("unique", "mean", "median")
SPREADS = ("mean", "median")


def _middle(col):
    """np.median's value of a 1-d float64 array by a stable sort (rank by (value, index), as the kernel counts ranks): the middle
    value, for an even length the half-sum of the two middle values; a NaN among them gives NaN."""
    if np.isnan(col).any():
        return np.float64(np.nan)
    s = np.sort(col, kind="stable")
    k = len(s)
    return (s[(k - 1) // 2] + s[k // 2]) / np.float64(2.0)


def assemble(poses, cell, n_cells, method="median", spread_method="mean", max_cover=32):
    """poses (N, 2, Tx, 17) f32, cell (N, Tx) int -> (pose (n_cells, 34) f32, count (n_cells,) i32, spread (n_cells,) f32)."""
    assert method in METHODS and spread_method in SPREADS and 1 <= max_cover <= 32
    poses = np.asarray(poses, np.float32)
    cell = np.asarray(cell).astype(np.int64)
    N, _, Tx, _ = poses.shape
    assert cell.shape == (N, Tx)
    rows = poses.transpose(0, 2, 3, 1).reshape(N * Tx, 34)            # pair (window, frame) -> x1,y1,...,x17,y17
    lists = [[] for _ in range(n_cells)]
    for pair, c in enumerate(cell.reshape(-1)):                        # ascending window index, then forecast frame
        if 0 <= c < n_cells:
            lists[c].append(pair)
    pose = np.zeros((n_cells, 34), np.float32)
    count = np.array([len(l) for l in lists], np.int32).reshape(n_cells)
    spread = np.zeros(n_cells, np.float32)
    with np.errstate(all="ignore"):
        for c, pairs in enumerate(lists):
            k = len(pairs)
            if k == 0:
                continue
            if k > max_cover:
                pose[c], spread[c] = np.nan, np.nan
                continue
            x = rows[pairs].astype(np.float64)                         # (k, 34)
            sd = np.zeros(34)
            for f in range(34):
                s = np.float64(0.0)
                for j in range(k):
                    s = s + x[j, f]
                mean = s / np.float64(k)
                ss = np.float64(0.0)
                for j in range(k):
                    d = x[j, f] - mean
                    ss = ss + d * d
                sd[f] = np.sqrt(ss / np.float64(k))
                pose[c, f] = np.float32(x[0, f] if method == "unique" else mean if method == "mean" else _middle(x[:, f]))
            if spread_method == "mean":
                s = np.float64(0.0)
                for f in range(34):
                    s = s + sd[f]
                spread[c] = np.float32(s / np.float64(34.0))
            else:
                spread[c] = np.float32(_middle(sd))
    return pose, count, spread


def box_sides(raw, vid_res):
    """(n, 34) f32 rows -> (L, R, T, B) int64 arrays: the bounding box as mcd_normalize_poses computes it (fp32 margin, clip,
    round-half-even; (0, 0, 0, 0) for a row without a non-zero x or without a non-zero y) -- tests/dataset_spec.py:bbox_centre."""
    raw = np.asarray(raw, np.float32)
    f32 = np.float32
    x, y = raw[:, 0::2], raw[:, 1::2]
    ok = (x != 0).any(1) & (y != 0).any(1)
    sides = []
    for v, size in ((x, vid_res[0]), (y, vid_res[1])):
        nz = v != 0
        lo = np.where(ok, np.where(nz, v, f32(np.inf)).min(1), f32(0))
        hi = np.where(ok, np.where(nz, v, f32(-np.inf)).max(1), f32(0))
        extra = f32(0.1) * ((hi - lo) + f32(1))
        top = f32(f32(size) - f32(1))
        a = np.rint(np.minimum(np.maximum(lo - extra, f32(0)), top)).astype(np.int64)
        b = np.rint(np.minimum(np.maximum(hi + extra, f32(0)), top)).astype(np.int64)
        sides += [np.where(ok, a, 0), np.where(ok, b, 0)]
    return tuple(sides)


def denormalize(norm, raw, vid_res, center=None, scale=None, count=None):
    """norm (n, 34) f32 interleaved, raw (n, 34) f32 -> (n, 34) f32 pixels: ((p * scale_k + center_k) * s + c), every operation a
    float64 operation, rounded to fp32 once; a degenerate side gives c; rows with count 0 are all zero."""
    norm = np.asarray(norm, np.float32)
    L, R, T, B = box_sides(raw, vid_res)
    s = np.zeros(norm.shape, np.float64)
    c = np.zeros(norm.shape, np.float64)
    s[:, 0::2], s[:, 1::2] = (R - L).astype(np.float64)[:, None], (B - T).astype(np.float64)[:, None]
    c[:, 0::2], c[:, 1::2] = (0.5 * (L + R).astype(np.float64))[:, None], (0.5 * (T + B).astype(np.float64))[:, None]
    with np.errstate(all="ignore"):
        t = norm.astype(np.float64)
        if center is not None:
            t = t * np.asarray(scale, np.float64)
            t = t + np.asarray(center, np.float64)
        t = t * s
        out = np.where(s != 0, t + c, c).astype(np.float32)
    if count is not None:
        out[np.asarray(count) == 0] = 0
    return out


def bits(a):
    """The bit patterns of an fp32 array with every NaN mapped to one pattern ("NaN payloads aside")."""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def ulp_distance(a, b):
    """Element-wise distance in fp32 units in the last place between two finite fp32 arrays."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))

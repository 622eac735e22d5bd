"""NumPy float64 restatement of mcd_forecast_fan (include/mocodad_hip.h), with loops in exactly the orders the header states: what the
kernel is held to bit for bit (tests/test_forecast_fan_gpu.py), and what is itself held to np.quantile / np.mean / np.std and a
brute-force mid-rank (tests/test_forecast_fan_host.py).  The value list of a cell's feature: for each covering pair in ascending pair
index the samples 0 .. S-1 in order, each mapped back through forecast_tta_ref.map_back when transforms are given.  Loops, no
vectorised reductions: NumPy's own sums are pairwise along a contiguous axis."""
import numpy as np

import forecast_tta_ref as TR

MAX_VALUES = 1024
MAX_LEVELS = 8


def check_levels(levels):
    lv = [float(q) for q in levels]
    assert 1 <= len(lv) <= MAX_LEVELS and all(0.0 <= q <= 1.0 for q in lv) and all(b > a for a, b in zip(lv, lv[1:])), lv
    return lv


def feature_stats64(x32, levels, observed=None):
    """One value list (K,) f32 in list order -> (quant (n_levels,), mean, std, rank | None) as FLOAT64, before the fp32 store: every
    operation a float64 operation in the stated order.  A NaN in the list: all NaN; a NaN observed: its rank NaN."""
    x32 = np.asarray(x32, np.float32).reshape(-1)
    K = len(x32)
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.float64(0.0)
        for j in range(K):
            s = s + x[j]
        mean = s / np.float64(K)
        ss = np.float64(0.0)
        for j in range(K):
            d = x[j] - mean
            ss = ss + d * d
        std = np.sqrt(ss / np.float64(K))
        if np.isnan(x).any():
            nan = np.float64(np.nan)
            return np.full(len(levels), nan, np.float64), mean, std, (None if observed is None else nan)
        xs = np.sort(x, kind="stable")            # ties by list position; -0.0 and +0.0 compare equal and keep their places
        quant = np.zeros(len(levels), np.float64)
        for l, q in enumerate(levels):
            h = np.float64(q) * np.float64(K - 1)
            i = int(np.floor(h))
            g = h - np.float64(i)
            if g == 0:
                quant[l] = xs[i]
            else:
                a = (np.float64(1.0) - g) * xs[i]
                b = g * xs[i + 1]
                quant[l] = a + b
        rank = None
        if observed is not None:
            o = np.float32(observed)
            if np.isnan(o):
                rank = np.float64(np.nan)
            else:
                below = int((x32 < o).sum())
                equal = int((x32 == o).sum())
                rank = (np.float64(below) + np.float64(equal) / np.float64(2.0)) / np.float64(K)
    return quant, mean, std, rank


def feature_stats(x32, levels, observed=None):
    """feature_stats64 rounded to fp32 once, as the kernel stores it -> (quant (n_levels,) f32, mean f32, std f32, rank f32 | None)."""
    quant, mean, std, rank = feature_stats64(x32, levels, observed)
    return quant.astype(np.float32), np.float32(mean), np.float32(std), (None if rank is None else np.float32(rank))


def fan(poses_all, cell, n_cells, levels=(0.1, 0.5, 0.9), observed=None, max_cover=32, trans=None, inv_affine=None):
    """poses_all (N, S, 2, Tx, 17) f32, cell (N, Tx) int, observed (n_cells, 2, 17) f32 | None ->
    (quant (n_levels, n_cells, 34) f32, mean (n_cells, 34), std (n_cells, 34), rank (n_cells, 34) | None, count (n_cells,) i32)."""
    lv = check_levels(levels)
    poses_all = np.ascontiguousarray(poses_all, np.float32)
    cell = np.asarray(cell).astype(np.int64).copy()
    N, S, _, Tx, _ = poses_all.shape
    assert cell.shape == (N, Tx) and S >= 1 and 1 <= max_cover <= (32 if trans is None else 64)
    if trans is not None:
        trans = np.asarray(trans).astype(np.int64).reshape(-1)
        inv = np.asarray(inv_affine, np.float64).reshape(-1, 6)
        ok = (trans >= 0) & (trans < len(inv))
        cell[~ok] = -1                                                     # a window outside the table: its pairs are ignored
        flat = poses_all.reshape(N * S, 2, Tx, 17)
        poses_all = TR.map_back(flat, np.repeat(np.where(ok, trans, 0), S), inv).reshape(N, S, 2, Tx, 17)
    rows = poses_all.transpose(0, 3, 1, 4, 2).reshape(N * Tx, S, 34)       # pair (window, frame) -> sample -> x1,y1,...,x17,y17
    lists = [[] for _ in range(n_cells)]
    for pair, c in enumerate(cell.reshape(-1)):                            # ascending pair index
        if 0 <= c < n_cells:
            lists[c].append(pair)
    quant = np.zeros((len(lv), n_cells, 34), np.float32)
    mean = np.zeros((n_cells, 34), np.float32)
    std = np.zeros((n_cells, 34), np.float32)
    rank = None if observed is None else np.zeros((n_cells, 34), np.float32)
    count = np.array([len(l) for l in lists], np.int32).reshape(n_cells)
    if observed is not None:
        obs = np.asarray(observed, np.float32).reshape(n_cells, 2, 17).transpose(0, 2, 1).reshape(n_cells, 34)
    for c, pairs in enumerate(lists):
        k = len(pairs)
        if k == 0:
            continue
        if k > max_cover or k * S > MAX_VALUES:
            quant[:, c], mean[c], std[c] = np.nan, np.nan, np.nan
            if rank is not None:
                rank[c] = np.nan
            continue
        x = rows[pairs].reshape(k * S, 34)                                 # list order: pair ascending, then sample
        for f in range(34):
            qf, mf, sf, rf = feature_stats(x[:, f], lv, None if observed is None else obs[c, f])
            quant[:, c, f], mean[c, f], std[c, f] = qf, mf, sf
            if rank is not None:
                rank[c, f] = rf
    return quant, mean, std, rank, count

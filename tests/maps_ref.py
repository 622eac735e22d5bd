"""The error maps of include/mocodad_hip.h (mcd_error_maps) restated in NumPy, in float64 on fp32 inputs -- the reference of
tests/test_error_maps_gpu.py and tests/test_error_maps_module_gpu.py.  The sample SELECTION is made on the fp32 losses, as the
library makes it: strict comparisons from 1e10 / -1 with the first of equal samples kept (best / worst), ranks by (loss, sample
index) (median, quantile), torch.quantile's ranks from the fp32 position, its weight in float64; a NaN among the losses makes the median / quantile map
NaN, and best / worst skip it."""
import numpy as np


def _split(strategy):
    return ("quantile", float(strategy.split(":")[1])) if strategy.startswith("quantile") else (strategy, 0.0)


def loss64(a, b, fn):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    if fn == "smooth_l1":
        return np.where(d < 1.0, 0.5 * d * d, d - 0.5)
    return d if fn == "l1" else d * d


def per_sample_maps(pose, gt, fn):
    """E (B,S,Tx,V) in float64; gt (B,C,Tx,V) = the ground-truth corrupt frames."""
    return loss64(pose, gt[:, None], fn).mean(axis=2)


def select(loss_row, strategy):
    """Sample selection on the fp32 losses of one window -> (lo index, hi index, weight) | None (a NaN map)."""
    name, q = _split(strategy)
    S = len(loss_row)
    if name in ("best", "worst"):
        cur, sel = (np.float32(1e10), -1) if name == "best" else (np.float32(-1), -1)
        for k in range(S):
            y = loss_row[k]
            if (y < cur) if name == "best" else (y > cur):
                cur, sel = y, k
        return None if sel < 0 else (sel, sel, 0.0)
    if np.isnan(loss_row).any():
        return None
    order = np.argsort(loss_row, kind="stable")          # by loss, then by sample index
    if name == "median":
        r = (S - 1) // 2
        return int(order[r]), int(order[r]), 0.0
    # ranks from the fp32 position, as the library takes them; the WEIGHT pos - lo in float64 from the fp32 q, like everything else
    # here (the fp32 product q (S - 1) may be fused into the subtraction on the device, which then rounds this very value once;
    # rounding the product first, as torch's two tensor ops do, moves the weight by up to half an ulp of pos)
    lo = int(np.floor(np.float32(q) * np.float32(S - 1)))
    hi = min(lo + 1, S - 1)
    return int(order[lo]), int(order[hi]), float(np.float32(q)) * (S - 1) - lo


def reference_maps(loss, pose, gt, fn, strategy, pose_agg=None):
    name, _ = _split(strategy)
    E = per_sample_maps(pose, gt, fn)
    if name == "all":
        return E
    if name == "mean":
        return E.sum(axis=1) / E.shape[1]
    if name in ("mean_pose", "median_pose"):
        return loss64(pose_agg, gt, fn).mean(axis=1)
    M = np.full((E.shape[0],) + E.shape[2:], np.nan)
    for b in range(E.shape[0]):
        s = select(loss[b], strategy)
        if s is not None:
            M[b] = E[b, s[0]] + s[2] * (E[b, s[1]] - E[b, s[0]])
    return M



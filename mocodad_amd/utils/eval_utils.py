"""Window scores -> per-frame clip scores (the step right after the hot path).

Reference: models/mocodad.py:362-425 and utils/eval_utils.py (compute_var_matrix :27-34, score_process
:100-106, pad_scores :133-149, get_avenue_mask :152-166, get_hr_ubnormal_mask :169-185).  The reference walks
(transform, clip, person) with three nested Python loops and an O(N) boolean filter at each level; here all
windows are grouped once and scattered with a single scatter-max (on the GPU through the C ABI's
mcd_scatter_max when a scorer is available, np.maximum.at otherwise)."""
import os
from glob import glob
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
from scipy.ndimage import gaussian_filter1d

# HR-Avenue: frames kept (1) / dropped (0) per test clip, run-length encoded (value, count)
_AVENUE_RLE = {
    1: [(1, 75), (0, 46), (1, 269), (0, 47), (1, 427), (0, 47), (1, 20), (0, 70), (1, 438)],
    2: [(1, 272), (0, 48), (1, 403), (0, 41), (1, 447)],
    3: [(1, 293), (0, 48), (1, 582)],
    6: [(1, 561), (0, 64), (1, 189), (0, 193), (1, 276)],
    16: [(1, 728), (0, 12)],
}


def get_avenue_mask() -> Dict[int, List[int]]:
    return {k: [v for v, n in rle for _ in range(n)] for k, rle in _AVENUE_RLE.items()}


def get_hr_ubnormal_mask(split: str) -> Dict[Tuple[int, int], np.ndarray]:
    sub = "testing" if "test" in split else "validating"
    out = {}
    for path in glob(f"./data/UBnormal/hr_bool_masks/{sub}/test_frame_mask/*"):
        scene, clip = map(int, os.path.basename(path).split(".")[0].split("_"))
        out[(scene, clip)] = np.load(path)
    return out


def compute_var_matrix(pos: np.ndarray, frames_pos: np.ndarray, n_frames: int) -> np.ndarray:
    """(w,) window scores + (w, seg_len) 1-based frame ids -> (w, n_frames), zero where a window is absent."""
    mat = np.zeros((pos.shape[0], n_frames))
    if pos.shape[0]:
        rows = np.repeat(np.arange(pos.shape[0]), frames_pos.shape[1])
        mat[rows, frames_pos.reshape(-1) - 1] = np.repeat(pos, frames_pos.shape[1])
    return mat


def score_process(score: np.ndarray, shift: int, kernel_size: float) -> np.ndarray:
    shifted = np.zeros_like(score)
    shifted[shift:] = score[:-shift]
    return gaussian_filter1d(shifted, kernel_size)


def pad_scores(score: np.ndarray, gt: np.ndarray, pad_size: int) -> np.ndarray:
    """Zero `pad_size` frames around every interval (within the first len(gt)-1 frames) where the person is absent."""
    n = len(gt)
    absent = np.zeros(n + 1, dtype=bool)
    absent[1:n] = score[:n - 1] == 0          # 1-shifted so that diff() marks run starts/ends
    edges = np.flatnonzero(np.diff(absent.astype(np.int8)))
    zero_ranges = []
    for start, stop in zip(edges[0::2], edges[1::2]):   # run covers frames start .. stop-1
        end = stop - 1
        if start == 0 and end == n - 2:
            continue
        lo = start if start == 0 else max(start - pad_size, 0)
        hi = end if end == n - 2 else min(end + pad_size, n)
        zero_ranges.append((lo, hi))
    for lo, hi in zero_ranges:
        score[lo:hi] = 0
    return score


def frame_score_rows(out, trans, meta, frames, gts, num_transform, scatter_max: Optional[Callable] = None):
    """Scatter-max every window score onto its frames.  Returns (mat (n_rows, n_frames_max), row_keys (n_rows, 4))
    with one row per (transform, scene, clip, person) in lexicographic order."""
    clip_ok = np.zeros(len(out), dtype=bool)
    for (sc, cl) in gts:
        clip_ok |= (meta[:, 0] == sc) & (meta[:, 1] == cl)
    sel = clip_ok & (trans >= 0) & (trans < num_transform)
    keys = np.stack([trans[sel], meta[sel, 0], meta[sel, 1], meta[sel, 2]], axis=1).astype(np.int64)
    row_keys, row = np.unique(keys, axis=0, return_inverse=True)
    row = row.reshape(-1)
    n_frames = max(len(g) for g in gts.values())
    o, f = np.asarray(out)[sel], np.asarray(frames)[sel]
    if scatter_max is not None and len(o):
        import torch
        mat = scatter_max(torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(f)),
                          torch.from_numpy(row.astype(np.int32)), len(row_keys), n_frames).cpu().numpy().astype(np.float64)
    else:
        mat = np.zeros((len(row_keys), n_frames))
        rr = np.repeat(row, f.shape[1])
        ff = f.reshape(-1) - 1
        ok = (ff >= 0) & (ff < n_frames)
        np.maximum.at(mat, (rr[ok], ff[ok]), np.repeat(o, f.shape[1])[ok])
    return mat, row_keys


def joint_score_rows(maps, trans, meta, frames, gts, num_transform: int, joint_scatter_max: Callable):
    """Per-joint frame scores of a dataset (eval_MoCoDAD.py --joint-scores): the error maps of every window (N, Tx, V) (device
    tensor, MoCoDAD.forward(return_maps=True)) with frames (N, Tx) = the 1-based frame id of each map row are averaged over the
    transforms -- a transform only negates or rotates coordinates, so a joint keeps its index; a torch op on the device, not a hot
    path -- and scatter-maxed (mcd_joint_scatter_max) onto one row per (scene, clip, person) of the clips in `gts`, in
    lexicographic order: the rows of frame_score_rows without the transform.  Every window (scene, clip, person, first frame) must
    be there once under every transform 0 .. num_transform - 1, in any order.
    -> (scores (n_rows, n_frames_max, V) fp32 NumPy, row_keys (n_rows, 3)); a frame no window forecasts stays 0."""
    import torch
    trans, meta, frames = np.asarray(trans), np.asarray(meta), np.asarray(frames)
    nt = max(1, int(num_transform))
    N = len(trans)
    n = N // nt
    order = np.lexsort((trans, meta[:, 3], meta[:, 2], meta[:, 1], meta[:, 0])) if N else np.zeros(0, np.int64)      # by window, then transform
    grid = order[:n * nt].reshape(n, nt)
    if n * nt != N or maps.shape[0] != N or not np.array_equal(trans[grid], np.tile(np.arange(nt), (n, 1))) \
            or not (meta[grid] == meta[grid[:, :1]]).all() or not (frames[grid] == frames[grid[:, :1]]).all() \
            or (n > 1 and (meta[grid[1:, 0]] == meta[grid[:-1, 0]]).all(1).any()):
        raise ValueError("joint scores need every window once under every transform 0 .. num_transform - 1, with the same frames")
    mean = maps[torch.from_numpy(grid.reshape(-1)).to(maps.device)].reshape(n, nt, *maps.shape[1:]).mean(1)
    meta, frames = meta[grid[:, 0]], frames[grid[:, 0]]
    sel = np.zeros(n, dtype=bool)
    for (sc, cl) in gts:
        sel |= (meta[:, 0] == sc) & (meta[:, 1] == cl)
    row_keys, row = np.unique(meta[sel, :3].astype(np.int64), axis=0, return_inverse=True)
    n_frames = max(len(g) for g in gts.values())
    idx = torch.from_numpy(np.flatnonzero(sel)).to(mean.device)
    out = joint_scatter_max(mean[idx], torch.from_numpy(np.ascontiguousarray(frames[sel], dtype=np.int32)),
                            torch.from_numpy(row.reshape(-1).astype(np.int32)), len(row_keys), n_frames)
    return out.cpu().numpy(), row_keys


# ------------------------------------------------------------------ forecast tracks (mcd_forecast_assemble)
FORECAST_TRANSFORMS = ("identity", "all")


def _forecast_transforms(transforms: str) -> bool:
    """'identity' | 'all' -> whether the windows of every transform contribute."""
    if transforms not in FORECAST_TRANSFORMS:
        raise ValueError(f"transforms must be one of {FORECAST_TRANSFORMS}, got {transforms!r}")
    return transforms == "all"


def forecast_max_cover(num_transform: int, n_corrupt: int, transforms: str = "identity") -> int:
    """The pairs a trajectory row can collect with fixed conditioning indices: n_corrupt windows of transform 0, under 'all' of
    each of the num_transform transforms -- at most 64 (MCD_FORECAST_VIEW_COVER), more is refused by name."""
    if not _forecast_transforms(transforms):
        return int(n_corrupt)
    cover = max(1, int(num_transform)) * int(n_corrupt)
    if cover > 64:
        raise ValueError(f"transforms='all' puts num_transform * n_corrupt = {int(num_transform)} * {int(n_corrupt)} = {cover} forecasts "
                         "on a row; the reduction holds 64 (use fewer transforms, or transforms='identity')")
    return cover


def forecast_cells_dense(row, frame_ids, trans, n_frames: int, transforms: str = "identity") -> np.ndarray:
    """cell (N, Tx) int32 for a dense (row, frame) matrix in the reference's layout (compute_fig_matrix, eval_utils.py:13-24):
    row * n_frames + f - 1 for the 1-based frame id f of every forecast frame; -1 (ignored) for a window of another transform
    than 0, the identity -- their forecasts live in rotated or flipped coordinates --, a negative row, or a frame outside
    [1, n_frames].  transforms='all': the windows of every transform keep their cells (mcd_forecast_assemble_view maps their
    forecasts back)."""
    row, f, trans = np.asarray(row, np.int64).reshape(-1, 1), np.asarray(frame_ids, np.int64), np.asarray(trans).reshape(-1, 1)
    ok = ((trans == 0) | _forecast_transforms(transforms)) & (row >= 0) & (f >= 1) & (f <= n_frames)
    return np.where(ok, row * n_frames + f - 1, -1).astype(np.int32)


def forecast_cells_aligned(base, map_frames, trans, row_stride: int = 34, transforms: str = "identity") -> np.ndarray:
    """cell (N, Tx) int32 = the global trajectory row of every forecast frame: base // 34 + its 0-based window frame index
    (TrajectoryWindows.base: a window's element offset into the frame-major buffer); -1 for a window of another transform than 0,
    unless transforms='all'."""
    base, mf, trans = np.asarray(base, np.int64).reshape(-1, 1), np.asarray(map_frames, np.int64), np.asarray(trans).reshape(-1, 1)
    return np.where((trans == 0) | _forecast_transforms(transforms), base // row_stride + mf, -1).astype(np.int32)


def _forecast_rows_and_cells(forecast_shape, trans, map_frames, *, windows=None, meta=None, frames=None, transforms: str = "identity",
                             num_transform: Optional[int] = None, caller: str = "forecast_track_rows"):
    """The trajectory rows of a dataset's windows and the cell of every forecast frame, for forecast_track_rows and forecast_fan_rows;
    forecast_shape: (N, ..., Tx, 17), the shape of the forecasts.
    -> (cell (N,Tx) int32, table (R,4) int64 = (scene, clip, person, frame id), extra: the trans= / inv_affine= keywords of the device
    call under transforms='all' (else empty))."""
    every = _forecast_transforms(transforms)
    trans, mf = np.asarray(trans).reshape(-1), np.asarray(map_frames, np.int64)
    if windows is not None:
        meta, frames, base = np.asarray(windows.meta), np.asarray(windows.frames), np.asarray(windows.base)
    elif meta is None or frames is None:
        raise ValueError(f"{caller} needs a TrajectoryWindows or the windows' meta and frames")
    else:
        meta, frames, base = np.asarray(meta), np.asarray(frames), None
    N, seg_len = frames.shape
    if len(trans) != N or len(meta) != N or mf.shape[0] != N or forecast_shape[0] != N or mf.shape[1] != forecast_shape[-2]:
        raise ValueError(f"need one forecast, transform, meta row, frame row and map_frames row per window, got {tuple(forecast_shape)}, "
                         f"{trans.shape}, {meta.shape}, {frames.shape}, {mf.shape}")
    ident = np.flatnonzero(trans == 0)
    keys = np.concatenate([np.repeat(meta[ident, :3].astype(np.int64), seg_len, axis=0), frames[ident].reshape(-1, 1).astype(np.int64)], axis=1)
    if base is not None:
        n_rows = int(windows.buffer.numel()) // 34
        cell = forecast_cells_aligned(base, mf, trans, transforms=transforms)
        row_of = (base[ident, None] // 34 + np.arange(seg_len)).reshape(-1)         # trajectory row of every covered window frame
        table = np.zeros((n_rows, 4), np.int64)
        table[row_of] = keys
    else:
        table, inv = np.unique(keys, axis=0, return_inverse=True)
        n_rows = len(table)
        if not every:
            dense = np.full((N, seg_len), -1, np.int64)
            dense[ident] = inv.reshape(len(ident), seg_len)
            cell = np.where(trans[:, None] == 0, np.take_along_axis(dense, mf, axis=1), -1).astype(np.int32)
        else:       # the row of every window's forecast frames, looked up in the table of the transform-0 rows (absent: ignored)
            fkeys = np.concatenate([np.repeat(meta[:, :3].astype(np.int64), mf.shape[1], axis=0),
                                    np.take_along_axis(frames.astype(np.int64), mf, axis=1).reshape(-1, 1)], axis=1)
            both, back = np.unique(np.concatenate([table, fkeys]), axis=0, return_inverse=True)
            row_of_key = np.full(len(both), -1, np.int64)
            back = back.reshape(-1)
            row_of_key[back[:n_rows]] = np.arange(n_rows)
            cell = row_of_key[back[n_rows:]].reshape(N, mf.shape[1]).astype(np.int32)
    import torch
    extra = {}
    if every:
        from .transforms import inverse_affine_table
        nt = int(num_transform) if num_transform is not None else (int(trans.max()) + 1 if N else 1)
        extra = {"trans": torch.from_numpy(np.ascontiguousarray(trans, dtype=np.int32)), "inv_affine": inverse_affine_table(nt)}
    return torch.from_numpy(np.ascontiguousarray(cell)), table, extra


def forecast_track_rows(poses, trans, map_frames, assemble: Callable, *, windows=None, meta=None, frames=None, method: str = "median",
                        spread_method: str = "mean", max_cover: int = 32, transforms: str = "identity", num_transform: Optional[int] = None):
    """Forecast tracks of a dataset (eval_MoCoDAD.py --forecast-tracks): the selected forecast of every window, poses (N,2,Tx,17)
    (forward(return_='all')), collapsed into one expected pose per trajectory row -- per tracked person and video frame.
    trans (N,): only windows of transform 0, the identity, contribute.  map_frames (N,Tx): the 0-based window frame index of each
    pose row (MoCoDAD.map_frames; per window under 'random_imp').  The trajectory rows come from `windows` (a TrajectoryWindows: a
    row is a row of its buffer, cell = base // 34 + frame index) or from meta (N,4) / frames (N,seg_len) (a row is a distinct
    (scene, clip, person, frame id) of the transform-0 windows, in lexicographic order).  assemble: engine.forecast_assemble (or a
    restatement of it).
    transforms='all' (eval_MoCoDAD.py --forecast-transforms all): the windows of EVERY transform contribute -- their cells are the
    trajectory row of their forecast frame like transform 0's, and `assemble` is also given trans= and inv_affine= (the inverse
    table of the transforms 0 .. num_transform - 1, default max(trans) + 1, utils.transforms.inverse_affine_table), with which it
    maps each forecast back before combining; a row's forecasts are combined transform-major in the order of the windows.  The
    rows themselves are still those the transform-0 windows cover.  max_cover may be up to 64 then.
    -> (pose (R,34), count (R,), spread (R,) as `assemble` returns them, rows (R,3) int64 = (scene, clip, person), frame_ids (R,)
    int64); a row no window forecasts -- the first n_cond rows of a track under a tail forecast -- has count 0 and a zero pose."""
    cell, table, extra = _forecast_rows_and_cells(tuple(poses.shape), trans, map_frames, windows=windows, meta=meta, frames=frames,
                                                  transforms=transforms, num_transform=num_transform)
    pose, count, spread = assemble(poses, cell, len(table), method=method, spread_method=spread_method, max_cover=max_cover, **extra)
    return pose, count, spread, table[:, :3], table[:, 3]


def forecast_fan_cover(n_samples: int, cover: int) -> int:
    """The values one row's list collects for a forecast fan: n_samples per covering pair -- at most MCD_FORECAST_FAN_VALUES (1024),
    more is refused by name.  -> cover."""
    from .._lib import MCD_FORECAST_FAN_VALUES as most
    if int(n_samples) * int(cover) > most:
        raise ValueError(f"a forecast fan puts n_samples * cover = {int(n_samples)} * {int(cover)} = {int(n_samples) * int(cover)} values on a "
                         f"row; the reduction holds {most} (use fewer samples, fewer transforms, or transforms='identity')")
    return int(cover)


def forecast_observed_rows(trans, *, windows=None, meta=None, frames=None, data=None):
    """The observed pose of every trajectory row, (R,2,17) fp32 in the frame-major layout, row for row with the tables of
    forecast_track_rows / forecast_fan_rows: a view of windows.buffer as it lies, or, without a TrajectoryWindows, scattered on the
    host from the transform-0 windows' own frames in data (N,2,seg_len,17) (overlapping windows hold the same row)."""
    import torch
    if windows is not None:
        return windows.buffer.view(-1, 2, 17)
    if meta is None or frames is None or data is None:
        raise ValueError("forecast_observed_rows needs a TrajectoryWindows, or the windows' meta and frames and the windows themselves (data)")
    trans, meta, frames = np.asarray(trans).reshape(-1), np.asarray(meta), np.asarray(frames)
    N, seg_len = frames.shape
    d = data.detach().cpu().numpy() if torch.is_tensor(data) else np.asarray(data)
    if d.shape != (N, 2, seg_len, 17) or len(trans) != N or len(meta) != N:
        raise ValueError(f"data must be the windows ({N}, 2, {seg_len}, 17) with one transform and meta row each, got {d.shape}, "
                         f"{trans.shape}, {meta.shape}")
    ident = np.flatnonzero(trans == 0)
    keys = np.concatenate([np.repeat(meta[ident, :3].astype(np.int64), seg_len, axis=0), frames[ident].reshape(-1, 1).astype(np.int64)], axis=1)
    table, inv = np.unique(keys, axis=0, return_inverse=True)      # (the row numbering of _forecast_rows_and_cells)
    obs = np.zeros((len(table), 2, 17), np.float32)
    obs[inv.reshape(-1)] = d[ident].astype(np.float32).transpose(0, 2, 1, 3).reshape(-1, 2, 17)
    return torch.from_numpy(obs)


def forecast_fan_rows(poses_all, trans, map_frames, fan: Callable, *, windows=None, meta=None, frames=None, data=None,
                      levels=(0.1, 0.5, 0.9), transforms: str = "identity", num_transform: Optional[int] = None, max_cover: int = 32):
    """The forecast fan of a dataset (eval_MoCoDAD.py --forecast-fan): ALL S samples of every window, poses_all (N,S,2,Tx,17)
    (forward(return_samples=True)), as per-row quantile bands, mean, standard deviation and the mid-rank of the observed row among
    them.  Rows, cells, transforms, num_transform and max_cover: as forecast_track_rows.  The observed rows are those of
    forecast_observed_rows: windows.buffer, or without a TrajectoryWindows the transform-0 windows' own frames in `data`.
    fan: engine.forecast_fan (or a restatement of it).  S * max_cover may not exceed 1024.
    -> (quant (n_levels,R,34), mean (R,34), std (R,34), rank (R,34), count (R,) as `fan` returns them, rows (R,3) int64 = (scene,
    clip, person), frame_ids (R,) int64)."""
    if poses_all.ndim != 5:
        raise ValueError(f"poses_all must be (N, S, 2, Tx, 17), got {tuple(poses_all.shape)}")
    forecast_fan_cover(poses_all.shape[1], max_cover)
    cell, table, extra = _forecast_rows_and_cells(tuple(poses_all.shape), trans, map_frames, windows=windows, meta=meta, frames=frames,
                                                  transforms=transforms, num_transform=num_transform, caller="forecast_fan_rows")
    if windows is None and data is None:
        raise ValueError("forecast_fan_rows needs the windows themselves (data) for the observed rows when there is no TrajectoryWindows")
    observed = forecast_observed_rows(trans, windows=windows, meta=meta, frames=frames, data=data)
    quant, mean, std, rank, count = fan(poses_all, cell, len(table), levels=levels, observed=observed, max_cover=max_cover, **extra)
    return quant, mean, std, rank, count, table[:, :3], table[:, 3]


def reference_std_score(spread, lift: float = 1e-7) -> np.ndarray:
    """The reference's MinMax step on the dense per-person spread vector (extract_single_pose, eval_utils.py:66-69:
    MinMaxScaler().fit_transform(std_vec + std_lift)), restated in float64 with sklearn's operations: scale = 1 / (max - min)
    (1 for a constant vector), x * scale + (0 - min * scale).  Host code: not a hot path."""
    x = np.asarray(spread, np.float64).reshape(-1) + lift
    if not len(x):
        return x
    lo, hi = np.nanmin(x), np.nanmax(x)
    rng = hi - lo
    scale = 1.0 / (rng if rng >= 10 * np.finfo(np.float64).eps else 1.0)
    return x * scale + (0.0 - lo * scale)


def post_process_scores(out, trans, meta, frames, gts: Dict[Tuple[int, int], np.ndarray], *, num_transform: int,
                        pad_size: int, filter_kernel_size: float, frames_shift: int, masks: Optional[Dict] = None,
                        scatter_max: Optional[Callable] = None) -> Tuple[np.ndarray, np.ndarray]:
    """-> (per-frame anomaly scores averaged over transforms, ground truth), both concatenated over clips in
    sorted file-name order, as fed to roc_auc_score at mocodad.py:424-428."""
    masks = masks or {}
    clip_keys = sorted(gts.keys(), key=lambda k: f"{k[0]:02d}_{k[1]:04d}")
    mat, row_keys = frame_score_rows(np.asarray(out), np.asarray(trans), np.asarray(meta), np.asarray(frames), gts,
                                     num_transform, scatter_max)
    per_transform, gt_cat = [], None
    for tr in range(num_transform):
        scores, gcat = [], []
        for (sc, cl) in clip_keys:
            gt = gts[(sc, cl)]
            n = gt.shape[0]
            rsel = np.flatnonzero((row_keys[:, 0] == tr) & (row_keys[:, 1] == sc) & (row_keys[:, 2] == cl))
            if len(rsel) == 0:
                raise ValueError(f"no pose windows for transform {tr}, clip {sc:02d}_{cl:04d} (need at least one array to stack)")
            persons = mat[rsel, :n].copy()
            if pad_size != -1:
                for p in range(persons.shape[0]):
                    pad_scores(persons[p], gt, pad_size)
            lg = np.log1p(persons)
            cs = persons.mean(0) + (lg.max(0) - lg.min(0))
            g = gt
            if (sc, cl) in masks:
                keep = np.asarray(masks[(sc, cl)]).astype(bool)
                cs, g = cs[keep], g[keep]
            if ("clip", cl) in masks:
                keep = np.asarray(masks[("clip", cl)]) == 1
                cs, g = cs[keep], g[keep]
            scores.append(score_process(cs, frames_shift, filter_kernel_size))
            gcat.append(g)
        per_transform.append(np.concatenate(scores))
        if gt_cat is None:
            gt_cat = np.concatenate(gcat)
    return np.mean(np.stack(per_transform, 0), 0), gt_cat


# ------------------------------------------------------------------ device path (mcd_frame_scores)
def gaussian_kernel1d(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """The weights scipy.ndimage.gaussian_filter1d(x, sigma) correlates with (order 0): radius int(truncate*sigma + 0.5)."""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum()


def frame_tables(gts: Dict[Tuple[int, int], np.ndarray], masks: Optional[Dict] = None):
    """Per-dataset tables of the device frame-score assembly: clips in ascending (scene, clip) key order (what the kernel
    binary-searches), their output offsets in sorted file-name order (the order the reference concatenates in), the
    position of every frame after the HR masks, and the concatenated ground truth."""
    masks = masks or {}
    by_name = sorted(gts.keys(), key=lambda k: f"{k[0]:02d}_{k[1]:04d}")
    slots = sorted(gts.keys(), key=lambda k: (int(k[0]) << 32) | (int(k[1]) & 0xffffffff))
    F = max(len(g) for g in gts.values())
    kept, gt_kept = {}, {}
    for (sc, cl) in by_name:
        g = np.asarray(gts[(sc, cl)])
        idx = np.arange(len(g))
        if (sc, cl) in masks:
            keep = np.asarray(masks[(sc, cl)]).astype(bool)
            idx, g = idx[keep], g[keep]
        if ("clip", cl) in masks:
            keep = np.asarray(masks[("clip", cl)]) == 1
            idx, g = idx[keep], g[keep]
        kept[(sc, cl)], gt_kept[(sc, cl)] = idx, g
    off, o = {}, 0
    for k in by_name:
        off[k] = o
        o += len(kept[k])
    dst = np.full((len(slots), F), -1, dtype=np.int32)
    for i, k in enumerate(slots):
        dst[i, kept[k]] = np.arange(len(kept[k]), dtype=np.int32)
    return {
        "clip_keys": np.array([(int(k[0]) << 32) | (int(k[1]) & 0xffffffff) for k in slots], dtype=np.int64),
        "clip_n_frames": np.array([len(gts[k]) for k in slots], dtype=np.int32),
        "frame_dst": dst,
        "clip_out_len": np.array([len(kept[k]) for k in slots], dtype=np.int32),
        "clip_out_off": np.array([off[k] for k in slots], dtype=np.int64),
        "total": o, "max_frames": F,
        "gt": np.concatenate([gt_kept[k] for k in by_name]) if by_name else np.zeros(0),
    }

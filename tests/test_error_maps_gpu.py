"""GPU: mcd_error_maps and mcd_joint_scatter_max driven alone, on synthetic loss_all / pose_all / data made with NumPy.

Reference: the definitions of include/mocodad_hip.h evaluated in float64 on the same fp32 inputs; the sample SELECTION is done on
the fp32 loss_all (strict comparisons from 1e10 / -1 with the first of equal samples kept; ranks by (loss, sample index); the
quantile's ranks from the fp32 position q (S - 1), its weight in float64: tests/maps_ref.py).  For the *_pose strategies the
reference starts from the pose_agg mcd_aggregate returns.

Tolerance (derived, not measured): every cell is a sum of non-negative terms with at most C + S + 8 roundings -- per coordinate the
difference, the square (x 0.5 is exact) or the -0.5, the sum over C, the division by C; then S - 1 additions and one division for
the mean, or one difference, one product and one sum for the interpolation -- so |err| <= (C + S + 8) 2^-24 |ref| + 1e-37 (the
smallest normal number's neighbourhood); for the *_pose strategies the same with S = 0.

Shapes: B in {1, 3, 257} (one window, a few, more than one round of a 65536-block grid is not needed: 257 = past a multiple of
the 256-thread blocks of the scatter), Tx in {1, 3, 12, 32} (17 cells < one wave ... 544 cells = several rounds of the 64 lanes),
S in {1, 2, 5, 64, 65} (one sample, both sides of the wave width), the three loss functions, the seven aggregations and ALL,
quantile at 0, 0.3 and 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from maps_ref import _split, loss64, per_sample_maps, reference_maps, select      # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ("smooth_l1", "l1", "mse")
STRATEGIES = ("all", "best", "worst", "mean", "median", "mean_pose", "median_pose", "quantile:0", "quantile:0.3", "quantile:1")
# every Tx x S at B = 3, then the other window counts on shapes that differ in both
SHAPES = [(3, Tx, S) for Tx in (1, 3, 12, 32) for S in (1, 2, 5, 64, 65)] + [(1, 3, 5), (1, 32, 64), (257, 3, 5), (257, 12, 2), (257, 1, 65)]


def _lib():
    from mocodad_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cfg(B, S, T, corrupt, loss_fn):
    L = _lib()
    c = L.ScoreCfg(n_windows=B, n_samples=S, noise_steps=2, seg_len=T, n_cond=T - len(corrupt), n_corrupt=len(corrupt), loss_fn=L.LOSS[loss_fn])
    for i, v in enumerate(corrupt):
        c.corrupt_idx[i] = v
    for i, v in enumerate(k for k in range(T) if k not in corrupt):
        c.cond_idx[i] = v
    return c


def device_maps(loss, pose, data, T, corrupt, loss_fn, strategy, view=None):
    """mcd_error_maps on device copies of the NumPy inputs -> NumPy (B,Tx,17) / (B,S,Tx,17)."""
    L = _lib()
    lib = L.lib()
    B, S, _, Tx, V = pose.shape
    name, q = _split(strategy)
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lo, po, da = d(loss), d(pose), d(data)
    out = torch.full((B, S, Tx, V) if name == "all" else (B, Tx, V), -7.0, device=DEV)
    cfg = _cfg(B, S, T, corrupt, loss_fn)
    keep = []
    v = None
    if view is not None:
        t = {k: d(a) for k, a in view.items() if k in ("base", "trans", "affine", "cond_mask")}
        keep.append(t)
        v = L.WindowView(base=_ptr(t.get("base")).value if "base" in t else None, stride_c=17, stride_t=34,
                         trans=_ptr(t.get("trans")).value if "trans" in t else None,
                         affine=_ptr(t.get("affine")).value if "affine" in t else None,
                         cond_mask=_ptr(t.get("cond_mask")).value if "cond_mask" in t else None)
    L.check(lib.mcd_error_maps(C.byref(cfg), 2, V, L.AGGR[name], C.c_float(q), _ptr(lo), _ptr(po), _ptr(da),
                               C.byref(v) if v is not None else None, _ptr(out), _stream()))
    return out.cpu().numpy()


def device_pose_agg(loss, pose, dense, T, corrupt, loss_fn, strategy, cond_mask=None):
    """pose_agg (B,C,Tx,V) of mcd_aggregate / mcd_aggregate_view on the DENSE windows."""
    L = _lib()
    lib = L.lib()
    B, S, _, Tx, V = pose.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lo, po, da = d(loss), d(pose), d(dense)
    agg, pagg = torch.empty(B, device=DEV), torch.empty(B, 2, Tx, V, device=DEV)
    cfg = _cfg(B, S, T, corrupt, loss_fn)
    if cond_mask is None:
        L.check(lib.mcd_aggregate(C.byref(cfg), 2, V, L.AGGR[strategy], C.c_float(0), _ptr(lo), _ptr(po), _ptr(da), _ptr(agg), _ptr(pagg), _stream()))
    else:
        m = d(cond_mask)
        v = L.WindowView(base=None, stride_c=0, stride_t=0, trans=None, affine=None, cond_mask=m.data_ptr())
        L.check(lib.mcd_aggregate_view(C.byref(cfg), 2, V, L.AGGR[strategy], C.c_float(0), _ptr(lo), _ptr(po), _ptr(da), C.byref(v), _ptr(agg),
                                       _ptr(pagg), _stream()))
    return pagg.cpu().numpy()


def bound(ref, S):
    return (2 + S + 8) * 2.0 ** -24 * np.abs(ref) + 1e-37


def assert_within(got, ref, S, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN cells differ"
    err = np.abs(got.astype(np.float64) - ref)[~nan]
    lim = bound(ref, S)[~nan]
    worst = float((err / lim).max()) if err.size else 0.0
    assert worst <= 1.0, f"{what}: |err| is {worst:.3f} x the bound"
    return worst


def inputs(B, Tx, S, seed, quantised=False):
    """data (B,2,T,17), pose (B,S,2,Tx,17), corrupt frames (the last Tx of T = Tx + min(3, 32 - Tx)), loss_all (B,S) fp32 = the
    window means of E (so the selection is the one a scoring call would make)."""
    rng = np.random.default_rng(seed)
    T = Tx + min(3, 32 - Tx)
    corrupt = list(range(T - Tx, T))
    data = rng.standard_normal((B, 2, T, 17)).astype(np.float32)
    pose = (data[:, None, :, T - Tx:] + rng.standard_normal((B, S, 2, Tx, 17)) * rng.choice([0.05, 0.7, 2.5], (B, S, 1, 1, 1))).astype(np.float32)
    if quantised:
        data, pose = np.round(data * 64) / 64, np.round(pose * 64) / 64
    return data.astype(np.float32), pose.astype(np.float32), T, corrupt


def window_losses(pose, gt, fn):
    return per_sample_maps(pose, gt, fn).mean(axis=(2, 3)).astype(np.float32)


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("B,Tx,S", SHAPES)
def test_maps_against_float64(B, Tx, S):
    data, pose, T, corrupt = inputs(B, Tx, S, seed=1000 * B + 10 * Tx + S)
    gt = data[:, :, corrupt]
    worst = {}
    for fn in LOSSES:
        loss = window_losses(pose, gt, fn)
        for strategy in STRATEGIES:
            name, _ = _split(strategy)
            got = device_maps(loss, pose, data, T, corrupt, fn, strategy)
            pagg = device_pose_agg(loss, pose, data, T, corrupt, fn, name) if name.endswith("_pose") else None
            ref = reference_maps(loss, pose, gt, fn, strategy, pagg)
            w = assert_within(got, ref, 0 if pagg is not None else S, f"{fn} {strategy}")
            worst[strategy] = max(worst.get(strategy, 0.0), w)
            if name not in ("all", "mean_pose", "median_pose"):
                # the map's mean is the aggregated loss up to rounding: against the float64 aggregate of the same selection
                agg = ref.mean(axis=(1, 2))
                np.testing.assert_allclose(got.astype(np.float64).mean(axis=(1, 2)), agg, rtol=(2 + S + 8) * 2.0 ** -24, atol=1e-37)
    print(f"B {B} Tx {Tx} S {S}: largest |err| / bound per strategy: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_ties_keep_the_first_sample_and_a_stable_order():
    """Duplicate losses with different poses: losses [2, 1, 3, 1, 2] -> best = sample 1 (not 3), worst = 2, median (rank 2 of the
    stable order 1, 3, 0, 4, 2) = sample 0 (not 4), quantile 0.3 (position 1.2) = samples 3 and 0."""
    B, Tx, S = 3, 3, 5
    data, pose, T, corrupt = inputs(B, Tx, S, seed=7)
    gt = data[:, :, corrupt]
    loss = np.tile(np.asarray([2, 1, 3, 1, 2], np.float32), (B, 1))
    assert select(loss[0], "best")[0] == 1 and select(loss[0], "worst")[0] == 2 and select(loss[0], "median")[0] == 0
    assert select(loss[0], "quantile:0.3")[:2] == (3, 0)
    E = per_sample_maps(pose, gt, "smooth_l1")
    for strategy, pick, other in (("best", 1, 3), ("median", 0, 4), ("worst", 2, 0)):
        got = device_maps(loss, pose, data, T, corrupt, "smooth_l1", strategy)
        assert_within(got, E[:, pick], S, strategy)
        assert np.abs(got - E[:, other]).max() > 1e-3, "the tied sample's map is a different one"
    got = device_maps(loss, pose, data, T, corrupt, "smooth_l1", "quantile:0.3")
    assert_within(got, reference_maps(loss, pose, gt, "smooth_l1", "quantile:0.3"), S, "quantile:0.3")
    # S = 65, ties across the wave's second round: samples 0 and 64 (lane 0 of both rounds) share the smallest loss
    data, pose, T, corrupt = inputs(2, 3, 65, seed=8)
    gt = data[:, :, corrupt]
    loss = np.tile(np.arange(65, 0, -1, dtype=np.float32), (2, 1))
    loss[:, 64] = loss[:, 0] = 0.5                                  # two smallest, lanes 0 of both rounds
    loss[:, 33] = loss[:, 32]                                       # a tie at the median rank
    for strategy in ("best", "worst", "median", "quantile:0.3", "quantile:0", "quantile:1"):
        got = device_maps(loss, pose, data, T, corrupt, "l1", strategy)
        assert_within(got, reference_maps(loss, pose, gt, "l1", strategy), 65, "S 65 " + strategy)
    assert select(loss[0], "best")[0] == 0 and select(loss[0], "quantile:0")[0] == 0 and select(loss[0], "quantile:0")[1] == 64


@pytest.mark.parametrize("S", [5, 65])
def test_nan_loss_stays_with_its_window(S):
    B, Tx = 4, 3
    data, pose, T, corrupt = inputs(B, Tx, S, seed=11 + S)
    gt = data[:, :, corrupt]
    loss = window_losses(pose, gt, "smooth_l1")
    bad = loss.copy()
    bad[1, S // 2] = np.nan                 # one diverged chain in window 1
    bad[2, :] = np.nan                      # every chain of window 2
    for strategy in STRATEGIES:
        name, _ = _split(strategy)
        clean = device_maps(loss, pose, data, T, corrupt, "smooth_l1", strategy)
        got = device_maps(bad, pose, data, T, corrupt, "smooth_l1", strategy)
        for b in (0, 3):
            assert np.array_equal(got[b].view(np.int32), clean[b].view(np.int32)), f"{strategy}: window {b} changed"
        if name in ("all", "mean", "mean_pose", "median_pose"):          # loss_all is not read
            assert np.array_equal(got.view(np.int32), clean.view(np.int32)), strategy
            continue
        ref = reference_maps(bad, pose, gt, "smooth_l1", strategy)
        assert_within(got, ref, S, "NaN " + strategy)
        if name in ("best", "worst"):       # strict comparisons skip the NaN: another sample, a finite map; all NaN: no sample
            assert np.isfinite(got[1]).all() and np.isnan(got[2]).all(), strategy
        else:
            assert np.isnan(got[1]).all() and np.isnan(got[2]).all(), strategy


def test_view_with_base_trans_affine():
    """Windows read through a view over a frame-major trajectory buffer, with a test-time transform: the ground truth is the
    TRANSFORMED frame.  The values are multiples of 1/64 and the affine entries of 1/4, so the transform is exact in fp32 and in
    float64 alike (whether or not the compiler contracts it) and the reference needs no model of its rounding."""
    B, Tx, S, T = 5, 3, 5, 6
    rng = np.random.default_rng(3)
    corrupt = [3, 4, 5]
    F = 40
    buf = (np.round(rng.standard_normal((F, 2, 17)) * 64) / 64).astype(np.float32)
    first = np.asarray([0, 7, 7, 20, 34], np.int64)                      # overlapping and distinct windows, the last one at the end
    trans = np.asarray([1, 0, 2, 3, 2], np.int32)
    affine = np.asarray([[1, 0, 0, 0, 1, 0], [-1, 0, 0, 0, 1, 0], [0, -1, 0.25, 1, 0, -0.5], [0.5, 0.25, 1, -0.25, 0.5, 2]], np.float32)
    win = np.stack([buf[f:f + T] for f in first]).transpose(0, 2, 1, 3)  # (B,C,T,V), untransformed
    A = affine[trans].reshape(B, 2, 3).astype(np.float64)
    x, y = win[:, 0].astype(np.float64), win[:, 1].astype(np.float64)
    dense = np.stack([A[:, 0, 0, None, None] * x + A[:, 0, 1, None, None] * y + A[:, 0, 2, None, None],
                      A[:, 1, 0, None, None] * x + A[:, 1, 1, None, None] * y + A[:, 1, 2, None, None]], axis=1)
    assert np.array_equal(dense, dense.astype(np.float32).astype(np.float64)), "the transform must be exact in fp32"
    dense = dense.astype(np.float32)
    gt = dense[:, :, corrupt]
    pose = (gt[:, None] + np.round(rng.standard_normal((B, S, 2, Tx, 17)) * 64) / 64).astype(np.float32)
    view = dict(base=first * 34, trans=trans, affine=affine)
    for fn in LOSSES:
        loss = window_losses(pose, gt, fn)
        for strategy in ("all", "best", "mean", "median", "quantile:0.3"):
            got = device_maps(loss, pose, buf.reshape(-1), T, corrupt, fn, strategy, view=view)
            assert_within(got, reference_maps(loss, pose, gt, fn, strategy), S, f"view {fn} {strategy}")
            # the dense, already transformed windows give the same bits
            assert np.array_equal(got.view(np.int32), device_maps(loss, pose, dense, T, corrupt, fn, strategy).view(np.int32))
        for name in ("mean_pose", "median_pose"):
            pagg = device_pose_agg(loss, pose, dense, T, corrupt, fn, name)
            got = device_maps(None, pose, buf.reshape(-1), T, corrupt, fn, name, view=view)
            assert_within(got, reference_maps(loss, pose, gt, fn, name, pagg), 0, f"view {fn} {name}")
    # a map taken against the UNtransformed frames is another map wherever the transform is not the identity
    loss = window_losses(pose, gt, "smooth_l1")
    got = device_maps(loss, pose, buf.reshape(-1), T, corrupt, "smooth_l1", "best", view=view)
    plain = device_maps(loss, pose, buf.reshape(-1), T, corrupt, "smooth_l1", "best", view=dict(base=first * 34))
    for b in range(B):
        same = np.array_equal(got[b], plain[b])
        assert same == (trans[b] == 0), f"window {b} (transform {trans[b]})"


def test_cond_mask_with_non_tail_corrupt_frames():
    """random_imp: the corrupt frames of a window are the CLEAR bits of its mask, ascending; cfg->corrupt_idx is ignored."""
    B, Tx, S, T = 6, 3, 5, 6
    rng = np.random.default_rng(5)
    data, pose, _, _ = inputs(B, Tx, S, seed=5)
    sets = [[0, 1, 2], [0, 2, 4], [1, 3, 5], [0, 4, 5], [3, 4, 5], [1, 2, 3]]           # the corrupt frames, window by window
    mask = np.asarray([sum(1 << t for t in range(T) if t not in s) for s in sets], np.int32)
    gt = np.stack([data[b][:, sets[b]] for b in range(B)])
    pose = (gt[:, None] + rng.standard_normal(pose.shape) * 0.5).astype(np.float32)
    wrong = list(range(T - Tx, T))                                                      # what corrupt_idx would say
    for fn in LOSSES:
        loss = window_losses(pose, gt, fn)
        for strategy in STRATEGIES:
            name, _ = _split(strategy)
            pagg = device_pose_agg(loss, pose, data, T, wrong, fn, name, cond_mask=mask) if name.endswith("_pose") else None
            got = device_maps(loss, pose, data, T, wrong, fn, strategy, view=dict(cond_mask=mask))
            assert_within(got, reference_maps(loss, pose, gt, fn, strategy, pagg), 0 if pagg is not None else S, f"mask {fn} {strategy}")
    # without the mask the tail frames are compared: equal only for the window whose set IS the tail
    got = device_maps(loss, pose, data, T, wrong, "mse", "best", view=dict(cond_mask=mask))
    tail = device_maps(loss, pose, data, T, wrong, "mse", "best")
    assert [bool(np.array_equal(got[b], tail[b])) for b in range(B)] == [s == wrong for s in sets]


# ---------------------------------------------------------------- mcd_joint_scatter_max
def device_scatter(maps, frames, row, n_rows, n_frames):
    L = _lib()
    lib = L.lib()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    m, f, r = d(maps), d(frames), d(row)
    out = torch.full((n_rows, n_frames, 17), 3.0, device=DEV)          # (the callee zeroes it)
    L.check(lib.mcd_joint_scatter_max(_ptr(m), _ptr(f), _ptr(r), int(len(row)), int(maps.shape[1]), n_rows, n_frames, _ptr(out), _stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("n,Tx,n_rows,n_frames", [(0, 3, 2, 5), (1, 1, 1, 1), (40, 3, 3, 20), (257, 12, 7, 64), (300, 32, 2, 50)])
def test_joint_scatter_max_is_np_maximum_at(n, Tx, n_rows, n_frames):
    rng = np.random.default_rng(n + Tx)
    maps = rng.standard_normal((n, Tx, 17)).astype(np.float32)          # negative values: clamped to 0
    maps[rng.random(maps.shape) < 0.01] = np.nan                        # a NaN adds 0
    first = rng.integers(-3, n_frames + 2, n)                           # 1-based frame ids, some outside [1, n_frames]
    frames = (first[:, None] + np.arange(Tx)[None]).astype(np.int32)
    row = rng.integers(0, n_rows, n).astype(np.int32)
    ref = np.zeros((n_rows, n_frames, 17), np.float32)
    clamped = np.fmax(maps, np.float32(0))
    ok = (frames >= 1) & (frames <= n_frames)
    ii, tt = np.nonzero(ok)
    np.maximum.at(ref, (row[ii], frames[ii, tt] - 1), clamped[ii, tt])
    got = device_scatter(maps, frames, row, n_rows, n_frames)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    if n >= 40:
        assert (~ok).any() and ok.any() and (ref > 0).any()
    if n == 40:
        assert (ref == 0).any()              # cells that no window reaches stay 0


def test_scatter_max_is_np_maximum_at():
    """The scalar mcd_scatter_max (the same kernel at row width 1), exactly: 37 windows of 4 frames onto 3 rows x 11 frames, with
    frame ids 0 and 12 (ignored), negative scores (clamped to 0) and NaN scores (a NaN adds 0)."""
    n, T, n_rows, n_frames = 37, 4, 3, 11
    rng = np.random.default_rng(37)
    scores = rng.standard_normal(n).astype(np.float32)
    scores[[5, 20]] = np.nan
    first = rng.integers(-2, n_frames + 1, n)
    first[:3] = (-3, 0, 9)                                              # frames -3 .. 0, 0 .. 3 and 9 .. 12
    frames = (first[:, None] + np.arange(T)[None]).astype(np.int32)
    row = rng.integers(0, n_rows, n).astype(np.int32)
    assert (frames == 0).any() and (frames == 12).any() and (scores < 0).any()
    ref = np.zeros((n_rows, n_frames), np.float32)
    ii, tt = np.nonzero((frames >= 1) & (frames <= n_frames))
    np.maximum.at(ref, (row[ii], frames[ii, tt] - 1), np.fmax(scores, np.float32(0))[ii])
    L = _lib()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    s, f, r = d(scores), d(frames), d(row)
    out = torch.full((n_rows, n_frames), 3.0, device=DEV)               # (the callee zeroes it)
    L.check(L.lib().mcd_scatter_max(_ptr(s), _ptr(f), _ptr(r), n, T, n_rows, n_frames, _ptr(out), _stream()))
    assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32))
    assert (ref > 0).any() and (ref == 0).any()

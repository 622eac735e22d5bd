"""Host: the forecast fan without a GPU.

  - tests/forecast_fan_ref.py, the float64 restatement the kernel is held to, against np.quantile(method='linear'), np.mean, np.std
    and a brute-force mid-rank on float64 copies of fp32 lists, on the restatement's FLOAT64 values before the fp32 store
    (forecast_fan_ref.feature_stats64).  The bounds, from the formulas alone (u = 2^-53, M = max|x| of the list, K its length; a
    chain of n roundings is bounded by (n + 1) u instead of n u / (1 - n u)):
      quantile  |diff| <= (4 (K - 1) + 9) u M.  h = fl(q (K - 1)) is within u (K - 1) of the product on either side, g = h - floor(h)
                is exact, and an error dg in g moves the value by dg |x[i+1] - x[i]| <= 2 M dg: 2 (K - 1) u M per side.  Then the
                restatement rounds 1 - g, two products and one sum (4 u M); a lerp a + (b - a) g rounds a difference of up to 2 M, a
                product and a sum (5 u M);
      mean      |diff| <= 2 (K + 1) u M.  A sum of K terms in any order errs by at most K u sum|x| <= K^2 u M; the division by K
                leaves K u M and adds one rounding of a value <= M, on each side;
      std       |diff| <= (3 K + 10) u M.  Per side: the deviations d_j carry the mean's error (K + 1) u M and their own rounding
                (2 u M, |d| <= 2 M), which moves sqrt(sum d^2 / K) by at most (K + 3) u M (it is a norm); the squares, the K-term
                sum of non-negative terms, the division and the root add a RELATIVE (K / 2 + 2) u to a value <= M: (1.5 K + 5) u M.
                A constant list gives exactly 0 on both sides: sums of up to 1024 equal fp32 values are exact in float64;
      rank      counts are integers and (below + equal / 2) / K is the same float64 operations on both sides: exact.
    The fp32 values the kernel is compared with are these float64 values rounded once (feature_stats).
  - at q = 0.5 and S = 1 the restatement equals forecast_ref.assemble(method='median') bit for bit (the mean too; the spread up to std's fp32 roundings);
  - forecast_fan_rows with the restatement as `fan` numbers the rows / frame ids / cells of forecast_track_rows, from a
    TrajectoryWindows and from meta / frames, under 'identity' and 'all';
  - every Python-level refusal, by name: engine.forecast_fan's checks (before anything touches a device), forecast_fan_rows',
    forward(return_samples=True)'s, and the driver's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import forecast_fan_ref as FF
import forecast_ref as FR
import forecast_tta_ref as TR
from mocodad_amd.utils.eval_utils import forecast_fan_cover, forecast_fan_rows, forecast_observed_rows, forecast_track_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS8 = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)
F32_ULP = 2.0 ** -23
U = 2.0 ** -53


def _lists():
    """(name, (K,) f32 list) at the lengths 1, 2, 15, 64, 65, 1024: random, tie-heavy, constant and +-0 lists."""
    rng = np.random.default_rng(11)
    out = []
    for K in (1, 2, 15, 64, 65, 1024):
        out.append((f"random{K}", (rng.normal(size=K) * 3).astype(np.float32)))
        out.append((f"ties{K}", rng.integers(-2, 3, K).astype(np.float32) / 4))
        out.append((f"constant{K}", np.full(K, 0.7, np.float32)))
        z = np.where(rng.integers(0, 2, K) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        z[:: 5] = rng.normal(size=len(z[:: 5])).astype(np.float32) if K > 2 else z[:: 5]
        out.append((f"zeros{K}", z))
    return out


@pytest.mark.parametrize("name,x", _lists(), ids=[n for n, _ in _lists()])
def test_restatement_against_numpy(name, x):
    K = len(x)
    x64 = x.astype(np.float64)
    M = float(np.abs(x64).max())
    quant, mean, std, _ = FF.feature_stats64(x, LEVELS8)
    assert quant.dtype == np.float64 and all(isinstance(v, np.float64) for v in (mean, std))
    d_q = float(np.abs(quant - np.quantile(x64, LEVELS8, method="linear")).max())
    d_m = abs(float(mean) - float(np.mean(x64)))
    d_s = abs(float(std) - float(np.std(x64)))
    b_q, b_m, b_s = (4 * (K - 1) + 9) * U * M, 2 * (K + 1) * U * M, (3 * K + 10) * U * M
    print(f"{name}: quantile diff {d_q:.3e} (bound {b_q:.3e}), mean {d_m:.3e} ({b_m:.3e}), std {d_s:.3e} ({b_s:.3e})")
    assert d_q <= b_q and d_m <= b_m and d_s <= b_s
    assert quant[0] == x.min() and quant[-1] == x.max(), "levels 0 and 1 are the smallest and the largest value"
    assert (np.diff(quant) >= 0).all()
    q32, m32, s32, _ = FF.feature_stats(x, LEVELS8)
    assert q32.dtype == np.float32 and np.array_equal(q32, quant.astype(np.float32)) and m32 == np.float32(mean) and s32 == np.float32(std)
    if name.startswith("constant"):
        assert std == 0 and mean == x64[0] and (quant == x64[0]).all()
    rng = np.random.default_rng(K)
    for obs in (x[0], x[K // 2], np.float32(0.0), np.float32(-0.0), np.float32(x64.min() - 1), np.float32(x64.max() + 1),
                np.float32(rng.normal())):
        rank = FF.feature_stats64(x, LEVELS8, obs)[3]
        below = sum(1 for v in x64 if v < np.float64(obs))
        equal = sum(1 for v in x64 if v == np.float64(obs))
        assert rank == (below + equal / 2) / K and 0.0 <= rank <= 1.0
        assert FF.feature_stats(x, LEVELS8, obs)[3] == np.float32(rank)


def test_restatement_keeps_the_stable_order_of_signed_zeros():
    """-0.0 and +0.0 compare equal: the sorted list keeps them in list order, and a level that lands on one gives ITS sign"""
    x = np.array([0.0, -0.0, -0.0, 0.0, -1.0], np.float32)          # sorted: -1, +0, -0, -0, +0
    quant, _, _, rank = FF.feature_stats(x, (0.25, 0.5, 0.75, 1.0), np.float32(-0.0))
    assert np.signbit(quant).tolist() == [False, True, True, False] and not quant.any()
    assert rank == np.float32((1 + 4 / 2) / 5)


def test_restatement_nan_rules():
    x = np.array([1.0, np.nan, 3.0], np.float32)
    quant, mean, std, rank = FF.feature_stats(x, (0.5,), np.float32(1.0))
    assert np.isnan(quant).all() and np.isnan(mean) and np.isnan(std) and np.isnan(rank)
    quant, mean, std, rank = FF.feature_stats(np.array([1.0, 2.0, 3.0], np.float32), (0.5,), np.float32(np.nan))
    assert quant[0] == 2 and mean == 2 and np.isfinite(std) and np.isnan(rank)


def _windows(rng, N, S, Tx, n_cells, spare=2):
    poses_all = rng.normal(size=(N, S, 2, Tx, 17)).astype(np.float32)
    cell = rng.integers(-spare, n_cells + spare, size=(N, Tx)).astype(np.int32)
    return poses_all, cell


def test_median_level_with_one_sample_is_forecast_assemble():
    """S = 1: the value list of a cell is the list mcd_forecast_assemble reduces -- q = 0.5 is its MEDIAN pose, the mean its MEAN
    pose, bit for bit, and the mean over the features of `std` its spread up to std's fp32 roundings; with transforms,
    forecast_tta_ref.assemble."""
    rng = np.random.default_rng(21)
    poses_all, cell = _windows(rng, 40, 1, 3, 12)
    quant, mean, std, rank, count = FF.fan(poses_all, cell, 12, levels=(0.5,), max_cover=32)
    for method, got in (("median", quant[0]), ("mean", mean)):
        pose, want_count, spread = FR.assemble(poses_all[:, 0], cell, 12, method, "mean", 32)
        assert np.array_equal(FR.bits(got), FR.bits(pose)) and np.array_equal(count, want_count)
    assert len(set(count.tolist())) > 4 and rank is None
    # the spread is the mean of the 34 float64 deviations, rounded once; `std` holds each rounded to fp32 (relative error 2^-24):
    # their mean lies within 2^-24 max(std) of it, and the spread's own rounding adds as much
    ok = (count > 0) & (count <= 32)
    mean_std = std.astype(np.float64).sum(1) / 34.0
    assert ok.sum() > 4 and (np.abs(mean_std - spread)[ok] <= F32_ULP * std.astype(np.float64).max(1)[ok]).all()
    trans = rng.integers(0, 5, 40)
    inv = TR.inverse_table(rng.normal(size=(5, 6)) + np.array([1, 0, 0, 0, 1, 0]))
    inv[0] = [1, 0, 0, 0, 1, 0]
    quant, mean, _, _, count = FF.fan(poses_all, cell, 12, levels=(0.5,), max_cover=64, trans=trans, inv_affine=inv)
    pose, want_count, _ = TR.assemble(poses_all[:, 0], cell, trans, inv, 12, "median", "mean", 64)
    assert np.array_equal(FR.bits(quant[0]), FR.bits(pose)) and np.array_equal(count, want_count)


def test_restatement_special_cells():
    """k = 0: zeros; k = max_cover + 1 or K = 1025: NaN with the true count; cells out of range are ignored"""
    S = 205
    poses_all = np.random.default_rng(2).normal(size=(9, S, 2, 1, 17)).astype(np.float32)
    cell = np.array([[0]] * 5 + [[1]] * 3 + [[7]])          # K = 1025 on cell 0, 615 on cell 1, nothing on cell 2; 7 is out of range
    obs = np.zeros((3, 2, 17), np.float32)
    quant, mean, std, rank, count = FF.fan(poses_all, cell, 3, observed=obs, max_cover=32)
    assert count.tolist() == [5, 3, 0]
    assert all(np.isnan(a[..., 0, :]).all() for a in (quant, mean, std, rank))
    assert all(np.isfinite(a[..., 1, :]).all() for a in (quant, mean, std, rank))
    assert not any(a[..., 2, :].any() for a in (quant, mean, std, rank))
    _, mean, _, _, count = FF.fan(poses_all[:, :2], cell, 3, max_cover=4)
    assert count.tolist() == [5, 3, 0] and np.isnan(mean[0]).all() and np.isfinite(mean[1]).all()


# ------------------------------------------------------------------------------------------------ forecast_fan_rows
def _ref_fan(poses_all, cell, n_cells, **kw):
    kw["observed"] = np.asarray(kw["observed"])
    return FF.fan(np.asarray(poses_all), np.asarray(cell), n_cells, **kw)


def _ref_assemble(poses, cell, n_cells, trans=None, inv_affine=None, **kw):
    if trans is None:
        return FR.assemble(poses.numpy(), cell.numpy(), n_cells, **kw)
    return TR.assemble(poses.numpy(), cell.numpy(), np.asarray(trans), np.asarray(inv_affine), n_cells, **kw)


@pytest.mark.parametrize("transforms", ["identity", "all"])
def test_forecast_fan_rows_numbers_the_rows_of_forecast_track_rows(transforms):
    """The fixture of tests/test_forecast_tracks_host.py (two persons, one with a gap in its frame ids, seg_len 5, 2 transforms),
    S = 1: rows, frame ids and counts are forecast_track_rows', the 0.5 level its median pose, from both sources; the observed
    rows are the trajectory buffer's, and those scattered from the windows themselves equal them."""
    from mocodad_amd.data.windows import TrajectoryWindows
    rng = np.random.default_rng(3)
    trajs = {(1, 2, 0): (5, rng.normal(size=(8, 2, 17)).astype(np.float32)), (1, 2, 3): (1, rng.normal(size=(7, 2, 17)).astype(np.float32))}
    tw = TrajectoryWindows(trajs, 5, 2)
    tw.frames[tw.meta[:, 2] == 3] += (tw.frames[tw.meta[:, 2] == 3] > 4).int() * 6
    N, Tx, cover = len(tw), 3, 3 if transforms == "identity" else 6
    mf = np.tile(np.arange(2, 5), (N, 1))
    poses_all = torch.from_numpy(rng.normal(size=(N, 1, 2, Tx, 17)).astype(np.float32))
    kw = dict(levels=(0.5,), transforms=transforms, num_transform=2, max_cover=cover)
    a = forecast_fan_rows(poses_all, tw.trans.numpy(), mf, _ref_fan, windows=tw, **kw)
    # the windows as a dense tensor: transform 0's are the trajectory rows themselves
    buf = tw.buffer.view(-1, 2, 17).numpy()
    data = np.zeros((N, 2, 5, 17), np.float32)
    ident = tw.trans.numpy() == 0
    for i in np.flatnonzero(ident):
        r0 = int(tw.base[i]) // 34
        data[i] = buf[r0:r0 + 5].transpose(1, 0, 2)
    data[~ident] = np.nan                                  # (only the transform-0 windows may be read for the observed rows)
    b = forecast_fan_rows(poses_all, tw.trans.numpy(), mf, _ref_fan, meta=tw.meta.numpy(), frames=tw.frames.numpy(), data=data, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(FR.bits(x) if np.asarray(x).dtype == np.float32 else np.asarray(x), FR.bits(y) if np.asarray(y).dtype == np.float32 else np.asarray(y))
    t = forecast_track_rows(poses_all[:, 0], tw.trans.numpy(), mf, _ref_assemble, windows=tw, method="median", max_cover=cover,
                            transforms=transforms, num_transform=2)
    assert len(a) == 7, "the fan's five outputs, rows and frame ids"
    quant, mean, std, rank, count, rows, fids = a
    assert np.array_equal(rows, t[3]) and np.array_equal(fids, t[4]) and np.array_equal(count, t[1])
    assert np.array_equal(FR.bits(quant[0]), FR.bits(t[0]))
    o_tw = forecast_observed_rows(tw.trans.numpy(), windows=tw)
    o_host = forecast_observed_rows(tw.trans.numpy(), meta=tw.meta.numpy(), frames=tw.frames.numpy(), data=data)
    assert count.max() == cover and tuple(o_tw.shape) == (15, 2, 17) and o_tw.data_ptr() == tw.buffer.data_ptr()
    assert o_host.dtype == torch.float32 and np.array_equal(FR.bits(o_host.numpy()), FR.bits(o_tw.numpy()))
    with pytest.raises(ValueError, match="forecast_observed_rows needs a TrajectoryWindows, or"):
        forecast_observed_rows(tw.trans.numpy(), meta=tw.meta.numpy(), frames=tw.frames.numpy())
    with pytest.raises(ValueError, match="data must be the windows"):
        forecast_observed_rows(tw.trans.numpy(), meta=tw.meta.numpy(), frames=tw.frames.numpy(), data=data[:, :, :4])
    assert rank.shape == (15, 34) and ((rank >= 0) & (rank <= 1)).all() and not rank[count == 0].any()
    with pytest.raises(ValueError, match="forecast_fan_rows needs a TrajectoryWindows or"):
        forecast_fan_rows(poses_all, tw.trans.numpy(), mf, _ref_fan, **kw)
    with pytest.raises(ValueError, match="needs the windows themselves"):
        forecast_fan_rows(poses_all, tw.trans.numpy(), mf, _ref_fan, meta=tw.meta.numpy(), frames=tw.frames.numpy(), **kw)
    with pytest.raises(ValueError, match="per window"):
        forecast_fan_rows(poses_all[:-1], tw.trans.numpy(), mf, _ref_fan, windows=tw, **kw)


def test_fan_cover_is_refused_by_name():
    assert forecast_fan_cover(50, 20) == 20 and forecast_fan_cover(1024, 1) == 1
    with pytest.raises(ValueError, match=r"n_samples \* cover = 50 \* 21 = 1050 values on a row; the reduction holds 1024"):
        forecast_fan_cover(50, 21)
    with pytest.raises(ValueError, match=r"17 \* 64 = 1088"):
        forecast_fan_rows(torch.zeros(2, 17, 2, 3, 17), np.zeros(2), np.zeros((2, 3)), _ref_fan, meta=np.zeros((2, 4)),
                          frames=np.zeros((2, 5)), max_cover=64)
    with pytest.raises(ValueError, match=r"poses_all must be \(N, S, 2, Tx, 17\)"):
        forecast_fan_rows(torch.zeros(2, 2, 3, 17), np.zeros(2), np.zeros((2, 3)), _ref_fan, meta=np.zeros((2, 4)), frames=np.zeros((2, 5)))


# ------------------------------------------------------------------------------------------------ refusals
def test_wrapper_argument_errors():
    """every check of engine.forecast_fan comes before anything touches a device (there is none here)"""
    from mocodad_amd.engine import forecast_fan, forecast_levels
    p, cell = torch.zeros(4, 5, 2, 3, 17), torch.zeros(4, 3, dtype=torch.int32)
    for levels, msg in (((), "levels must hold 1 .. 8 values, got 0"), (tuple(np.linspace(0, 1, 9)), "levels must hold 1 .. 8 values, got 9"),
                        ((0.5, 0.1), "levels must be strictly ascending"), ((0.5, 0.5), "levels must be strictly ascending"),
                        ((-0.1, 0.5), r"levels must lie in \[0, 1\]"), ((0.5, 1.5), r"levels must lie in \[0, 1\]"),
                        ((float("nan"),), r"levels must lie in \[0, 1\]"), (("a",), "levels must be a sequence of numbers"),
                        (0.5, "levels must be a sequence of numbers")):
        with pytest.raises(ValueError, match=msg):
            forecast_fan(p, cell, 6, levels=levels)
    assert forecast_levels([0, 1]) == (0.0, 1.0)
    for kw, msg in ((dict(max_cover=0), "max_cover must be in 1 .. 32"), (dict(max_cover=33), "max_cover must be in 1 .. 32"),
                    (dict(max_cover=65, trans=torch.zeros(4, dtype=torch.int32), inv_affine=np.zeros((1, 6))), "max_cover must be in 1 .. 64"),
                    (dict(trans=torch.zeros(4, dtype=torch.int32)), "trans and inv_affine go together"),
                    (dict(inv_affine=np.zeros((1, 6))), "trans and inv_affine go together"),
                    (dict(trans=torch.zeros(3, dtype=torch.int32), inv_affine=np.zeros((1, 6))), "trans must be an integer"),
                    (dict(trans=torch.zeros(4), inv_affine=np.zeros((1, 6))), "trans must be an integer"),
                    (dict(trans=torch.zeros(4, dtype=torch.int32), inv_affine=np.zeros((0, 6))), "inv_affine must be"),
                    (dict(trans=torch.zeros(4, dtype=torch.int32), inv_affine=np.zeros((2, 5))), "inv_affine must be"),
                    (dict(observed=torch.zeros(6, 34)), "observed must be a float32"),
                    (dict(observed=torch.zeros(6, 2, 17, dtype=torch.float64)), "observed must be a float32"),
                    (dict(out=(None,) * 3, device="cuda:0"), "five buffers"),
                    (dict(out=(None, None, None, torch.zeros(6, 34), None), device="cuda:0"), r"out\[3\] \(rank\) must be None without observed"),
                    (dict(out=(torch.zeros(3, 6, 34), None, None, None, None), device="cuda:0"), r"out\[0\] \(quant\) must be"),
                    (dict(out=(None, torch.zeros(6, 34), None, None, None), device="cuda:0"), r"out\[1\] \(mean\) must be"),
                    (dict(out=(None, None, None, None, torch.zeros(6)), device="cuda:0"), r"out\[4\] \(count\) must be"),
                    (dict(workspace=torch.zeros(6 * 32, dtype=torch.int32), device="cuda:0"), "workspace must be")):
        with pytest.raises(ValueError, match=msg):
            forecast_fan(p, cell, 6, **kw)
    with pytest.raises(ValueError, match="n_cells must be >= 0"):
        forecast_fan(p, cell, -1)
    for bad in (torch.zeros(4, 2, 3, 17), torch.zeros(4, 0, 2, 3, 17), torch.zeros(4, 5, 3, 3, 17), torch.zeros(4, 5, 2, 33, 17),
                torch.zeros(4, 5, 2, 3, 16)):
        with pytest.raises(ValueError, match=r"poses_all must have shape \(N, S, 2, Tx, 17\)"):
            forecast_fan(bad, cell, 6)
    with pytest.raises(ValueError, match="cell must be an integer"):
        forecast_fan(p, torch.zeros(4, 2, dtype=torch.int32), 6)
    with pytest.raises(ValueError, match="cell must be an integer"):
        forecast_fan(p, torch.zeros(4, 3), 6)


def test_library_rejects_bad_arguments_before_any_device_call():
    """the C entry itself (there is no GPU here: a device call would not come back as MCD_EINVAL)"""
    import ctypes as C
    from mocodad_amd import _lib
    L = _lib.lib()
    assert _lib.MCD_FORECAST_FAN_VALUES == 1024 and _lib.MCD_FORECAST_FAN_LEVELS == 8
    one = C.c_void_p(8)          # (a non-null address nobody reads)

    def call(n=2, S=5, Tx=3, n_cells=4, levels=(0.1, 0.5, 0.9), n_levels=None, cover=3, trans=None, inv=None, nt=0, observed=one, rank=one,
             poses=one, cell=one, ws=one, quant=one, count=one):
        lv = (C.c_double * max(len(levels), 1))(*levels) if levels is not None else None
        rc = L.mcd_forecast_fan(poses, cell, trans, inv, nt, n, S, Tx, n_cells, lv, len(levels) if n_levels is None else n_levels, cover,
                                observed, ws, quant, one, one, rank, count, None)
        return rc, L.mcd_last_error().decode()

    EINVAL = -1
    for kw, msg in ((dict(n=-1), "need n, n_cells >= 0"), (dict(n_cells=-1), "need n, n_cells >= 0"), (dict(Tx=0), "n_corrupt"), (dict(Tx=33), "n_corrupt"),
                    (dict(cover=0), "max_cover <= 32"), (dict(cover=33), "max_cover <= 32"), (dict(cover=65, trans=one, inv=one, nt=1), "max_cover <= 64"),
                    (dict(S=0), "n_samples >= 1"), (dict(n=2**31 // 3 + 1), "exceeds 2^31 - 1"),
                    (dict(trans=one), "trans needs inv_affine"), (dict(trans=one, inv=one, nt=0), "n_transform >= 1"),
                    (dict(levels=()), "n_levels <= 8"), (dict(n_levels=9), "n_levels <= 8"), (dict(levels=None, n_levels=1), "null argument"),
                    (dict(levels=(-0.5,)), "levels outside"), (dict(levels=(0.5, 1.5)), "levels outside"), (dict(levels=(float("nan"),)), "levels outside"),
                    (dict(levels=(0.5, 0.5)), "strictly ascending"), (dict(levels=(0.9, 0.1)), "strictly ascending"),
                    (dict(observed=None), "go together"), (dict(rank=None), "go together"),
                    (dict(ws=None), "null argument"), (dict(quant=None), "null argument"), (dict(count=None), "null argument"),
                    (dict(poses=None), "null argument"), (dict(cell=None), "null argument")):
        rc, err = call(**kw)
        assert rc == EINVAL and msg in err, (kw, rc, err)
    assert call(n_cells=0)[0] == 0 and call(n_cells=0, observed=None, rank=None, ws=None, quant=None, count=None, poses=None, cell=None)[0] == 0


def test_forward_refuses_the_random_aggregation():
    from helpers import golden_weights, make_args
    from mocodad_amd.models.mocodad import MoCoDAD
    _, cfg = golden_weights("inject")
    m = MoCoDAD(make_args(cfg, aggregation_strategy="random"))
    batch = [torch.zeros(2, 2, 6, 17), torch.zeros(2), torch.zeros(2, 4), torch.zeros(2, 6)]
    with pytest.raises(ValueError, match="return_samples: the 'random' aggregation"):
        m.forward(batch, return_samples=True)
    with pytest.raises(ValueError, match="return_samples: the 'random' aggregation"):
        m.forward(batch, "random", return_samples=True)


def _refused(tmp_path, config, over, extra=(), env=None):
    with open(os.path.join(ROOT, "configs", config)) as f:
        cfg = yaml.safe_load(f)
    cfg.update(over)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    # no device is visible to the child: a refusal that came after a GPU call would fail differently
    e = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", **(env or {}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", str(p), "--synthetic", "2", "--random-init",
                        "--forecast-fan", str(tmp_path / "f.npz"), *extra], capture_output=True, text=True, timeout=300, cwd=ROOT, env=e)
    assert r.returncode != 0 and not (tmp_path / "f.npz").exists()
    return r.stderr


def test_driver_refusals(tmp_path):
    err = _refused(tmp_path, "hr_avenue_test.yaml", {}, env=dict(WORLD_SIZE="2"))
    assert "--forecast-fan runs in one process" in err, err[-2000:]
    err = _refused(tmp_path, "ubnormal_latent_test.yaml", {})
    assert "--forecast-fan needs the pose model, or the latent model with latent_score_space: 'pose'" in err, err[-2000:]
    err = _refused(tmp_path, "hr_avenue_test.yaml", {}, extra=("--joint-scores", str(tmp_path / "j.npz")))
    assert "--forecast-fan and --joint-scores are separate runs" in err, err[-2000:]
    err = _refused(tmp_path, "hr_avenue_test.yaml", {}, extra=("--forecast-tracks", str(tmp_path / "t.npz")))
    assert "--forecast-tracks and --forecast-fan are separate runs" in err and not (tmp_path / "t.npz").exists(), err[-2000:]
    err = _refused(tmp_path, "hr_avenue_test.yaml", dict(aggregation_strategy="random"))
    assert "--forecast-fan: not aggregation_strategy 'random'" in err, err[-2000:]


@pytest.mark.parametrize("levels,msg", [(",", "--forecast-levels must hold 1 .. 8 values, got 0"),
                                        ("0,.1,.2,.3,.4,.5,.6,.7,.8", "--forecast-levels must hold 1 .. 8 values, got 9"),
                                        ("0.9,0.1", "--forecast-levels must be strictly ascending"),
                                        ("0.5,1.5", "--forecast-levels must lie in [0, 1]"), ("0.5,x", "could not convert")])
def test_driver_refuses_bad_levels(tmp_path, levels, msg):
    err = _refused(tmp_path, "hr_avenue_test.yaml", {}, extra=("--forecast-levels", levels))
    assert "--forecast-fan" in err and msg in err, err[-2000:]


def test_driver_refuses_more_values_than_a_row_holds(tmp_path):
    """hr_avenue_test.yaml: 3 forecast frames per window, 5 transforms -- 342 samples x 3 and 70 samples x 15 pass 1024"""
    over = dict(seg_len=6, conditioning_indices=[0, 1, 2], num_transform=5)
    err = _refused(tmp_path, "hr_avenue_test.yaml", dict(over, n_generated_samples=342))
    assert "--forecast-fan" in err and "n_samples * cover = 342 * 3 = 1026 values on a row; the reduction holds 1024" in err, err[-2000:]
    err = _refused(tmp_path, "hr_avenue_test.yaml", dict(over, n_generated_samples=70), extra=("--forecast-transforms", "all"))
    assert "--forecast-fan" in err and "n_samples * cover = 70 * 15 = 1050 values on a row; the reduction holds 1024" in err, err[-2000:]
    err = _refused(tmp_path, "hr_avenue_test.yaml", dict(over, num_transform=22), extra=("--forecast-transforms", "all"))
    assert "--forecast-fan" in err and "22 * 3 = 66 forecasts" in err, err[-2000:]

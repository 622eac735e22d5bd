"""GPU: the forecast fan -- mcd_forecast_fan against the float64 restatement of tests/forecast_fan_ref.py BIT FOR BIT (NaN payloads
aside), forward(return_samples=True) on the pose model and on the latent model in pose space, and eval_MoCoDAD.py --forecast-fan on
the dataset fixture and on synthetic clips.

Shapes: a few cells per case, with the list lengths K = k * S at which the kernel takes another path -- 1 (no sort stage), 2, 15
(3 windows x 5 samples), 64 and 65 (a power of two and one more: the padding), 1024 (the largest list; two joints per LDS group)
and 1025 (NaN with its count), k = max_cover + 1, an uncovered cell, cells outside the output, 1 and 8 levels, Tx = 1 and 12, with
and without transforms (5 transforms x 3 frames x 5 samples = 75 values)."""
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
from dataset_spec import DATASET, ROOT, load_dataset_golden
from helpers import golden_weights, make_args
from mocodad_amd.utils.transforms import affine_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG_LEN = 6
VID_RES = (640, 360)
LEVELS8 = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)
NAMES = ("quant", "mean", "std", "rank", "count")


def _fan(poses_all, cell, n_cells, **kw):
    from mocodad_amd.engine import forecast_fan
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    kw = {k: t(v) if k in ("observed", "trans") else v for k, v in kw.items()}
    return tuple(None if o is None else o.cpu().numpy() for o in forecast_fan(t(poses_all), t(cell), n_cells, device=DEV, **kw))


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            assert g is None and w is None, (what, name)
        elif name == "count":
            assert np.array_equal(g, w), (what, name, g, w)
        else:
            bad = np.argwhere(FR.bits(g) != FR.bits(w))
            assert not len(bad), (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _cells(rng, N, Tx, covers, spare=(-7, -1)):
    """cell (N, Tx): cell c is named by covers[c] pairs drawn without replacement; the other pairs name cells outside the output
    (negative, or n_cells and beyond)."""
    n_cells = len(covers)
    assert sum(covers) <= N * Tx
    flat = np.where(rng.integers(0, 2, N * Tx) == 1, rng.integers(spare[0], spare[1] + 1, N * Tx), rng.integers(n_cells, n_cells + 3, N * Tx))
    slots = rng.permutation(N * Tx)
    at = 0
    for c, k in enumerate(covers):
        flat[slots[at:at + k]] = c
        at += k
    return flat.reshape(N, Tx).astype(np.int32)


def _values(rng, shape, kind):
    if kind == "random":
        return rng.normal(size=shape).astype(np.float32)
    x = (rng.integers(-3, 4, size=shape) / 4).astype(np.float32)          # ties: seven values, a quarter apart ...
    return np.where((x == 0) & (rng.integers(0, 2, size=shape) == 1), np.float32(-0.0), x).astype(np.float32)      # ... and both zeros


#        name             N   S    Tx  covers              max_cover  levels
CASES = [("K1_K2",         6,  1,   1,  [1, 2, 0, 3],       32,        (0.5,)),
         ("K2_K64_over",   70, 2,   1,  [1, 32, 33],        32,        LEVELS8),
         ("K15_K65_Tx12",  4,  5,   12, [3, 13, 1, 0, 7],   32,        (0.1, 0.5, 0.9)),
         ("K1024",         12, 32,  3,  [32, 1],            32,        (0.1, 0.5, 0.9)),
         ("K1025",         11, 205, 1,  [5, 4, 1],          8,         (0.0, 0.3, 1.0)),
         ("cover_plus_1",  4,  3,   3,  [5, 4, 0],          4,         LEVELS8)]


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fan_bits(case, kind):
    name, N, S, Tx, covers, max_cover, levels = case
    rng = np.random.default_rng(len(name) * 1000 + N)
    poses_all, cell = _values(rng, (N, S, 2, Tx, 17), kind), _cells(rng, N, Tx, covers)
    observed = _values(rng, (len(covers), 2, 17), kind)
    want = FF.fan(poses_all, cell, len(covers), levels, observed, max_cover)
    assert want[4].tolist() == covers
    _same(_fan(poses_all, cell, len(covers), levels=levels, observed=observed, max_cover=max_cover), want, (name, kind))
    got = _fan(poses_all, cell, len(covers), levels=levels, max_cover=max_cover)          # no observed: no rank, the rest unchanged
    assert got[3] is None
    _same(got[:3] + (want[3],) + got[4:], want, (name, kind, "no rank"))
    for c, k in enumerate(covers):
        out = [a[..., c, :] for a in want[:4]]
        if k == 0:
            assert not any(o.any() for o in out)
        elif k > max_cover or k * S > 1024:
            assert all(np.isnan(o).all() for o in out)
        else:
            assert all(np.isfinite(o).all() for o in out)
            if kind == "ties":
                assert ((want[3][c] > 0) & (want[3][c] < 1)).any(), "some observed coordinate ties with values of the list"


def test_levels_zero_and_one_are_the_smallest_and_the_largest_value():
    rng = np.random.default_rng(4)
    N, S, Tx = 9, 4, 2
    poses_all, cell = _values(rng, (N, S, 2, Tx, 17), "random"), _cells(rng, N, Tx, [7, 1, 4])
    quant = _fan(poses_all, cell, 3, levels=LEVELS8)[0]
    rows = poses_all.transpose(0, 3, 1, 4, 2).reshape(N * Tx, S, 34)
    for c in range(3):
        vals = rows[cell.reshape(-1) == c].reshape(-1, 34)
        assert np.array_equal(quant[0, c], vals.min(0)) and np.array_equal(quant[-1, c], vals.max(0))
        assert (np.diff(quant[:, c], axis=0) >= 0).all()


def _tta(rng, kind="random", S=5, Tx=3, covers=(15, 64, 65, 2, 0), N=60):
    """windows of transforms -1 .. 5 against a table of 5 (row 0 the identity): the windows outside the table are ignored"""
    inv = TR.inverse_table(affine_table(5).numpy())
    assert TR.is_identity_row(inv[0]) and not any(TR.is_identity_row(m) for m in inv[1:])
    poses_all = _values(rng, (N, S, 2, Tx, 17), kind)
    cell = _cells(rng, N, Tx, list(covers))
    trans = rng.integers(0, 5, N).astype(np.int32)
    outside = np.flatnonzero((cell < 0).all(1) | (cell >= len(covers)).all(1))[:4]          # windows that name no cell of the output
    trans[outside] = [-1, 5, 6, -3][:len(outside)]
    return poses_all, cell, trans, inv


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_fan_bits_with_every_transform(kind):
    """75 values (5 transforms x 3 frames x 5 samples), 320 (64 pairs), 65 pairs (NaN with its count), 10, none"""
    rng = np.random.default_rng(75)
    poses_all, cell, trans, inv = _tta(rng, kind)
    observed = _values(rng, (5, 2, 17), kind)
    want = FF.fan(poses_all, cell, 5, (0.1, 0.5, 0.9), observed, 64, trans, inv)
    assert want[4].tolist() == [15, 64, 65, 2, 0] and np.isnan(want[1][2]).all() and np.isfinite(want[1][[0, 1, 3]]).all()
    _same(_fan(poses_all, cell, 5, observed=observed, max_cover=64, trans=trans, inv_affine=inv), want, kind)
    # a window whose transform is outside the table is ignored like a cell outside the output
    cell2, trans2 = cell.copy(), trans.copy()
    i = int(np.flatnonzero((cell == 0).any(1))[0])
    trans2[i] = 5
    want2 = FF.fan(poses_all, cell2, 5, (0.1, 0.5, 0.9), observed, 64, trans2, inv)
    assert want2[4][0] < 15
    _same(_fan(poses_all, cell2, 5, observed=observed, max_cover=64, trans=trans2, inv_affine=inv), want2, (kind, "outside the table"))


def test_a_nan_sample_reaches_only_its_feature_and_a_nan_observed_only_its_rank():
    rng = np.random.default_rng(8)
    N, S, Tx = 6, 5, 3
    poses_all, cell = _values(rng, (N, S, 2, Tx, 17), "random"), _cells(rng, N, Tx, [3, 5, 2])
    i, tx = [int(v[0]) for v in np.nonzero(cell == 1)]
    poses_all[i, 2, 1, tx, 4] = np.nan                          # y of joint 4, a sample of a pair of cell 1: feature 9
    observed = _values(rng, (3, 2, 17), "random")
    observed[0, 0, 7] = np.nan                                  # x of joint 7 of cell 0: feature 14
    want = FF.fan(poses_all, cell, 3, LEVELS8, observed, 32)
    got = _fan(poses_all, cell, 3, levels=LEVELS8, observed=observed)
    _same(got, want, "nan")
    nan = [np.isnan(a) for a in got[:4]]
    assert nan[0][:, 1, 9].all() and nan[1][1, 9] and nan[2][1, 9] and nan[3][1, 9] and nan[3][0, 14]
    assert nan[0].sum() == 8 and nan[1].sum() == 1 and nan[2].sum() == 1 and nan[3].sum() == 2
    # under a transform that is no identity row, the NaN reaches both coordinates of its joint (the map mixes x and y)
    inv = TR.inverse_table(affine_table(5).numpy())
    trans = np.full(N, 1, np.int32)
    want = FF.fan(poses_all, cell, 3, LEVELS8, observed, 64, trans, inv)
    got = _fan(poses_all, cell, 3, levels=LEVELS8, observed=observed, max_cover=64, trans=trans, inv_affine=inv)
    _same(got, want, "nan, mapped")
    nan = np.isnan(got[1])
    assert nan[1, 8] and nan[1, 9] and nan.sum() == 2 and np.isnan(got[3]).sum() == 3


def test_two_calls_on_a_garbage_workspace_give_the_same_bits():
    """600 windows of 5 transforms on 40 cells, three launches of the claim kernel's workgroups: the slots the pairs get differ
    from run to run, the workspace and the outputs start as different garbage, and nothing in the result depends on either"""
    from mocodad_amd.engine import forecast_fan
    rng = np.random.default_rng(6)
    N, S, Tx, n_cells = 600, 3, 3, 40
    poses_all = torch.from_numpy(_values(rng, (N, S, 2, Tx, 17), "ties"))
    cell = torch.from_numpy(rng.integers(-2, n_cells + 2, size=(N, Tx)).astype(np.int32))
    trans = torch.from_numpy(rng.integers(0, 5, N).astype(np.int32))
    inv = TR.inverse_table(affine_table(5).numpy())
    observed = torch.from_numpy(_values(rng, (n_cells, 2, 17), "ties"))
    res = []
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        ws = torch.randint(-2**31, 2**31 - 1, (n_cells * 64 + 5,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
        out = (torch.full((3, n_cells, 34), float(seed), device=DEV), torch.full((n_cells, 34), float(seed), device=DEV),
               torch.full((n_cells, 34), float(seed), device=DEV), torch.full((n_cells, 34), float(seed), device=DEV),
               torch.full((n_cells,), seed, device=DEV, dtype=torch.int32))
        r = forecast_fan(poses_all, cell, n_cells, observed=observed, max_cover=64, trans=trans, inv_affine=inv, out=out, workspace=ws)
        assert all(a is b for a, b in zip(r, out))
        res.append(tuple(t.cpu().numpy() for t in r))
    for a, b in zip(*res):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    want = FF.fan(poses_all.numpy(), cell.numpy(), n_cells, (0.1, 0.5, 0.9), observed.numpy(), 64, trans.numpy(), inv)
    _same(res[0], want, "garbage workspace")
    assert want[4].max() > 40 and (want[4] > 0).all()


def test_empty_calls():
    from mocodad_amd.engine import forecast_fan
    observed = np.ones((4, 2, 17), np.float32)
    got = _fan(np.zeros((0, 3, 2, 3, 17), np.float32), np.zeros((0, 3), np.int32), 4, observed=observed)          # n == 0: zeros
    assert got[0].shape == (3, 4, 34) and all(not a.any() for a in got)
    got = _fan(np.zeros((0, 3, 2, 3, 17), np.float32), np.zeros((0, 3), np.int32), 4, max_cover=64, trans=np.zeros(0, np.int32),
               inv_affine=np.eye(2, 3).reshape(1, 6))
    assert got[3] is None and all(not a.any() for a in got if a is not None)
    r = forecast_fan(torch.zeros(2, 3, 2, 3, 17), torch.zeros(2, 3, dtype=torch.int32), 0, observed=torch.zeros(0, 2, 17), device=DEV)
    assert [tuple(t.shape) for t in r] == [(3, 0, 34), (0, 34), (0, 34), (0, 34), (0,)]                           # n_cells == 0: nothing


def test_one_sample_is_forecast_assemble():
    """S = 1: the list of a cell is the list mcd_forecast_assemble reduces.  The 0.5 level is its MEDIAN pose and the mean its MEAN
    pose, bit for bit.  Its 'mean' spread is the mean of the 34 float64 deviations rounded to fp32 once, where `std` holds each
    deviation rounded to fp32 (relative error 2^-24 each): the float64 mean of `std` lies within 2^-24 max(std) of the unrounded
    spread, and the spread's own rounding adds at most as much -- the bound asserted is 2^-23 max(std) per cell."""
    from mocodad_amd.engine import forecast_assemble
    rng = np.random.default_rng(31)
    N, Tx, n_cells = 40, 3, 12
    poses = torch.from_numpy(_values(rng, (N, 2, Tx, 17), "random"))
    cell = torch.from_numpy(rng.integers(-2, n_cells + 2, size=(N, Tx)).astype(np.int32))
    quant, mean, std, _, count = _fan(poses[:, None], cell, n_cells, levels=(0.5,))
    med = [t.cpu().numpy() for t in forecast_assemble(poses, cell, n_cells, method="median", spread_method="mean", device=DEV)]
    avg = [t.cpu().numpy() for t in forecast_assemble(poses, cell, n_cells, method="mean", spread_method="mean", device=DEV)]
    assert np.array_equal(count, med[1]) and len(set(count.tolist())) > 4
    assert np.array_equal(FR.bits(quant[0]), FR.bits(med[0])) and np.array_equal(FR.bits(mean), FR.bits(avg[0]))
    d = np.abs(std.astype(np.float64).sum(1) / 34.0 - avg[2].astype(np.float64))
    bound = 2.0 ** -23 * std.astype(np.float64).max(1)
    print("one sample | mean of std against the spread, per cell: largest diff / bound =", (d[bound > 0] / bound[bound > 0]).max())
    assert (d <= bound).all()
    inv = TR.inverse_table(affine_table(5).numpy())
    trans = torch.from_numpy(rng.integers(0, 5, N).astype(np.int32))
    quant, mean, _, _, count = _fan(poses[:, None], cell, n_cells, levels=(0.5,), max_cover=64, trans=trans, inv_affine=inv)
    med = [t.cpu().numpy() for t in forecast_assemble(poses, cell, n_cells, method="median", max_cover=64, trans=trans, inv_affine=inv, device=DEV)]
    assert np.array_equal(count, med[1]) and np.array_equal(FR.bits(quant[0]), FR.bits(med[0]))


# ---------------------------------------------------------------- the module surface
def _tracks(seg_len=6, nt=2):
    from mocodad_amd.data.windows import TrajectoryWindows
    rng = np.random.default_rng(21)
    trajs = {(1, 1, p): (3 + p, (rng.normal(size=(n, 2, 17)) * 0.3).astype(np.float32)) for p, n in ((0, 13), (2, 9), (5, 6))}
    return TrajectoryWindows(trajs, seg_len, nt).to(DEV)          # 8 + 4 + 1 windows x 2 transforms


def _eq(a, b):
    if torch.is_tensor(a) and torch.is_tensor(b):
        return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    return a is b or type(a) is type(b)          # (the window view a batch carries)


def _check_forward(m, aggrs, **fw):
    """return_samples: the loss of the same aggregation on the non-fused path, the samples of aggr_strategy 'all', the list
    otherwise unchanged, and unchanged when the keyword is off"""
    from mocodad_amd.engine import forecast_fan
    from mocodad_amd.utils.eval_utils import forecast_fan_rows
    tw = _tracks()
    N, S, Tx = len(tw), m.n_generated_samples, m.n_frames_corrupt
    with torch.no_grad():
        every = m.forward(tw.batch(0, N), aggr_strategy="all", return_="all", window_offset=0, **fw)[1]
        assert tuple(every.shape) == (N, S, 2, Tx, 17) and torch.isfinite(every).all()
        for aggr in aggrs:
            plain = m.forward(tw.batch(0, N), aggr_strategy=aggr, window_offset=0, **fw)
            off = m.forward(tw.batch(0, N), aggr_strategy=aggr, window_offset=0, return_samples=False, **fw)
            assert len(plain) == len(off) == 5 and all(_eq(a, b) for a, b in zip(plain, off)), aggr
            # (return_ 'all' wants a pose: the pose model then scores and aggregates in separate calls; the latent model's one-call
            # path states the bits of that sequence)
            unfused = m.forward(tw.batch(0, N), aggr_strategy=aggr, return_="all", window_offset=0, **fw)
            on = m.forward(tw.batch(0, N), aggr_strategy=aggr, window_offset=0, return_samples=True, **fw)
            assert len(on) == 7 and all(_eq(a, b) for a, b in zip(plain[1:], on[1:5])), aggr
            assert torch.equal(on[0], unfused[0]), (aggr, "the loss of the non-fused call")
            assert torch.equal(on[-2], every) and torch.equal(on[-1].cpu(), m.map_frames(None, N).cpu()), aggr
            both = m.forward(tw.batch(0, N), aggr_strategy=aggr, window_offset=0, return_maps=True, return_samples=True, **fw)
            maps = m.forward(tw.batch(0, N), aggr_strategy=aggr, window_offset=0, return_maps=True, **fw)
            assert len(both) == 9 and torch.equal(both[-4], maps[-2]) and torch.equal(both[-2], every), aggr
    got = forecast_fan_rows(every, tw.trans.numpy(), on[-1].cpu().numpy(), forecast_fan, windows=tw, max_cover=Tx)
    ref = lambda p, c, n, **kw: FF.fan(p.cpu().numpy(), c.numpy(), n, **{k: (v.cpu().numpy() if k == "observed" else v) for k, v in kw.items()})
    want = forecast_fan_rows(every, tw.trans.numpy(), on[-1].cpu().numpy(), ref, windows=tw, max_cover=Tx)
    _same(tuple(t.cpu().numpy() for t in got[:5]), want[:5], "forecast_fan_rows")
    assert len(got) == 7 and np.array_equal(got[5], want[5]) and np.array_equal(got[6], want[6]) and got[4].max().item() == Tx


def test_pose_model_returns_its_samples():
    from mocodad_amd.models.mocodad import MoCoDAD
    sd, cfg = golden_weights("inject")
    m = MoCoDAD(make_args(cfg, noise_steps=3, n_generated_samples=3, model_return_value="loss", aggregation_strategy="best")).to(DEV)
    m.load_state_dict(sd)
    _check_forward(m, ("best", "mean", "median", "median_pose", "quantile:0.3"))
    with pytest.raises(ValueError, match="return_samples: the 'random' aggregation"):
        m.forward(_tracks().batch(0, 2), aggr_strategy="random", return_samples=True)


def test_latent_model_in_pose_space_returns_its_samples():
    from test_latent_forecast_gpu import diffusion_module
    m, sd = diffusion_module()
    m.load_decoder(sd)
    try:
        _check_forward(m, ("best", "mean", "mean_pose"), space="pose")
        with pytest.raises(ValueError, match="return_samples: in latent space"):
            m.forward(_tracks().batch(0, 2), return_samples=True, space="latent")
    finally:
        m._decoder_sd = m._decoder = None


# ---------------------------------------------------------------- the driver
def _run_driver(cfg_path, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", cfg_path, *extra]
    r = subprocess.run(cmd + (["--forecast-fan", str(out)] if out else []), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "AUC:" in r.stdout and ("forecast fan:" in r.stdout) == bool(out), r.stdout[-2000:]
    return r.stdout, (np.load(out) if out else None)


def _auc(stdout):
    return stdout.split("AUC:")[1].split()[0]


def _fan_checks(z, levels, S, Tx, pixels):
    rows, R, L = z["rows"], len(z["rows"]), len(levels)
    keys = {"rows", "row_columns", "frames", "levels", "observed_norm", "bands_norm", "mean_norm", "std_norm", "rank", "count", "n_samples",
            "joint_names"} | ({"observed", "bands"} if pixels else set())
    assert set(z.files) == keys, sorted(z.files)
    assert R > 0 and rows.shape == (R, 3) and z["frames"].shape == (R,) and z["count"].shape == (R,)
    assert z["bands_norm"].shape == (L, R, 34) and z["bands_norm"].dtype == np.float32 and np.array_equal(z["levels"], np.asarray(levels))
    assert all(z[k].shape == (R, 34) for k in ("observed_norm", "mean_norm", "std_norm", "rank"))
    assert int(z["n_samples"]) == S and list(z["joint_names"])[0] == "nose" and 0 < z["count"].max() <= Tx
    spaces = [z["bands_norm"]] + ([z["bands"]] if pixels else [])
    if pixels:
        assert z["bands"].shape == (L, R, 34) and z["observed"].shape == (R, 34)
    for b in spaces:
        assert np.isfinite(b).all() and (np.diff(b, axis=0) >= 0).all(), "the bands are ordered per feature"
        assert not b[:, z["count"] == 0].any()
    has = z["count"] > 0
    assert ((z["rank"] >= 0) & (z["rank"] <= 1)).all() and (z["std_norm"][has] > 0).any() and not z["rank"][~has].any()


def test_driver_on_the_dataset_fixture(tmp_path):
    from mocodad_amd.data import trajectories as T
    from mocodad_amd.engine import forecast_fan
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    from mocodad_amd.utils.eval_utils import forecast_fan_rows
    from test_dataset_gpu import _driver_config, _write_scaler
    g = load_dataset_golden()
    cfg_path = _driver_config(tmp_path, g)
    args = load_config(cfg_path)
    _write_scaler(args.ckpt_dir, g["train_center"], g["train_scale"])
    torch.manual_seed(123)
    sd = MoCoDAD(args).state_dict()
    torch.save({"state_dict": sd}, os.path.join(args.ckpt_dir, args.load_ckpt))
    levels = (0.05, 0.5, 0.95)
    stdout, z = _run_driver(cfg_path, tmp_path / "f.npz", "--forecast-levels", "0.05,0.5,0.95")
    plain, _ = _run_driver(cfg_path, None)
    assert _auc(stdout) == _auc(plain), "the AUC line is the same with and without the flag"
    assert "device bytes held for poses_all" in stdout and "_norm outputs only" not in stdout
    _fan_checks(z, levels, 2, 3, pixels=True)
    raw = T.load_raw(DATASET, "test", SEG_LEN)
    assert np.array_equal(z["observed"], raw.poses) and np.array_equal(z["frames"], raw.frames)
    # one offline call over all windows: the same samples (the noise is keyed by the global window id), the same bands
    m = MoCoDAD(args).to(DEV)
    m.load_state_dict(sd)
    tw = T.load_dataset(args, DEV)[0]
    with torch.no_grad():
        out = m.forward(tw.batch(0, len(tw)), return_samples=True, window_offset=0)
    got = forecast_fan_rows(out[-2], tw.trans.numpy(), out[-1].cpu().numpy(), forecast_fan, windows=tw, levels=levels, max_cover=3)
    assert np.array_equal(FR.bits(z["bands_norm"]), FR.bits(got[0].cpu().numpy())) and np.array_equal(z["count"], got[4].cpu().numpy())
    assert np.array_equal(FR.bits(z["rank"]), FR.bits(got[3].cpu().numpy())) and np.array_equal(z["rows"], got[5])
    for l in range(3):
        want = FR.denormalize(z["bands_norm"][l], raw.poses, VID_RES, g["train_center"], g["train_scale"], z["count"])
        assert np.array_equal(FR.bits(z["bands"][l]), FR.bits(want))
    assert np.array_equal(z["observed_norm"], tw.buffer.view(-1, 2, 17).transpose(1, 2).reshape(-1, 34).cpu().numpy())


def test_driver_on_synthetic_clips_with_every_transform(tmp_path):
    from mocodad_amd.data import synthetic
    from mocodad_amd.data.windows import TrajectoryWindows
    from mocodad_amd.engine import forecast_fan
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    from mocodad_amd.utils.eval_utils import forecast_fan_rows
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(noise_steps=4, n_generated_samples=2, exp_dir=str(tmp_path / "exp"), aggregation_strategy="mean")      # selects no pose
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    common = ("--synthetic", "2", "--random-init", "--device-windows", "--frames-per-clip", "30")
    stdout, z = _run_driver(str(p), tmp_path / "f.npz", *common, "--forecast-transforms", "all")
    plain, _ = _run_driver(str(p), None, *common)
    assert _auc(stdout) == _auc(plain), "the AUC line is the same with and without the flag"
    assert "_norm outputs only" in stdout
    _fan_checks(z, (0.1, 0.5, 0.9), 2, 15, pixels=False)
    assert set(np.unique(z["count"])) == {0, 5, 10, 15}
    args = load_config(str(p))
    trajs, _ = synthetic.make_trajectories(n_clips=2, frames_per_clip=30, seed=args.seed)
    tw = TrajectoryWindows(trajs, args.seg_len, args.num_transform).to(DEV)
    torch.manual_seed(int(args.seed))
    m = MoCoDAD(args).to(DEV)
    with torch.no_grad():
        out = m.forward(tw.batch(0, len(tw)), return_samples=True, window_offset=0)
    got = forecast_fan_rows(out[-2], tw.trans.numpy(), out[-1].cpu().numpy(), forecast_fan, windows=tw, max_cover=15, transforms="all",
                            num_transform=args.num_transform)
    assert np.array_equal(FR.bits(z["bands_norm"]), FR.bits(got[0].cpu().numpy())) and np.array_equal(z["count"], got[4].cpu().numpy())
    assert np.array_equal(FR.bits(z["mean_norm"]), FR.bits(got[1].cpu().numpy())) and np.array_equal(FR.bits(z["std_norm"]), FR.bits(got[2].cpu().numpy()))


def test_driver_on_host_windows(tmp_path):
    """--synthetic without --device-windows: no TrajectoryWindows -- the rows are the distinct (scene, clip, person, frame id) of the
    transform-0 windows, the observed rows are scattered on the host from the windows themselves and reach the kernel as a host
    tensor; the npz is that of the other sources, equal to forecast_fan_rows over one offline call on the same windows."""
    from mocodad_amd.data import synthetic
    from mocodad_amd.engine import forecast_fan
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    from mocodad_amd.utils.eval_utils import forecast_fan_rows, forecast_observed_rows
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(noise_steps=4, n_generated_samples=2, exp_dir=str(tmp_path / "exp"))
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    stdout, z = _run_driver(str(p), tmp_path / "f.npz", "--synthetic", "2", "--random-init", "--frames-per-clip", "30")
    assert "_norm outputs only" in stdout
    _fan_checks(z, (0.1, 0.5, 0.9), 2, 3, pixels=False)
    args = load_config(str(p))
    data, trans, meta, frames, _ = synthetic.make_dataset(n_clips=2, frames_per_clip=30, seg_len=args.seg_len, num_transform=args.num_transform,
                                                          seed=args.seed)
    torch.manual_seed(int(args.seed))
    m = MoCoDAD(args).to(DEV)
    with torch.no_grad():
        out = m.forward([data, trans, meta, frames], return_samples=True, window_offset=0)
    src = dict(meta=meta.numpy(), frames=frames.numpy(), data=data)
    got = forecast_fan_rows(out[-2], trans.numpy(), out[-1].cpu().numpy(), forecast_fan, max_cover=3, **src)
    for key, g in zip(("bands_norm", "mean_norm", "std_norm", "rank"), got[:4]):
        assert np.array_equal(FR.bits(z[key]), FR.bits(g.cpu().numpy())), key
    assert np.array_equal(z["count"], got[4].cpu().numpy()) and np.array_equal(z["rows"], got[5]) and np.array_equal(z["frames"], got[6])
    obs = forecast_observed_rows(trans.numpy(), **src)
    assert obs.device.type == "cpu" and np.array_equal(z["observed_norm"], obs.transpose(1, 2).reshape(-1, 34).numpy())
    # every observed row is the frame of a transform-0 window that covers it
    i = int(np.flatnonzero(trans.numpy() == 0)[3])
    r = int(np.flatnonzero((z["rows"] == meta[i, :3].numpy()).all(1) & (z["frames"] == int(frames[i, 2])))[0])
    assert np.array_equal(z["observed_norm"][r], data[i, :, 2].T.reshape(34).numpy())

"""GPU: forecasts from every test-time transform on the dataset path -- mcd_forecast_assemble_view (engine.forecast_assemble with
trans= and inv_affine=) against the float64 restatement of tests/forecast_tta_ref.py BIT FOR BIT (NaN payloads aside), against
mcd_forecast_assemble where the two must coincide, and eval_utils.forecast_track_rows(transforms='all') on the dataset fixture with
a random-init pose model.

Shapes: 5 transforms x 7 windows x 3 forecast frames piled onto 8 cells (105 pairs, one partial workgroup of the claim launch);
Tx = 12 with 60 pairs on one cell, and 61 on a list of 60 (the NaN rule) and of 64; 600 windows onto 8 cells of 58 .. 65 pairs (8 claim
workgroups; a full list of 64 and one past it)."""
import numpy as np
import pytest
import torch

import forecast_ref as FR
import forecast_tta_ref as TR
from mocodad_amd.utils.transforms import affine_table, inverse_affine_rows, inverse_affine_table
from test_forecast_tracks_gpu import DEV, _same

pytestmark = pytest.mark.gpu
# rows with rotation, flip, shear and translation (the shipped transforms have no translation: the general form is exercised here)
AFFINE = [[1, 0, 0, 0, 1, 0], [-1, 0, 0.25, 0, 1, -0.5], [0.6, -0.8, 0.1, 0.8, 0.6, 0.2], [1.25, 0.5, -0.75, -0.25, 0.8, 2.0],
          [0.7071067690849304, -0.7071067690849304, 0.0, 0.7071067690849304, 0.7071067690849304, 0.0]]


def _view(poses, cell, trans, inv, n_cells, **kw):
    from mocodad_amd.engine import forecast_assemble
    t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return tuple(o.cpu().numpy() for o in forecast_assemble(t(poses), t(cell), n_cells, device=DEV, trans=t(trans), inv_affine=t(inv), **kw))


def _plain(poses, cell, n_cells, **kw):
    from mocodad_amd.engine import forecast_assemble
    return tuple(o.cpu().numpy() for o in forecast_assemble(torch.from_numpy(poses), torch.from_numpy(cell), n_cells, device=DEV, **kw))


def test_five_transforms_of_seven_windows_on_eight_cells():
    """transform-major windows as the dataset orders them, every cell covered by several transforms; two windows carry a transform
    outside the table (-1 and 5) and are ignored; all three methods with both spreads"""
    rng = np.random.default_rng(1)
    inv = TR.inverse_table(AFFINE)
    assert np.array_equal(inv, inverse_affine_rows(AFFINE).numpy())
    poses = (rng.normal(size=(35, 2, 3, 17)) * rng.choice([0.01, 1.0, 5.0], size=(35, 1, 1, 1))).astype(np.float32)
    trans = np.repeat(np.arange(5), 7).astype(np.int32)
    cell = np.tile(np.arange(7)[:, None] + np.arange(3)[None], (5, 1)).astype(np.int32)      # window w forecasts rows w .. w + 2 (9 rows)
    cell[cell >= 8] = 9                                                                        # ... the ninth is outside the output
    trans[[5, 20]] = [-1, 5]
    for method in FR.METHODS:
        for sm in FR.SPREADS:
            got = _view(poses, cell, trans, inv, 8, method=method, spread_method=sm, max_cover=64)
            want = TR.assemble(poses, cell, trans, inv, 8, method, sm, 64)
            _same(got, want, (method, sm))
    assert want[1].tolist() == [5, 10, 15, 15, 15, 14, 13, 8] and np.isfinite(want[0]).all()
    # the same call is mcd_forecast_assemble fed the restatement's mapped poses (the ignored windows' cells set to -1)
    mapped = TR.map_back(poses, np.clip(trans, 0, 4), inv)
    c2 = cell.copy()
    c2[[5, 20]] = -1
    _same(_view(poses, cell, trans, inv, 8, max_cover=32), _plain(mapped, c2, 8, max_cover=32), "plain on mapped poses")
    # and the map matters: without it the result differs
    assert not np.array_equal(_plain(poses, c2, 8)[0], got[0])


def test_sixty_pairs_on_a_cell_and_sixty_one():
    rng = np.random.default_rng(2)
    inv = inverse_affine_table(5).numpy()
    poses = rng.normal(size=(6, 2, 12, 17)).astype(np.float32)
    trans = np.array([0, 1, 2, 3, 4, 2], np.int32)
    cell = np.zeros((6, 12), np.int32)
    cell[5] = -1
    cell[5, 0] = 1                                                   # cell 1: one pair; cell 2: none
    for method, sm in (("median", "median"), ("mean", "mean"), ("unique", "mean")):
        got = _view(poses, cell, trans, inv, 3, method=method, spread_method=sm, max_cover=64)
        _same(got, TR.assemble(poses, cell, trans, inv, 3, method, sm, 64), (method, sm, 60))
        assert got[1].tolist() == [60, 1, 0] and np.isfinite(got[0]).all() and got[2][0] > 0 and got[2][1] == 0
    cell[5, 1] = 0                                                   # 61 pairs on a list of 60 (5 transforms x 12 frames): NaN and the
    got61 = _view(poses, cell, trans, inv, 3, method="median", spread_method="median", max_cover=60)      # true count, the neighbours untouched
    _same(got61, TR.assemble(poses, cell, trans, inv, 3, "median", "median", 60), 61)
    assert got61[1].tolist() == [61, 1, 0] and np.isnan(got61[0][0]).all() and np.isnan(got61[2][0])
    assert np.isfinite(got61[0][1]).all() and got61[2][1] == 0 and not got61[0][2].any()
    wide = _view(poses, cell, trans, inv, 3, method="median", spread_method="median", max_cover=64)       # a list of 64 holds them
    _same(wide, TR.assemble(poses, cell, trans, inv, 3, "median", "median", 64), "61 of 64")
    assert wide[1].tolist() == [61, 1, 0] and np.isfinite(wide[0]).all()


def test_a_nan_forecast_reaches_only_the_cells_it_covers():
    rng = np.random.default_rng(3)
    inv = TR.inverse_table(AFFINE)
    poses = rng.normal(size=(10, 2, 3, 17)).astype(np.float32)
    trans = np.repeat(np.arange(5), 2).astype(np.int32)
    cell = np.tile(np.array([[0, 1, 2], [1, 2, 3]], np.int32), (5, 1))
    poses[6, 1, 0, 4] = np.nan                                       # transform 3 (shear), window 0, frame 0 -> cell 0, joint 4: x and y
    poses[1, 0, 2, 9] = np.nan                                       # the identity, window 1, frame 2 -> cell 3, joint 9: x only
    got = _view(poses, cell, trans, inv, 4, method="mean", spread_method="mean", max_cover=64)
    _same(got, TR.assemble(poses, cell, trans, inv, 4, "mean", "mean", 64), "nan")
    nan = np.isnan(got[0])
    assert np.flatnonzero(nan[0]).tolist() == [8, 9] and np.flatnonzero(nan[3]).tolist() == [18]
    assert not nan[1].any() and not nan[2].any() and np.isnan(got[2][[0, 3]]).all() and np.isfinite(got[2][[1, 2]]).all()


def test_negative_zero_keeps_its_sign_under_the_identity_row():
    inv = TR.inverse_table(AFFINE)
    poses = np.full((2, 2, 1, 17), -0.0, np.float32)
    poses[:, 1, 0, 3] = np.nan                                       # a NaN y beside a -0.0 x: the identity copies both
    trans = np.array([0, 0], np.int32)
    cell = np.array([[0], [1]], np.int32)
    got = _view(poses, cell, trans, inv, 2, method="unique", spread_method="mean", max_cover=64)
    assert np.signbit(np.delete(got[0], 7, axis=1)).all() and np.isnan(got[0][:, 7]).all() and np.signbit(got[0][:, 6]).all()
    _same(got, TR.assemble(poses, cell, trans, inv, 2, "unique", "mean", 64), "-0.0")
    _same(got, _plain(poses, cell, 2, method="unique", spread_method="mean"), "the existing entry on the same input")


def test_all_identity_equals_the_existing_entry():
    rng = np.random.default_rng(4)
    poses = rng.normal(size=(257, 2, 3, 17)).astype(np.float32)
    cell = rng.integers(-2, 60, size=(257, 3)).astype(np.int32)
    trans = np.zeros(257, np.int32)
    ident = inverse_affine_table(1).numpy()
    for method, sm in (("median", "mean"), ("mean", "median")):
        _same(_view(poses, cell, trans, ident, 58, method=method, spread_method=sm, max_cover=32),
              _plain(poses, cell, 58, method=method, spread_method=sm, max_cover=32), (method, sm))


def test_six_hundred_windows_twice():
    rng = np.random.default_rng(11)
    inv = TR.inverse_table(AFFINE)
    poses = rng.normal(size=(600, 2, 3, 17)).astype(np.float32)
    trans = np.repeat(np.arange(5), 120).astype(np.int32)
    cell = np.full(1800, -1, np.int32)
    picks = rng.permutation(1800)
    lo = 0
    for c in range(8):
        cell[picks[lo:lo + 58 + c]] = c
        lo += 58 + c
    cell = cell.reshape(600, 3)
    assert len({int(p) // 256 for p in picks[:58]}) > 4, "a cell's pairs come from several workgroups"
    tp, tc, tt, ti = (torch.from_numpy(a).to(DEV) for a in (poses, cell, trans, inv))
    a = _view(tp, tc, tt, ti, 8, method="median", spread_method="median", max_cover=64)
    b = _view(tp, tc, tt, ti, 8, method="median", spread_method="median", max_cover=64)
    assert a[1].tolist() == list(range(58, 66)) and np.isnan(a[0][7]).all() and np.isfinite(a[0][:7]).all()
    _same(a, b, "second run")
    _same(a, TR.assemble(poses, cell, trans, inv, 8, "median", "median", 64), "restatement")


def test_empty_calls_and_caller_buffers():
    from mocodad_amd.engine import forecast_assemble
    inv = inverse_affine_table(5)
    z = forecast_assemble(torch.zeros(0, 2, 3, 17), torch.zeros(0, 3, dtype=torch.int32), 4, device=DEV, trans=torch.zeros(0, dtype=torch.int32),
                          inv_affine=inv, max_cover=64)
    assert not z[0].any() and not z[1].any() and not z[2].any() and tuple(z[0].shape) == (4, 34)
    out = (torch.full((4, 34), 9.0, device=DEV), torch.full((4,), 9, device=DEV, dtype=torch.int32), torch.full((4,), 9.0, device=DEV))
    ws = torch.full((4 * 64,), -5, device=DEV, dtype=torch.int32)
    rng = np.random.default_rng(2)
    poses, cell = rng.normal(size=(5, 2, 3, 17)).astype(np.float32), rng.integers(0, 4, (5, 3)).astype(np.int32)
    trans = np.arange(5, dtype=np.int64)                                # (any integer type)
    res = forecast_assemble(torch.from_numpy(poses), torch.from_numpy(cell), 4, device=DEV, out=out, workspace=ws, max_cover=64,
                            trans=torch.from_numpy(trans), inv_affine=inv)
    assert all(x is y for x, y in zip(res, out))
    _same(tuple(t.cpu().numpy() for t in res), TR.assemble(poses, cell, trans, inv.numpy(), 4, max_cover=64), "caller buffers")


# ---------------------------------------------------------------- the dataset fixture
@pytest.fixture(scope="module")
def fixture_run(tmp_path_factory):
    """One scoring call of a random-init pose model over the fixture's test split (5 transforms) -> the selected forecasts."""
    from dataset_spec import load_dataset_golden
    from test_stream_forecast_gpu import Offline
    from test_stream_gpu import _model
    g = load_dataset_golden()
    m, args = _model(tmp_path_factory.mktemp("forecast_tta"), g)
    return m, Offline(m, args, g)


def _rows(off, m, assemble, **kw):
    from mocodad_amd.utils.eval_utils import forecast_track_rows
    tw = off.tw
    mf = m.map_frames(None, len(tw)).cpu().numpy()
    return forecast_track_rows(off.pose_agg, tw.trans.numpy(), mf, assemble, windows=tw, **kw)


def test_forecast_track_rows_all_on_the_dataset_fixture(fixture_run):
    from mocodad_amd.engine import forecast_assemble
    m, off = fixture_run
    tw, NT = off.tw, 5
    seen = {}

    def ref(p, c, n, trans=None, inv_affine=None, **kw):
        seen["trans"], seen["inv"] = trans.numpy(), inv_affine.numpy()
        return TR.assemble(p.cpu().numpy(), c.numpy(), trans.numpy(), inv_affine.numpy(), n, **kw)

    for method, sm in (("median", "mean"), ("mean", "median"), ("unique", "mean")):
        got = _rows(off, m, forecast_assemble, method=method, spread_method=sm, transforms="all", max_cover=15)
        want = _rows(off, m, ref, method=method, spread_method=sm, transforms="all", max_cover=15)
        _same(tuple(t.cpu().numpy() for t in got[:3]), want[:3], (method, sm))
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert np.array_equal(seen["inv"], TR.inverse_table(affine_table(NT).numpy())) and np.array_equal(seen["trans"], tw.trans.numpy())
    # every row's count is the sum of what each transform alone gives (each one: the windows of that transform, nothing else)
    count = got[1].cpu().numpy()
    alone = []
    for t in range(NT):
        tr = np.where(tw.trans.numpy() == t, t, -1)
        mf = m.map_frames(None, len(tw)).cpu().numpy()
        from mocodad_amd.utils.eval_utils import forecast_cells_aligned
        cell = torch.from_numpy(forecast_cells_aligned(tw.base.numpy(), mf, tr, transforms="all"))
        alone.append(forecast_assemble(off.pose_agg, cell, len(count), trans=torch.from_numpy(tr.astype(np.int32)),
                                       inv_affine=inverse_affine_table(NT), max_cover=15)[1].cpu().numpy())
    assert np.array_equal(count, np.sum(alone, axis=0)) and all(np.array_equal(a, alone[0]) for a in alone)
    assert count.max() == 15 and set(np.unique(count)) == {0, 5, 10, 15}
    # 'identity' is the call without the keyword, and its counts are one transform's
    ident = _rows(off, m, forecast_assemble, transforms="identity")
    plain = _rows(off, m, forecast_assemble)
    _same(tuple(t.cpu().numpy() for t in ident[:3]), tuple(t.cpu().numpy() for t in plain[:3]), "identity")
    assert np.array_equal(plain[1].cpu().numpy(), alone[0]) and np.array_equal(ident[3], plain[3]) and np.array_equal(ident[4], plain[4])
    assert np.array_equal(got[3], plain[3]) and np.array_equal(got[4], plain[4])            # the same rows, in the same order
    assert np.isfinite(got[0].cpu().numpy()).all() and not np.array_equal(got[0].cpu().numpy(), plain[0].cpu().numpy())


def test_forecast_track_rows_all_by_meta_and_frames(fixture_run):
    """The other source of the rows (meta / frames instead of a TrajectoryWindows): the same cells up to the numbering of the rows."""
    from mocodad_amd.engine import forecast_assemble
    from mocodad_amd.utils.eval_utils import forecast_track_rows
    m, off = fixture_run
    tw = off.tw
    mf = m.map_frames(None, len(tw)).cpu().numpy()
    a = _rows(off, m, forecast_assemble, transforms="all", max_cover=15)
    b = forecast_track_rows(off.pose_agg, tw.trans.numpy(), mf, forecast_assemble, meta=tw.meta.numpy(), frames=tw.frames.numpy(),
                            transforms="all", max_cover=15)
    key_a = {(tuple(int(v) for v in k), int(f)): i for i, (k, f) in enumerate(zip(a[3], a[4]))}
    pa, ca, sa = (t.cpu().numpy() for t in a[:3])
    pb, cb, sb = (t.cpu().numpy() for t in b[:3])
    assert len(b[3]) > 100
    for i, (k, f) in enumerate(zip(b[3], b[4])):
        j = key_a[(tuple(int(v) for v in k), int(f))]
        assert cb[i] == ca[j] and np.array_equal(FR.bits(pb[i]), FR.bits(pa[j])) and np.array_equal(FR.bits(sb[i]), FR.bits(sa[j]))


# ---------------------------------------------------------------- the driver
def test_driver_with_every_transform(tmp_path):
    """eval_MoCoDAD.py --forecast-tracks --forecast-transforms all on synthetic clips: the output of the option's default with
    five times the counts (a row is forecast by 0 .. 3 windows of each of the 5 transforms), and other poses."""
    import os
    import yaml
    from dataset_spec import ROOT
    from test_forecast_tracks_gpu import _run_driver, _track_checks
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(noise_steps=4, n_generated_samples=2, exp_dir=str(tmp_path / "exp"))
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    common = ("--synthetic", "2", "--random-init", "--device-windows", "--frames-per-clip", "30")
    _, one = _run_driver(str(p), tmp_path / "one.npz", *common)
    _, every = _run_driver(str(p), tmp_path / "all.npz", *common, "--forecast-transforms", "all")
    _track_checks(one, 3, 3)                     # the leading n_cond rows of a track have no forecast, the next one has one ...
    _track_checks(every, 3, 3, max_cover=15)     # ... and under 'all' five (the counts below): the shape checks, counts up to 15
    assert sorted(every.files) == sorted(one.files) and np.array_equal(every["rows"], one["rows"]) and np.array_equal(every["frames"], one["frames"])
    assert np.array_equal(every["count"], 5 * one["count"]) and every["count"].max() == 15
    assert not np.array_equal(every["expected_norm"], one["expected_norm"])

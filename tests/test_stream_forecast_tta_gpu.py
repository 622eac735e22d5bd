"""GPU: the expected pose of every row of a live stream from the windows of EVERY transform (PoseStream(forecasts=ForecastCfg(...,
transforms='all')): mcd_stream_forecast_group_tta / mcd_stream_forecast_flush_tta on the forecast ring with a transform axis) against
the dataset path on the same rows -- ONE scoring call over the split, eval_utils.forecast_track_rows(transforms='all') with
engine.forecast_assemble (mcd_forecast_assemble_view), engine.denormalize_poses -- with the same given noise, window by window.
Every comparison is exact.  The helpers are those of tests/test_stream_forecast_gpu.py and tests/test_stream_latent_pose_gpu.py; the
NumPy model of the ring is tests/forecast_tta_ref.py."""
import numpy as np
import pytest
import torch

import forecast_tta_ref as TR
from dataset_spec import load_dataset_golden, stress_rows
from mocodad_amd.engine import denormalize_poses, forecast_assemble
from mocodad_amd.stream import ForecastCfg, PoseStream, forecast_cover, ticks_by_frame
from mocodad_amd.utils.eval_utils import forecast_track_rows
from mocodad_amd.utils.transforms import affine_table, inverse_affine_table
from test_stream_forecast_gpu import (FIELDS, N_COND, Offline, _check_against_offline, _model_with, _np, _same_rows, _same_tick,
                                      _stream_rows, off_tracks)
from test_stream_gpu import DEV, NT, SEG_LEN, VID_RES, _bits, _model, _replay

pytestmark = pytest.mark.gpu
CFGS = [("unique", "mean"), ("mean", "median"), ("median", "mean")]


def rows_all(off, method, spread):
    """Offline.rows with the windows of every transform: {(key, frame id): (expected, expected_norm, count, spread)}."""
    tw, g = off.tw, off.g
    mf = off.m.map_frames(None, len(tw)).cpu().numpy()
    pose, count, spr, keys, fids = forecast_track_rows(off.pose_agg, tw.trans.numpy(), mf, forecast_assemble, windows=tw, method=method,
                                                       spread_method=spread, transforms="all", max_cover=NT * off.pose_agg.shape[2])
    expected = denormalize_poses(pose, tw.raw.poses, VID_RES, g["train_center"], g["train_scale"], count=count)
    pose, count, spr, expected = (t.cpu().numpy() for t in (pose, count, spr, expected))
    return {(tuple(int(v) for v in k), int(f)): (expected[i], pose[i], count[i], spr[i]) for i, (k, f) in enumerate(zip(keys, fids))}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    g = load_dataset_golden()
    m, args = _model(tmp_path_factory.mktemp("stream_forecast_tta"), g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
    return dict(g=g, model=m, args=args, kw=kw, offline=Offline(m, args, g))


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, spread", CFGS)
def test_fixture_replay_equals_the_dataset_path_bit_for_bit(setup, method, spread):
    """ring_len = seg_len: every ring wraps.  Every kept row exactly once (finals and tails: _stream_rows), expected_norm, count and
    spread those of forecast_track_rows(transforms='all'), expected = engine.denormalize_poses of it (rows_all)."""
    m, off = setup["model"], setup["offline"]
    got, ticks = _stream_rows(m, off, setup["kw"], ForecastCfg(method, spread, "all"))
    counts = _check_against_offline(got, rows_all(off, method, spread), off_tracks())
    assert counts == {0, NT, 2 * NT, 3 * NT}
    assert len(np.unique(np.stack([v[1] for v in got.values()]))) > 1000 and len(np.unique(np.stack([v[4] for v in got.values()]))) > 100
    if method == "median":       # ... and it is not the forecast of transform 0 alone
        ident = off.rows(method, spread)
        assert any(not np.array_equal(_bits(got[k][1]), _bits(ident[k][1])) for k in got)


def test_the_state_that_is_allocated(setup):
    st = PoseStream(setup["model"], forecasts=ForecastCfg(transforms="all"), **setup["kw"])
    r = st.rings
    assert tuple(r.forecast_tta_ring.shape) == (18, SEG_LEN, NT, 3, 34) and tuple(r.observed_ring.shape) == (18, SEG_LEN, 34)
    assert r.forecast_ring is None and r._fstate is None and r._tstate is not None
    assert np.array_equal(r.inv_affine.cpu().numpy(), TR.inverse_table(affine_table(NT).numpy())) and r.inv_affine.dtype == torch.float64


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_push_many_of_three_ticks_equals_push(setup):
    m, tracks = setup["model"], off_tracks()
    kw = dict(setup["kw"], max_tracks=32, ring_len=SEG_LEN + 2, forecasts=ForecastCfg("mean", "median", "all"), max_idle=3)
    a, b = PoseStream(m, **kw), PoseStream(m, **kw)
    feed = [(keys, fids, poses) for _, keys, fids, poses in ticks_by_frame(tracks)]
    ta = [a.push(*t) for t in feed]
    tb = []
    for i in range(0, len(feed), 3):
        tb += b.push_many(feed[i:i + 3])
    assert len(ta) == len(tb) == len(feed)
    for x, y in zip(ta, tb):
        _same_tick(x, y)
        assert x.forecast is x.final.forecast and len(x.forecast) == len(x.final)
    assert sum(len(t.closed) for t in ta) > 0 and sum(len(t.final) for t in ta) > 100
    assert sum(int((t.closed.forecast.count > 0).sum()) for t in ta) > 0
    assert max(int(t.forecast.count.max()) for t in ta if len(t.forecast)) == 3 * NT
    ca, cb = a.close_all(), b.close_all()
    assert ca.keys == cb.keys and torch.equal(ca.values, cb.values) and len(ca) > 0
    _same_rows(ca.forecast, cb.forecast)
    assert torch.equal(a.rings.forecast_tta_ring, b.rings.forecast_tta_ring) and torch.equal(a.rings.observed_ring, b.rings.observed_ring)
    assert torch.equal(a.rings.frame_scores_ring, b.rings.frame_scores_ring) and torch.equal(a.ring, b.ring)
    assert bool((a.rings.forecast_tta_ring != 0).any(-1).any(-1).all(-1).any()), "some row holds a cell of every transform"


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_a_reused_slot_starts_clean(setup):
    """One slot, max_idle = 1, ring_len = seg_len + 1: track A wraps the ring, goes idle and is closed; track B takes the slot over.
    B's forecasts are those of a fresh stream that only ever saw B -- no cell of A, of any transform, is read."""
    m = setup["model"]
    kw = dict(setup["kw"], max_tracks=1, max_idle=1, ring_len=SEG_LEN + 1, forecasts=ForecastCfg(transforms="all"))
    S, ns = m.n_generated_samples, m.noise_steps
    raw = stress_rows(3 * SEG_LEN + 6, seed=21)
    gen = torch.Generator().manual_seed(5)
    used, fresh = PoseStream(m, **kw), PoseStream(m, **kw)
    A, Bk = (1, 1, 1), (1, 1, 2)
    for i in range(SEG_LEN + 3):
        nz = torch.randn(S, ns - 1, NT, 2, 3, 17, generator=gen).to(DEV) if i >= SEG_LEN - 1 else None
        used.push([A], [i + 1], raw[i:i + 1], noise=nz)
    assert bool((used.rings.forecast_tta_ring != 0).any())
    used.push([], [], np.zeros((0, 34), np.float32))
    rows_b = raw[SEG_LEN + 3:]
    ticks = []
    for i in range(len(rows_b)):
        nz = torch.randn(S, ns - 1, NT, 2, 3, 17, generator=gen).to(DEV) if i >= SEG_LEN - 1 else None
        tu = used.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        tf = fresh.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        if i == 0:
            assert tu.closed.keys == [A] * (SEG_LEN - 1) and tu.closed.forecast.count.tolist() == [2 * NT, 3 * NT, 3 * NT, 2 * NT, NT]
            assert np.array_equal(_bits(tu.closed.forecast.observed.cpu().numpy()), _bits(raw[4:SEG_LEN + 3]))
        else:
            assert len(tu.closed) == 0
        assert torch.equal(tu.scores, tf.scores) and torch.equal(tu.final.values, tf.final.values)
        _same_rows(tu.forecast, tf.forecast, i)
        ticks.append(tu)
    counts = torch.cat([t.forecast.count for t in ticks]).tolist()
    assert counts[:6] == [0, 0, 0, NT, 2 * NT, 3 * NT] and len(counts) == len(rows_b) - SEG_LEN + 1
    cu, cf = used.close([Bk]), fresh.close([Bk])
    _same_rows(cu.forecast, cf.forecast)
    assert torch.equal(cu.values, cf.values) and cu.forecast.count.tolist() == [3 * NT, 3 * NT, 3 * NT, 2 * NT, NT]


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_in_between_corrupt_frames_on_a_longer_ring(tmp_path):
    """Frames 2 and 3 of 6 are forecast; two synthetic tracks of 2 seg_len + 1 and seg_len rows on ring_len = seg_len + 2.  Against
    the NumPy model of the ring fed with every tick's selected forecasts of every transform, and against
    engine.forecast_assemble(trans=, inv_affine=) over each track's windows in transform-major order."""
    g = load_dataset_golden()
    m, _ = _model_with(tmp_path, g, conditioning_strategy="inbetween_imp", conditioning_indices=[0, 1, 4, 5])
    sc = m.scorer()
    cidx, Tt, L = [2, 3], SEG_LEN, SEG_LEN + 2
    assert sc.corrupt_idx == cidx
    S, ns = m.n_generated_samples, m.noise_steps
    lens = {(1, 1, 1): 2 * Tt + 1, (1, 1, 2): Tt}
    raws = {k: stress_rows(n, seed=31 + k[2]) for k, n in lens.items()}
    cs = dict(center=g["train_center"], scale=g["train_scale"])
    inv = inverse_affine_table(NT)
    st = PoseStream(m, vid_res=VID_RES, max_tracks=2, ring_len=L, forecasts=ForecastCfg("median", "median", "all"), **cs)
    model = TR.TtaRingModel(2, L, Tt, cidx, inv.numpy(), "median", "median", VID_RES, cs["center"].astype(np.float64),
                            cs["scale"].astype(np.float64))
    gen = torch.Generator().manual_seed(9)
    got, ref, agg_of = {}, {}, {k: {} for k in lens}

    def take(fs, into):
        f = _np(fs.forecast)
        for i, (k, fid) in enumerate(zip(fs.keys, fs.frames)):
            assert (k, int(fid)) not in into
            into[(k, int(fid))] = tuple(f[name][i] for name in FIELDS)

    for r in range(max(lens.values())):
        keys = [k for k, n in lens.items() if r < n]
        ne = sum(r >= Tt - 1 for _ in keys)
        nz = torch.randn(S, ns - 1, NT * ne, 2, 2, 17, generator=gen).to(DEV) if ne else None
        tick = st.push(keys, [r + 1] * len(keys), np.stack([raws[k][r] for k in keys]), noise=nz)
        for k in keys:
            model.store_row(st.table.slot_of[k], r, raws[k][r])
        if ne:      # the same windows, still in the ring, scored again with the same noise: the selected forecasts of the tick
            _, la, pa = sc.score_fused(tick.windows, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy, noise=nz,
                                       loss_fn=m.loss_name, want_all=True, want_poses=True)
            pose_agg = sc.aggregate(None, la, pa, m.aggregation_strategy, noise_steps=ns, loss_fn=m.loss_name)[0].cpu().numpy()
            for j, k in enumerate(tick.final.keys):              # (transform-major: window j of transform t is entry t * ne + j)
                agg_of[k][r] = np.stack([pose_agg[t * ne + j] for t in range(NT)])
                for t in range(NT):
                    model.store_window(st.table.slot_of[k], r, t, pose_agg[t * ne + j])
            for j, k in enumerate(tick.final.keys):
                ref[(k, r - Tt + 2)] = model.final(st.table.slot_of[k], r)
        take(tick.final, got)
        done = [k for k in keys if r == lens[k] - 1]
        if done:
            for k in done:
                for i, res in enumerate(model.flush(st.table.slot_of[k], r)):
                    ref[(k, r - Tt + 3 + i)] = res
            take(st.close(done), got)
    assert sorted(got) == sorted(ref) and len(got) == sum(lens.values())
    for key in got:
        _same_rows(dict(zip(FIELDS, got[key])), dict(zip(FIELDS, ref[key])), key)
    counts = set()
    for k, n in lens.items():
        ends = sorted(agg_of[k])
        assert ends == list(range(Tt - 1, n))
        poses = torch.from_numpy(np.stack([agg_of[k][e] for e in ends]).transpose(1, 0, 2, 3, 4).reshape(NT * len(ends), 2, 2, 17).copy())
        cell = torch.tensor([[e - Tt + 1 + c for c in cidx] for e in ends] * NT, dtype=torch.int32)
        trans = torch.arange(NT, dtype=torch.int32).repeat_interleave(len(ends))
        pose, count, spr = forecast_assemble(poses, cell, n, method="median", spread_method="median", device=DEV, trans=trans,
                                             inv_affine=inv, max_cover=NT * 2)
        exp = denormalize_poses(pose, raws[k], VID_RES, cs["center"], cs["scale"], count=count).cpu().numpy()
        pose, count, spr = pose.cpu().numpy(), count.cpu().numpy(), spr.cpu().numpy()
        for r in range(n):
            e, nrm, obs, cnt, s = got[(k, r + 1)]
            assert cnt == count[r] == NT * len(forecast_cover(cidx, Tt, r, n - 1)), (k, r)
            assert np.array_equal(_bits(nrm), _bits(pose[r])) and np.array_equal(_bits(s), _bits(spr[r])), (k, r)
            assert np.array_equal(_bits(e), _bits(exp[r])) and np.array_equal(_bits(obs), _bits(raws[k][r])), (k, r)
            counts.add(int(cnt))
    assert counts == {0, NT, 2 * NT}


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_aggregation_worst(tmp_path):
    g = load_dataset_golden()
    m, args = _model_with(tmp_path, g, aggregation_strategy="worst")
    assert m.aggregation_strategy == "worst"
    off = Offline(m, args, g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
    got, _ = _stream_rows(m, off, kw, ForecastCfg("median", "mean", "all"))
    assert _check_against_offline(got, rows_all(off, "median", "mean"), off_tracks()) == {0, NT, 2 * NT, 3 * NT}


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_latent_module_in_pose_space(tmp_path):
    import test_stream_latent_pose_gpu as LP
    g = load_dataset_golden()
    m, args = LP.pose_model(tmp_path, g)
    try:
        off = LP.Offline(m, args, g)
        tracks = LP._tracks()
        kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
        ticks, tails, _ = LP.replay(m, off, tracks, kw, forecasts=ForecastCfg("median", "mean", "all"))
        got = LP._forecast_rows(ticks, tails)
        assert LP.NT == NT
        counts = _check_against_offline(got, rows_all(off, "median", "mean"), tracks)
        assert counts == {0, NT, 2 * NT, 3 * NT}
    finally:
        m._decoder_sd = m._decoder = None


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_identity_is_todays_stream(setup):
    """ForecastCfg(transforms='identity') against ForecastCfg() as it was: every field of every tick and tail, every ring; the new
    state is not allocated."""
    m, tracks = setup["model"], off_tracks()
    old = PoseStream(m, ring_len=SEG_LEN, forecasts=ForecastCfg("median", "mean"), **setup["kw"])
    new = PoseStream(m, ring_len=SEG_LEN, forecasts=ForecastCfg("median", "mean", transforms="identity"), **setup["kw"])
    for st in (old, new):
        assert st.rings.forecast_tta_ring is None and st.rings._tstate is None and st.rings.inv_affine is None
        assert tuple(st.rings.forecast_ring.shape) == (18, SEG_LEN, 3, 34)

    def both(keys, fids, poses, metas):
        to, tn = old.push(keys, fids, poses), new.push(keys, fids, poses)
        _same_tick(to, tn)
        return to

    ticks, _ = _replay([old, new], tracks, both)
    assert sum(len(t.final) for t in ticks) == 283 and max(int(t.forecast.count.max()) for t in ticks if len(t.forecast)) == 3
    assert torch.equal(old.rings.forecast_ring, new.rings.forecast_ring) and torch.equal(old.rings.observed_ring, new.rings.observed_ring)
    assert torch.equal(old.ring, new.ring) and torch.equal(old.rings.frame_scores_ring, new.rings.frame_scores_ring)


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals(setup):
    m = setup["model"]
    with pytest.raises(ValueError, match="transforms must be one of"):
        PoseStream(m, forecasts=ForecastCfg(transforms="every"), **setup["kw"])
    with pytest.raises(ValueError, match="22 \\* 3"):
        PoseStream(m, forecasts=ForecastCfg(transforms="all"), num_transform=22, **setup["kw"])
    from mocodad_amd.engine import StreamRings
    with pytest.raises(ValueError, match="exceeds 64"):
        StreamRings(2, SEG_LEN, SEG_LEN, 22, VID_RES, forecasts=("median", "mean", 3, "all"))
    with pytest.raises(ValueError, match="'identity' or 'all'"):
        StreamRings(2, SEG_LEN, SEG_LEN, NT, VID_RES, forecasts=("median", "mean", 3, "both"))

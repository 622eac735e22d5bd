"""GPU: the expected pose of every row of a live stream (PoseStream(forecasts=ForecastCfg(...)): mcd_stream_forecast_group /
mcd_stream_forecast_flush on the forecast and observed rings) against the dataset path on the same rows -- ONE scoring call over
the split, mcd_aggregate's pose_agg, eval_utils.forecast_track_rows with engine.forecast_assemble, engine.denormalize_poses -- with
the same given noise, window by window.  Every comparison is exact (`_bits`): a compared value is a copy or the output of an
order-fixed float64 reduction on the bits of a scoring launch whose result does not depend on the batch it ran in.  The helpers
(model, tracks, replay) are those of tests/test_stream_gpu.py; the NumPy model of the ring is tests/stream_forecast_ref.py."""
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from dataset_spec import DATASET, ROOT, load_dataset_golden, stress_rows
from mocodad_amd.data import trajectories as T
from mocodad_amd.data.windows import WindowBatch
from mocodad_amd.engine import denormalize_poses, forecast_assemble
from mocodad_amd.stream import ForecastCfg, PoseStream, forecast_cover, ticks_by_frame
from mocodad_amd.utils.eval_utils import forecast_track_rows
from stream_forecast_ref import RingModel
from test_stream_gpu import DEV, NT, SEG_LEN, VID_RES, _bits, _model, _replay, _tracks

pytestmark = pytest.mark.gpu
N_COND = 3           # the fixture's model: frames 0 .. 2 condition, 3 .. 5 are forecast
FIELDS = ("expected", "expected_norm", "observed", "count", "spread")
CFGS = [("unique", "mean"), ("mean", "median"), ("median", "mean")]


def _model_with(tmp, g, **over):
    """test_stream_gpu._model with other settings (that helper takes none): the same seeds, the scaler next to it."""
    from sklearn.preprocessing import RobustScaler
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(data_dir=DATASET, test_path=os.path.join(DATASET, "testing", "test_frame_mask"), exp_dir=str(tmp / "exp"),
               dataset_choice="HR-STC", dir_name="fixture", noise_steps=4, n_generated_samples=2, batch_size=256,
               seg_len=SEG_LEN, vid_res=list(VID_RES), num_transform=NT, seed=11)
    cfg.update(over)
    p = tmp / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    args = load_config(str(p))
    sc = RobustScaler(quantile_range=(10.0, 90.0))
    sc.center_, sc.scale_ = g["train_center"], g["train_scale"]
    os.makedirs(args.ckpt_dir, exist_ok=True)
    with open(os.path.join(args.ckpt_dir, "local_robust.pickle"), "wb") as f:
        pickle.dump(sc, f)
    torch.manual_seed(123)
    m = MoCoDAD(args).to(DEV)
    m.save_tensors = False
    return m, args


def _np(fr):
    return {k: getattr(fr, k).cpu().numpy() for k in FIELDS}


def _same_rows(a, b, what=""):
    """Two ForecastRows (or dicts of the five fields, arrays or scalars): the same bits."""
    for k in FIELDS:
        x, y = (a[k], b[k]) if isinstance(a, dict) else (getattr(a, k), getattr(b, k))
        x, y = (np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v) for v in (x, y))
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(x, y) if k == "count" else np.array_equal(_bits(x), _bits(y)), (what, k)


class Offline:
    """The dataset path on the fixture's test split for one model: ONE scoring call with a given noise tensor -> the selected
    forecast of every window; `rows(method, spread)` -> {(key, frame id): (expected, expected_norm, count, spread)}."""

    def __init__(self, m, args, g, nan_sample=None):
        self.m, self.g = m, g
        sc = m.scorer()
        self.tw = tw = T.load_dataset(args, DEV)[0]
        self.n = n = tw.n_samples
        S, ns, Tx = m.n_generated_samples, m.noise_steps, m.n_frames_corrupt
        self.noise = torch.randn(S, ns - 1, NT * n, 2, Tx, 17, generator=torch.Generator().manual_seed(7)).to(DEV)
        if nan_sample is not None:
            self.noise[:, :, nan_sample] = float("nan")          # (the transform-0 instance of that window)
        wb = WindowBatch(tw.buffer, tw.base.to(DEV), tw.trans.to(DEV), tw.affine, SEG_LEN)
        self.scores, loss_all, poses_all = sc.score_fused(wb, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy,
                                                          noise=self.noise, loss_fn=m.loss_name, want_all=True, want_poses=True)
        self.pose_agg = sc.aggregate(None, loss_all, poses_all, m.aggregation_strategy, noise_steps=ns, loss_fn=m.loss_name)[0]
        assert tuple(self.pose_agg.shape) == (NT * n, 2, Tx, 17)
        self.sample_of = {tuple(int(v) for v in r): i for i, r in enumerate(tw.meta[:n].numpy())}

    def rows(self, method, spread):
        tw, g = self.tw, self.g
        mf = self.m.map_frames(None, len(tw)).cpu().numpy()
        pose, count, spr, keys, fids = forecast_track_rows(self.pose_agg, tw.trans.numpy(), mf, forecast_assemble, windows=tw,
                                                           method=method, spread_method=spread)
        expected = denormalize_poses(pose, tw.raw.poses, VID_RES, g["train_center"], g["train_scale"], count=count)
        pose, count, spr, expected = (t.cpu().numpy() for t in (pose, count, spr, expected))
        return {(tuple(int(v) for v in k), int(f)): (expected[i], pose[i], count[i], spr[i]) for i, (k, f) in enumerate(zip(keys, fids))}


def _stream_rows(m, off, kw, cfg, **more):
    """Replay the fixture through a PoseStream with forecasts on (off's noise, window by window) -> ({(key, frame id): the five
    fields of the row}, the ticks); every row comes exactly once, with a final or with a tail."""
    stream = PoseStream(m, ring_len=SEG_LEN, forecasts=cfg, **kw, **more)
    n = off.n

    def on_tick(keys, fids, poses, plan_meta):
        idx = torch.from_numpy(np.asarray([t * n + off.sample_of[mm] for t in range(NT) for mm in plan_meta], np.int64)).to(DEV)
        tick = stream.push(keys, fids, poses, noise=off.noise[:, :, idx] if len(idx) else None)
        assert np.array_equal(_bits(tick.scores.cpu().numpy()), _bits(off.scores[idx].cpu().numpy()))
        return tick

    ticks, tails = _replay([stream], off_tracks(), on_tick)
    got = {}

    def take(fs):
        assert fs.forecast is not None and len(fs.forecast) == len(fs)
        f = _np(fs.forecast)
        assert f["expected"].shape == f["expected_norm"].shape == f["observed"].shape == (len(fs), 34) and f["count"].dtype == np.int32
        for i, (k, fid) in enumerate(zip(fs.keys, fs.frames)):
            assert (k, int(fid)) not in got
            got[(k, int(fid))] = tuple(f[name][i] for name in FIELDS)
    for tick in ticks:
        assert tick.forecast is tick.final.forecast and len(tick.closed) == 0
        take(tick.final)
    for _, fs in tails:
        take(fs)
    return got, ticks


_TRACKS = []


def off_tracks():
    if not _TRACKS:
        _TRACKS.extend(_tracks())
    return _TRACKS


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    g = load_dataset_golden()
    m, args = _model(tmp_path_factory.mktemp("stream_forecast"), g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
    return dict(g=g, model=m, args=args, kw=kw, offline=Offline(m, args, g), cache={})


def _check_against_offline(got, want, tracks):
    kept = [(k, f, p) for k, f, p in tracks if len(f) >= SEG_LEN]
    assert len(got) == len(want) == sum(len(f) for _, f, _ in kept)
    counts, zeros = set(), 0
    for k, f, p in kept:
        for i, fid in enumerate(f):
            e, nrm, obs, cnt, spr = got[(k, int(fid))]
            we, wn, wc, ws = want[(k, int(fid))]
            assert cnt == wc and np.array_equal(_bits(nrm), _bits(wn)) and np.array_equal(_bits(spr), _bits(ws)), (k, fid)
            assert np.array_equal(_bits(e), _bits(we)), (k, fid)
            assert np.array_equal(_bits(obs), _bits(p[i])), (k, fid)                       # the CSV row
            if i < N_COND:              # no window forecasts the first n_cond rows of a track
                assert cnt == 0 and not e.any() and not nrm.any() and spr == 0
                zeros += 1
            counts.add(int(cnt))
    assert zeros == N_COND * len(kept)
    return counts


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, spread", CFGS)
def test_fixture_replay_equals_the_dataset_path_bit_for_bit(setup, method, spread):
    m, off = setup["model"], setup["offline"]
    got, _ = _stream_rows(m, off, setup["kw"], ForecastCfg(method, spread))
    setup["cache"][(method, spread)] = got
    want = off.rows(method, spread)
    counts = _check_against_offline(got, want, off_tracks())
    assert counts == {0, 1, 2, 3}
    norm = np.stack([v[1] for v in got.values()])
    assert len(np.unique(norm)) > 1000 and len(np.unique(np.stack([v[0] for v in got.values()]))) > 1000      # (not a constant)
    assert len(np.unique(np.stack([v[4] for v in got.values()]))) > 100


def test_forecast_cfg_defaults(setup):
    st = PoseStream(setup["model"], forecasts=ForecastCfg(), **setup["kw"])
    assert (st.forecasts.method, st.forecasts.spread) == ("median", "mean")
    assert tuple(st.rings.forecast_ring.shape) == (18, SEG_LEN, 3, 34) and tuple(st.rings.observed_ring.shape) == (18, SEG_LEN, 34)


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_in_between_corrupt_frames_on_a_longer_ring(tmp_path):
    """Frames 2 and 3 of 6 are forecast (inbetween_imp, conditioning_indices [0, 1, 4, 5]); two synthetic tracks of 2 seg_len + 1
    and seg_len rows on ring_len = seg_len + 2.  Against engine.forecast_assemble on scorer.aggregate's pose_agg of every tick's
    windows, and against the NumPy model of the ring fed with the same forecasts."""
    g = load_dataset_golden()
    m, _ = _model_with(tmp_path, g, conditioning_strategy="inbetween_imp", conditioning_indices=[0, 1, 4, 5])
    sc = m.scorer()
    cidx, Tt, L = [2, 3], SEG_LEN, SEG_LEN + 2
    assert sc.corrupt_idx == cidx
    S, ns = m.n_generated_samples, m.noise_steps
    lens = {(1, 1, 1): 2 * Tt + 1, (1, 1, 2): Tt}
    raws = {k: stress_rows(n, seed=31 + k[2]) for k, n in lens.items()}
    cs = dict(center=g["train_center"], scale=g["train_scale"])
    st = PoseStream(m, vid_res=VID_RES, max_tracks=2, ring_len=L, forecasts=ForecastCfg("median", "median"), **cs)
    model = RingModel(2, L, Tt, cidx, "median", "median", VID_RES, cs["center"].astype(np.float64), cs["scale"].astype(np.float64))
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
            for j, k in enumerate(tick.final.keys):              # (transform 0: the first n_emit windows of the tick)
                agg_of[k][r] = pose_agg[j]
                model.store_window(st.table.slot_of[k], r, pose_agg[j])
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
    for key in got:                                                  # the NumPy model of the ring
        _same_rows(dict(zip(FIELDS, got[key])), dict(zip(FIELDS, ref[key])), key)
    counts = set()
    for k, n in lens.items():                                        # the dataset path's assembly over the track's windows
        ends = sorted(agg_of[k])
        assert ends == list(range(Tt - 1, n))
        poses = torch.from_numpy(np.stack([agg_of[k][e] for e in ends]))
        cell = torch.tensor([[e - Tt + 1 + c for c in cidx] for e in ends], dtype=torch.int32)
        pose, count, spr = forecast_assemble(poses, cell, n, method="median", spread_method="median", device=DEV)
        exp = denormalize_poses(pose, raws[k], VID_RES, cs["center"], cs["scale"], count=count).cpu().numpy()
        pose, count, spr = pose.cpu().numpy(), count.cpu().numpy(), spr.cpu().numpy()
        for r in range(n):
            e, nrm, obs, cnt, s = got[(k, r + 1)]
            assert cnt == count[r] == len(forecast_cover(cidx, Tt, r, n - 1)), (k, r)
            assert np.array_equal(_bits(nrm), _bits(pose[r])) and np.array_equal(_bits(s), _bits(spr[r])), (k, r)
            assert np.array_equal(_bits(e), _bits(exp[r])) and np.array_equal(_bits(obs), _bits(raws[k][r])), (k, r)
            counts.add(int(cnt))
    assert counts == {0, 1, 2}


# 3 ---------------------------------------------------------------------------------------------------------------------
def _same_tick(a, b, forecast=True):
    assert np.array_equal(a.meta, b.meta) and np.array_equal(a.frames, b.frames) and np.array_equal(a.trans, b.trans)
    assert a.first_window_id == b.first_window_id and torch.equal(a.scores, b.scores)
    assert (a.windows is None) == (b.windows is None)
    if a.windows is not None:
        assert torch.equal(a.windows.base, b.windows.base) and torch.equal(a.windows.trans, b.windows.trans)
    for x, y in ((a.final, b.final), (a.closed, b.closed)):
        assert x.keys == y.keys and np.array_equal(x.frames, y.frames) and torch.equal(x.values, y.values)
        if forecast:
            _same_rows(x.forecast, y.forecast)
    assert a.clip is None and b.clip is None


def test_push_many_of_three_ticks_equals_push(setup):
    """K = 3 ticks per call on ring_len = seg_len + 2 (groups of up to three ticks: a track's three windows are stored before the
    first of its three final rows is read) against tick-by-tick pushes: every field, both new rings, close_all.  (The draws are the
    in-kernel ones: keyed by the global window id, the same in both streams.)"""
    m, tracks = setup["model"], off_tracks()
    kw = dict(setup["kw"], max_tracks=32, ring_len=SEG_LEN + 2, forecasts=ForecastCfg("mean", "median"), max_idle=3)
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
    assert sum(len(t.closed) for t in ta) > 0 and sum(len(t.final) for t in ta) > 100        # idle tails and finals both occur
    assert sum(int((t.closed.forecast.count > 0).sum()) for t in ta) > 0
    ca, cb = a.close_all(), b.close_all()
    assert ca.keys == cb.keys and torch.equal(ca.values, cb.values) and len(ca) > 0
    _same_rows(ca.forecast, cb.forecast)
    assert torch.equal(a.rings.forecast_ring, b.rings.forecast_ring) and torch.equal(a.rings.observed_ring, b.rings.observed_ring)
    assert torch.equal(a.rings.frame_scores_ring, b.rings.frame_scores_ring) and torch.equal(a.ring, b.ring)
    assert bool((a.rings.forecast_ring != 0).any()) and bool((a.rings.observed_ring != 0).any())


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_a_reused_slot_starts_clean(setup):
    """One slot, max_idle = 1, ring_len = seg_len + 1: track A wraps the ring, goes idle and is closed; track B takes the slot over.
    B's forecasts are those of a fresh stream that only ever saw B -- no cell of A is read (given noise, the same for both)."""
    m = setup["model"]
    kw = dict(setup["kw"], max_tracks=1, max_idle=1, ring_len=SEG_LEN + 1, forecasts=ForecastCfg())
    S, ns = m.n_generated_samples, m.noise_steps
    raw = stress_rows(3 * SEG_LEN + 6, seed=21)
    gen = torch.Generator().manual_seed(5)
    used, fresh = PoseStream(m, **kw), PoseStream(m, **kw)
    A, Bk = (1, 1, 1), (1, 1, 2)
    for i in range(SEG_LEN + 3):                       # A: four windows, the ring wraps
        nz = torch.randn(S, ns - 1, NT, 2, 3, 17, generator=gen).to(DEV) if i >= SEG_LEN - 1 else None
        used.push([A], [i + 1], raw[i:i + 1], noise=nz)
    assert bool((used.rings.forecast_ring != 0).any()) and bool((used.rings.observed_ring != 0).any())
    used.push([], [], np.zeros((0, 34), np.float32))   # an empty tick: A is idle
    rows_b = raw[SEG_LEN + 3:]
    ticks = []
    for i in range(len(rows_b)):
        nz = torch.randn(S, ns - 1, NT, 2, 3, 17, generator=gen).to(DEV) if i >= SEG_LEN - 1 else None
        tu = used.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        tf = fresh.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        if i == 0:                                     # A's tail comes back with the tick that closes it, forecasts too
            assert tu.closed.keys == [A] * (SEG_LEN - 1) and len(tu.closed.forecast) == SEG_LEN - 1
            assert tu.closed.forecast.count.tolist() == [2, 3, 3, 2, 1] and used.table.slot_of[Bk] == 0      # (row 4: no window starts at row -1)
            assert np.array_equal(_bits(tu.closed.forecast.observed.cpu().numpy()), _bits(raw[4:SEG_LEN + 3]))
        else:
            assert len(tu.closed) == 0
        assert torch.equal(tu.scores, tf.scores) and torch.equal(tu.final.values, tf.final.values)
        _same_rows(tu.forecast, tf.forecast, i)
        ticks.append(tu)
    counts = torch.cat([t.forecast.count for t in ticks]).tolist()
    assert counts[:4] == [0, 0, 0, 1] and counts[4:6] == [2, 3] and len(counts) == len(rows_b) - SEG_LEN + 1
    cu, cf = used.close([Bk]), fresh.close([Bk])
    _same_rows(cu.forecast, cf.forecast)
    assert torch.equal(cu.values, cf.values) and cu.forecast.count.tolist() == [3, 3, 3, 2, 1]


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_off_is_the_stream_without_the_argument(setup):
    """forecasts=None: every Tick field and both rings are those of a stream built without the argument, nothing is allocated and
    the scorer is asked for no poses; switching it ON changes none of the existing fields, and ON together with joint_scores=True
    leaves joint_final bit-identical."""
    m, tracks = setup["model"], off_tracks()
    sc = m.scorer()
    sc._map_bufs.clear()
    plain = PoseStream(m, ring_len=SEG_LEN, **setup["kw"])
    off = PoseStream(m, ring_len=SEG_LEN, forecasts=None, **setup["kw"])
    for st in (plain, off):
        assert st.rings.forecast_ring is None and st.rings.observed_ring is None and st.rings._fstate is None and st.forecasts is None

    def both(keys, fids, poses, metas):
        tp, to = plain.push(keys, fids, poses), off.push(keys, fids, poses)
        _same_tick(tp, to, forecast=False)
        assert to.forecast is None and to.final.forecast is None and to.closed.forecast is None
        return tp

    ticks, tails = _replay([plain, off], tracks, both)
    assert sum(len(t.final) for t in ticks) == 283 and not sc._map_bufs
    assert torch.equal(plain.ring, off.ring) and torch.equal(plain.rings.frame_scores_ring, off.rings.frame_scores_ring)
    for _, fs in tails:
        assert fs.forecast is None
    on = PoseStream(m, ring_len=SEG_LEN, forecasts=ForecastCfg(), **setup["kw"])
    joint = PoseStream(m, ring_len=SEG_LEN, joint_scores=True, **setup["kw"])
    jon = PoseStream(m, ring_len=SEG_LEN, joint_scores=True, forecasts=ForecastCfg(), **setup["kw"])
    at = [0]

    def with_forecasts(keys, fids, poses, metas):
        tn, tj, tb = on.push(keys, fids, poses), joint.push(keys, fids, poses), jon.push(keys, fids, poses)
        _same_tick(ticks[at[0]], tn, forecast=False)
        _same_tick(ticks[at[0]], tb, forecast=False)
        assert tn.forecast is not None and len(tn.forecast) == len(tn.final) and tn.joint_final is None
        assert torch.equal(tj.joint_final, tb.joint_final) and torch.equal(tj.closed.joints, tb.closed.joints)
        _same_rows(tn.forecast, tb.forecast)
        at[0] += 1
        return tn

    _, tails_on = _replay([on, joint, jon], tracks, with_forecasts)
    assert at[0] == len(ticks)
    for (_, fa), (_, fb) in zip(tails, tails_on):
        assert fa.keys == fb.keys and torch.equal(fa.values, fb.values) and fb.forecast is not None
    for st in (on, jon):
        assert torch.equal(plain.ring, st.ring) and torch.equal(plain.rings.frame_scores_ring, st.rings.frame_scores_ring)
    assert torch.equal(joint.rings.joint_scores_ring, jon.rings.joint_scores_ring)
    # with both options on, the maps launch reads the losses and poses the forecasts asked for -- they are written once: the
    # scorer's own buffers for poses nobody asked for stay unused
    sc._map_bufs.clear()
    both_on = PoseStream(m, ring_len=SEG_LEN, joint_scores=True, forecasts=ForecastCfg(), **dict(setup["kw"], max_tracks=64))
    feed = [(keys, fids, poses) for _, keys, fids, poses in ticks_by_frame(tracks)][:SEG_LEN + 2]
    assert sum(len(both_on.push(*t).final) for t in feed) > 0 and not sc._map_bufs


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_aggregation_worst(tmp_path):
    g = load_dataset_golden()
    m, args = _model_with(tmp_path, g, aggregation_strategy="worst")
    assert m.aggregation_strategy == "worst"
    off = Offline(m, args, g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
    got, _ = _stream_rows(m, off, kw, ForecastCfg("median", "mean"))
    assert _check_against_offline(got, off.rows("median", "mean"), off_tracks()) == {0, 1, 2, 3}
    best = Offline(*_model(tmp_path, g), g)
    assert not torch.equal(best.pose_agg, off.pose_agg)            # (the selection matters: worst is not best)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_a_window_with_nan_noise_contributes_zeros(setup):
    """One window whose given noise is all NaN: no sample passes, pose_agg is zero (mcd_aggregate's rule), the stream stores zeros.
    Only the <= n_corrupt rows that window forecasts differ from the clean replay, counts are unchanged, and the rows still equal
    the dataset path under the same noise."""
    m, g, clean_off = setup["model"], setup["g"], setup["offline"]
    tw = clean_off.tw
    meta, frames = tw.meta[:clean_off.n].numpy(), tw.frames[:clean_off.n].numpy()
    length = {k: len(f) for k, f, _ in off_tracks()}
    fid_pos = {k: {int(x): i for i, x in enumerate(f)} for k, f, _ in off_tracks()}
    # a window in the middle of a long track: its three forecast rows are each forecast by three windows
    pick = next(i for i, mm in enumerate(meta) if length[tuple(int(v) for v in mm[:3])] >= 2 * SEG_LEN + 2
                and fid_pos[tuple(int(v) for v in mm[:3])][int(mm[3])] == SEG_LEN)
    key = tuple(int(v) for v in meta[pick][:3])
    hit = {(key, int(f)) for f in frames[pick][N_COND:]}
    off = Offline(m, setup["args"], g, nan_sample=pick)
    assert not off.pose_agg[pick].any() and bool(clean_off.pose_agg[pick].any())
    got, _ = _stream_rows(m, off, setup["kw"], ForecastCfg("median", "mean"))
    _check_against_offline(got, off.rows("median", "mean"), off_tracks())
    clean = setup["cache"].get(("median", "mean")) or _stream_rows(m, clean_off, setup["kw"], ForecastCfg("median", "mean"))[0]
    changed = set()
    for rk in clean:
        assert got[rk][3] == clean[rk][3]                               # counts
        assert np.array_equal(_bits(got[rk][2]), _bits(clean[rk][2]))   # observed
        if any(not np.array_equal(_bits(got[rk][i]), _bits(clean[rk][i])) for i in (0, 1, 4)):
            changed.add(rk)
    assert changed and changed <= hit and all(got[rk][3] == 3 for rk in hit)
    assert all(np.isfinite(got[rk][1]).all() for rk in hit)             # zeros, not NaNs, entered the median


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_the_three_refusals(setup):
    class Latent:
        is_latent = True
    with pytest.raises(NotImplementedError, match="needs the pose model"):
        PoseStream(Latent(), vid_res=VID_RES, forecasts=ForecastCfg())
    m = setup["model"]
    for aggr in ("mean", "median", "quantile:0.3"):
        m.aggregation_strategy = aggr
        try:
            with pytest.raises(ValueError, match="best or worst"):
                PoseStream(m, forecasts=ForecastCfg(), **setup["kw"])
        finally:
            m.aggregation_strategy = "best"
    with pytest.raises(ValueError, match="method must be one of"):
        PoseStream(m, forecasts=ForecastCfg(method="mode"), **setup["kw"])
    with pytest.raises(ValueError, match="spread must be one of"):
        PoseStream(m, forecasts=ForecastCfg(spread="unique"), **setup["kw"])

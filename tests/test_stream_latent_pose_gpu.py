"""GPU: live pose streams scored by the latent model IN POSE SPACE (PoseStream over a MoCoDADlatent module with a loaded stage-1
decoder, `latent_score_space: 'pose'` or space='pose': the tick's scoring call is engine.LatentPoseScorer.score =
mcd_latent_score_pose) with per-joint frame scores and expected poses, against the dataset path on the committed fixture: ONE offline
pose-space call over the split with the same given noise, window by window, then mcd_joint_scatter_max, engine.forecast_assemble and
engine.denormalize_poses.  Every comparison is exact: a compared value is a copy, a maximum, a fixed-order float64 reduction, or the
output of a launch that does not depend on its batch, its chunking or its sample split (tests/test_latent_pose_call_gpu.py).

Fixture settings of tests/test_stream_latent_gpu.py: configs/ubnormal_latent_test.yaml on tests/golden/dataset, seg_len 6 (3 + 3),
noise_steps 4, 2 samples, 5 transforms, 283 windows, at most 18 tracks; the stage-1 state dict is random-init and shares the frozen
tensors with the module (as tests/test_latent_forecast_gpu.py builds one)."""
import copy

import numpy as np
import pytest
import torch

from dataset_spec import load_dataset_golden, stress_rows
from mocodad_amd.data import trajectories as T
from mocodad_amd.data.windows import WindowBatch
from mocodad_amd.engine import denormalize_poses, forecast_assemble
from mocodad_amd.stream import ForecastCfg, PoseStream, forecast_cover, ticks_by_frame
from mocodad_amd.utils.eval_utils import compute_var_matrix, forecast_track_rows
from test_stream_forecast_gpu import FIELDS, _check_against_offline, _np, _same_rows
from test_stream_latent_gpu import DEV, NT, SEG_LEN, VID_RES, _bits, _model, _replay, _tracks

pytestmark = pytest.mark.gpu
N_COND = 3
CFGS = [("median", "mean"), ("mean", "median"), ("unique", "mean")]


def stage1_of(m, args, seed=321):
    """A random-init stage-1 ('pretrain') state dict whose shared tensors -- the down path, to_time_dim, the condition encoder --
    are the module's own: what stage 2 trained from it, both frozen, would hold."""
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    a = copy.copy(args)
    a.stage = "pretrain"
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        sd = {k: v.detach().clone().cpu() for k, v in MoCoDADlatentPretrain(a).state_dict().items()}
    own = m.state_dict()
    assert all(k in sd for k in own if k.startswith(("model.", "condition_encoder.")))
    sd.update({k: v.detach().clone().cpu() for k, v in own.items() if k in sd})
    return sd


def pose_model(tmp, g, **over):
    m, args = _model(tmp, g, **over)
    m.load_decoder(stage1_of(m, args))
    return m, args


class Offline:
    """The dataset path in pose space on the fixture's test split: ONE LatentPoseScorer.score call with a given noise tensor."""

    def __init__(self, m, args, g):
        self.m, self.g = m, g
        ps = m.pose_scorer()
        self.tw = tw = T.load_dataset(args, DEV)[0]
        self.n = n = tw.n_samples
        S, ns, D = m.n_generated_samples, m.noise_steps, m.latent_embedding_dim
        self.noise = torch.randn(S, ns - 1, NT * n, D, generator=torch.Generator().manual_seed(7)).to(DEV)
        wb = WindowBatch(tw.buffer, tw.base.to(DEV), tw.trans.to(DEV), tw.affine, SEG_LEN)
        r = ps.score(wb, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy, noise=self.noise, loss_fn=m.loss_name,
                     want_all=True, want_poses=True, want_maps=True, want_selected=True)
        self.scores, self.loss_all, self.poses_all, self.maps, self.pose_agg = (x.clone() for x in r)
        assert tuple(self.pose_agg.shape) == (NT * n, 2, 3, 17) and tuple(self.maps.shape) == (NT * n, 3, 17)
        self.sample_of = {tuple(int(v) for v in r_): i for i, r_ in enumerate(tw.meta[:n].numpy())}

    def rows(self, method, spread):
        tw, g = self.tw, self.g
        mf = self.m.map_frames(None, len(tw)).cpu().numpy()
        pose, count, spr, keys, fids = forecast_track_rows(self.pose_agg, tw.trans.numpy(), mf, forecast_assemble, windows=tw,
                                                           method=method, spread_method=spread)
        expected = denormalize_poses(pose, tw.raw.poses, VID_RES, g["train_center"], g["train_scale"], count=count)
        pose, count, spr, expected = (t.cpu().numpy() for t in (pose, count, spr, expected))
        return {(tuple(int(v) for v in k), int(f)): (expected[i], pose[i], count[i], spr[i]) for i, (k, f) in enumerate(zip(keys, fids))}


def replay(m, off, tracks, kw, **opts):
    """The fixture through a pose-space PoseStream (ring_len = seg_len: every ring wraps) with off's noise, window by window
    -> (ticks, tails, the index of every tick's windows in the offline call)."""
    stream = PoseStream(m, ring_len=SEG_LEN, space="pose", **kw, **opts)
    n, idx_of_tick = off.n, []

    def on_tick(keys, fids, poses, plan_meta):
        idx = np.asarray([t * n + off.sample_of[mm] for t in range(NT) for mm in plan_meta], np.int64)
        tick = stream.push(keys, fids, poses, noise=off.noise[:, :, torch.from_numpy(idx).to(DEV)] if len(idx) else None)
        assert [tuple(int(v) for v in r) for r in tick.meta[:len(plan_meta)]] == plan_meta
        idx_of_tick.append(idx)
        return tick

    ticks, tails = _replay([stream], tracks, on_tick)
    torch.cuda.synchronize()
    return ticks, tails, idx_of_tick


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    g = load_dataset_golden()
    m, args = pose_model(tmp_path_factory.mktemp("stream_latent_pose"), g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
    off = Offline(m, args, g)
    assert off.n == 283
    tracks = _tracks()
    ticks, tails, idx = replay(m, off, tracks, kw, joint_scores=True, forecasts=ForecastCfg(*CFGS[0]))
    return dict(g=g, model=m, args=args, kw=kw, off=off, tracks=tracks, ticks=ticks, tails=tails, idx_of_tick=idx)


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_window_scores_are_the_offline_pose_space_scores(run):
    off, m = run["off"], run["model"]
    offline = off.scores.cpu().numpy()
    compared, sizes = 0, set()
    for tick, idx in zip(run["ticks"], run["idx_of_tick"]):
        got = tick.scores.cpu().numpy()
        assert got.shape == idx.shape and np.array_equal(_bits(got), _bits(offline[idx]))
        compared += len(idx)
        sizes.add(len(idx))
    assert compared == 283 * NT and len(sizes) > 3
    assert np.isfinite(offline).all() and len(np.unique(offline)) > 1000      # (not a constant: the test can fail)
    # ... and they are NOT the latent-space losses the same windows get (what a stream of this module returned before)
    wb = WindowBatch(off.tw.buffer, off.tw.base.to(DEV), off.tw.trans.to(DEV), off.tw.affine, SEG_LEN)
    lat = m.scorer().score(wb, n_samples=m.n_generated_samples, noise_steps=m.noise_steps, aggregation=m.aggregation_strategy,
                           noise=off.noise, loss_fn=m.loss_name)[0]
    assert not np.array_equal(_bits(lat.cpu().numpy()), _bits(offline))


def test_frame_scores_equal_the_offline_row_maximum_and_the_auc(run):
    off, tracks, m = run["off"], run["tracks"], run["model"]
    tw, n, offline = off.tw, off.n, off.scores.cpu().numpy()
    got = {}

    def take(fs):
        vals = fs.values.cpu().numpy()
        for k, f, v in zip(fs.keys, fs.frames, vals):
            assert (k, int(f)) not in got
            got[(k, int(f))] = v
    for tick in run["ticks"]:
        take(tick.final)
    for _, fs in run["tails"]:
        take(fs)
    meta, frames = tw.meta[:n].numpy(), tw.frames[:n].numpy()
    kept = [(k, f) for k, f, _ in tracks if len(f) >= SEG_LEN]
    assert len(kept) == 14 and len(got) == sum(len(f) for _, f in kept)
    n_frames, compared = int(frames.max()), 0
    for k, f in kept:
        sel = np.flatnonzero((meta[:, :3] == np.asarray(k)).all(1))
        for t in range(NT):
            want = np.nanmax(compute_var_matrix(offline[t * n + sel], frames[sel], n_frames), axis=0)
            for fid in f:
                assert np.float64(got[(k, int(fid))][t]) == want[fid - 1], (k, t, fid)
                compared += 1
    assert compared == NT * sum(len(f) for _, f in kept)
    out = np.full(NT * n, np.nan, np.float32)
    for tick, idx in zip(run["ticks"], run["idx_of_tick"]):
        out[idx] = tick.scores.cpu().numpy()
    trans, meta_all, frames_all = tw.trans.long().numpy(), tw.meta.numpy(), tw.frames.numpy()
    auc = m.post_processing(out, None, trans, meta_all, frames_all)
    assert np.isfinite(auc) and auc == m.post_processing(offline, None, trans, meta_all, frames_all)


def test_joint_finals_and_tails_equal_the_scatter_max_of_the_offline_maps(run):
    off, tracks = run["off"], run["tracks"]
    tw, n = off.tw, off.n
    meta, frames = tw.meta[:n].numpy(), tw.frames[:n].numpy()
    kept = [(k, f) for k, f, _ in tracks if len(f) >= SEG_LEN]
    track_of = {k: i for i, (k, _) in enumerate(kept)}
    row = np.asarray([t * len(kept) + track_of[tuple(int(v) for v in mm[:3])] for t in range(NT) for mm in meta], np.int32)
    n_frames = int(frames.max())
    want = run["model"].decoder().joint_scatter_max(off.maps, torch.from_numpy(np.tile(frames[:, N_COND:], (NT, 1))), torch.from_numpy(row),
                                                    NT * len(kept), n_frames).cpu().numpy()
    got = {}

    def take(fs):
        assert fs.joints is not None and tuple(fs.joints.shape) == (len(fs), NT, 17)
        for k, f, v in zip(fs.keys, fs.frames, fs.joints.cpu().numpy()):
            assert (k, int(f)) not in got
            got[(k, int(f))] = v
    for tick in run["ticks"]:
        assert tick.joint_final is tick.final.joints and len(tick.closed) == 0
        take(tick.final)
    for _, fs in run["tails"]:
        take(fs)
    assert len(got) == sum(len(f) for _, f in kept)
    compared = zeros = 0
    for k, f in kept:
        for i, fid in enumerate(f):
            for t in range(NT):
                w = want[t * len(kept) + track_of[k], fid - 1]
                assert np.array_equal(_bits(got[(k, int(fid))][t]), _bits(w)), (k, fid, t)
                if i < N_COND:          # rows no window forecasts are zero
                    assert not w.any()
                    zeros += 1
                compared += 1
    assert compared == NT * sum(len(f) for _, f in kept) and zeros == NT * N_COND * len(kept)
    assert (want > 0).sum() > 1000 and len(np.unique(want)) > 1000         # (not a constant: the test can fail)


def _forecast_rows(ticks, tails):
    got = {}

    def take(fs):
        assert fs.forecast is not None and len(fs.forecast) == len(fs)
        f = _np(fs.forecast)
        for i, (k, fid) in enumerate(zip(fs.keys, fs.frames)):
            assert (k, int(fid)) not in got
            got[(k, int(fid))] = tuple(f[name][i] for name in FIELDS)
    for tick in ticks:
        assert tick.forecast is tick.final.forecast
        take(tick.final)
    for _, fs in tails:
        take(fs)
    return got


@pytest.mark.parametrize("method, spread", CFGS)
def test_forecasts_equal_the_dataset_path(run, method, spread):
    off = run["off"]
    if (method, spread) == CFGS[0]:
        ticks, tails = run["ticks"], run["tails"]           # (the replay with both options on)
    else:
        ticks, tails, _ = replay(run["model"], off, run["tracks"], run["kw"], forecasts=ForecastCfg(method, spread))
    got = _forecast_rows(ticks, tails)
    counts = _check_against_offline(got, off.rows(method, spread), run["tracks"])
    assert counts == {0, 1, 2, 3}
    assert len(np.unique(np.stack([v[1] for v in got.values()]))) > 1000 and len(np.unique(np.stack([v[0] for v in got.values()]))) > 1000


# 2 ---------------------------------------------------------------------------------------------------------------------
def _same_tick(a, b):
    assert np.array_equal(a.meta, b.meta) and np.array_equal(a.frames, b.frames) and np.array_equal(a.trans, b.trans)
    assert a.first_window_id == b.first_window_id and torch.equal(a.scores, b.scores)
    assert (a.windows is None) == (b.windows is None)
    if a.windows is not None:
        assert torch.equal(a.windows.base, b.windows.base) and torch.equal(a.windows.trans, b.windows.trans)
    for x, y in ((a.final, b.final), (a.closed, b.closed)):
        assert x.keys == y.keys and np.array_equal(x.frames, y.frames) and torch.equal(x.values, y.values)
        assert (x.joints is None) == (y.joints is None) and (x.forecast is None) == (y.forecast is None)
        if x.joints is not None:
            assert torch.equal(x.joints, y.joints)
        if x.forecast is not None:
            _same_rows(x.forecast, y.forecast)
    assert (a.joint_final is None) == (b.joint_final is None)
    if a.joint_final is not None:
        assert torch.equal(a.joint_final, b.joint_final)
    assert a.clip is None and b.clip is None


def test_push_many_of_three_ticks_equals_push(run):
    m, tracks = run["model"], run["tracks"]
    kw = dict(run["kw"], max_tracks=32, ring_len=SEG_LEN + 2, joint_scores=True, forecasts=ForecastCfg("mean", "median"), max_idle=3,
              space="pose")
    a, b = PoseStream(m, **kw), PoseStream(m, **kw)
    feed = [(keys, fids, poses) for _, keys, fids, poses in ticks_by_frame(tracks)]
    ta = [a.push(*t) for t in feed]
    tb = []
    for i in range(0, len(feed), 3):
        tb += b.push_many(feed[i:i + 3])
    assert len(ta) == len(tb) == len(feed)
    for x, y in zip(ta, tb):
        _same_tick(x, y)
        assert x.joint_final is not None and x.forecast is not None
    assert sum(len(t.closed) for t in ta) > 0 and sum(len(t.final) for t in ta) > 100
    ca, cb = a.close_all(), b.close_all()
    assert ca.keys == cb.keys and torch.equal(ca.values, cb.values) and torch.equal(ca.joints, cb.joints) and len(ca) > 0
    _same_rows(ca.forecast, cb.forecast)
    for ring in ("ring",):
        assert torch.equal(getattr(a, ring), getattr(b, ring))
    for ring in ("frame_scores_ring", "joint_scores_ring", "forecast_ring", "observed_ring"):
        assert torch.equal(getattr(a.rings, ring), getattr(b.rings, ring)), ring
    assert bool((a.rings.forecast_ring != 0).any()) and bool((a.rings.joint_scores_ring != 0).any())


def test_a_reused_slot_starts_clean(run):
    m = run["model"]
    kw = dict(run["kw"], max_tracks=1, max_idle=1, ring_len=SEG_LEN + 1, joint_scores=True, forecasts=ForecastCfg(), space="pose")
    S, ns, D = m.n_generated_samples, m.noise_steps, m.latent_embedding_dim
    raw = stress_rows(3 * SEG_LEN + 6, seed=21)
    gen = torch.Generator().manual_seed(5)
    used, fresh = PoseStream(m, **kw), PoseStream(m, **kw)
    A, Bk = (1, 1, 1), (1, 1, 2)
    draw = lambda: torch.randn(S, ns - 1, NT, D, generator=gen).to(DEV)
    for i in range(SEG_LEN + 3):                       # A: four windows, the ring wraps
        used.push([A], [i + 1], raw[i:i + 1], noise=draw() if i >= SEG_LEN - 1 else None)
    assert bool((used.rings.forecast_ring != 0).any()) and float(used.rings.joint_scores_ring.abs().sum()) > 0
    used.push([], [], np.zeros((0, 34), np.float32))   # an empty tick: A is idle
    rows_b = raw[SEG_LEN + 3:]
    for i in range(len(rows_b)):
        nz = draw() if i >= SEG_LEN - 1 else None
        tu = used.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        tf = fresh.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        if i == 0:
            assert tu.closed.keys == [A] * (SEG_LEN - 1) and used.table.slot_of[Bk] == 0
            assert tu.closed.forecast.count.tolist() == [2, 3, 3, 2, 1]
        else:
            assert len(tu.closed) == 0
        assert torch.equal(tu.scores, tf.scores) and torch.equal(tu.final.values, tf.final.values)
        assert torch.equal(tu.joint_final, tf.joint_final)
        _same_rows(tu.forecast, tf.forecast, i)
    cu, cf = used.close([Bk]), fresh.close([Bk])
    _same_rows(cu.forecast, cf.forecast)
    assert torch.equal(cu.values, cf.values) and torch.equal(cu.joints, cf.joints) and cu.forecast.count.tolist() == [3, 3, 3, 2, 1]


def test_perf_mode_is_parity_mode_fed_the_exported_draws(run):
    m, tracks = run["model"], run["tracks"]
    kw = dict(run["kw"], ring_len=SEG_LEN, joint_scores=True, forecasts=ForecastCfg(), space="pose")
    a, b = PoseStream(m, **kw), PoseStream(m, **kw)
    ps = m.pose_scorer()
    compared = [0]

    def on_tick(keys, fids, poses, metas):
        ta = a.push(keys, fids, poses)
        nw = ta.scores.numel()
        assert ta.first_window_id == compared[0] and nw == NT * len(metas)
        noise = ps.philox_noise(nw, n_samples=m.n_generated_samples, noise_steps=m.noise_steps, seed=m.seed,
                                first_window_id=ta.first_window_id) if nw else None
        _same_tick(ta, b.push(keys, fids, poses, noise=noise))
        compared[0] += nw
        return ta

    _replay([a, b], tracks, on_tick)
    assert compared[0] == 283 * NT == a.n_emitted


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_six_plus_six_frames_on_a_longer_ring(tmp_path):
    """A 6 + 6 model (the project / unproject launches, one window per workgroup) on two synthetic tracks of 2 seg_len + 1 rows,
    ring_len = seg_len + 3: the tick's windows, still in the ring, scored again offline with the same noise; then the dataset
    path's assembly over each track's windows."""
    g = load_dataset_golden()
    Tt, L = 12, 15
    m, _ = pose_model(tmp_path, g, seg_len=Tt, conditioning_indices=list(range(6)))
    ps, dec = m.pose_scorer(), m.decoder()
    cidx = list(range(6, 12))
    assert ps.corrupt_idx == cidx and ps.seg_len == Tt
    S, ns, D = m.n_generated_samples, m.noise_steps, m.latent_embedding_dim
    n_rows = 2 * Tt + 1
    keys = [(1, 1, 1), (1, 1, 2)]
    raws = {k: stress_rows(n_rows, seed=31 + k[2]) for k in keys}
    cs = dict(center=g["train_center"], scale=g["train_scale"])
    st = PoseStream(m, vid_res=VID_RES, max_tracks=2, ring_len=L, joint_scores=True, forecasts=ForecastCfg("median", "median"), space="pose", **cs)
    gen = torch.Generator().manual_seed(9)
    fc, joints, agg_of, maps_of = {}, {}, {k: {} for k in keys}, {k: {} for k in keys}

    def take(fs):
        f, j = _np(fs.forecast), fs.joints.cpu().numpy()
        for i, (k, fid) in enumerate(zip(fs.keys, fs.frames)):
            assert (k, int(fid)) not in fc
            fc[(k, int(fid))] = tuple(f[name][i] for name in FIELDS)
            joints[(k, int(fid))] = j[i]

    for r in range(n_rows):
        ne = 2 if r >= Tt - 1 else 0
        nz = torch.randn(S, ns - 1, NT * ne, D, generator=gen).to(DEV) if ne else None
        tick = st.push(keys, [r + 1] * 2, np.stack([raws[k][r] for k in keys]), noise=nz)
        if ne:
            o = ps.score(tick.windows, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy, noise=nz, loss_fn=m.loss_name,
                         want_maps=True, want_selected=True)
            assert torch.equal(tick.scores, o[0])
            for j, k in enumerate(tick.final.keys):
                agg_of[k][r] = o[4][j].cpu().numpy()                        # transform 0: the first n_emit windows
                maps_of[k][r] = o[3][j::ne].cpu().numpy()                   # every transform of that track's window
        take(tick.final)
    take(st.close(keys))
    assert len(fc) == 2 * n_rows
    counts = set()
    for k in keys:
        ends = sorted(agg_of[k])
        assert ends == list(range(Tt - 1, n_rows))
        cell = torch.tensor([[e - Tt + 1 + c for c in cidx] for e in ends], dtype=torch.int32)
        pose, count, spr = forecast_assemble(torch.from_numpy(np.stack([agg_of[k][e] for e in ends])), cell, n_rows, method="median",
                                             spread_method="median", device=DEV)
        exp = denormalize_poses(pose, raws[k], VID_RES, cs["center"], cs["scale"], count=count).cpu().numpy()
        pose, count, spr = pose.cpu().numpy(), count.cpu().numpy(), spr.cpu().numpy()
        maps = torch.from_numpy(np.stack([maps_of[k][e] for e in ends]))    # (windows, NT, 6, 17)
        nwin = len(ends)
        want_j = dec.joint_scatter_max(maps.permute(1, 0, 2, 3).reshape(NT * nwin, 6, 17), (cell + 1).repeat(NT, 1),
                                       torch.arange(NT, dtype=torch.int32).repeat_interleave(nwin), NT, n_rows).cpu().numpy()
        for r in range(n_rows):
            e, nrm, obs, cnt, s = fc[(k, r + 1)]
            assert cnt == count[r] == len(forecast_cover(cidx, Tt, r, n_rows - 1)), (k, r)
            assert np.array_equal(_bits(nrm), _bits(pose[r])) and np.array_equal(_bits(s), _bits(spr[r])), (k, r)
            assert np.array_equal(_bits(e), _bits(exp[r])) and np.array_equal(_bits(obs), _bits(raws[k][r])), (k, r)
            assert np.array_equal(_bits(joints[(k, r + 1)]), _bits(want_j[:, r])), (k, r)
            counts.add(int(cnt))
    assert counts == set(range(0, 7)) and len(np.unique(np.stack(list(joints.values())))) > 500


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_option_off_is_the_stream_without_the_new_arguments(tmp_path):
    """A latent-space stream of a module WITH a loaded decoder: every field and ring equals the stream built without the new
    argument, joint scores and forecasts stay refused, and the decoder is never packed."""
    g = load_dataset_golden()
    m, _ = pose_model(tmp_path, g)
    assert m.latent_score_space == "latent" and m._decoder_sd is not None
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18, ring_len=SEG_LEN)
    plain, off = PoseStream(m, **kw), PoseStream(m, space="latent", **kw)
    assert plain.space == off.space == "latent" and not plain.pose_space
    sc = m.scorer()
    assert plain.scorer is sc and off.scorer is sc

    def both(keys, fids, poses, metas):
        tp, to = plain.push(keys, fids, poses), off.push(keys, fids, poses)
        _same_tick(tp, to)
        assert to.joint_final is None and to.forecast is None
        return tp

    ticks, tails = _replay([plain, off], _tracks(), both)
    assert sum(len(t.final) for t in ticks) == 283
    assert torch.equal(plain.ring, off.ring) and torch.equal(plain.rings.frame_scores_ring, off.rings.frame_scores_ring)
    for st in (plain, off):
        assert st.rings.forecast_ring is None and st.rings.observed_ring is None
    with pytest.raises(NotImplementedError, match="a latent has no joints"):
        PoseStream(m, joint_scores=True, **kw)
    with pytest.raises(NotImplementedError, match="needs the pose model"):
        PoseStream(m, forecasts=ForecastCfg(), **kw)
    assert m._decoder is None and m._pose_scorer is None          # a latent-space stream never packs a decoder
    # the module's own space decides when the keyword is absent
    m.latent_score_space = "pose"
    try:
        st = PoseStream(m, joint_scores=True, **kw)
        assert st.pose_space and st.scorer is m.pose_scorer() and m._decoder is not None
        assert PoseStream(m, space="latent", **kw).scorer is sc
    finally:
        m.latent_score_space = "latent"


def test_the_refusals(tmp_path):
    g = load_dataset_golden()
    m, args = _model(tmp_path, g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"])

    class Latent:
        is_latent = True
    with pytest.raises(NotImplementedError, match="a latent has no joints"):
        PoseStream(Latent(), vid_res=VID_RES, joint_scores=True)
    with pytest.raises(NotImplementedError, match="needs the pose model"):
        PoseStream(Latent(), vid_res=VID_RES, forecasts=ForecastCfg())
    # pose space without a loaded decoder: forward's message, before any device call (no scorer is packed)
    m._scorer = None
    with pytest.raises(RuntimeError, match="needs the stage-1 decoder: call load_decoder first"):
        PoseStream(m, space="pose", **kw)
    with pytest.raises(RuntimeError, match="needs the stage-1 decoder: call load_decoder first"):
        PoseStream(m, space="pose", joint_scores=True, forecasts=ForecastCfg(), **kw)
    assert m._scorer is None
    m.load_decoder(stage1_of(m, args))
    for aggr in ("mean", "median", "quantile:0.3"):
        m.aggregation_strategy = aggr
        try:
            with pytest.raises(ValueError, match="best or worst"):
                PoseStream(m, space="pose", forecasts=ForecastCfg(), **kw)
            assert PoseStream(m, space="pose", joint_scores=True, **kw).pose_space        # (joint scores take any loss aggregation)
        finally:
            m.aggregation_strategy = "best"
    m.aggregation_strategy = "mean_pose"
    try:
        with pytest.raises(ValueError, match="PoseStream needs one loss per window"):
            PoseStream(m, space="pose", **kw)
    finally:
        m.aggregation_strategy = "best"
    with pytest.raises(ValueError, match="space must be"):
        PoseStream(m, space="joint", **kw)

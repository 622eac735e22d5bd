"""Live pose streams on the GPU (mocodad_amd/stream.py: PoseStream over mcd_stream_push_group / mcd_stream_frame_scores_group /
mcd_stream_flush, a tick being a group of one) against the dataset path on the same rows.  Every comparison is exact: a compared value is a copy, a maximum, or
the output of a scoring launch whose result does not depend on the batch it ran in (tests/test_multirank_gpu.py)."""
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from dataset_spec import DATASET, ROOT, load_dataset_golden, normalise, stress_rows
from mocodad_amd.data import trajectories as T
from mocodad_amd.data.windows import WindowBatch
from mocodad_amd.stream import PoseStream, ticks_by_frame
from mocodad_amd.utils.eval_utils import compute_var_matrix

pytestmark = pytest.mark.gpu
SEG_LEN = 6
VID_RES = (640, 360)
DEV = "cuda:0"
NT = 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _model(tmp, g):
    """A random-init MoCoDAD on the fixture's settings: noise_steps 4, 2 samples, 5 transforms; its scaler next to it."""
    from sklearn.preprocessing import RobustScaler
    from mocodad_amd.models.mocodad import MoCoDAD
    from mocodad_amd.utils.argparser import load_config
    with open(os.path.join(ROOT, "configs", "hr_avenue_test.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(data_dir=DATASET, test_path=os.path.join(DATASET, "testing", "test_frame_mask"), exp_dir=str(tmp / "exp"),
               dataset_choice="HR-STC", dir_name="fixture", noise_steps=4, n_generated_samples=2, batch_size=256,
               seg_len=SEG_LEN, vid_res=list(VID_RES), num_transform=NT, seed=11)
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


def _tracks(split="test"):
    files = T.list_trajectory_files(T.trajectories_root(DATASET, split))
    return [(key,) + T.read_trajectory_csv(path) for key, path in files]


def _replay(streams, tracks, on_tick, per_clip=False):
    """Feed `tracks` in frame order: on_tick(keys, fids, poses, metas) -> Tick, with metas = the (scene, clip, person, first
    frame) of the windows the tick emits, in emit order.  A track is closed on every stream right after its last row, so slots
    are reused.  Returns the ticks and the FrameScores of every close of streams[0]."""
    frames_of = {k: f for k, f, _ in tracks}
    pos = {k: 0 for k in frames_of}
    ticks, tails = [], []
    for _, keys, fids, poses in ticks_by_frame(tracks, per_clip):
        metas = [k + (int(frames_of[k][pos[k] - SEG_LEN + 1]),) for k in keys if pos[k] + 1 >= SEG_LEN]
        ticks.append(on_tick(keys, fids, poses, metas))
        done = []
        for k in keys:
            pos[k] += 1
            if pos[k] == len(frames_of[k]):
                done.append(k)
        if done:
            closed = [st.close(done) for st in streams]
            tails.append((done, closed[0]))
    return ticks, tails


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The fixture's test split scored offline (load_dataset + ONE score_fused call with a given noise tensor) and replayed
    through a PoseStream (ring_len = seg_len: every ring wraps several times) with the same noise, window by window."""
    g = load_dataset_golden()
    tmp = tmp_path_factory.mktemp("stream")
    m, args = _model(tmp, g)
    sc = m.scorer()
    tw, _ = T.load_dataset(args, DEV)
    n = tw.n_samples
    assert n == 283 and len(tw) == NT * n
    S, ns = m.n_generated_samples, m.noise_steps
    noise = torch.randn(S, ns - 1, NT * n, 2, 3, 17, generator=torch.Generator().manual_seed(7)).to(DEV)
    wb = WindowBatch(tw.buffer, tw.base.to(DEV), tw.trans.to(DEV), tw.affine, SEG_LEN)
    offline, _, _ = sc.score_fused(wb, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy, noise=noise,
                                   loss_fn=m.loss_name)
    offline = offline.cpu().numpy()
    sample_of = {tuple(int(v) for v in r): i for i, r in enumerate(tw.meta[:n].numpy())}

    tracks = _tracks()
    stream = PoseStream(m, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18, ring_len=SEG_LEN)
    idx_of_tick, mats = [], []

    def on_tick(keys, fids, poses, plan_meta):
        ne = len(plan_meta)
        idx = np.asarray([t * n + sample_of[mm] for t in range(NT) for mm in plan_meta], np.int64)
        tick = stream.push(keys, fids, poses, noise=noise[:, :, torch.from_numpy(idx).to(DEV)] if ne else None)
        assert [tuple(int(v) for v in r) for r in tick.meta[:ne]] == plan_meta
        idx_of_tick.append(idx)
        if ne:
            mats.append((plan_meta, WindowBatch(stream.ring, tick.windows.base[:ne], None, None, SEG_LEN).materialize().cpu()))
        else:
            assert tick.windows is None and tick.scores.numel() == 0 and len(tick.final) == 0
        return tick

    ticks, tails = _replay([stream], tracks, on_tick)
    torch.cuda.synchronize()
    return dict(g=g, model=m, args=args, tw=tw, n=n, offline=offline, tracks=tracks, ticks=ticks, tails=tails,
                idx_of_tick=idx_of_tick, mats=mats, stream=stream)


def _rows_to_window(rows34):
    """(seg_len, 34) interleaved normalised rows -> (C, T, V)."""
    return np.ascontiguousarray(rows34.reshape(-1, 17, 2).transpose(2, 0, 1))


@pytest.mark.parametrize("scaled, ring_len", [(True, SEG_LEN), (False, SEG_LEN), (True, SEG_LEN + 3)])
def test_ring_holds_the_normalised_rows_of_interleaved_synthetic_tracks(tmp_path, scaled, ring_len):
    g = load_dataset_golden()
    m, _ = _model(tmp_path, g)
    n_tracks, n_rows = 5, 40
    raw = stress_rows(n_tracks * n_rows, seed=3).reshape(n_tracks, n_rows, 34)
    rng = np.random.default_rng(4)
    center, scale = (rng.normal(0, 0.2, 34).astype(np.float32), rng.uniform(0.05, 1.5, 34)) if scaled else (None, None)
    want = normalise(raw.reshape(-1, 34), VID_RES, center, scale).reshape(n_tracks, n_rows, 34)
    stream = PoseStream(m, vid_res=VID_RES, center=center, scale=scale, max_tracks=n_tracks, ring_len=ring_len)
    pos = [0] * n_tracks
    compared = tick_no = 0
    while min(pos) < n_rows:
        # interleaved: track i starts at tick 2 i and skips every (i + 3)-th tick
        live = [i for i in range(n_tracks) if pos[i] < n_rows and tick_no >= 2 * i and tick_no % (i + 3) != 0]
        tick_no += 1
        if not live:
            continue
        tick = stream.push([(1, 1, i) for i in live], [1 + tick_no] * len(live), np.stack([raw[i, pos[i]] for i in live]))
        for i in live:
            pos[i] += 1
        emit = [i for i in live if pos[i] >= SEG_LEN]
        assert len(tick.final) == len(emit) and tick.scores.numel() == NT * len(emit)
        if emit:
            base = tick.windows.base
            host_base = [stream.table.base_offset(stream.table.slot_of[(1, 1, i)], pos[i] - SEG_LEN) for i in emit]
            assert base.cpu().tolist() == host_base * NT
            assert tick.windows.trans.cpu().tolist() == [t for t in range(NT) for _ in emit]
            got = WindowBatch(stream.ring, base[:len(emit)], None, None, SEG_LEN).materialize().cpu().numpy()
            for w, i in zip(got, emit):
                assert np.array_equal(_bits(w), _bits(_rows_to_window(want[i, pos[i] - SEG_LEN:pos[i]]))), (i, pos[i])
                compared += 1
    assert compared == n_tracks * (n_rows - SEG_LEN + 1)
    with pytest.raises(ValueError, match="NaN"):
        stream.push([(1, 1, 0)], [99], np.full((1, 34), np.nan, np.float32))


def test_fixture_windows_in_the_ring_equal_the_reference_x_local(run):
    g = run["g"]
    x = g["X_local"]
    ref = np.ascontiguousarray(x.reshape(*x.shape[:2], 17, 2).transpose(0, 3, 1, 2))        # (N, C, T, V), utils/dataset.py:255,271
    theirs = {tuple(int(v) for v in r): i for i, r in enumerate(g["meta"])}
    compared = 0
    for metas, mat in run["mats"]:
        for mm, w in zip(metas, mat.numpy()):
            assert np.array_equal(_bits(w), _bits(ref[theirs[mm]])), mm
            compared += 1
    assert compared == 283


def test_window_scores_equal_the_offline_scores_bit_for_bit(run):
    compared = 0
    for tick, idx in zip(run["ticks"], run["idx_of_tick"]):
        got = tick.scores.cpu().numpy()
        assert got.shape == idx.shape
        print(f"tick of {len(idx)} windows: max |stream - offline| = "
              f"{float(np.abs(got - run['offline'][idx]).max()) if len(idx) else 0.0:.3e}")
        assert np.array_equal(_bits(got), _bits(run["offline"][idx]))
        compared += len(idx)
    assert compared == 283 * NT
    assert np.isfinite(run["offline"]).all() and len(np.unique(run["offline"])) > 1000      # (not a constant: the test can fail)


def test_perf_mode_is_replayable_from_the_emitted_window_count(run):
    m, tracks = run["model"], run["tracks"]
    g = run["g"]
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18, ring_len=SEG_LEN)
    a, b = PoseStream(m, **kw), PoseStream(m, **kw)
    sc = m.scorer()
    compared = [0]

    def on_tick(keys, fids, poses, metas):
        ta = a.push(keys, fids, poses)
        nw = ta.scores.numel()
        assert ta.first_window_id == compared[0] and nw == NT * len(metas)
        noise = sc.philox_noise(nw, n_samples=m.n_generated_samples, noise_steps=m.noise_steps, seed=m.seed,
                                first_window_id=ta.first_window_id) if nw else None
        tb = b.push(keys, fids, poses, noise=noise)
        assert np.array_equal(_bits(ta.scores.cpu().numpy()), _bits(tb.scores.cpu().numpy()))
        compared[0] += nw
        return ta

    _replay([a, b], tracks, on_tick)
    assert compared[0] == 283 * NT == a.n_emitted


def test_frame_scores_cover_every_row_once_and_equal_the_offline_maximum(run):
    tw, n, offline, tracks = run["tw"], run["n"], run["offline"], run["tracks"]
    got = {}

    def take(fs):
        vals = fs.values.cpu().numpy()
        assert vals.shape == (len(fs), NT) and len(fs.frames) == len(fs)
        for k, f, v in zip(fs.keys, fs.frames, vals):
            assert (k, int(f)) not in got, (k, f)
            got[(k, int(f))] = v
    for tick in run["ticks"]:
        take(tick.final)
        assert len(tick.closed) == 0
    lens = {k: len(f) for k, f, _ in tracks}
    for done, fs in run["tails"]:
        assert len(fs) == (SEG_LEN - 1) * sum(lens[k] >= SEG_LEN for k in done)      # closed short tracks return nothing
        take(fs)
    meta, frames = tw.meta[:n].numpy(), tw.frames[:n].numpy()
    kept = [(k, f) for k, f, _ in tracks if len(f) >= SEG_LEN]
    assert len(kept) == 14 and len(got) == sum(len(f) for _, f in kept)
    n_frames = int(frames.max())
    compared = 0
    for k, f in kept:
        assert len(np.unique(f)) == len(f)
        sel = np.flatnonzero((meta[:, :3] == np.asarray(k)).all(1))
        for t in range(NT):
            want = np.nanmax(compute_var_matrix(offline[t * n + sel], frames[sel], n_frames), axis=0)
            for fid in f:
                assert np.float64(got[(k, int(fid))][t]) == want[fid - 1], (k, t, fid)
                compared += 1
    assert compared == NT * sum(len(f) for _, f in kept)


def test_stream_scores_in_dataset_order_give_the_offline_auc(run):
    m, tw, n = run["model"], run["tw"], run["n"]
    out = np.full(NT * n, np.nan, np.float32)
    for tick, idx in zip(run["ticks"], run["idx_of_tick"]):
        out[idx] = tick.scores.cpu().numpy()
    assert not np.isnan(out).any()
    trans, meta, frames = tw.trans.long().numpy(), tw.meta.numpy(), tw.frames.numpy()
    auc = m.post_processing(out, None, trans, meta, frames)
    ref = m.post_processing(run["offline"], None, trans, meta, frames)
    assert np.isfinite(auc) and auc == ref
    # the config's padding (12 frames around every absence) and smoothing (sigma 30) flatten clips of 40 frames: once more
    # without the padding and with sigma 2, where the frame scores keep their shape
    pad, sigma = m.anomaly_score_pad_size, m.anomaly_score_filter_kernel_size
    try:
        m.anomaly_score_pad_size, m.anomaly_score_filter_kernel_size = -1, 2
        auc = m.post_processing(out, None, trans, meta, frames)
        ref = m.post_processing(run["offline"], None, trans, meta, frames)
    finally:
        m.anomaly_score_pad_size, m.anomaly_score_filter_kernel_size = pad, sigma
    print(f"AUC without padding, sigma 2: stream {auc!r}, offline {ref!r}")
    assert np.isfinite(auc) and auc == ref


def test_max_idle_flushes_the_tail_and_rejected_settings(tmp_path):
    g = load_dataset_golden()
    m, args = _model(tmp_path, g)
    stream = PoseStream(m, vid_res=VID_RES, max_tracks=2, max_idle=1, ring_len=SEG_LEN + 2)
    raw = stress_rows(SEG_LEN + 2, seed=9)
    a, b = (1, 1, 1), (1, 1, 2)
    finals = []
    for i in range(SEG_LEN + 1):
        finals.append(stream.push([a], [10 + i], raw[i:i + 1]))
    assert len(stream.push([b], [99], raw[:1]).closed) == 0
    tick = stream.push([b], [100], raw[1:2])            # a idle for one tick: closed at the start of the next, its tail comes back
    assert tick.closed.keys == [a] * (SEG_LEN - 1) and tick.closed.frames.tolist() == list(range(12, 17))
    w0, w1 = (t.scores.cpu().numpy() for t in finals[-2:])
    tail = tick.closed.values.cpu().numpy()
    assert np.array_equal(finals[-2].final.values.cpu().numpy()[0], np.maximum(w0, 0))          # row 0: window 0 alone
    assert np.array_equal(finals[-1].final.values.cpu().numpy()[0], np.maximum(np.maximum(w0, w1), 0))
    assert np.array_equal(tail[:-1], np.tile(np.maximum(np.maximum(w0, w1), 0), (SEG_LEN - 2, 1)))
    assert np.array_equal(tail[-1], np.maximum(w1, 0))                                          # the last row: window 1 alone
    m2, _ = _model(tmp_path, g)
    m2.conditioning_strategy = "random_imp"
    with pytest.raises(ValueError, match="random_imp"):
        PoseStream(m2, vid_res=VID_RES)

"""Live pose streams scored by the latent model (PoseStream over a MoCoDADlatent module: the rings and the three stream kernels
of tests/test_stream_gpu.py, the tick's scoring call = engine.LatentScorer.score) against the dataset path on the same rows of
the committed dataset fixture.  Every comparison is exact: a compared value is a copy, a maximum, or the output of a scoring call
whose result does not depend on the batch it ran in (tests/test_latent_gpu.py: batch splits are bit-identical)."""
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from dataset_spec import DATASET, ROOT, load_dataset_golden
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


def _model(tmp, g, **over):
    """A random-init MoCoDADlatent on the fixture's settings: noise_steps 4, 2 samples, 5 transforms; its scaler next to it."""
    from sklearn.preprocessing import RobustScaler
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    from mocodad_amd.utils.argparser import load_config
    with open(os.path.join(ROOT, "configs", "ubnormal_latent_test.yaml")) as f:
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
    m = MoCoDADlatent(args).to(DEV)
    m.save_tensors = False
    return m, args


def _tracks(split="test"):
    files = T.list_trajectory_files(T.trajectories_root(DATASET, split))
    return [(key,) + T.read_trajectory_csv(path) for key, path in files]


def _replay(streams, tracks, on_tick):
    """Feed `tracks` in frame order: on_tick(keys, fids, poses, metas) -> Tick, with metas = the (scene, clip, person, first
    frame) of the windows the tick emits, in emit order.  A track is closed on every stream right after its last row, so slots
    are reused.  Returns the ticks and the FrameScores of every close of streams[0]."""
    frames_of = {k: f for k, f, _ in tracks}
    pos = {k: 0 for k in frames_of}
    ticks, tails = [], []
    for _, keys, fids, poses in ticks_by_frame(tracks):
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
    """The fixture's test split scored offline (load_dataset + ONE LatentScorer.score call with a given noise tensor) and
    replayed through a PoseStream (ring_len = seg_len: every ring wraps several times) with the same noise, window by window."""
    g = load_dataset_golden()
    tmp = tmp_path_factory.mktemp("stream_latent")
    m, args = _model(tmp, g)
    sc = m.scorer()
    tw, _ = T.load_dataset(args, DEV)
    n = tw.n_samples
    assert n == 283 and len(tw) == NT * n
    S, ns, D = m.n_generated_samples, m.noise_steps, m.latent_embedding_dim
    noise = torch.randn(S, ns - 1, NT * n, D, generator=torch.Generator().manual_seed(7)).to(DEV)
    wb = WindowBatch(tw.buffer, tw.base.to(DEV), tw.trans.to(DEV), tw.affine, SEG_LEN)
    offline = sc.score(wb, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy, noise=noise, loss_fn=m.loss_name)[0]
    offline = offline.cpu().numpy()
    sample_of = {tuple(int(v) for v in r): i for i, r in enumerate(tw.meta[:n].numpy())}

    tracks = _tracks()
    stream = PoseStream(m, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18, ring_len=SEG_LEN)
    idx_of_tick = []

    def on_tick(keys, fids, poses, plan_meta):
        ne = len(plan_meta)
        idx = np.asarray([t * n + sample_of[mm] for t in range(NT) for mm in plan_meta], np.int64)
        tick = stream.push(keys, fids, poses, noise=noise[:, :, torch.from_numpy(idx).to(DEV)] if ne else None)
        assert [tuple(int(v) for v in r) for r in tick.meta[:ne]] == plan_meta
        idx_of_tick.append(idx)
        if not ne:
            assert tick.windows is None and tick.scores.numel() == 0 and len(tick.final) == 0
        return tick

    ticks, tails = _replay([stream], tracks, on_tick)
    torch.cuda.synchronize()
    return dict(g=g, model=m, args=args, tw=tw, n=n, offline=offline, tracks=tracks, ticks=ticks, tails=tails,
                idx_of_tick=idx_of_tick, stream=stream)


def test_window_scores_equal_the_offline_scores_bit_for_bit(run):
    compared, sizes = 0, set()
    for tick, idx in zip(run["ticks"], run["idx_of_tick"]):
        got = tick.scores.cpu().numpy()
        assert got.shape == idx.shape
        assert np.array_equal(_bits(got), _bits(run["offline"][idx]))
        compared += len(idx)
        sizes.add(len(idx))
    assert compared == 283 * NT and len(sizes) > 3          # ticks of different sizes
    assert np.isfinite(run["offline"]).all() and len(np.unique(run["offline"])) > 1000      # (not a constant: the test can fail)


def test_perf_mode_is_parity_mode_fed_the_exported_draws(run):
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


def test_a_pose_aggregation_is_refused_with_the_existing_message(tmp_path):
    g = load_dataset_golden()
    m, _ = _model(tmp_path, g, aggregation_strategy="mean_pose")
    with pytest.raises(ValueError, match="PoseStream needs one loss per window"):
        PoseStream(m, vid_res=VID_RES)

"""GPU: per-joint frame scores of a live stream (PoseStream(joint_scores=True): mcd_error_maps on every tick's windows,
mcd_stream_joint_scores_group / mcd_stream_joint_flush on the joint ring) against the dataset path on the committed fixture --
ONE score_fused(want_maps=True) call over the split and mcd_joint_scatter_max -- with the same given noise, window by window.
Every comparison is exact: a compared value is a copy, a maximum, or the output of a launch whose result does not depend on the
batch it ran in.  The helpers (model, tracks, replay) are those of tests/test_stream_gpu.py."""
import numpy as np
import pytest
import torch

from dataset_spec import load_dataset_golden, stress_rows
from mocodad_amd.data import trajectories as T
from mocodad_amd.data.windows import WindowBatch
from mocodad_amd.stream import PoseStream, ticks_by_frame
from test_stream_gpu import DEV, NT, SEG_LEN, VID_RES, _bits, _model, _replay, _tracks

pytestmark = pytest.mark.gpu
N_COND = 3           # the fixture's model: frames 0 .. 2 condition, 3 .. 5 are forecast


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    g = load_dataset_golden()
    m, args = _model(tmp_path_factory.mktemp("stream_joint"), g)
    kw = dict(vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=18)
    return dict(g=g, model=m, args=args, tracks=_tracks(), kw=kw)


def test_joint_finals_equal_the_dataset_scatter_bit_for_bit(setup):
    m, args, tracks = setup["model"], setup["args"], setup["tracks"]
    sc = m.scorer()
    tw, _ = T.load_dataset(args, DEV)
    n = tw.n_samples
    S, ns = m.n_generated_samples, m.noise_steps
    noise = torch.randn(S, ns - 1, NT * n, 2, 3, 17, generator=torch.Generator().manual_seed(7)).to(DEV)
    wb = WindowBatch(tw.buffer, tw.base.to(DEV), tw.trans.to(DEV), tw.affine, SEG_LEN)
    offline, _, _, maps = sc.score_fused(wb, n_samples=S, noise_steps=ns, aggregation=m.aggregation_strategy, noise=noise,
                                         loss_fn=m.loss_name, want_maps=True)
    assert maps.shape == (NT * n, 3, 17) and torch.isfinite(maps).all()
    # the dataset path: one row per (transform, track), the frame ids of the forecast rows of every window
    meta, frames = tw.meta[:n].numpy(), tw.frames[:n].numpy()
    kept = [(k, f) for k, f, _ in tracks if len(f) >= SEG_LEN]
    track_of = {k: i for i, (k, _) in enumerate(kept)}
    row = np.asarray([t * len(kept) + track_of[tuple(int(v) for v in mm[:3])] for t in range(NT) for mm in meta], np.int32)
    n_frames = int(frames.max())
    want = sc.joint_scatter_max(maps, torch.from_numpy(np.tile(frames[:, N_COND:], (NT, 1))), torch.from_numpy(row), NT * len(kept),
                                n_frames).cpu().numpy()
    sample_of = {tuple(int(v) for v in r): i for i, r in enumerate(meta)}

    stream = PoseStream(m, ring_len=SEG_LEN, joint_scores=True, **setup["kw"])
    scores_ok = [0]

    def on_tick(keys, fids, poses, plan_meta):
        idx = np.asarray([t * n + sample_of[mm] for t in range(NT) for mm in plan_meta], np.int64)
        tick = stream.push(keys, fids, poses, noise=noise[:, :, torch.from_numpy(idx).to(DEV)] if len(idx) else None)
        assert np.array_equal(_bits(tick.scores.cpu().numpy()), _bits(offline[torch.from_numpy(idx).to(DEV)].cpu().numpy()))
        scores_ok[0] += len(idx)
        return tick

    ticks, tails = _replay([stream], tracks, on_tick)
    got = {}

    def take(fs):
        assert fs.joints is not None and tuple(fs.joints.shape) == (len(fs), NT, 17)
        for k, f, v in zip(fs.keys, fs.frames, fs.joints.cpu().numpy()):
            assert (k, int(f)) not in got
            got[(k, int(f))] = v
    for tick in ticks:
        assert tick.joint_final is tick.final.joints and len(tick.closed) == 0
        take(tick.final)
    for _, fs in tails:
        take(fs)
    assert scores_ok[0] == NT * n and len(got) == sum(len(f) for _, f in kept)
    compared = zeros = 0
    for k, f in kept:
        for i, fid in enumerate(f):
            for t in range(NT):
                w = want[t * len(kept) + track_of[k], fid - 1]
                assert np.array_equal(_bits(got[(k, int(fid))][t]), _bits(w)), (k, fid, t)
                if i < N_COND:          # no window forecasts the first n_cond rows of a track
                    assert not w.any()
                    zeros += 1
                compared += 1
    assert compared == NT * sum(len(f) for _, f in kept) and zeros == NT * N_COND * len(kept)
    assert (want > 0).sum() > 1000 and len(np.unique(want)) > 1000         # (not a constant: the test can fail)


def _same_tick(a, b, joints=True):
    assert np.array_equal(a.meta, b.meta) and np.array_equal(a.frames, b.frames) and np.array_equal(a.trans, b.trans)
    assert a.first_window_id == b.first_window_id
    assert torch.equal(a.scores, b.scores)
    assert (a.windows is None) == (b.windows is None)
    if a.windows is not None:
        assert torch.equal(a.windows.base, b.windows.base) and torch.equal(a.windows.trans, b.windows.trans)
    for x, y in ((a.final, b.final), (a.closed, b.closed)):
        assert x.keys == y.keys and np.array_equal(x.frames, y.frames) and torch.equal(x.values, y.values)
        if joints:
            assert torch.equal(x.joints, y.joints)
    if joints:
        assert torch.equal(a.joint_final, b.joint_final)
    assert a.clip is None and b.clip is None


def test_push_many_of_three_ticks_equals_push(setup):
    """K = 3 ticks per call on ring_len = seg_len + 2 (groups of up to three ticks) against tick-by-tick pushes: every field, bit
    for bit.  (The draws are the in-kernel ones: keyed by the global window id, the same in both streams.)"""
    m, tracks = setup["model"], setup["tracks"]
    kw = dict(setup["kw"], max_tracks=32, ring_len=SEG_LEN + 2, joint_scores=True, max_idle=3)      # (no explicit close: idle slots)
    a, b = PoseStream(m, **kw), PoseStream(m, **kw)
    feed = [(keys, fids, poses) for _, keys, fids, poses in ticks_by_frame(tracks)]
    ta = [a.push(*t) for t in feed]
    tb = []
    for i in range(0, len(feed), 3):
        tb += b.push_many(feed[i:i + 3])
    assert len(ta) == len(tb) == len(feed)
    for x, y in zip(ta, tb):
        _same_tick(x, y)
    assert sum(len(t.closed) for t in ta) > 0 and sum(len(t.final) for t in ta) > 100        # idle tails and finals both occur
    ca, cb = a.close_all(), b.close_all()
    assert ca.keys == cb.keys and torch.equal(ca.values, cb.values) and torch.equal(ca.joints, cb.joints) and len(ca) > 0
    assert torch.equal(a.rings.joint_scores_ring, b.rings.joint_scores_ring)
    assert torch.equal(a.rings.frame_scores_ring, b.rings.frame_scores_ring) and torch.equal(a.ring, b.ring)


def test_a_reused_slot_starts_clean(setup):
    """One slot, max_idle = 1: track A fills the joint ring, goes idle and is closed; track B takes the slot over.  B's per-joint
    scores are those of a fresh stream that only ever saw B -- no cell of A survives (with given noise, the same for both)."""
    m = setup["model"]
    kw = dict(setup["kw"], max_tracks=1, max_idle=1, ring_len=SEG_LEN + 1)
    S, ns = m.n_generated_samples, m.noise_steps
    raw = stress_rows(3 * SEG_LEN + 6, seed=21)
    gen = torch.Generator().manual_seed(5)
    used, fresh = PoseStream(m, joint_scores=True, **kw), PoseStream(m, joint_scores=True, **kw)
    A, Bk = (1, 1, 1), (1, 1, 2)
    for i in range(SEG_LEN + 3):                       # A: four windows, the ring wraps
        nz = torch.randn(S, ns - 1, NT, 2, 3, 17, generator=gen).to(DEV) if i >= SEG_LEN - 1 else None
        used.push([A], [i + 1], raw[i:i + 1], noise=nz)
    assert float(used.rings.joint_scores_ring.abs().sum()) > 0
    used.push([], [], np.zeros((0, 34), np.float32))   # an empty tick: A is idle
    rows_b = raw[SEG_LEN + 3:]
    ticks = []
    for i in range(len(rows_b)):
        nz = torch.randn(S, ns - 1, NT, 2, 3, 17, generator=gen).to(DEV) if i >= SEG_LEN - 1 else None
        tu = used.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        tf = fresh.push([Bk], [100 + i], rows_b[i:i + 1], noise=nz)
        if i == 0:                                     # A's tail comes back with the tick that closes it, per joint too
            assert tu.closed.keys == [A] * (SEG_LEN - 1) and tuple(tu.closed.joints.shape) == (SEG_LEN - 1, NT, 17)
            assert float(tu.closed.joints.sum()) > 0 and used.table.slot_of[Bk] == 0
        else:
            assert len(tu.closed) == 0
        assert torch.equal(tu.scores, tf.scores) and torch.equal(tu.final.values, tf.final.values)
        assert torch.equal(tu.joint_final, tf.joint_final)
        ticks.append(tu)
    finals = torch.cat([t.joint_final for t in ticks])
    assert finals.shape[0] == len(rows_b) - SEG_LEN + 1 and not finals[:N_COND].any() and (finals[N_COND:] > 0).any()
    cu, cf = used.close([Bk]), fresh.close([Bk])
    assert torch.equal(cu.joints, cf.joints) and torch.equal(cu.values, cf.values) and (cu.joints > 0).any()


def test_off_is_the_stream_without_the_argument(setup):
    """joint_scores=False: every Tick field and both rings are those of a stream built without the argument, no ring is allocated
    and the scorer is asked for no poses (its map buffers stay empty); switching it ON changes none of the existing fields."""
    m, tracks = setup["model"], setup["tracks"]
    sc = m.scorer()
    sc._map_bufs.clear()
    plain = PoseStream(m, ring_len=SEG_LEN, **setup["kw"])
    off = PoseStream(m, ring_len=SEG_LEN, joint_scores=False, **setup["kw"])
    assert off.rings.joint_scores_ring is None and off.rings._jstate is None

    def both(keys, fids, poses, metas):
        tp, to = plain.push(keys, fids, poses), off.push(keys, fids, poses)
        _same_tick(tp, to, joints=False)
        assert to.joint_final is None and to.final.joints is None and to.closed.joints is None
        return tp

    ticks, tails = _replay([plain, off], tracks, both)
    assert sum(len(t.final) for t in ticks) == 283 and not sc._map_bufs
    assert torch.equal(plain.ring, off.ring) and torch.equal(plain.rings.frame_scores_ring, off.rings.frame_scores_ring)
    for _, fs in tails:
        assert fs.joints is None
    on = PoseStream(m, ring_len=SEG_LEN, joint_scores=True, **setup["kw"])
    at = [0]

    def with_joints(keys, fids, poses, metas):
        tn = on.push(keys, fids, poses)
        _same_tick(ticks[at[0]], tn, joints=False)
        assert tn.joint_final is not None and tuple(tn.joint_final.shape) == (len(tn.final), NT, 17)
        at[0] += 1
        return tn

    _replay([on], tracks, with_joints)
    assert at[0] == len(ticks) and sc._map_bufs
    assert torch.equal(plain.ring, on.ring) and torch.equal(plain.rings.frame_scores_ring, on.rings.frame_scores_ring)


def test_latent_model_is_refused(setup):
    class Latent:
        is_latent = True
    with pytest.raises(NotImplementedError, match="a latent has no joints"):
        PoseStream(Latent(), vid_res=VID_RES, joint_scores=True)

"""GPU: WHERE the error-map kernels write -- the entries ABI 15 adds (mcd_error_maps, mcd_joint_scatter_max,
mcd_stream_joint_scores_group, mcd_stream_joint_flush) under the instrument of tests/test_buffer_bounds_gpu.py: every device buffer
the Python layer allocates lies between guard bands with a poisoned interior, inputs the test owns are passed between bands of NaNs
and of finite random floats, and after the call (a) no guard byte changed, (b) no output element was left unwritten, (c) / (d) every
output equals the call outside the region bit for bit.  Shapes: 3 windows x 3 samples (17 .. 51 cells: a partial wave), a stream
with every slot live whose joint ring wraps, through push and through push_many with three ticks per group."""
import numpy as np
import pytest
import torch

import test_buffer_bounds_gpu as BB
from test_buffer_bounds_gpu import DEV, _randn, _scorer, run

pytestmark = pytest.mark.gpu

# tests/test_buffer_bounds_gpu.py ends with an audit: every declaration of include/mocodad_hip.h that writes a caller's buffer
# must be in its list of entries exercised between guard bands.  The four entries of ABI 15 are exercised HERE, with that
# module's own `run`, so this module adds them to that list when it is imported -- at collection, before any test runs.  A session
# that selects the other file without this one reports them as not exercised, which is then the case.
NEW_ENTRIES = ["mcd_error_maps", "mcd_joint_scatter_max", "mcd_stream_joint_scores_group", "mcd_stream_joint_flush"]
BB.COVERED += [e for e in NEW_ENTRIES if e not in BB.COVERED]


@pytest.mark.parametrize("strategy", ["all", "best", "mean", "median", "quantile:0.3", "mean_pose", "median_pose"])
def test_error_maps(strategy):
    sc, data, _ = _scorer("sk_inject6")
    poses, loss = _randn(3, 3, 2, 3, 17, seed=1), _randn(3, 3, seed=2).abs()
    r = run("mcd_error_maps", lambda T, data, loss, poses: {"maps": sc.error_maps(data, loss, poses, strategy)},
            {"data": data, "loss": loss, "poses": poses})
    assert tuple(r["maps"].shape) == ((3, 3, 3, 17) if strategy == "all" else (3, 3, 17)) and torch.isfinite(r["maps"]).all()


def test_error_maps_behind_a_scoring_call():
    """score_fused(want_maps=True): the poses and per-sample losses nobody asked for go to the scorer's own buffers -- guarded too."""
    sc, data, _ = _scorer("sk_inject6")

    def call(T, data):
        sc._map_bufs.clear()          # (a cached buffer would not be a guarded one)
        agg, _, _, maps = sc.score_fused(data, n_samples=3, noise_steps=3, aggregation="best", seed=5, want_maps=True)
        return {"agg": agg, "maps": maps}

    r = run("mcd_error_maps (score_fused want_maps)", call, {"data": data}, [sc])
    sc._map_bufs.clear()
    mean = r["maps"].double().mean(dim=(1, 2))
    assert ((mean - r["agg"].double()).abs() <= 2 * (2 * 3 * 17 + 16) * 2.0 ** -24 * r["agg"].double()).all()


def test_joint_scatter_max():
    """3 rows x 7 frames; frame ids 0, -2, 8 and 100 fall outside 1 .. 7 and are dropped."""
    sc, _, _ = _scorer("sk_inject6")
    frames = torch.tensor([[1, 2, 3], [0, 1, 7], [7, 8, 100], [-2, 4, 5], [5, 6, 7]], dtype=torch.int32)
    row = torch.tensor([0, 1, 2, 0, 2], dtype=torch.int32)
    maps = _randn(5, 3, 17, seed=3)
    r = run("mcd_joint_scatter_max", lambda T, maps: {"out": sc.joint_scatter_max(maps, frames, row, 3, 7)}, {"maps": maps})
    want = np.zeros((3, 7, 17), np.float32)
    for m, fr, ro in zip(maps.numpy(), frames.tolist(), row.tolist()):
        for k, f in enumerate(fr):
            if 1 <= f <= 7:
                want[ro, f - 1] = np.maximum(want[ro, f - 1], np.maximum(m[k], 0))
    assert np.array_equal(r["out"].cpu().numpy(), want)


@pytest.fixture(scope="module")
def stream_env(tmp_path_factory):
    from dataset_spec import load_dataset_golden
    from test_stream_many_gpu import _model
    g = load_dataset_golden()
    return g, _model(tmp_path_factory.mktemp("maps_bounds"), g)[0]


def _replay(g, model, ring_len, how):
    """3 tracks on a stream of exactly 3 slots, 2 ring_len + seg_len frames: every position of the joint ring is written and the
    ring wraps; then everything is closed (mcd_stream_joint_flush)."""
    from mocodad_amd.stream import PoseStream
    from test_stream_many_gpu import SEG_LEN, VID_RES
    model.scorer()._map_bufs.clear()
    st = PoseStream(model, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=3, ring_len=ring_len,
                    joint_scores=True)
    keys = [(1, 1, 1), (1, 1, 2), (1, 2, 1)]
    rng = np.random.default_rng(7)
    ticks = [(keys, [f + 1] * 3, rng.uniform(20, 300, (3, 34)).astype(np.float32)) for f in range(2 * ring_len + SEG_LEN)]
    res = []
    if how == "push":
        res = [st.push(*t) for t in ticks]
    else:
        for lo in range(0, len(ticks), 3):
            res += st.push_many(ticks[lo:lo + 3])
    out = {}
    for i, t in enumerate(res):
        out[f"scores{i}"], out[f"final{i}"], out[f"joint{i}"] = t.scores, t.final.values, t.joint_final
    assert sorted(st.table.slot_of.values()) == [0, 1, 2], "every slot, the last included, is live"
    tails = st.close_all()
    out.update(tails=tails.values, joint_tails=tails.joints, ring=st.ring, frame_scores_ring=st.rings.frame_scores_ring,
               joint_scores_ring=st.rings.joint_scores_ring)
    return out


@pytest.mark.parametrize("how", ["push", "push_many3"])
@pytest.mark.parametrize("extra", [0, 2], ids=["L6", "L8"])
def test_stream_replay_with_joint_scores(stream_env, extra, how):
    from test_stream_many_gpu import SEG_LEN
    g, model = stream_env
    r = run("mcd_stream_joint_scores_group + joint_flush" + (" (PoseStream.push)" if how == "push" else ""),
            lambda T: _replay(g, model, SEG_LEN + extra, how), None, [model.scorer()], partial=["ring", "frame_scores_ring", "joint_scores_ring"])
    model.scorer()._map_bufs.clear()
    assert tuple(r["joint_scores_ring"].shape) == (3, 5, SEG_LEN + extra, 17) and bool((r["joint_scores_ring"] > 0).any())
    assert tuple(r["joint_tails"].shape) == (3 * (SEG_LEN - 1), 5, 17) and bool((r["joint_tails"] > 0).any())


def test_the_new_entries_were_exercised_here():
    """What the audit's list is told above is true: each new entry saw guarded allocations under `run` in this module."""
    ran = " ".join(BB.ALLOC)
    for e in NEW_ENTRIES:
        assert e.replace("mcd_stream_", "") in ran or e in ran, (e, sorted(BB.ALLOC))

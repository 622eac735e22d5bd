"""GPU: WHERE the launches of mcd_latent_score_pose write -- a pose-space stream of the latent model with joint scores and forecasts
on, under the instrument of tests/test_buffer_bounds_gpu.py: every device buffer the Python layer allocates (the call's one
workspace with its five regions, the aggregated and per-sample losses, the poses, the error maps, the rings, the outputs of every
tick and of every close) lies between guard bands with a poisoned interior, and after the calls (a) no guard byte changed, (b) no
output element was left unwritten, (c) every output equals the call outside the region bit for bit.  Shapes as
tests/test_stream_forecast_bounds_gpu.py: 1, 5 and 65 emitting tracks (x 5 transforms = 5, 25, 325 windows: a partial two-window
workgroup of the 3-frame rows at 5 and 325, eleven 32-row tiles of the unproject launch with a partial last one at 325 x 2 samples);
one `push`, one `push_many` group of three ticks whose last tick emits no window, one more tick without a window, then the close
of everything."""
import numpy as np
import pytest
import torch

import test_buffer_bounds_gpu as BB
from test_buffer_bounds_gpu import run

pytestmark = pytest.mark.gpu

# tests/test_buffer_bounds_gpu.py ends with an audit: every declaration of include/mocodad_hip.h that writes a caller's buffer must be
# in its list of entries exercised between guard bands.  The new entry is exercised HERE, with that module's own `run`, so this
# module adds it to that list when it is imported -- at collection, before any test runs.
NEW_ENTRIES = ["mcd_latent_score_pose"]
BB.COVERED += [e for e in NEW_ENTRIES if e not in BB.COVERED]
FIELDS = ("expected", "expected_norm", "observed", "count", "spread")
ENTRY = "mcd_latent_score_pose (pose-space stream)"


@pytest.fixture(scope="module")
def stream_env(tmp_path_factory):
    from dataset_spec import load_dataset_golden
    from test_stream_latent_pose_gpu import pose_model
    g = load_dataset_golden()
    return g, pose_model(tmp_path_factory.mktemp("latent_pose_bounds"), g)[0]


def _replay(g, model, n):
    from mocodad_amd.stream import ForecastCfg, PoseStream
    from test_stream_latent_gpu import SEG_LEN, VID_RES
    st = PoseStream(model, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=n + 2, ring_len=SEG_LEN + 2,
                    joint_scores=True, forecasts=ForecastCfg("median", "median"), space="pose")
    keys = [(1, 1 + i // 16, i) for i in range(n)]
    rng = np.random.default_rng(7)
    rows = lambda k: rng.uniform(20, 300, (k, 34)).astype(np.float32)
    res = [st.push(keys, [f + 1] * n, rows(n)) for f in range(SEG_LEN - 1)]           # no window yet: the raw rows only
    res.append(st.push(keys, [SEG_LEN] * n, rows(n)))                                   # one push: n windows
    late, later = (9, 9, 1), (9, 9, 2)
    res += st.push_many([(keys, [SEG_LEN + 1] * n, rows(n)), (keys, [SEG_LEN + 2] * n, rows(n)),
                         ([late], [1], rows(1))])                                       # one group; its final tick emits no window
    res.append(st.push([later], [1], rows(1)))                                          # a tick of its own without a window
    assert [len(t.final) for t in res] == [0] * (SEG_LEN - 1) + [n, n, n, 0, 0]
    out = {}
    for i, t in enumerate(res):
        assert len(t.forecast) == len(t.final) == len(t.joint_final)
        out[f"scores{i}"], out[f"final{i}"], out[f"joints{i}"] = t.scores, t.final.values, t.joint_final
        for name in FIELDS:
            out[f"{name}{i}"] = getattr(t.forecast, name)
    tails = st.close_all()
    assert len(tails) == n * (SEG_LEN - 1) == len(tails.forecast)
    out["tails"], out["tail_joints"] = tails.values, tails.joints
    for name in FIELDS:
        out[f"tail_{name}"] = getattr(tails.forecast, name)
    out.update(ring=st.ring, frame_scores_ring=st.rings.frame_scores_ring, forecast_ring=st.rings.forecast_ring,
               observed_ring=st.rings.observed_ring, joint_scores_ring=st.rings.joint_scores_ring)
    return out


@pytest.mark.parametrize("n", [1, 5, 65])
def test_pose_space_stream_replay_between_guard_bands(stream_env, n):
    from test_stream_latent_gpu import SEG_LEN
    g, model = stream_env
    ps = model.pose_scorer()
    r = run(ENTRY, lambda T: _replay(g, model, n), None, [ps, model.scorer(), model.decoder()],
            partial=["ring", "frame_scores_ring", "forecast_ring", "observed_ring", "joint_scores_ring"])
    assert tuple(r["forecast_ring"].shape) == (n + 2, SEG_LEN + 2, 3, 34) and bool((r["forecast_ring"][:n] != 0).any())
    assert bool((r["joint_scores_ring"][:n] != 0).any())
    for i in range(SEG_LEN - 1, SEG_LEN + 2):
        assert torch.isfinite(r[f"scores{i}"]).all() and r[f"scores{i}"].numel() == 5 * n and bool((r[f"scores{i}"] > 0).all())
    counts = torch.cat([torch.stack([r[f"count{i}"] for i in range(SEG_LEN - 1, SEG_LEN + 2)]), r["tail_count"].view(n, SEG_LEN - 1).T])
    assert counts[:, 0].tolist() == [0, 0, 0, 1, 2, 3, 2, 1] and bool((counts == counts[:, :1]).all())
    # the call's workspace went through the proxy: the LatentPoseScorer allocates it, not the two handles' scorers
    assert any("_workspace" in a for a in BB.ALLOC[ENTRY]), BB.ALLOC[ENTRY]


@pytest.mark.parametrize("B,S", [(1, 1), (3, 3), (33, 2)], ids=["B1S1", "B3S3", "B33S2"])
def test_the_call_alone_with_every_output(stream_env, B, S):
    """LatentPoseScorer.score with all six outputs on dense windows passed between NaN and between finite bands, parity and perf mode"""
    import latentp_ref as R
    _, model = stream_env
    ps = model.pose_scorer()
    ns, D = model.noise_steps, model.latent_embedding_dim
    data = R.windows(B, 6, 500 + B)
    noise = torch.randn(S, ns - 1, B, D, generator=torch.Generator().manual_seed(41))

    def call(T, data, noise=None):
        out = T.empty(B, device=BB.DEV, dtype=torch.float32)
        r = ps.score(data, n_samples=S, noise_steps=ns, aggregation="best", noise=noise, seed=3, first_window_id=17, out=out, want_all=True,
                     want_poses=True, want_maps=True, want_selected=True, want_latents=True)
        assert r[0] is out
        return dict(zip(("loss_agg", "loss_all", "pose_all", "maps", "pose_agg", "latent_all"), r))

    for parity in (False, True):
        r = run("mcd_latent_score_pose", call, {"data": data, **({"noise": noise} if parity else {})}, [ps])
        assert tuple(r["pose_all"].shape) == (B, S, 2, 3, 17) and torch.isfinite(r["loss_all"]).all()
        assert torch.equal(r["loss_agg"], r["loss_all"].min(1).values)


def test_the_new_entry_was_exercised_here():
    """What the audit's list is told above is true: the new entry saw guarded allocations under `run` in this module."""
    for e in NEW_ENTRIES:
        assert any(k.startswith(e) and BB.ALLOC[k] for k in BB.ALLOC), (e, sorted(BB.ALLOC))

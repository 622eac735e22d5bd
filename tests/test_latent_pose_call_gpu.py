"""GPU: mcd_latent_score_pose (engine.LatentPoseScorer.score) against the sequence of four entries it replaces --
LatentScorer.score('all', want_latents, want_cond) -> LatentReconstructor.decode_samples -> aggregate -> error_maps -- bit for bit on
every output.  The call makes the launches of those entries in their order, none of which depends on its batch, its chunking or its
sample split (tests/test_latent_gpu.py, tests/test_latent_forecast_gpu.py), so every comparison is torch.equal: there is no tolerance.

Shapes: 3 + 3 and 6 + 6 frames (the second takes the project / unproject launches, one window per workgroup); B = 1 (a partial
two-window workgroup of the 3-frame rows), 2 and 33 (one past the 32-window tile of project / unproject); S = 1, 2 and 5 (the sample
split over workgroups occurs at the small B); dense windows and a WindowBatch view with transforms; a given noise tensor and the
in-kernel draws with first_window_id != 0; the five loss aggregations.  D = 32, noise_steps 4, seeded random-init models whose
stage-1 state dict shares the frozen tensors (as tests/test_latent_forecast_host.py builds one)."""
import ctypes as C
import itertools

import pytest
import torch

import latent_ref as LR
import latentp_ref as R
from helpers import make_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, D, SEED, FIRST = 4, 32, 5, 1000
AGGRS = ["best", "worst", "mean", "median", "quantile:0.3"]
_pairs = {}


def pair(t):
    """-> (MoCoDADlatent of t + t frames on the device with its decoder loaded, LatentScorer, LatentReconstructor, LatentPoseScorer),
    once per session; the module is this file's own (its seed is used nowhere else)"""
    if t not in _pairs:
        from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
        over = {} if t == 3 else dict(seg_len=2 * t, conditioning_indices=list(range(t)))
        m, _ = LR.random_latent_model(D, [48, D], seed=140 + t, ns=NS, S=2, tame=True, **over)
        cfg = LR.load_fixture("B")[2]
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(150 + t)
            sd = {k: v.detach().clone() for k, v in
                  MoCoDADlatentPretrain(make_args(cfg, stage="pretrain", latent_embedding_dim=D, **over)).state_dict().items()}
        sd.update({k: v.detach().clone() for k, v in m.state_dict().items() if k in sd})
        m = m.to(DEV)
        m.load_decoder(sd)
        _pairs[t] = (m, m.scorer(), m.decoder(), m.pose_scorer())
        assert len(_pairs[t][1].corrupt_idx) == t and _pairs[t][1].seg_len == 2 * t
    return _pairs[t]


def windows(t, B, view):
    """dense (B,2,2t,17) windows, or a WindowBatch of stride-1 windows over one buffer with the five test-time transforms"""
    if not view:
        return R.windows(B, 2 * t, 300 + B).to(DEV)
    from mocodad_amd.data.windows import WindowBatch
    from mocodad_amd.utils.transforms import affine_table
    buf = torch.randn((B + 2 * t - 1) * 34, generator=torch.Generator().manual_seed(400 + B)).to(DEV)
    base = (torch.arange(B, dtype=torch.int64) * 34).to(DEV)
    return WindowBatch(buf, base, (torch.arange(B, dtype=torch.int32) % 5).to(DEV), affine_table(5).to(DEV), 2 * t)


def sequence(sc, dec, data, S, kw):
    """the first two entries of the sequence -> (latents, poses_all, loss_all), each a copy"""
    _, _, lat, _, cond = sc.score(data, n_samples=S, noise_steps=NS, aggregation="all", want_latents=True, want_cond=True, **kw)
    poses, loss_all = dec.decode_samples(data, lat, cond, want_poses=True, loss_fn=kw["loss_fn"])
    return lat.clone(), poses.clone(), loss_all.clone()


def rest(dec, data, poses, loss_all, aggr, fn):
    """... and the last two under one aggregation -> (loss_agg, selected pose | None, maps)"""
    sel, agg = dec.aggregate(data if torch.is_tensor(data) else None, loss_all, poses, aggr, noise_steps=NS, loss_fn=fn)
    return agg, sel, dec.error_maps(data, loss_all, poses, aggr, loss_fn=fn)


def noise_kw(given, B, S, fn="smooth_l1"):
    if given:
        g = torch.Generator().manual_seed(77 + B + S)
        return dict(noise=torch.randn(S, NS - 1, B, D, generator=g).to(DEV), seed=0, first_window_id=0, loss_fn=fn)
    return dict(noise=None, seed=SEED, first_window_id=FIRST, loss_fn=fn)


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 2, 33])
@pytest.mark.parametrize("t", [3, 6])
def test_every_output_is_the_sequences_bit_for_bit(t, B, S):
    _, sc, dec, ps = pair(t)
    compared = 0
    for view, given in itertools.product((False, True), (True, False)):
        data = windows(t, B, view)
        kw = noise_kw(given, B, S)
        lat, poses, loss_all = sequence(sc, dec, data, S, kw)
        assert tuple(poses.shape) == (B, S, 2, t, 17) and torch.isfinite(loss_all).all() and torch.isfinite(poses).all()
        for aggr in AGGRS:
            agg, sel, maps = rest(dec, data, poses, loss_all, aggr, kw["loss_fn"])
            r = ps.score(data, n_samples=S, noise_steps=NS, aggregation=aggr, want_all=True, want_poses=True, want_maps=True,
                         want_selected=True, want_latents=True, **kw)
            assert torch.equal(r[0], agg), (aggr, view, given)
            assert torch.equal(r[1], loss_all) and torch.equal(r[2], poses) and torch.equal(r[5], lat), (aggr, view, given)
            assert tuple(maps.shape) == (B, t, 17) and torch.equal(r[3], maps), (aggr, view, given)
            if aggr in ("best", "worst"):
                assert sel is not None and torch.equal(r[4], sel), (aggr, view, given)
            else:
                assert sel is None and r[4] is None
            compared += 1
        if S > 1:       # (not a constant: the aggregations differ, so the comparison can fail)
            assert not torch.equal(rest(dec, data, poses, loss_all, "best", "smooth_l1")[0], rest(dec, data, poses, loss_all, "worst", "smooth_l1")[0])
    assert compared == 4 * len(AGGRS)


def test_the_in_kernel_draws_are_keyed_by_the_window_id():
    """first_window_id moves the draws, and a batch split at b0 with first_window_id + b0 gives the same windows the same bits"""
    _, _, _, ps = pair(3)
    data = windows(3, 5, False)
    kw = dict(n_samples=2, noise_steps=NS, aggregation="best", want_all=True, seed=SEED)
    a = ps.score(data, first_window_id=FIRST, **kw)[1].clone()
    b = ps.score(data, first_window_id=FIRST + 1, **kw)[1].clone()
    assert not torch.equal(a, b)
    tail = ps.score(data[2:].contiguous(), first_window_id=FIRST + 2, **kw)[1]
    assert torch.equal(tail, a[2:])


@pytest.mark.parametrize("loss_fn", ["l1", "mse"])
def test_the_other_loss_functions(loss_fn):
    _, sc, dec, ps = pair(6)
    data, kw = windows(6, 3, True), noise_kw(False, 3, 2, loss_fn)
    lat, poses, loss_all = sequence(sc, dec, data, 2, kw)
    agg, sel, maps = rest(dec, data, poses, loss_all, "median", loss_fn)
    r = ps.score(data, n_samples=2, noise_steps=NS, aggregation="median", want_all=True, want_maps=True, **kw)
    assert torch.equal(r[0], agg) and torch.equal(r[1], loss_all) and torch.equal(r[3], maps)


@pytest.mark.parametrize("t,B,S", [(3, 2, 5), (6, 33, 2)])
def test_every_combination_of_optional_outputs(t, B, S):
    """Which optional outputs are NULL decides where loss_all, the latents and pose_all live (the caller's buffer or the workspace) and
    whether the decode launches write poses at all: no combination changes a bit of what is returned."""
    _, sc, dec, ps = pair(t)
    data, kw = windows(t, B, False), noise_kw(True, B, S)
    lat, poses, loss_all = sequence(sc, dec, data, S, kw)
    agg, sel, maps = rest(dec, data, poses, loss_all, "worst", "smooth_l1")
    want = dict(want_all=loss_all, want_poses=poses, want_maps=maps, want_selected=sel, want_latents=lat)
    names = list(want)
    for flags in itertools.product((False, True), repeat=len(names)):
        on = dict(zip(names, flags))
        r = ps.score(data, n_samples=S, noise_steps=NS, aggregation="worst", **on, **kw)
        assert len(r) == 4 + on["want_selected"] + on["want_latents"]
        assert torch.equal(r[0], agg), on
        got = dict(want_all=r[1], want_poses=r[2], want_maps=r[3], want_selected=r[4] if on["want_selected"] else None,
                   want_latents=r[-1] if on["want_latents"] else None)
        for n in names:
            assert (got[n] is None) if not on[n] else torch.equal(got[n], want[n]), (n, on)
    out = torch.full((B,), -7.0, device=DEV)
    r = ps.score(data, n_samples=S, noise_steps=NS, aggregation="worst", out=out, **kw)
    assert r[0] is out and torch.equal(out, agg)


@pytest.mark.parametrize("t", [3, 6])
def test_a_nan_window_changes_no_bit_of_another(t):
    _, _, _, ps = pair(t)
    data, kw = windows(t, 5, False), noise_kw(True, 5, 2)
    call = lambda d: [x.clone() for x in ps.score(d, n_samples=2, noise_steps=NS, aggregation="best", want_all=True, want_poses=True,
                                                  want_maps=True, want_selected=True, want_latents=True, **kw)]
    clean = call(data)
    bad = data.clone()
    bad[2, 0, t + 1, 4] = float("nan")      # a corrupt frame of window 2
    got = call(bad)
    keep = [0, 1, 3, 4]
    assert not torch.isfinite(got[1][2]).any()
    for a, b in zip(got, clean):
        assert torch.equal(a[keep], b[keep])
    for a, b in zip(call(data), clean):       # the call after starts clean
        assert torch.equal(a, b)


def test_no_windows():
    _, _, _, ps = pair(3)
    r = ps.score(torch.empty(0, 2, 6, 17), n_samples=2, noise_steps=NS, aggregation="mean", want_all=True, want_poses=True, want_maps=True)
    assert [tuple(x.shape) for x in r] == [(0,), (0, 2), (0, 2, 2, 3, 17), (0, 3, 17)]


def test_workspace_query():
    m, sc, dec, ps = pair(6)
    q = lambda B, S: int(ps.L.mcd_latent_pose_workspace_bytes(sc._h, dec._h, B, S))
    r256 = lambda n: (n + 255) // 256 * 256
    for B, S in ((1, 1), (33, 5)):
        parts = (int(sc.L.mcd_latent_workspace_bytes(sc._h, B)), B * S * 4, B * S * D * 4, B * S * 2 * 6 * 17 * 4,
                 int(dec.L.mcd_latent_decode_workspace_bytes(dec._h, B, S)))
        assert q(B, S) == sum(r256(p) for p in parts)
    assert q(0, 2) == 0 and q(2, 0) == 0 and q(2, 1025) == 0
    assert int(ps.L.mcd_latent_pose_workspace_bytes(dec._h, sc._h, 2, 2)) == 0 and int(ps.L.mcd_latent_pose_workspace_bytes(sc._h, sc._h, 2, 2)) == 0


def test_mismatched_or_swapped_handles_are_refused_by_name_with_no_launch():
    """Every refusal comes before the first launch: the outputs (real device buffers, prefilled) keep their fill."""
    from mocodad_amd import _lib
    from mocodad_amd.engine import LatentPoseScorer, LatentReconstructor
    m3, sc3, dec3, ps3 = pair(3)
    _, sc6, dec6, _ = pair(6)
    other = R.random_ae_model(3, 3, 48, seed=961)[0].to(DEV).scorer()      # an autoencoder of another latent size
    assert isinstance(other, LatentReconstructor) and other.latent_dim == 48
    L = sc3.L
    B, S = 2, 2
    data = windows(3, B, False)
    tab = sc3.table(NS)
    ws = torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    outs = {k: torch.full(shape, -7.0, device=DEV) for k, shape in
            dict(agg=(B,), loss=(B, S), poses=(B, S, 2, 3, 17), sel=(B, 2, 3, 17), maps=(B, 3, 17), lat=(B, S, D + 4)).items()}
    noise = torch.zeros(S * (NS - 1) * B * D + 4, device=DEV)
    err = lambda: L.mcd_last_error().decode()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(w, ae, cfg=None, workspace=None, aggr="best", lat_off=0, noise_p=None, view=None, sel=True):
        cfg = sc3._score_cfg(B, S, NS) if cfg is None else cfg
        return L.mcd_latent_score_pose(w, ae, C.byref(cfg), P(data), view, noise_p, 0, 0, P(tab), P(ws) if workspace is None else workspace,
                                       _lib.AGGR[aggr], C.c_float(0.3), P(outs["agg"]), P(outs["loss"]), P(outs["poses"]),
                                       P(outs["sel"]) if sel else None, P(outs["maps"]), P(outs["lat"], lat_off), None)

    assert call(dec3._h, sc3._h) == -4 and "diffusion-stage handle" in err() and "first" in err()
    assert call(dec3._h, dec3._h) == -4 and "diffusion-stage handle" in err()
    assert call(sc3._h, sc3._h) == -4 and "autoencoder handle" in err() and "second" in err()
    assert call(sc3._h, dec6._h) == -1 and "frame split" in err()
    assert call(sc6._h, dec3._h) == -1 and "frame split" in err()
    assert call(sc3._h, other._h) == -1 and "latent_dim" in err()
    assert call(sc3._h, dec3._h, workspace=P(ws, 4)) == -1 and "workspace must be 16-byte aligned" in err()
    assert call(sc3._h, dec3._h, workspace=C.c_void_p(0)) == -1 and "workspace" in err()
    assert call(sc3._h, dec3._h, lat_off=4) == -1 and "latent_all must be 16-byte aligned" in err()
    assert call(sc3._h, dec3._h, noise_p=P(noise, 4)) == -1 and "noise must be 16-byte aligned" in err()
    assert call(sc3._h, dec3._h, aggr="mean_pose") == -1 and "aggregates losses" in err()
    assert call(sc3._h, dec3._h, aggr="all") == -1 and "aggregates losses" in err()
    assert call(sc3._h, dec3._h, aggr="mean") == -1 and "pose_agg" in err()
    assert call(sc3._h, dec3._h, cfg=sc3._score_cfg(B, 0, NS)) == -1 and "n_samples" in err()
    assert call(sc3._h, dec3._h, cfg=sc3._score_cfg(B, 1025, NS)) == -4 and "n_samples" in err()
    assert call(sc3._h, dec3._h, cfg=sc6._score_cfg(B, S, NS)) == -1 and "frame split" in err()
    bad = sc3._score_cfg(B, S, NS)
    bad.corrupt_idx[1] = 9
    assert call(sc3._h, dec3._h, cfg=bad) == -1 and "corrupt_idx" in err()
    mask = torch.zeros(B, device=DEV, dtype=torch.int32)
    view = _lib.WindowView(base=None, stride_c=0, stride_t=0, trans=None, affine=None, cond_mask=mask.data_ptr())
    assert call(sc3._h, dec3._h, view=C.byref(view)) == -1 and "cond_mask" in err()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == -7.0).all()), f"{k} was written by a refused call"
    assert call(sc3._h, dec3._h, aggr="mean", sel=False) == 0       # ... and the same buffers, accepted, are written
    torch.cuda.synchronize()
    assert bool((outs["agg"] != -7.0).all()) and bool((outs["maps"] != -7.0).all())
    with pytest.raises(ValueError, match="differ in seg_len"):
        LatentPoseScorer(sc3, dec6)
    with pytest.raises(ValueError, match="differ in latent_dim"):
        LatentPoseScorer(sc3, other)
    with pytest.raises(TypeError):
        LatentPoseScorer(dec3, sc3)
    assert m3.pose_scorer() is ps3                                    # built once

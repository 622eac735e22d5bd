"""GPU: WHERE the kernels write.  Every call below is made through mocodad_amd.engine / mocodad_amd.stream inside
guarded.guarded(): each device buffer those modules allocate lies between two guard bands of at least 4096 bytes, and an `empty`
one starts full of the all-ones pattern (tests/guarded.py).  After the call and a synchronize:

  (a) every guard byte of every buffer is untouched (GuardedTorch.check);
  (b) no element of an output whose contract is "every element is written" still holds the all-ones pattern -- every output
      below except the workspaces, the staging buffer and the stream / clip rings;
  (c) every output equals, bit for bit, that of the same call made outside the region;
  (d) inputs the test owns (dense windows, window-view buffers, noise, cond, x, emb, skip, loss_all / poses_all, raw pose rows)
      are passed once between bands of all-ones NaNs and once between bands of finite random floats (guarded_copy): the outputs
      of both equal (c)'s, so no result depends on memory outside its inputs.

Shapes: the smallest with a partial workgroup, a clamped slot, a tile edge or a launch tail -- 1 and 3 windows x 1 and 3 samples
(nine chains: the last workgroup is partial at 2 and at 4 chains per workgroup), 5 rows for the single passes and encoders, 33
windows on the 32-window projection tile, 64 / 65 / 8193 samples round the aggregation's LDS limits, 255 / 256 / 257 pose rows,
streams with every slot live whose rings wrap.  Seeded random-init models (tests/test_chain_bits_gpu.py) and the latent fixtures.

177 cases; the module runs in 4.2 s on the MI355X (6.2 s with tests/test_call_errors_gpu.py beside it), no case above 1 s.

Guarded allocations seen per entry, from the proxy's registry (the last test prints the full list with line numbers):
  mcd_score_view          _score: loss (B,S), poses (B,S,2,Tx,17) for Tx = 3, 7, 9, 12, 15, 27; _workspace 768 B .. 5.9 MB
  mcd_score_fused         the test's out (B,); _score: loss (B,S); _workspace as above
  mcd_score               (direct ctypes call: the engine calls mcd_score_view) the test's loss, poses and workspace
  mcd_unet_forward        unet_forward: empty_like x at 3, 7, 13, 32 frames; _pass_workspace at 13 and 32 frames
  mcd_layer_forward       layer_forward: out of every stage at 3 and at 13 frames; _pass_workspace at 13 frames
  mcd_cond_encode         cond_encode: (5,16)   (no scratch: the entry is given the condition frames alone; the gather scratch of
                          a runtime channel list is part of a scoring call's workspace, covered by that model's mcd_score_view call)
  mcd_aggregate[_view]    _out_vector (3,); aggregate: pose (3,2,3,17)
  mcd_philox_noise        philox_noise (2,2,3,2,3,17) and (2,2,3,2,13,17);  mcd_latent_philox_noise: philox_noise (2,2,3,32)
  mcd_random_imp_masks    random_imp_masks (3,) int32
  mcd_latent_encode       encode: cond (B,16), z0 (B,D)    (H and the gather buffer of this entry come from the stream-ordered
                          allocator inside the library: not guarded here, guarded as workspace regions under mcd_latent_score)
  mcd_latent_denoise      denoise: empty_like x (B,D)
  mcd_latent_score        the test's out (B,); score: loss (B,2), latents (B,2,D), code (B,D); _workspace 512 B .. 513 536 B
  mcd_normalize_poses     normalize_poses (n,2,17);  mcd_scatter_max: scatter_max (3,7)
  mcd_frame_scores        FrameScoreAssembler.__call__: workspace (384,) uint8, out (15,) float64
  mcd_stream_push_group, _frame_scores_group, _flush     (through PoseStream.push, a group of one tick, and push_many)
                          StreamRings.__init__: zeros ring (3*2*L*34,), zeros frame_scores (3,5,L); PoseStream.__init__: staging
                          int32; _run_group: scores; StreamRings.push_group: base int64, trans int32;
                          frame_scores_group: final (n,5); flush: (n*5,5); the scorer's _workspace
  mcd_stream_clip_update, _clip_emit
                          ClipRings.__init__: zeros sum, lmax, lmin (2,5,90|92) float64, n int32; emit: (n_out,) float64

Findings: none.  No guard byte changed, no output element was left unwritten, and no output depended on the bands round its
inputs, in any case; the sensitivity test shows the instrument fires (136 of 136 and 2448 of 2448 bytes of the row past the
end, minus float bytes that happen to equal the guard byte).  No kernel or launch was changed.
"""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_chain_bits_gpu as CB  # noqa: E402
from guarded import GuardViolation, guarded, guarded_copy, unwritten  # noqa: E402
from helpers import golden_weights, make_args  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, SEED, FIRST = CB.NS, CB.SEED, CB.FIRST
T0 = time.time()
ALLOC = {}      # C entry (or group of entries) -> the guarded allocations seen under it, in first-seen order
_cache = {}

# the other score_kernel rows: no_condition at 7 and at 12 frames
POSE = dict(CB.POSE, sk_nocond7=("no_condition", 7, None, "AE", 0, None), sk_nocond12=("no_condition", 12, None, "AE", 0, None))


def _scorer(name):
    """-> (HipScorer, windows (3, 2, seg_len, 17), (3,) int32 masks | None), one handle per name for the module"""
    if name not in _cache:
        strategy, seg_len, ci, arch, generic, sets = POSE[name]
        m, data = CB._pose_model(strategy, seg_len, tuple(ci) if isinstance(ci, list) else ci, arch)
        sc = m.build_scorer(torch.device(DEV))
        if generic:
            sc.set_option("generic_unet", 1)
        _cache[name] = (sc, data, None if sets is None else CB._mask32(sets))
    return _cache[name]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _raw(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu() if t.numel() else torch.empty(0, dtype=torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_raw(a), _raw(b))


def run(entry, call, inputs=None, scorers=(), partial=(), options=None):
    """call(T, **inputs) -> {output name: device tensor}; T is the module to allocate caller-owned outputs with (torch outside the
    region, the proxy inside).  Asserts (a) .. (d); returns the outputs of the call outside the region."""
    inputs = {k: v.to(DEV) for k, v in (inputs or {}).items()}
    ref = {k: v.clone() for k, v in call(torch, **inputs).items()}
    torch.cuda.synchronize()
    for fill in (("nan", "finite") if inputs else (None,)):
        with guarded(**(options or {})) as g:
            for sc in scorers:
                sc._ws.clear()          # (the scorer's cached workspace is not a guarded one)
            out = call(g, **{k: guarded_copy(v, fill, seed=i) for i, (k, v) in enumerate(inputs.items())})
            torch.cuda.synchronize()
            seen = ALLOC.setdefault(entry, [])
            seen += [a for a in dict.fromkeys(g.allocations()) if a not in seen]
            assert g.registry, f"{entry}: no allocation went through the proxy"
            g.check()                                                                                    # (a)
            assert sorted(out) == sorted(ref)
            for name, t in out.items():
                if name not in partial:
                    assert unwritten(t) == 0, f"{entry} {name} ({fill}): {unwritten(t)} of {t.numel()} elements never written"   # (b)
                assert _same(t, ref[name]), f"{entry} {name}: differs from the call outside the region (input bands: {fill})"    # (c), (d)
        for sc in scorers:
            sc._ws.clear()
    return ref


# ------------------------------------------------------------------------------------------------ trajectories
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("bs", [(1, 1), (3, 3)], ids=["B1S1", "B3S3"])
@pytest.mark.parametrize("name", list(POSE))
def test_trajectory_calls(name, bs, split):
    """mcd_score_view (score with want_poses) and mcd_score_fused with the caller's out= ('median', want_all), perf mode and
    parity mode with a guarded noise tensor."""
    sc, data, mask = _scorer(name)
    B, S = bs
    data, Tx = data[:B], len(sc.corrupt_idx)
    mask = None if mask is None else mask[:B].to(DEV)
    noise = _randn(S, NS - 1, B, 2, Tx, 17, seed=41)
    kw = dict(n_samples=S, noise_steps=NS, seed=SEED, first_window_id=FIRST, cond_mask=mask)

    def view_call(T, data, noise=None):
        loss, poses = sc.score(data, noise=noise, want_poses=True, **kw)
        return {"loss_out": loss, "pose_out": poses}

    def fused_call(T, data, noise=None):
        out = T.empty(B, device=DEV, dtype=torch.float32)
        agg, loss, _ = sc.score_fused(data, noise=noise, aggregation="median", want_all=True, out=out, **kw)
        assert agg is out
        return {"loss_agg": out, "loss_all": loss}

    sc.set_option("split", split)
    try:
        for parity in (False, True):
            inputs = {"data": data, **({"noise": noise} if parity else {})}
            r = run("mcd_score_view", view_call, inputs, [sc])
            assert tuple(r["loss_out"].shape) == (B, S) and tuple(r["pose_out"].shape) == (B, S, 2, Tx, 17)
            assert torch.isfinite(r["loss_out"]).all() and torch.isfinite(r["pose_out"]).all()
            f = run("mcd_score_fused", fused_call, inputs, [sc])
            assert torch.equal(f["loss_all"], r["loss_out"]) and torch.equal(f["loss_agg"], r["loss_out"].median(1).values)
    finally:
        sc.set_option("split", 0)


@pytest.mark.parametrize("name", list(POSE))
def test_trajectory_calls_on_a_window_view(name):
    """Windows read in place from a buffer whose first window starts at element 0 and whose last window ends at its last
    element (stride-1 windows over B + seg_len - 1 frames): the loader's clamped slots must not read past either end."""
    from mocodad_amd.data.windows import WindowBatch
    sc, _, mask = _scorer(name)
    B, S, T = 3, 3, sc.seg_len
    mask = None if mask is None else mask.to(DEV)
    buf = _randn((B + T - 1) * 34, seed=43)
    base = (torch.arange(B, dtype=torch.int64) * 34).to(DEV)

    def call(T_, buffer):
        loss, poses = sc.score(WindowBatch(buffer, base, None, None, T), n_samples=S, noise_steps=NS, seed=SEED, first_window_id=FIRST,
                               want_poses=True, cond_mask=mask)
        return {"loss_out": loss, "pose_out": poses}

    r = run("mcd_score_view", call, {"buffer": buf}, [sc])
    dense = buf.view(B + T - 1, 2, 17).unfold(0, T, 1).permute(0, 1, 3, 2).contiguous()       # (B, 2, T, 17)
    loss, poses = sc.score(dense, n_samples=S, noise_steps=NS, seed=SEED, first_window_id=FIRST, want_poses=True, cond_mask=mask)
    assert torch.equal(loss, r["loss_out"]) and torch.equal(poses, r["pose_out"])


def test_mcd_score_the_entry_without_a_view():
    """mcd_score is not reached through the engine (which calls mcd_score_view): a direct call on buffers from the proxy."""
    from test_call_errors_gpu import _ptr, make_cfg
    from test_call_layout_gpu import _Of
    sc, data, _ = _scorer("sk_inject6")
    B, S = 3, 3
    cfg = make_cfg(_Of(sc), B=B, S=S, ns=NS)
    need = int(sc.L.mcd_score_workspace_bytes(sc._h, C.byref(cfg)))
    table = sc.table(NS)

    def call(T, data):
        loss = T.empty(B, S, device=DEV, dtype=torch.float32)
        poses = T.empty(B, S, 2, 3, 17, device=DEV, dtype=torch.float32)
        ws = T.empty(max(need, 256), device=DEV, dtype=torch.uint8)
        rc = sc.L.mcd_score(sc._h, C.byref(cfg), _ptr(data), None, SEED, FIRST, _ptr(table), _ptr(ws), _ptr(loss), _ptr(poses), None)
        assert rc == 0, sc.L.mcd_last_error().decode()
        return {"loss_out": loss, "pose_out": poses}

    r = run("mcd_score", call, {"data": data})
    loss, poses = sc.score(data, n_samples=S, noise_steps=NS, seed=SEED, first_window_id=FIRST, want_poses=True)
    assert torch.equal(loss, r["loss_out"]) and torch.equal(poses, r["pose_out"])


# ------------------------------------------------------------------------------------------------ single passes and layers
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("name", ["sk_inject6", "sk_nocond7", "tl_concat13", "tl_random32"], ids=["T3", "T7", "T13", "T32"])
def test_unet_forward(name, rows):
    sc, _, _ = _scorer(name)
    inputs = {"x": _randn(rows, 2, sc.t_unet, 17, seed=51)}
    if sc.strategy == "inject":
        inputs["cond"] = _randn(rows, 16, seed=52)
    r = run("mcd_unet_forward", lambda T, x, cond=None: {"eps_out": sc.unet_forward(x, 1, cond, noise_steps=NS)}, inputs, [sc])
    assert tuple(r["eps_out"].shape) == (rows, 2, sc.t_unet, 17) and torch.isfinite(r["eps_out"]).all()


@pytest.mark.parametrize("stage", range(15))
@pytest.mark.parametrize("name", ["sk_inject6", "tl_concat13"], ids=["T3", "T13"])
def test_layer_forward(name, stage):
    """Every stage alone, B = 3.  At 13 frames (slab-tiled kernel) stages 3, 5, 7, 9 are joint resampler + layer, 7 and 9 with
    their skip input, and the resamplers 11 .. 14 do not exist on their own: the library refuses them before any launch."""
    sc, _, _ = _scorer(name)
    B, T = 3, sc.t_unet
    tiled = T > 12
    cin, vin, cout, vout = sc._STAGES[stage]
    if tiled and stage >= 11:
        with pytest.raises(RuntimeError, match="joint resamplers are part of stages"):
            sc.layer_forward(stage, _randn(B, cin, T, vin, seed=1), _randn(B, 16, seed=2))
        return
    inputs = {"emb": _randn(B, 16, seed=62)}
    if tiled and stage in sc._FUSED_IN:
        fin, fvin = sc._FUSED_IN[stage]
        inputs["x"] = _randn(B, fin, T, fvin, seed=61)
        if stage in (7, 9):
            inputs["skip"] = _randn(B, cin, T, vin, seed=63)
    else:
        inputs["x"] = _randn(B, cin, T, vin, seed=61)
    r = run("mcd_layer_forward", lambda T_, x, emb, skip=None: {"out": sc.layer_forward(stage, x, emb, skip)}, inputs, [sc])
    assert tuple(r["out"].shape) == (B, cout, T, vout) and torch.isfinite(r["out"]).all()


COND = [("AE", 1, {}), ("AE", 3, {}), ("AE", 20, {}), ("AE", 21, {}), ("E_unet", 3, {}), ("E_unet", 12, {}),
        ("E", 3, dict(channels=[24, 40], h_dim=8))]         # the last: a runtime channel list (gather scratch)


@pytest.mark.parametrize("arch,t,over", COND, ids=[f"{a}-{t}" for a, t, _ in COND])
def test_cond_encode(arch, t, over):
    """5 rows: 'AE' at 1, 3, 20 and 21 condition frames (20 is the last cond_fast_kernel row, 21 the plain kernel), 'E_unet' at 3
    and 12, 'E' with a channel list the library holds no instance for (and one scoring call of that model: its gather scratch)."""
    from mocodad_amd.models.mocodad import MoCoDAD
    _, cfg = golden_weights("inject")
    m, gen = CB._seeded(lambda: MoCoDAD(make_args(cfg, conditioning_strategy="inject", seg_len=t + 3, conditioning_indices=list(range(t)),
                                                  conditioning_architecture=arch, **over)), 9100 + 7 * t + len(arch))
    sc = m.build_scorer(torch.device(DEV))
    r = run("mcd_cond_encode", lambda T, cond_data: {"emb_out": sc.cond_encode(cond_data)},
            {"cond_data": torch.randn(5, 2, t, 17, generator=gen)}, [sc])
    assert tuple(r["emb_out"].shape) == (5, 16) and torch.isfinite(r["emb_out"]).all()
    if arch == "E":
        # mcd_cond_encode is given the condition frames alone (nothing to gather): the gather scratch of a runtime channel list is a
        # region of a scoring call's workspace
        def score(T, data):
            loss, poses = sc.score(data, n_samples=3, noise_steps=NS, seed=SEED, first_window_id=FIRST, want_poses=True)
            return {"loss_out": loss, "pose_out": poses}
        s = run("mcd_score_view", score, {"data": torch.randn(3, 2, t + 3, 17, generator=gen)}, [sc])
        assert torch.isfinite(s["loss_out"]).all()


# ------------------------------------------------------------------------------------------------ aggregation
AGGRS = ["best", "worst", "mean", "median", "quantile:0.3", "mean_pose", "median_pose"]


@pytest.mark.parametrize("S", [1, 64, 65])
@pytest.mark.parametrize("strategy", AGGRS)
def test_aggregate(strategy, S):
    sc, data, _ = _scorer("sk_inject6")
    B = 3
    inputs = {"data": data, "loss_all": _randn(B, S, seed=71).abs(), "poses_all": _randn(B, S, 2, 3, 17, seed=72)}

    def call(T, data, loss_all, poses_all):
        pose, loss = sc.aggregate(data, loss_all, poses_all, strategy, noise_steps=NS)
        return {"loss_agg": loss, **({"pose_agg": pose} if pose is not None else {})}

    r = run("mcd_aggregate", call, inputs)
    assert ("pose_agg" in r) == (strategy in ("best", "worst", "mean_pose", "median_pose")) and torch.isfinite(r["loss_agg"]).all()
    if strategy == "mean":
        np.testing.assert_allclose(r["loss_agg"].cpu().numpy(), inputs["loss_all"].double().mean(1).numpy(), rtol=1e-5)


@pytest.mark.parametrize("strategy", AGGRS[:5])
def test_aggregate_beyond_the_lds_staging(strategy):
    """S = 8193: one sample more than AGG_LDS_MAX, the samples are read where they lie.  Losses only."""
    sc, _, _ = _scorer("sk_inject6")
    B, S = 3, 8193
    la = _randn(B, S, seed=73).abs()
    r = run("mcd_aggregate", lambda T, loss_all: {"loss_agg": sc.aggregate(None, loss_all, None, strategy, noise_steps=NS)[1]},
            {"loss_all": la})
    want = {"best": la.min(1).values, "worst": la.max(1).values, "median": la.median(1).values}.get(strategy)
    if want is not None:
        assert torch.equal(r["loss_agg"].cpu(), want)


@pytest.mark.parametrize("strategy", AGGRS)
def test_aggregate_view(strategy):
    """mcd_aggregate_view: the *_pose strategies take each window's corrupt frames from its condition mask."""
    sc, data, mask = _scorer("sk_random6")
    B, S = 3, 3
    mask = mask.to(DEV)
    inputs = {"data": data, "loss_all": _randn(B, S, seed=74).abs(), "poses_all": _randn(B, S, 2, 3, 17, seed=75)}

    def call(T, data, loss_all, poses_all):
        pose, loss = sc.aggregate(data, loss_all, poses_all, strategy, noise_steps=NS, cond_mask=mask)
        return {"loss_agg": loss, **({"pose_agg": pose} if pose is not None else {})}

    run("mcd_aggregate_view", call, inputs)


# ------------------------------------------------------------------------------------------------ draw exports
@pytest.mark.parametrize("name", ["sk_inject6", "draw13"])
def test_philox_noise(name):
    """B = 3, S = 2, ns = 3 at 3 and 13 corrupt frames: 1224 and 5304 elements, no multiple of 256."""
    sc = _draw13() if name == "draw13" else _scorer(name)[0]
    r = run("mcd_philox_noise", lambda T: {"noise_out": sc.philox_noise(3, n_samples=2, noise_steps=NS, seed=SEED, first_window_id=FIRST)})
    assert tuple(r["noise_out"].shape) == (2, NS - 1, 3, 2, len(sc.corrupt_idx), 17) and r["noise_out"].numel() % 256
    assert torch.isfinite(r["noise_out"]).all()


def _draw13():
    if "draw13" not in _cache:
        from mocodad_amd.models.mocodad import MoCoDAD
        _, cfg = golden_weights("inject")
        m = MoCoDAD(make_args(cfg, conditioning_strategy="no_condition", seg_len=13, conditioning_indices=None, noise_steps=NS,
                              n_generated_samples=2))
        _cache["draw13"] = m.build_scorer(torch.device(DEV))
    return _cache["draw13"]


def test_latent_philox_noise():
    sc, _ = CB._latent()
    r = run("mcd_latent_philox_noise", lambda T: {"noise_out": sc.philox_noise(3, n_samples=2, noise_steps=NS, seed=SEED, first_window_id=FIRST)})
    assert tuple(r["noise_out"].shape) == (2, NS - 1, 3, 32) and torch.isfinite(r["noise_out"]).all()


def test_random_imp_masks_through_the_proxy():
    """(tests/test_random_imp_device_gpu.py keeps its own 8 guard words; here the engine's allocation between two bands.)"""
    sc, _, _ = _scorer("sk_random6")
    r = run("mcd_random_imp_masks", lambda T: {"masks_out": sc.random_imp_masks(3, seed=SEED, first_window_id=FIRST)})
    assert all(bin(int(v) & 0x3F).count("1") == 3 and 0 <= int(v) < 64 for v in r["masks_out"].cpu())


# ------------------------------------------------------------------------------------------------ latent model
def _latent(name):
    if ("latent", name) not in _cache:
        import latent_ref as R
        import latentt_fixtures as TT
        import latentx_fixtures as X
        from mocodad_amd.models.mocodad_latent import MoCoDADlatent
        sd, _, cfg, _ = X.load(name) if name in X.NAMES else TT.load(name) if name in TT.NAMES else R.load_fixture(name)
        m = MoCoDADlatent(make_args(cfg))
        m.load_state_dict(sd, strict=False)
        _cache[("latent", name)] = m.to(DEV).scorer()
    return _cache[("latent", name)]


LATENT = [("A_benign", 1), ("A_benign", 3), ("S12", 1), ("S12", 3), ("S12", 33), ("U", 1), ("U", 3), ("G", 1), ("G", 3)]


@pytest.mark.parametrize("name,B", LATENT, ids=[f"{n}-B{b}" for n, b in LATENT])
def test_latent_calls(name, B):
    """encode, denoise and score (perf mode and parity mode; loss_agg, loss_all, latents and code) of the fixtures: A_benign
    (3 + 3 frames, two launches), S12 (6 + 6: projection launch, H in the workspace; 33 windows = one past its 32-window tile), U
    ('E_unet') and G (runtime channel list: gather scratch).  S = 2, ns = 3."""
    sc = _latent(name)
    S, D = 2, sc.latent_dim
    data = _randn(B, 2, sc.seg_len, 17, seed=81)

    def encode(T, data):
        cond, z0 = sc.encode(data, noise_steps=NS)
        return {"cond_emb_out": cond, "z0_out": z0}

    e = run("mcd_latent_encode", encode, {"data": data}, [sc])
    assert tuple(e["z0_out"].shape) == (B, D) and torch.isfinite(e["z0_out"]).all() and torch.isfinite(e["cond_emb_out"]).all()
    run("mcd_latent_denoise", lambda T, x, cond: {"eps_out": sc.denoise(x, 1, cond, noise_steps=NS)},
        {"x": _randn(B, D, seed=82), "cond": _randn(B, 16, seed=83)}, [sc])

    def score(T, data, noise=None):
        out = T.empty(B, device=DEV, dtype=torch.float32)
        agg, loss, lat, code = sc.score(data, n_samples=S, noise_steps=NS, aggregation="median", noise=noise, seed=SEED, first_window_id=FIRST,
                                        want_all=True, want_latents=True, want_code=True, out=out)
        assert agg is out
        return {"loss_agg": out, "loss_all": loss, "latent_all": lat, "latent_code": code}

    for inputs in ({"data": data}, {"data": data, "noise": _randn(S, NS - 1, B, D, seed=84)}):
        r = run("mcd_latent_score", score, inputs, [sc])
        assert torch.equal(r["latent_code"], e["z0_out"]) and torch.isfinite(r["loss_all"]).all()


# ------------------------------------------------------------------------------------------------ loader and post-processing
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_normalize_poses(n, scaled):
    from mocodad_amd.engine import normalize_poses
    rng = np.random.default_rng(90 + n)
    raw = torch.from_numpy(rng.uniform(20, 300, (n, 34)).astype(np.float32))
    center, scale = (rng.normal(0, 0.2, 34), rng.uniform(0.5, 2.0, 34)) if scaled else (None, None)
    r = run("mcd_normalize_poses", lambda T, raw: {"out": normalize_poses(raw, (640, 360), center, scale, device=DEV)}, {"raw": raw})
    assert tuple(r["out"].shape) == (n, 2, 17) and torch.isfinite(r["out"]).all()


def test_scatter_max():
    """3 rows x 7 frames; frame ids 0, -2, 8 and 100 fall outside 1 .. 7 and are dropped."""
    sc, _, _ = _scorer("sk_inject6")
    frames = torch.tensor([[1, 2, 3], [0, 1, 7], [7, 8, 100], [-2, 4, 5], [5, 6, 7]], dtype=torch.int32)
    row = torch.tensor([0, 1, 2, 0, 2], dtype=torch.int32)
    scores = torch.tensor([0.5, 0.25, 0.75, 1.5, 0.125])
    r = run("mcd_scatter_max", lambda T, scores: {"out": sc.scatter_max(scores, frames, row, 3, 7)}, {"scores": scores})
    want = torch.zeros(3, 7)
    for s, fr, ro in zip(scores, frames, row):
        for f in fr:
            if 1 <= int(f) <= 7:
                want[int(ro), int(f) - 1] = max(float(want[int(ro), int(f) - 1]), float(s))
    assert torch.equal(r["out"].cpu(), want)


def test_scatter_max_ignores_rows_outside_the_output():
    """Rows -1 and n_rows = 3 among valid ones, 7 frames: a store through such a row would land one 28-byte row before / behind the
    interior -- inside the guard band, where it is reported -- and must not happen; the valid rows equal np.maximum.at.  (Only
    inside the region: the call is not repeated on an unguarded buffer.)"""
    sc, _, _ = _scorer("sk_inject6")
    frames = torch.tensor([[1, 2, 3], [1, 2, 3], [5, 6, 7], [5, 6, 7], [3, 4, 5], [6, 7, 8], [2, 3, 4]], dtype=torch.int32)
    row = torch.tensor([0, -1, 2, 3, 1, 3, -1], dtype=torch.int32)
    scores = torch.tensor([0.5, 9.0, 0.75, 8.0, 1.5, 7.0, 6.0])
    with guarded() as g:
        out = sc.scatter_max(guarded_copy(scores.to(DEV), "nan"), frames, row, 3, 7)
        torch.cuda.synchronize()
        g.check()
        assert g.registry and unwritten(out) == 0
    want = np.zeros((3, 7), np.float32)
    ok = ((row >= 0) & (row < 3)).numpy()
    ii, kk = np.nonzero(ok[:, None] & (frames.numpy() >= 1) & (frames.numpy() <= 7))
    np.maximum.at(want, (row.numpy()[ii], frames.numpy()[ii, kk] - 1), scores.numpy()[ii])
    assert (want > 0).sum() == 9 and np.array_equal(out.cpu().numpy(), want)


def test_frame_score_assembler():
    """The two-clip example of test_frame_scores_gpu.test_device_frame_scores_error_and_fallback, one window per clip: the float64
    `out` and the assembler's workspace."""
    from mocodad_amd.engine import FrameScoreAssembler
    gts = {(1, 1): np.array([0, 0, 1, 1, 0, 0, 0, 0]), (1, 2): np.array([0, 1, 0, 0, 0, 0, 0])}
    meta = np.array([[1, 1, 1, 1], [1, 2, 1, 1]])
    frames = (meta[:, 3:4] + np.arange(6)[None]).astype(np.int32)

    def call(T, scores):
        asm = FrameScoreAssembler(gts, {}, num_transform=1, pad_size=-1, filter_kernel_size=2, frames_shift=1, device=DEV)
        pds = asm(scores, torch.zeros(2, dtype=torch.int64), meta, frames)
        assert pds.dtype == np.float64 and pds.ndim == 1 and pds.size == asm.total
        return {"out": torch.from_numpy(pds).to(DEV)}

    r = run("mcd_frame_scores", call, {"scores": torch.tensor([0.5, 0.75])})
    assert torch.isfinite(r["out"]).all() and float(r["out"].max()) > 0


# ------------------------------------------------------------------------------------------------ streams
@pytest.fixture(scope="module")
def stream_env(tmp_path_factory):
    from dataset_spec import load_dataset_golden
    from test_stream_many_gpu import _model
    g = load_dataset_golden()
    return g, _model(tmp_path_factory.mktemp("bounds"), g)[0]


def _replay(g, model, ring_len, how, clip):
    """3 tracks in 2 clips on a stream of exactly 3 slots (2 clip slots), 2 ring_len + seg_len frames: every ring position, both
    copies, is written and the ring wraps; then everything is closed (mcd_stream_flush) -> {output or ring: tensor}"""
    from mocodad_amd.stream import ClipScoreCfg, PoseStream
    from test_stream_many_gpu import SEG_LEN, VID_RES
    st = PoseStream(model, vid_res=VID_RES, center=g["train_center"], scale=g["train_scale"], max_tracks=3, ring_len=ring_len,
                    clip_scores=ClipScoreCfg(sigma=2.0, shift=2, max_clips=2) if clip else None)
    assert st.rings.n_slots == 3 and st.rings.ring_len == ring_len
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
        out[f"scores{i}"], out[f"final{i}"] = t.scores, t.final.values
        if clip:
            out[f"clip{i}"] = t.clip.values
    assert sorted(st.table.slot_of.values()) == [0, 1, 2], "every slot, the last included, is live"
    if clip:
        for c in ((1, 1), (1, 2)):
            tails, cf = st.close_clip(c)
            out[f"tails{c}"], out[f"clip_tail{c}"] = tails.values, cf.values
        rings = {"clip_sum": st.clip_rings.sum, "clip_lmax": st.clip_rings.lmax, "clip_lmin": st.clip_rings.lmin, "clip_n": st.clip_rings.n}
    else:
        out["tails"] = st.close_all().values
        rings = {}
    rings.update(ring=st.ring, frame_scores_ring=st.rings.frame_scores_ring)
    assert sum(v.numel() for k, v in out.items() if k.startswith("scores")) == st.n_emitted > 0
    out.update(rings)
    return out


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("how", ["push", "push_many3"])
@pytest.mark.parametrize("extra", [0, 2], ids=["L6", "L8"])
def test_stream_replay(stream_env, extra, how, clip):
    """ring_len = seg_len (a group of push_many is one tick) and seg_len + 2 (three ticks per group), through push, push_many with
    K = 3 and the closing flush; with clip_scores at sigma = 2 the float64 clip rings and emit outputs too.  (b) does not apply to
    the rings: a cell no row reached keeps its zero."""
    from test_stream_many_gpu import SEG_LEN
    g, model = stream_env
    names = (["clip_sum", "clip_lmax", "clip_lmin", "clip_n"] if clip else []) + ["ring", "frame_scores_ring"]
    entry = "mcd_stream_push_group + frame_scores_group" + (" (PoseStream.push: groups of one tick)" if how == "push" else "")
    r = run(entry + " + flush" + (" + clip_update + clip_emit" if clip else ""),
            lambda T: _replay(g, model, SEG_LEN + extra, how, clip), None, [model.scorer()], partial=names)
    ring = r["ring"].view(3, 2, SEG_LEN + extra, 34)
    assert torch.equal(ring[:, 0], ring[:, 1]) and bool((ring != 0).any(-1).all()), "both copies of every ring position were written"


# ------------------------------------------------------------------------------------------------ sensitivity
def test_the_guard_sees_one_row_past_the_end():
    """A guard that never fires proves nothing.  With short_rows = 1 the proxy hands out tensors whose registered interior is one
    leading-index row shorter: the kernel's legitimate last row lands in the tail guard (inside the backing tensor: nothing
    faults), and check() must name that allocation and the offsets of that row."""
    from mocodad_amd.engine import normalize_poses
    raw = torch.from_numpy(np.random.default_rng(3).uniform(20, 300, (5, 34)).astype(np.float32)).to(DEV)
    want = normalize_poses(raw, (640, 360), device=DEV)
    sc = _scorer("sk_inject6")[0]
    noise = sc.philox_noise(3, n_samples=2, noise_steps=NS, seed=SEED, first_window_id=FIRST)
    for what, row_bytes, shape in (("normalize_poses", 136, "(5, 2, 17)"), ("philox_noise", (NS - 1) * 3 * 2 * 3 * 17 * 4, "(2, 2, 3, 2, 3, 17)")):
        with guarded(short_rows=1) as g:
            got = normalize_poses(raw, (640, 360), device=DEV) if what == "normalize_poses" else \
                sc.philox_noise(3, n_samples=2, noise_steps=NS, seed=SEED, first_window_id=FIRST)
            torch.cuda.synchronize()
            assert torch.equal(got, want if what == "normalize_poses" else noise)
            v = g.violations()
            with pytest.raises(GuardViolation) as ei:
                g.check()
        assert len(v) == 1, v
        name, side, first, last, _, count = v[0]
        print(f"bounds | sensitivity: {name}: {side} guard, offsets {first} .. {last}, {count} bytes")
        assert name.startswith("engine.py:") and what in name and f"empty {shape} float32" in name and side == "tail"
        # the whole row, up to float bytes that happen to equal the guard byte
        assert first < 4 and row_bytes - 4 <= last < row_bytes and count > 0.9 * row_bytes
        assert name in str(ei.value) and "tail guard" in str(ei.value)


# ------------------------------------------------------------------------------------------------ coverage of the C ABI
COVERED = ["mcd_cond_encode", "mcd_unet_forward", "mcd_layer_forward", "mcd_philox_noise", "mcd_random_imp_masks", "mcd_score",
           "mcd_score_view", "mcd_score_fused", "mcd_aggregate", "mcd_aggregate_view", "mcd_scatter_max", "mcd_normalize_poses",
           "mcd_stream_flush", "mcd_stream_push_group", "mcd_stream_frame_scores_group",
           "mcd_stream_clip_update", "mcd_stream_clip_emit", "mcd_frame_scores", "mcd_latent_encode", "mcd_latent_denoise",
           "mcd_latent_score", "mcd_latent_philox_noise"]


def test_every_entry_that_writes_a_caller_buffer_is_in_the_list():
    """The declarations of include/mocodad_hip.h with a non-const data pointer (or the stream / clip state, whose rings the
    caller owns), packers and debug aids aside, are the entries exercised above.  Prints what the proxy registered."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mocodad_hip.h")).read(), flags=re.S)
    writers = []
    for name, params in re.findall(r"\bint\s+(mcd_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        if name.startswith(("mcd_pack", "mcd_debug", "mcd_set", "mcd_latent_set", "mcd_plan")):
            continue
        ps = [p.strip() for p in params.split(",")]
        if any(re.match(r"(float|double|int32_t|int64_t)\s*\*", p) or p.startswith(("const mcd_stream_state_t*", "const mcd_clip_state_t*"))
               or p == "void* workspace" for p in ps):
            writers.append(name)
    assert sorted(writers) == sorted(COVERED)
    for entry, seen in ALLOC.items():
        print(f"bounds | {entry}:")
        for a in seen:
            print(f"bounds |     {a}")
    print(f"bounds | module run time so far {time.time() - T0:.1f} s")

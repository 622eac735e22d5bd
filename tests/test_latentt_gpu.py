"""GPU: the latent model at 5 .. 12 corrupt frames -- a condition-encoder launch, the encode launch that leaves the last layer's
output H in the workspace, latent_project_kernel (to_time_dim as one MFMA launch over all windows), the chain launch -- against
the vectors the reference's MoCoDADlatent produced (tests/golden/gen_latentt_golden.py), against the CPU restatement at every new
frame count, at the projection's 32-window tile edge, against float64, and the bit-identity properties the 3-frame rows are held
to (tests/test_latentx_gpu.py).

Gates.  The project's: |got - ref| <= 1e-4 max(1, max|ref|) per compared tensor.  Against float64 (test_longest_shape_vs_fp64):
max|gpu - ref64| <= 4 max|cpu32 - ref64| as tests/test_latent_shapes_gpu.py sets it, the right side being the fp32 CPU
restatement's own error on the same inputs; for z0 the larger of two fp32 orders of to_time_dim (F.linear, and
latent_ref.linear_k_chain: the fully sequential K = 7 680 chain, which no split MFMA chain is worse than).  Every compared figure
of that test is printed (`latent-frames |` rows; the recorded run is profiles/latent_frames_fp64.txt)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import latent_ref as R
import latentt_fixtures as X
from helpers import make_args
from latent_ref import _perturb
from oracle import mocodad_oracle as O

pytestmark = pytest.mark.gpu

_models, _random, _edge = {}, {}, {}


def close(got, ref, what):
    ref = np.asarray(ref)
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=what)


def model(name):
    """The module with the fixture's weights on cuda:0 (one per fixture and session)."""
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    if name not in _models:
        sd, _, cfg, _ = X.load(name)
        m = MoCoDADlatent(make_args(cfg))
        m.load_state_dict(sd, strict=False)
        _models[name] = m.to("cuda:0")
    return _models[name]


@pytest.mark.parametrize("nb", [5, 1])
@pytest.mark.parametrize("name", X.NAMES)
def test_encode_and_score_vs_reference(name, nb):
    _, _, _, io = X.load(name)
    D, ns, S, B = (int(v) for v in io["sizes"])
    m = model(name)
    data, noise = torch.from_numpy(io["data"])[:nb], torch.from_numpy(io["noise"])[:, :, :nb].contiguous()
    cond, z0 = m.scorer().encode(data, noise_steps=ns)
    close(cond, io["cond_emb"][:nb], "cond_emb")
    close(z0, io["z0"][:nb], "z0")
    _, loss_all, lat, code = m.scorer().score(data, n_samples=S, noise_steps=ns, noise=noise, want_latents=True, want_code=True)
    close(code, io["z0"][:nb], "latent_code")
    close(lat, io["latent_all"][:nb], "latent_all")
    close(loss_all, io["loss_all"][:nb], "loss_all")
    batch = X.batch_of(data)
    out = m.forward(batch, aggr_strategy="all", return_="all", noise=noise)
    close(out[0], io["loss_all"][:nb], "forward all: loss")
    close(out[1], io["latent_all"][:nb], "forward all: latents")
    for a in X.AGGRS:
        tag = a.replace(":", "_")
        loss, sel = m.forward(batch, aggr_strategy=a, return_="all", noise=noise)[:2]
        close(loss, io[f"loss_{tag}"][:nb], f"forward {a}: loss")
        assert (sel is None) == (f"sel_{tag}" not in io)
        if sel is not None:
            close(sel, io[f"sel_{tag}"][:nb], f"forward {a}: selected latent")
        close(m.forward(batch, aggr_strategy=a, return_="loss", noise=noise)[0], io[f"loss_{tag}"][:nb], f"forward {a}: loss only")


def random_model(tx, tc=3, D=32, arch="AE", hostile=False, **over):
    """-> (MoCoDADlatent on the CPU, cloned fp32 state_dict, (cond_idx, corrupt_idx)): fixture S12's settings at tc condition + tx
    corrupt frames, seeded random-init weights with perturbed BatchNorm statistics and PReLU slopes; hostile: every BatchNorm
    gain log-uniform in 0.1x .. 10x, as the hostile fixtures.  Built once per argument set and session: read-only."""
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    key = (tx, tc, D, arch, hostile, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _random:
        _, _, cfg, _ = X.load("S12")
        gen = torch.Generator().manual_seed(1000 * tx + 10 * tc + D)
        with torch.random.fork_rng(), torch.no_grad():
            torch.manual_seed(17 * tx + tc)
            m = MoCoDADlatent(make_args(cfg, conditioning_architecture=arch, seg_len=tc + tx, conditioning_indices=list(range(tc)),
                                        latent_embedding_dim=D, hidden_sizes=[48, D], noise_steps=3, n_generated_samples=2, **over))
            _perturb(m, gen)
            if hostile:
                for mod in m.modules():
                    if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
                        mod.weight.data.copy_(torch.exp((torch.rand(mod.weight.shape, generator=gen) * 2 - 1) * np.log(10.0)))
        ci, xi = m._frame_split()
        assert (len(ci), len(xi)) == (tc, tx)
        _random[key] = (m, {k: v.detach().clone() for k, v in m.state_dict().items()}, (ci, xi))
    return _random[key]


def inputs(tx, tc, D, B, ns=3, S=2, scale=1.0):
    g = torch.Generator().manual_seed(31 * tx + tc + B)
    data = torch.randn(B, 2, tc + tx, 17, generator=g) * scale
    return data.clamp(-5, 5) if scale != 1.0 else data, torch.randn(S, ns - 1, B, D, generator=g)


CASES = [(tx, 3, 32, "AE", {}) for tx in range(5, 13)] + [
    (12, 12, 16, "E_unet", {}), (12, 12, 128, "E_unet", {}), (12, 3, 32, "E", dict(channels=[16, 8], h_dim=24))]


@pytest.mark.parametrize("tx,tc,D,arch,over", CASES, ids=[f"{c[0]}+{c[1]}-D{c[2]}-{c[3]}" for c in CASES])
def test_every_new_frame_count_vs_cpu_restatement(tx, tc, D, arch, over):
    """5 windows in parity mode against tests/latent_ref.py (pinned at these lengths by tests/test_latentt_golden.py).  12 frames
    also with the widest and the narrowest latent behind 12 'E_unet' condition frames, and with a runtime channel list (the
    condition encoder as a gather and a launch: five launches)."""
    m, sd, (ci, xi) = random_model(tx, tc, D, arch, **over)
    data, noise = inputs(tx, tc, D, 5)
    with torch.no_grad():
        rc, rz, rlat, rloss = R.score(sd, data, noise, noise_steps=3, cond_idx=ci, corrupt_idx=xi)
    sc = m.to("cuda:0").scorer()
    cond, z0 = sc.encode(data, noise_steps=3)
    close(cond, rc.numpy(), "cond_emb")
    close(z0, rz.numpy(), "z0")
    _, loss_all, lat, code = sc.score(data, n_samples=2, noise_steps=3, noise=noise, want_latents=True, want_code=True)
    assert torch.equal(code, z0)
    close(lat, rlat.numpy(), "latent_all")
    close(loss_all, rloss.numpy(), "loss_all")
    assert torch.isfinite(loss_all).all()


def edge_reference(tx):
    """33 windows at tx corrupt frames: the scorer, the windows, the CPU restatement's (cond_emb, z0) and the GPU's -- once."""
    if tx not in _edge:
        m, sd, (ci, xi) = random_model(tx)
        data, _ = inputs(tx, 3, 32, 33)
        with torch.no_grad():
            ref = R.encode(sd, data, ci, xi)
        sc = m.to("cuda:0").scorer()
        got = [t.clone() for t in sc.encode(data)]
        _edge[tx] = (sc, data, ref, got)
    return _edge[tx]


@pytest.mark.parametrize("B", [1, 32, 33])
def test_projection_tile_edge_vs_cpu_restatement(B):
    """One window (31 zero columns), exactly one tile of 32, and a second workgroup holding one window, at 12 frames."""
    sc, data, ref, _ = edge_reference(12)
    cond, z0 = sc.encode(data[:B])
    close(cond, ref[0][:B].numpy(), "cond_emb")
    close(z0, ref[1][:B].numpy(), "z0")
    agg, _, _, code = sc.score(data[:B], n_samples=2, noise_steps=3, seed=1, aggregation="mean", want_code=True)
    assert torch.equal(code, z0) and torch.isfinite(agg).all() and agg.shape == (B,)


@pytest.mark.parametrize("tx", [6, 12])
def test_a_window_does_not_depend_on_its_batch(tx):
    """z0 of a window from a call of its own equals its z0 inside the 33-window batch at positions 0, 31 and 32 (first and last
    column of the first projection tile, the second tile's only column); a repeated call is bit-identical; so is the whole scoring
    call on the halves of a batch."""
    sc, data, _, (cond, z0) = edge_reference(tx)
    for b in (0, 31, 32):
        c1, z1 = sc.encode(data[b:b + 1])
        assert torch.equal(z1, z0[b:b + 1]), b
        assert torch.equal(c1, cond[b:b + 1]), b
    c2, z2 = sc.encode(data)
    assert torch.equal(z2, z0) and torch.equal(c2, cond)
    assert torch.equal(sc.encode(data[5:33])[1], z0[5:33])      # (another alignment of the windows to the tile)
    kw = dict(n_samples=2, noise_steps=3, seed=9, aggregation="best", want_all=True, want_latents=True, want_code=True)
    whole = [t.clone() for t in sc.score(data, first_window_id=50, **kw)]
    again = sc.score(data, first_window_id=50, **kw)
    a, b = sc.score(data[:7], first_window_id=50, **kw), sc.score(data[7:], first_window_id=57, **kw)
    for w, g, x, y in zip(whole, again, a, b):
        assert torch.equal(w, g) and torch.equal(w, torch.cat([x, y]))
    assert torch.equal(whole[3], z0) and torch.isfinite(whole[1]).all()


@pytest.mark.parametrize("name", ["S12", "S24"])
def test_window_views_score_like_materialised_windows(name):
    from mocodad_amd.data import synthetic
    from mocodad_amd.data.windows import TrajectoryWindows
    m = model(name)
    trajs, _ = synthetic.make_trajectories(n_clips=2, frames_per_clip=40, persons_per_clip=2)
    tw = TrajectoryWindows(trajs, seg_len=m.n_frames, num_transform=2)
    dense = tw.materialize()
    sc = m.scorer()
    tw.to("cuda:0")
    kw = dict(n_samples=2, noise_steps=4, seed=3, aggregation="best", want_all=True, want_latents=True, want_code=True)
    a = sc.score(tw.batch(0, len(tw))[0], **kw)
    b = sc.score(dense, **kw)
    assert len(tw) > 33 and torch.isfinite(a[1]).all()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ca, za = sc.encode(tw.batch(0, len(tw))[0])
    cb, zb = sc.encode(dense)
    assert torch.equal(ca, cb) and torch.equal(za, zb)


def test_workspace_grows_by_h_for_the_new_rows_only():
    """mcd_latent_workspace_bytes: + B x 640 T floats (rounded up to 256 bytes) where the projection is a launch of its own."""
    sc12 = edge_reference(12)[0]
    m3, _, _ = random_model(3)
    sc3 = m3.to("cuda:0").scorer()
    ws = lambda sc, B: int(sc.L.mcd_latent_workspace_bytes(sc._h, B))
    r256 = lambda n: (n + 255) // 256 * 256
    for B in (1, 33):
        assert ws(sc3, B) == r256(B * 16 * 4) + r256(B * 32 * 4)
        assert ws(sc12, B) == ws(sc3, B) + r256(B * 640 * 12 * 4)
    sc12.set_option("split_encode", 1)      # changes nothing for a row without a fused form
    assert ws(sc12, 33) == ws(sc3, 33) + r256(33 * 640 * 12 * 4)
    sc, data, _, (cond, z0) = edge_reference(12)
    assert torch.equal(sc.encode(data)[1], z0)
    sc12.set_option("split_encode", 0)


def _down_path(sd, data, xi, e):
    """latent_ref.encode's down path up to to_time_dim's input (B, 64 T 10)"""
    h = data[:, :, list(xi)]
    for b, i in O.UNET_DOWN:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    h = O.joint_resample(sd, "model.down1", h)
    for b, i in O.UNET_MID1:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    h = O.joint_resample(sd, "model.down2", h)
    for b, i in O.UNET_MID2:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    return h.reshape(h.shape[0], -1)


def _row(what, got, ref64, cpu32s):
    """Prints one `latent-frames |` row -> (max|gpu - ref64|, yardstick, max|ref64|)"""
    assert ref64.dtype == torch.float64 and torch.isfinite(ref64).all(), what
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), what
    err, top = (got - ref64).abs().max().item(), ref64.abs().max().item()
    yards = [(c.double() - ref64).abs().max().item() for c in cpu32s]
    yard = max(yards)
    print(f"latent-frames | 12+12 D128 B33 hostile | {what:18s} | max|ref64| {top:9.3e} | gpu {err:9.3e} | cpu32 " +
          " / ".join(f"{y:9.3e}" for y in yards) + f" | ratio {err / yard if yard > 0 else float('inf'):6.2f} | rel {err / max(1.0, top):9.3e}")
    return err, yard, top


def test_longest_shape_vs_fp64():
    """12 + 12 frames, D 128, 33 windows, hostile-scale weights and windows (x3, clipped to +-5), 'E_unet'.

    Yardstick: the fp32 CPU restatement's error against the same restatement in float64 (latent_ref.to_f64) on the same inputs;
    for z0 the larger of to_time_dim as F.linear and as latent_ref.linear_k_chain (one sequential chain over K = 7 680), both on
    the fp32 restatement's own H.  The fp64 chain is fed the GPU's own cond_emb and latent code, as tests/test_latent_shapes_gpu.py
    does, so the losses judge the chain launch alone.  Gate: 4 x the yardstick and the project's 1e-4 gate, per tensor."""
    tx = tc = 12
    m, sd, (ci, xi) = random_model(tx, tc, 128, "E_unet", hostile=True)
    data, noise = inputs(tx, tc, 128, 33, scale=3.0)
    sd64 = R.to_f64(sd)
    with torch.no_grad():
        rc64, rz64 = R.encode(sd64, data.double(), ci, xi)
        rc32, rz32 = R.encode(sd, data, ci, xi)
        e32 = O.pos_encoding(torch.full((33, 1), -1.0), 16) + rc32
        h32 = _down_path(sd, data, xi, e32)
        w, b = sd["model.to_time_dim.weight"], sd["model.to_time_dim.bias"]
        assert h32.shape == (33, 7680) and torch.equal(F.linear(h32, w, b), rz32)
        rz32_chain = R.linear_k_chain(h32, w, b)
    sc = m.to("cuda:0").scorer()
    cond, z0 = sc.encode(data, noise_steps=3)
    _, loss, lat, code = sc.score(data, n_samples=2, noise_steps=3, noise=noise, want_all=True, want_latents=True, want_code=True)
    assert torch.equal(code, z0)
    with torch.no_grad():
        c, z = cond.cpu(), code.cpu()
        lat64 = R.chain(sd64, c.double(), z.double(), noise.double(), 3)
        lat32 = R.chain(sd, c, z, noise, 3)
        rows = [_row("cond_emb", cond, rc64, [rc32]),
                _row("z0", z0, rz64, [rz32, rz32_chain]),
                _row("latents", lat, lat64, [lat32]),
                _row("smooth_l1", loss, R.losses(lat64, z.double()), [R.losses(lat32, z)])]
    for what, (err, yard, top) in zip(("cond_emb", "z0", "latents", "smooth_l1"), rows):
        assert err <= 1e-4 * max(1.0, top), (what, err, top)
        assert err <= 4 * yard, (what, err, yard)


def test_live_stream_at_seg_len_12():
    """PoseStream over a 6 + 6 latent module, three synthetic tracks of 16 frames (five windows each): a tick's window scores equal
    forward on the tick's materialised windows with the same draws, and every frame score -- finalised by a tick or returned by
    close -- equals the maximum of those scores over the windows that hold the frame, bit for bit."""
    from mocodad_amd.stream import PoseStream
    SEG, NF, NT = 12, 16, 2
    m, _, _ = random_model(6, 6, 32, "AE", num_transform=NT, aggregation_strategy="best", model_return_value="loss")
    m = m.to("cuda:0")
    assert m.n_frames == SEG and m.n_frames_corrupt == 6
    S, ns, D = m.n_generated_samples, m.noise_steps, m.latent_embedding_dim
    rng = np.random.default_rng(5)
    keys = [(1, 1, p) for p in (1, 2, 3)]
    poses = rng.uniform(50, 300, size=(3, NF, 34)).astype(np.float32)
    stream = PoseStream(m, vid_res=(640, 360), max_tracks=4)
    win_scores = {k: [] for k in keys}        # per track: (NT,) scores of its windows in order
    final = {}
    g = torch.Generator().manual_seed(3)
    for f in range(NF):
        ne = 3 if f >= SEG - 1 else 0
        noise = torch.randn(S, ns - 1, NT * ne, D, generator=g).cuda() if ne else None
        tick = stream.push(keys, [f + 1] * 3, poses[:, f], noise=noise)
        if not ne:
            assert tick.windows is None and tick.scores.numel() == 0
            continue
        dense = tick.windows.materialize()
        assert tuple(dense.shape) == (NT * 3, 2, SEG, 17)
        batch = [dense, torch.from_numpy(tick.trans), torch.from_numpy(tick.meta), torch.from_numpy(tick.frames)]
        ref = m.forward(batch, aggr_strategy=None, return_="loss", noise=noise)[0]
        assert torch.equal(tick.scores, ref) and torch.isfinite(ref).all()
        sc = tick.scores.cpu().numpy().reshape(NT, 3)
        for j, k in enumerate(tick.final.keys):
            win_scores[k].append(sc[:, j])
        for k, fr, v in zip(tick.final.keys, tick.final.frames, tick.final.values.cpu().numpy()):
            final[(k, int(fr))] = v
    tail = stream.close_all()
    for k, fr, v in zip(tail.keys, tail.frames, tail.values.cpu().numpy()):
        assert (k, int(fr)) not in final
        final[(k, int(fr))] = v
    assert len(final) == 3 * NF
    n_win = NF - SEG + 1
    for k in keys:
        w = np.stack(win_scores[k])      # (windows, NT)
        assert w.shape == (n_win, NT) and len(np.unique(w)) == w.size
        for r in range(NF):
            holds = [i for i in range(n_win) if i <= r < i + SEG]
            assert np.array_equal(final[(k, r + 1)], w[holds].max(axis=0)), (k, r)

"""GPU: the latent model's pretrain stage (MoCoDADlatentPretrain, engine.LatentReconstructor, mcd_latent_reconstruct) -- [condition
encoder] -> encode -> [project] -> unproject -> decode -- against the vectors the reference's MoCoDADlatent (stage 'pretrain')
produced (tests/golden/gen_latentp_golden.py), against the CPU restatement (tests/latentp_ref.py, pinned to those vectors by
tests/test_latentp_golden.py) at every frame count, at the unproject launch's 32-window tile edge, and against float64; the
bit-identity properties (a window alone / in a batch, window views, z_in = z0, non-finite windows) as the diffusion stage is held to.

Gates.  The project's: |got - ref| <= 1e-4 max(1, max|ref|) per compared tensor.  Against float64 (test_rows_vs_fp64, over
latentp_ref.FP64_CASES: every corrupt frame count and latent size, both ends of the condition length, 'E_unet' and a runtime
channel list, hostile-scale weights, the decode launch alone on latents of unit and of generated scale, the three loss functions;
45 windows each): pose_ref.gated's rule with latentp_ref.X -- err <= 2 X yard on max and on rms, on cond_emb, z0, pose and loss,
yard the larger error of two fp32 evaluation orders of the restatement, for z0 of those and of to_time_dim as one sequential
k-chain -- plus the 1e-4 gate.  Its rows (`pose-fp64 |`) are recorded in profiles/latent_recon_fp64.txt.

Found (MI355X, 100 rows of 28 cases): no launch misses a gate, no kernel was changed, and no evaluation order beyond the three
named above was needed.  Worst ratio to the yardstick, max / rms: cond_emb 1.81 / 1.69 (gate 4), z0 0.50 / 0.57 (gate 3; against
the two conv orders alone, without the k-chain, 2.38 / 1.90), pose 2.45 / 1.70 (gate 4), loss 2.10 / 1.66 (gate 5) -- the first,
third and fourth on the hostile 12 + 12 fixture; worst error relative to max(1, max|ref64|) 2.2e-6 (hostile poses of 1.5e3),
7.6e-7 otherwise.  l1 and mse sit where smooth_l1 does (loss ratios 0.64 .. 1.38 against 0.70 .. 1.38 on the same poses), and
latents of generated scale (x 31.6) leave the decode launch's ratios where unit latents do (pose 0.93 .. 1.29 against 1.10 ..
1.43).  The yardstick is fp32 arithmetic of the CPU at hand (these ratios: the MI355X
host's); X covers both CPUs seen (tests/test_latentp_fp64_host.py).
Run time: the module alone 7.3 s for its 73 tests on one MI355X with 16 CPU threads; of the 28 cases none takes more than
0.6 s, most of it the CPU references (shared with the host test's within a session)."""
import numpy as np
import pytest
import torch

import latentp_ref as R
from helpers import make_args

pytestmark = pytest.mark.gpu

_models, _edge = {}, {}


def close(got, ref, what):
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=what)


def batch_of(data):
    B, T = data.shape[0], data.shape[2]
    return [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, T, dtype=torch.int32)]


def model(name):
    """The module with the fixture's weights on cuda:0 (one per fixture and session)."""
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    if name not in _models:
        sd, _, cfg, _ = R.load_fixture(name)
        m = MoCoDADlatentPretrain(make_args(cfg))
        m.load_state_dict(sd, strict=False)
        _models[name] = m.to("cuda:0")
    return _models[name]


@pytest.mark.parametrize("nb", [5, 1])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_reconstruction_vs_reference(name, nb):
    _, _, _, io = R.load_fixture(name)
    m = model(name)
    got = {k: [] for k in ("pose", "loss", "cond_emb", "z0")}
    for b in range(0, 5, nb):
        pose, loss, cond, z0 = m.scorer().reconstruct(torch.from_numpy(io["data"][b:b + nb]), want_code=True)
        for k, v in zip(("pose", "loss", "cond_emb", "z0"), (pose, loss, cond, z0)):
            got[k].append(v)
    for k in got:
        close(torch.cat(got[k]), io[k], k)
    data = torch.from_numpy(io["data"][:nb])
    out = m.forward(batch_of(data))
    assert len(out) == 5
    close(out[0], io["pose"][:nb], "forward: pose")
    assert torch.equal(out[1].cpu(), data[:, :, [int(i) for i in io["corrupt_idx"]]])      # the corrupt frames, not the window
    close(m.forward(batch_of(data), return_="loss")[0], io["loss"][:nb], "forward: loss")
    loss, pose = m.forward(batch_of(data), return_="all")[:2]
    close(loss, io["loss"][:nb], "forward all: loss")
    close(pose, io["pose"][:nb], "forward all: pose")


@pytest.mark.parametrize("name", R.FIXTURES)
def test_test_loop_gives_the_post_processing_value(name):
    _, _, _, io = R.load_fixture(name)
    m = model(name)
    data = torch.from_numpy(io["data"])
    for hooks in (("on_test_epoch_start", "test_step", "on_test_epoch_end"),
                  ("on_validation_epoch_start", "validation_step", "on_validation_epoch_end")):
        getattr(m, hooks[0])()
        for i, (a, b) in enumerate(((0, 2), (2, 5))):
            getattr(m, hooks[1])(batch_of(data[a:b]), i)
        rec = getattr(m, hooks[2])()
        ref = float(io["rec_loss"])
        assert abs(rec - ref) <= 1e-4 * max(1.0, abs(ref)), (hooks[2], rec, ref)
    pose = m.forward(batch_of(data))
    assert abs(m.post_processing(pose[0].cpu().numpy(), pose[1].cpu().numpy(), None, None, None) - ref) <= 1e-4 * max(1.0, abs(ref))


CASES = [(t, 3, 32) for t in R.FRAME_COUNTS] + [(3, 3, 16), (3, 3, 128), (12, 12, 16), (12, 12, 128)]


@pytest.mark.parametrize("t,tc,D", CASES, ids=[f"{c[0]}+{c[1]}-D{c[2]}" for c in CASES])
def test_every_frame_count_vs_cpu_restatement(t, tc, D):
    m, sd = R.random_ae_model(t, tc, D, seed=100 * t + D)
    data = R.windows(3, t + tc, 7 * t + D)
    ci, xi = m._frame_split()
    with torch.no_grad():
        ref = R.reconstruct(sd, data, ci, xi)
    pose, loss, cond, z0 = m.to("cuda:0").scorer().reconstruct(data, want_code=True)
    for what, g, r in zip(("cond_emb", "z0", "pose", "loss"), (cond, z0, pose, loss), ref):
        close(g, r, what)
    assert torch.isfinite(loss).all()


def edge_reference(t):
    """33 windows at t + 3 frames: the scorer, the windows, the restatement's results, the GPU's (pose, loss, cond_emb, z0) -- once."""
    if t not in _edge:
        m, sd = R.random_ae_model(t, 3, 32, seed=900 + t)
        data = R.windows(33, t + 3, 50 + t)
        ci, xi = m._frame_split()
        with torch.no_grad():
            ref = R.reconstruct(sd, data, ci, xi)
        sc = m.to("cuda:0").scorer()
        got = [v.clone() for v in sc.reconstruct(data, want_code=True)]
        _edge[t] = (sc, sd, (ci, xi), data, ref, got)
    return _edge[t]


@pytest.mark.parametrize("B", [1, 32, 33])
def test_unproject_tile_edge_vs_cpu_restatement(B):
    """One window (31 zero columns), exactly one tile of 32, and a second workgroup holding one window, at 12 frames."""
    sc, _, _, data, ref, _ = edge_reference(12)
    pose, loss, cond, z0 = sc.reconstruct(data[:B], want_code=True)
    for what, g, r in zip(("cond_emb", "z0", "pose", "loss"), (cond, z0, pose, loss), ref):
        close(g, r[:B], what)


@pytest.mark.parametrize("t", [3, 12])
def test_a_window_does_not_depend_on_its_batch(t):
    """A window's four results from a call of its own are the bits it has at every position of the 33-window batch; a repeated
    call is bit-identical, and so is a call on a part of the batch at another alignment to the unproject tile."""
    sc, _, _, data, _, got = edge_reference(t)
    for b in range(33):
        one = sc.reconstruct(data[b:b + 1], want_code=True)
        for g, o in zip(got, one):
            assert torch.equal(o, g[b:b + 1]), b
    for g, a in zip(got, sc.reconstruct(data, want_code=True)):
        assert torch.equal(g, a)
    for g, a in zip(got, sc.reconstruct(data[5:33], want_code=True)):
        assert torch.equal(g[5:33], a)


@pytest.mark.parametrize("name", ["P6", "P12"])
def test_window_views_equal_materialised_windows(name):
    from mocodad_amd.data import synthetic
    from mocodad_amd.data.windows import TrajectoryWindows
    m = model(name)
    trajs, _ = synthetic.make_trajectories(n_clips=2, frames_per_clip=40, persons_per_clip=2)
    tw = TrajectoryWindows(trajs, seg_len=m.n_frames, num_transform=2)
    dense = tw.materialize()
    sc = m.scorer()
    tw.to("cuda:0")
    a = sc.reconstruct(tw.batch(0, len(tw))[0], want_code=True)
    b = sc.reconstruct(dense, want_code=True)
    assert len(tw) > 33 and torch.isfinite(a[1]).all()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("t", [3, 12])
def test_z_in(t):
    sc, sd, (ci, xi), data, _, got = edge_reference(t)
    data = data[:7]
    own = sc.reconstruct(data, z=got[3][:7], want_code=True)
    for g, o in zip(got, own):
        assert torch.equal(o, g[:7])
    z = torch.randn(7, 32, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = R.reconstruct(sd, data, ci, xi, z=z)
    pose, loss, cond, z0 = sc.reconstruct(data, z=z, want_code=True)
    close(pose, ref[2], "pose of the caller's latents")
    close(loss, ref[3], "loss of the caller's latents")
    assert torch.equal(z0, got[3][:7]) and torch.equal(cond, got[2][:7])      # still the window's own code


def test_decode_latents_of_the_module():
    m = model("P12")
    _, _, _, io = R.load_fixture("P12")
    data = torch.from_numpy(io["data"])
    close(m.decode_latents(batch_of(data), torch.from_numpy(io["z0"])), io["pose"], "decode_latents(z0)")


@pytest.mark.parametrize("t", [3, 12])
@pytest.mark.parametrize("where", ["corrupt", "cond", "z_in"])
def test_nonfinite_window_stays_alone(t, where):
    """B = 7 with a NaN in window 3 -- in a corrupt frame, in a condition frame, in its z_in row: every other window's four outputs
    keep the bits of the clean call, and window 3 yields what it yields as a one-window call."""
    sc, _, _, data, _, _ = edge_reference(t)
    data = data[:7].clone()
    z = torch.randn(7, 32, generator=torch.Generator().manual_seed(5)) if where == "z_in" else None
    clean = [v.clone() for v in sc.reconstruct(data, z=z, want_code=True)]
    if where == "corrupt":
        data[3, 1, 3 + t // 2, 5] = float("nan")
    elif where == "cond":
        data[3, 0, 1, 9] = float("nan")
    else:
        z[3, 17] = float("nan")
    bad = [v.clone() for v in sc.reconstruct(data, z=z, want_code=True)]
    alone = sc.reconstruct(data[3:4], z=None if z is None else z[3:4], want_code=True)
    keep = [0, 1, 2, 4, 5, 6]
    for c, b, a in zip(clean, bad, alone):
        assert torch.equal(b[keep], c[keep])
        assert torch.equal(torch.isnan(b[3:4]), torch.isnan(a)) and torch.equal(torch.nan_to_num(b[3:4]), torch.nan_to_num(a))
    assert not torch.isfinite(bad[1][3]) and torch.isfinite(bad[1][keep]).all()      # (NaN, or the Inf a PReLU's median makes of one)


@pytest.mark.parametrize("name", list(R.FP64_CASES))
def test_rows_vs_fp64(name):
    """One reconstruct call on the case's 45 windows: cond_emb, z0, the reconstructed pose and the per-window loss against the
    restatement in float64, yardstick and factor as the module docstring says.  The decode-alone cases hand the restatement the
    same latents and compare pose and loss only."""
    c = R.fp64_case(name)
    pose, loss, cond, z0 = c["m"].to("cuda:0").scorer().reconstruct(c["data"], c["z"], want_code=True, loss_fn=c["loss_fn"])
    got, missed = (cond, z0, pose, loss), []
    for i, what, kind in R.compared(name):      # every tensor's row is printed before the case fails
        try:
            R.gated("recon", name, what, kind, got[i], c["ref"][i], R.yard_of(c, i))
        except AssertionError as e:
            missed.append(e.args[0])
    assert not missed, missed


def test_rejected_calls():
    """Calls refused before any launch: a handle of the wrong kind (the message names the kind the call needs), null and
    misaligned arguments, a frame split that is not the packed one; n_windows <= 0 is MCD_OK before anything is read."""
    import ctypes as C

    from mocodad_amd import _lib
    sc, _, _, data, _, _ = edge_reference(3)
    L, h = sc.L, sc._h
    cfg = sc._score_cfg(2, 1, 2)
    P_, ODD = C.c_void_p(0x1000), C.c_void_p(0x1004)
    err = lambda: L.mcd_last_error().decode()
    rec = lambda h_, cfg_, data=P_, tab=P_, ws=P_, z=None: L.mcd_latent_reconstruct(h_, C.byref(cfg_), data, None, tab, ws, z, P_, P_, None, None, None)
    assert L.mcd_latent_score(h, C.byref(cfg), P_, None, None, 0, 0, P_, P_, 1, C.c_float(0), P_, None, None, None, None) == -4
    assert "diffusion-stage handle" in err()
    assert L.mcd_latent_denoise(h, P_, P_, P_, 1, 2, P_, None) == -4 and "diffusion-stage handle" in err()
    assert rec(h, sc._score_cfg(0, 1, 2), data=None, tab=None, ws=None) == 0
    assert rec(h, cfg, data=None) == -1 and "null argument" in err()
    assert rec(h, cfg, ws=None) == -1 and "workspace" in err()
    assert rec(h, cfg, ws=ODD) == -1 and "workspace must be 16-byte aligned" in err()
    assert rec(h, cfg, z=ODD) == -1 and "z_in must be 16-byte aligned" in err()
    other = sc._score_cfg(2, 1, 2)
    other.n_cond, other.n_corrupt = 2, 4
    ws = torch.empty(int(L.mcd_latent_workspace_bytes(h, 2)), dtype=torch.uint8, device="cuda:0")
    d = data[:2].cuda()
    assert rec(h, other, data=C.c_void_p(d.data_ptr()), tab=C.c_void_p(sc.table(2).data_ptr()), ws=C.c_void_p(ws.data_ptr())) == -1
    assert "frame split" in err()
    import latent_ref
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    dsd, _, dcfg, _ = latent_ref.load_fixture("B")
    dm = MoCoDADlatent(make_args(dcfg))
    dm.load_state_dict(dsd, strict=False)
    dsc = dm.to("cuda:0").scorer()
    assert rec(dsc._h, dsc._score_cfg(2, 1, 2)) == -4 and "autoencoder handle" in err()
    # the workspace of a diffusion-stage handle is what it was: cond_emb and z0 at 3 frames
    r256 = lambda n: (n + 255) // 256 * 256
    assert int(L.mcd_latent_workspace_bytes(dsc._h, 33)) == r256(33 * 16 * 4) + r256(33 * 32 * 4)
    assert int(L.mcd_latent_workspace_bytes(h, 33)) == r256(33 * 16 * 4) + r256(33 * 32 * 4) + r256(33 * 640 * 3 * 4)

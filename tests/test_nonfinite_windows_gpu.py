"""GPU: a window with non-finite poses stays alone.  The reference scores every window independently (models/mocodad.py:155-180,
models/mocodad_latent.py:97-129): a window whose poses hold a NaN or an Inf comes back non-finite and no other window moves.
Here several windows share a workgroup's LDS as MFMA columns, padded k-steps read the next window's rows against zero
coefficients (NaN x 0 = NaN), and the jointly computed encodings -- cond_emb in score_kernel's prologue, cond_fast_kernel,
cond_unet_kernel and latent_encode_kernel, z0 in the latter -- are never recomputed by a trajectory: the kernels test the joint
result and re-run such windows alone (csrc/mcd_encode_kernel.hpp, "Window isolation").

Per case: score the finite batch; poison one window (NaN, +inf) in slot 0 of a workgroup, in slot 1 and in the last window (whose
workgroup holds a clamped duplicate slot: B = 5 at two windows per workgroup, B = 6 at four); score again; every other window's
outputs are bit-identical (torch.equal), the poisoned window's per-sample losses are all non-finite and its outputs are those of
its own B = 1 call (same NaN mask, equal bits elsewhere); a last call on the finite batch equals the first.  Seeded random-init
models (perturbed BatchNorm statistics and PReLU slopes), the caller's noise (parity mode), ns = 3, S = 2.
Recorded (profiles/nonfinite_windows.txt): 22 passed on this commit; on the parent's kernels the 'E_unet', latent and overflow
cases fail (9), the shipped-encoder pose cases pass."""
import functools

import pytest
import torch

from helpers import golden_weights, make_args
from latent_ref import _perturb

pytestmark = pytest.mark.gpu

NS, S, D = 3, 2, 32
VALUES = (float("nan"), float("inf"))


def _poison(x, k, v, where, frame, joint, coord):
    """One coordinate of window k, or -- aimed at the pad rows -- joints 0 .. 14 of its FIRST frame: the rows a padded k-step of the
    previous window's last frame reads (the 10- / 12-joint stages and the resamplers; a 17-joint mix reads its own joint 16 again,
    mcd_device.hpp mix_stage)."""
    bad = x.clone()
    if where == "one":
        bad[k, coord, frame, joint] = v
    else:
        bad[k, :, 0, 0:15] = v
    return bad


def _seeded(build, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(), torch.no_grad():
        torch.manual_seed(seed + 1)
        m = build()
        _perturb(m, gen)
    return m


@functools.lru_cache(maxsize=None)
def _pose_model(arch, n_cond, n_corrupt):
    from mocodad_amd.models.mocodad import MoCoDAD
    _, cfg = golden_weights("inject")
    return _seeded(lambda: MoCoDAD(make_args(cfg, conditioning_strategy="inject", seg_len=n_cond + n_corrupt,
                                             conditioning_indices=list(range(n_cond)), conditioning_architecture=arch)),
                   4201 + 10 * n_cond + n_corrupt + (100 if arch == "E_unet" else 0))


def _pose_scorer(arch, n_cond, n_corrupt):
    return _pose_model(arch, n_cond, n_corrupt).build_scorer(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _latent_model(arch):
    from latent_ref import load_fixture
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    cfg = load_fixture("B")[2]
    return _seeded(lambda: MoCoDADlatent(make_args(cfg, conditioning_architecture=arch, seg_len=6, conditioning_indices=[0, 1, 2],
                                                   latent_embedding_dim=D, hidden_sizes=[48, D], noise_steps=NS, n_generated_samples=S)),
                   5303 + (100 if arch == "E_unet" else 0))


def _latent_scorer(arch):
    return _latent_model(arch).build_scorer(torch.device("cuda:0"))


def _windows(B, seg_len, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, seg_len, 17, generator=gen).clamp(-2, 2), gen


def _same(a, b):
    """Same NaN mask, equal bits elsewhere (+-inf compare equal to themselves)."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _check(tag, clean, bad, solo, k, B, loss_names, finite_names=()):
    """clean / bad: {name: (B, ...)} of the finite and the poisoned batch; solo: the poisoned window's own B = 1 call."""
    others = [b for b in range(B) if b != k]
    for name in clean:
        c, p = clean[name].cpu(), bad[name].cpu()
        moved = [b for b in others if not torch.equal(p[b], c[b])]
        print(f"nonfinite-windows | {tag} {name}: neighbours that moved {moved}; poisoned window finite elements "
              f"{int(torch.isfinite(p[k]).sum())} / {p[k].numel()}")
        assert torch.isfinite(c).all(), f"{tag} {name}: the finite batch is not finite"
        assert not moved, f"{tag} {name}: windows {moved} changed with window {k} poisoned"
        assert _same(p[k:k + 1], solo[name]), f"{tag} {name}: the poisoned window differs from its own B = 1 call"
    for name in loss_names:
        assert not torch.isfinite(bad[name].cpu()[k]).any(), f"{tag} {name}: the poisoned window has a finite per-sample loss"
    for name in finite_names:
        assert torch.isfinite(bad[name].cpu()[k]).all(), f"{tag} {name}: the reference keeps this output finite"


# ------------------------------------------------------------------------------------------------ pose model
def _pose_outputs(sc, data, noise):
    """Every entry the issue names: score, and score_fused with best / mean / median."""
    out = {}
    loss, poses = sc.score(data, n_samples=S, noise_steps=NS, noise=noise, want_poses=True)
    out["score.loss"], out["score.poses"] = loss, poses
    for aggr in ("best", "mean", "median"):
        agg, all_, poses = sc.score_fused(data, n_samples=S, noise_steps=NS, aggregation=aggr, noise=noise, want_all=True, want_poses=True)
        out[f"fused.{aggr}.agg"], out[f"fused.{aggr}.loss"], out[f"fused.{aggr}.poses"] = agg, all_, poses
    return {k: v.cpu() for k, v in out.items()}


def _aggregation_follows_torch(tag, out):
    """best skips a NaN loss (the reference's strict comparison from 1e10), mean / median return NaN: as tests/test_samples50_gpu.py."""
    for aggr in ("best", "mean", "median"):
        all_, agg = out[f"fused.{aggr}.loss"], out[f"fused.{aggr}.agg"]
        if aggr == "best":
            ref = torch.where(torch.isnan(all_), torch.full_like(all_, 1e10), all_).min(1)[0]
        else:
            ref = all_.mean(1) if aggr == "mean" else all_.median(1)[0]
        assert torch.equal(torch.isnan(agg), torch.isnan(ref)), (tag, aggr, agg, ref)
        ok = ~torch.isnan(ref)
        torch.testing.assert_close(agg[ok], ref[ok], rtol=2e-6, atol=2e-6)


POSE_SHAPES = [("AE", 3, 3, 5), ("AE", 2, 2, 5), ("AE", 1, 1, 6), ("E_unet", 3, 3, 5)]


@pytest.mark.parametrize("split", [1, 0, S], ids=["split1", "split0", "splitS"])
@pytest.mark.parametrize("arch,n_cond,n_corrupt,B", POSE_SHAPES, ids=[f"{a}-{c}+{x}" for a, c, x, _ in POSE_SHAPES])
def test_a_poisoned_condition_frame_stays_alone(arch, n_cond, n_corrupt, B, split):
    """Pose model under `inject`: 3 + 3, 2 + 2 and 1 + 1 frames (two, two and four windows per workgroup of the trajectory kernel)
    with the shipped encoder, 3 + 3 with 'E_unet'; split 1 (the encoder inside the trajectory kernel for the shipped one), the
    library's choice, and S (chain-major: the condition encoder is its own launch)."""
    sc = _pose_scorer(arch, n_cond, n_corrupt)
    sc.set_option("split", split)
    seg = n_cond + n_corrupt
    data, gen = _windows(B, seg, 900 + seg)
    noise = torch.randn(S, NS - 1, B, 2, n_corrupt, 17, generator=gen)
    clean = _pose_outputs(sc, data, noise)
    for k in (0, 1, B - 1):
        for v, where in [(v, "one") for v in VALUES] + [(VALUES[0], "first-frame")]:
            bad = _poison(data, k, v, where, n_cond // 2, 5, 1)
            tag = f"{arch} {n_cond}+{n_corrupt} split={split} window {k} value {v} {where}"
            got = _pose_outputs(sc, bad, noise)
            solo = _pose_outputs(sc, bad[k:k + 1], noise[:, :, k:k + 1])
            _check(tag, clean, got, solo, k, B, [n for n in clean if n.endswith(".loss")])
            _aggregation_follows_torch(tag, got)
    again = _pose_outputs(sc, data, noise)
    for name in clean:
        assert torch.equal(again[name], clean[name]), f"{name}: the call after a poisoned one does not start clean"


def test_a_nan_in_a_corrupt_frame_leaves_the_generated_poses_finite():
    """Under `inject` the corrupt frames are only the loss's ground truth: the reference's generated poses stay finite, the
    losses do not -- and the recovery overwrites nothing it need not."""
    sc = _pose_scorer("AE", 3, 3)
    sc.set_option("split", 1)
    B = 5
    data, gen = _windows(B, 6, 906)
    noise = torch.randn(S, NS - 1, B, 2, 3, 17, generator=gen)
    clean = _pose_outputs(sc, data, noise)
    for k in (0, 1, B - 1):
        bad = data.clone()
        bad[k, 0, 4, 2] = float("nan")
        got = _pose_outputs(sc, bad, noise)
        solo = _pose_outputs(sc, bad[k:k + 1], noise[:, :, k:k + 1])
        _check(f"corrupt-frame NaN window {k}", clean, got, solo, k, B, [n for n in clean if n.endswith(".loss")],
               [n for n in clean if n.endswith(".poses")])
        for name in clean:
            if name.endswith(".poses"):
                assert torch.equal(got[name], clean[name]), f"{name}: the generated poses do not depend on the corrupt frames"


# ------------------------------------------------------------------------------------------------ condition encoders alone
@pytest.mark.parametrize("arch,t", [("AE", 1), ("AE", 2), ("AE", 3), ("E_unet", 1), ("E_unet", 3)], ids=lambda x: str(x))
def test_cond_encode_keeps_a_poisoned_window_alone(arch, t):
    """HipScorer.cond_encode: cond_fast_kernel<1,4>, <2,3>, <3,2> and cond_unet_kernel<1,4>, <3,2>."""
    sc = _pose_scorer(arch, t, 3)
    B = 6 if t == 1 else 5
    data, _ = _windows(B, t + 3, 950 + t)
    cond = data[:, :, :t].contiguous()
    clean = {"cond_emb": sc.cond_encode(cond).cpu()}
    for k in (0, 1, B - 1):
        for v, where in [(v, "one") for v in VALUES] + [(VALUES[0], "first-frame")]:
            bad = _poison(cond, k, v, where, t - 1, 16, 0)
            got = {"cond_emb": sc.cond_encode(bad).cpu()}
            solo = {"cond_emb": sc.cond_encode(bad[k:k + 1]).cpu()}
            _check(f"cond_encode {arch} t={t} window {k} value {v} {where}", clean, got, solo, k, B, ["cond_emb"])
    assert torch.equal(sc.cond_encode(cond).cpu(), clean["cond_emb"])


# ------------------------------------------------------------------------------------------------ latent model
def _latent_outputs(sc, data, noise):
    cond, z0 = sc.encode(data, noise_steps=NS)
    _, loss, lat, code = sc.score(data, n_samples=S, noise_steps=NS, aggregation="all", noise=noise, want_latents=True, want_code=True)
    return {"encode.cond_emb": cond.cpu(), "encode.z0": z0.cpu(), "score.loss": loss.cpu(), "score.latents": lat.cpu(), "score.code": code.cpu()}


@pytest.mark.parametrize("form", ["fused", "split_encode", "E_unet"])
def test_latent_model_keeps_a_poisoned_window_alone(form):
    """MoCoDADlatent at 3 + 3 frames: the two-launch form (latent_encode_kernel<3,2,true>), MCD_LATENT_OPT_SPLIT_ENCODE
    (cond_fast_kernel<3,2> + latent_encode_kernel<3,2,false>) and 'E_unet' (cond_unet_kernel<3,2> + the same).  A non-finite
    condition frame reaches the neighbour's z0 through cond_emb, a non-finite corrupt frame through the shared down path."""
    sc = _latent_scorer("E_unet" if form == "E_unet" else "AE")
    if form == "split_encode":
        sc.set_option("split_encode", 1)
    B = 5
    data, gen = _windows(B, 6, 977)
    noise = torch.randn(S, NS - 1, B, D, generator=gen)
    clean = _latent_outputs(sc, data, noise)
    for k in (0, 1, B - 1):
        for frame in (1, 4):        # a condition frame, a corrupt frame
            for v in VALUES:
                bad = data.clone()
                bad[k, 1, frame, 9] = v
                got = _latent_outputs(sc, bad, noise)
                solo = _latent_outputs(sc, bad[k:k + 1], noise[:, :, k:k + 1])
                # (a corrupt frame is no input of the condition encoder: the reference's cond_emb stays finite)
                _check(f"latent {form} window {k} frame {frame} value {v}", clean, got, solo, k, B, ["score.loss"],
                       ["encode.cond_emb"] if frame == 4 else [])
                assert not torch.isfinite(got["encode.z0"][k]).any()
    again = _latent_outputs(sc, data, noise)
    for name in clean:
        assert torch.equal(again[name], clean[name]), f"{name}: the call after a poisoned one does not start clean"


# ------------------------------------------------------------------------------------------------ overflow
BIG = 3e38      # finite poses whose ENCODING is not: asserted below on the window's own B = 1 call


def test_a_window_whose_encoding_overflows_stays_alone():
    """No pose is non-finite, so no test of the loaded poses could see this window coming: what is tested is the encoders' result."""
    B = 5
    data, gen = _windows(B, 6, 991)
    k = 2
    bad = data.clone()
    bad[k] = BIG
    assert torch.isfinite(bad).all()
    pose = _pose_scorer("AE", 3, 3)
    cond = data[:, :, :3].contiguous()
    cbad = bad[:, :, :3].contiguous()
    solo = {"cond_emb": pose.cond_encode(cbad[k:k + 1]).cpu()}
    assert not torch.isfinite(solo["cond_emb"]).all(), f"cond_emb of poses of {BIG:g} is finite: {solo['cond_emb']}"
    _check("overflow cond_encode", {"cond_emb": pose.cond_encode(cond).cpu()}, {"cond_emb": pose.cond_encode(cbad).cpu()}, solo, k, B, [])
    noise = torch.randn(S, NS - 1, B, 2, 3, 17, generator=gen)
    for split in (1, S):
        pose.set_option("split", split)
        _check(f"overflow pose split={split}", _pose_outputs(pose, data, noise), _pose_outputs(pose, bad, noise),
               _pose_outputs(pose, bad[k:k + 1], noise[:, :, k:k + 1]), k, B, ["score.loss", "fused.best.loss"])
    lat = _latent_scorer("AE")
    lnoise = torch.randn(S, NS - 1, B, D, generator=gen)
    lsolo = _latent_outputs(lat, bad[k:k + 1], lnoise[:, :, k:k + 1])
    assert not torch.isfinite(lsolo["encode.cond_emb"]).all()
    _check("overflow latent", _latent_outputs(lat, data, lnoise), _latent_outputs(lat, bad, lnoise), lsolo, k, B, ["score.loss"])

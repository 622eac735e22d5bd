"""GPU: the latent model's three-launch form -- a condition-encoder kernel of the pose model (cond_unet_kernel, cond_encode_kernel
behind a gather, cond_fast_kernel at another frame count), then the encode launch reading cond_emb, then the chain launch --
against the vectors the reference's MoCoDADlatent produced (tests/golden/gen_latentx_golden.py), against the CPU restatement for
1 .. 12 condition frames, against the fused form on the shipped configuration, and the bit-identity properties the two-launch
form is held to (tests/test_latent_gpu.py).

Gate (the project's): |got - ref| <= 1e-4 max(1, max|ref|) per compared tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import latent_ref as R
import latentx_fixtures as X
from conftest import ROOT
from helpers import make_args
from latent_ref import _perturb

pytestmark = pytest.mark.gpu

_models = {}


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
    """5 windows: two per workgroup, the last workgroup holds one; and a single window."""
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


@pytest.mark.parametrize("arch,tc", [("AE", 1), ("AE", 2), ("AE", 7), ("AE", 12), ("E_unet", 1), ("E_unet", 12), ("E96", 12)])
def test_condition_frame_counts_vs_cpu_restatement(arch, tc):
    """The ends of 1 .. 12 and 7: where cond_fast_kernel / cond_unet_kernel change their windows per workgroup and LDS plan.
    E96 = 'E' with channels [96], h_dim 16 at 12 condition frames: three 96 x 12 x 17 activation buffers (235 KB) do not fit the
    LDS, so cond_encode_kernel keeps its third one in the workspace, behind the gathered frames.
    Random-init perturbed weights, 5 windows, parity mode against tests/latent_ref.py (pinned by tests/test_latentx_golden.py)."""
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    _, _, cfg, _ = X.load("U")
    if arch == "E96":
        arch, cfg = "E", dict(cfg, channels=[96], h_dim=16)
    T, D, ns, S, B = tc + 3, 32, 3, 2, 5
    gen = torch.Generator().manual_seed(100 * tc + len(arch))
    torch.manual_seed(7 + tc)
    with torch.no_grad():
        m = MoCoDADlatent(make_args(cfg, conditioning_architecture=arch, seg_len=T, conditioning_indices=list(range(tc)),
                                    noise_steps=ns, n_generated_samples=S))
        _perturb(m, gen)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        ci, xi = m._frame_split()
        assert (len(ci), len(xi)) == (tc, 3)
        data = torch.randn(B, 2, T, 17, generator=gen)
        noise = torch.randn(S, ns - 1, B, D, generator=gen)
        rc, rz, rlat, rloss = R.score(sd, data, noise, noise_steps=ns, cond_idx=ci, corrupt_idx=xi)
    sc = m.to("cuda:0").scorer()
    cond, z0 = sc.encode(data, noise_steps=ns)
    close(cond, rc.numpy(), "cond_emb")
    close(z0, rz.numpy(), "z0")
    _, loss_all, lat, code = sc.score(data, n_samples=S, noise_steps=ns, noise=noise, want_latents=True, want_code=True)
    close(code, rz.numpy(), "latent_code")
    close(lat, rlat.numpy(), "latent_all")
    close(loss_all, rloss.numpy(), "loss_all")
    assert torch.isfinite(loss_all).all()


def test_split_encode_equals_the_fused_form_on_the_shipped_configuration():
    """MCD_LATENT_OPT_SPLIT_ENCODE: cond_fast_kernel<3,2> + the encode launch reading cond_emb, against the one fused launch, on
    the same handle (A_benign, 37 windows).  Both run cond_fast_body and the same remainder on the same values: cond_emb, z0 and
    everything the chain launch makes of them are bit-identical."""
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    sd, _, cfg, io = R.load_fixture("A_benign")
    m = MoCoDADlatent(make_args(cfg))
    m.load_state_dict(sd, strict=False)
    sc = m.build_scorer(torch.device("cuda:0"))
    data, noise = torch.from_numpy(io["data"]), torch.from_numpy(io["noise"])
    kw = dict(n_samples=3, noise_steps=10, noise=noise, aggregation="best", want_all=True, want_latents=True, want_code=True)
    fused = [t.clone() for t in sc.encode(data, noise_steps=10)]
    fused_s = [t.clone() for t in sc.score(data, **kw)]
    need = int(sc.L.mcd_latent_workspace_bytes(sc._h, 37))
    sc.set_option("split_encode", 1)
    assert int(sc.L.mcd_latent_workspace_bytes(sc._h, 37)) == need        # (a pure function of the handle and n_windows)
    split = sc.encode(data, noise_steps=10)
    split_s = sc.score(data, **kw)
    for f, s, what in zip(fused, split, ("cond_emb", "z0")):
        print(f"{what}: max |fused - split| = {(f - s).abs().max().item():.3e}  bit-identical: {torch.equal(f, s)}")
        close(s, f.cpu().numpy(), f"{what}: split form vs fused form")
        close(s, io[what], f"{what}: split form vs reference")
    for f, s, what in zip(fused, split, ("cond_emb", "z0")):
        assert torch.equal(f, s), what
    for f, s in zip(fused_s, split_s):
        assert torch.equal(f, s)
    sc.set_option("split_encode", 0)
    assert torch.equal(sc.encode(data, noise_steps=10)[1], fused[1])      # (the fused form again: a repeat is bit-identical)
    with pytest.raises(ValueError, match="unknown option"):
        sc.set_option("bogus", 1)


@pytest.mark.parametrize("name", ["U", "C7"])
def test_window_views_score_like_materialised_windows(name):
    from mocodad_amd.data import synthetic
    from mocodad_amd.data.windows import TrajectoryWindows
    m = model(name)
    trajs, _ = synthetic.make_trajectories(n_clips=2, frames_per_clip=30, persons_per_clip=2)
    tw = TrajectoryWindows(trajs, seg_len=m.n_frames, num_transform=5)
    dense = tw.materialize()
    sc = m.scorer()
    tw.to("cuda:0")
    kw = dict(n_samples=2, noise_steps=4, seed=3, aggregation="best", want_all=True, want_latents=True, want_code=True)
    a = sc.score(tw.batch(0, len(tw))[0], **kw)
    b = sc.score(dense, **kw)
    assert len(tw) > 64 and torch.isfinite(a[1]).all()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ca, za = sc.encode(tw.batch(0, len(tw))[0])
    cb, zb = sc.encode(dense)
    assert torch.equal(ca, cb) and torch.equal(za, zb)


@pytest.mark.parametrize("name", ["U", "C7"])
def test_batch_split_repeats_streams_and_poisoned_lds_are_bit_identical(name):
    from mocodad_amd import _lib
    L = _lib.lib()
    _, _, _, io = X.load(name)
    D, ns, S, B = (int(v) for v in io["sizes"])
    sc = model(name).scorer()
    data, noise = torch.from_numpy(io["data"]).cuda(), torch.from_numpy(io["noise"]).cuda()
    kw = dict(n_samples=S, noise_steps=ns, aggregation="mean", want_all=True, want_latents=True)
    for parity in (False, True):
        nz = (lambda lo, hi: noise[:, :, lo:hi].contiguous()) if parity else (lambda lo, hi: None)
        whole = [t.clone() for t in sc.score(data, noise=nz(0, B), seed=5, first_window_id=100, **kw)[:3]]
        assert torch.isfinite(whole[1]).all()
        a = sc.score(data[:2], noise=nz(0, 2), seed=5, first_window_id=100, **kw)
        b = sc.score(data[2:], noise=nz(2, B), seed=5, first_window_id=102, **kw)
        for w, x, y in zip(whole, a[:3], b[:3]):
            assert torch.equal(w, torch.cat([x, y])), parity
        again = sc.score(data, noise=nz(0, B), seed=5, first_window_id=100, **kw)[:3]
        torch.cuda.synchronize()
        outs = []
        for st in (torch.cuda.Stream(), torch.cuda.Stream()):
            with torch.cuda.stream(st):
                outs.append(sc.score(data, noise=nz(0, B), seed=5, first_window_id=100, **kw)[:3])
        torch.cuda.synchronize()
        assert L.mcd_debug_poison_lds(None) == 0
        poisoned = sc.score(data, noise=nz(0, B), seed=5, first_window_id=100, **kw)[:3]
        assert L.mcd_debug_poison_lds(None) == 0
        enc = sc.encode(data, noise_steps=ns)
        for got in [again, poisoned] + outs:
            for w, g in zip(whole, got):
                assert torch.equal(w, g), parity
        close(enc[0], io["cond_emb"], "cond_emb after poisoning")
        close(enc[1], io["z0"], "z0 after poisoning")


def test_driver_end_to_end_with_the_unet_condition_encoder(tmp_path):
    """eval_MoCoDAD.py on the latent YAML with conditioning_architecture 'E_unet' runs the test loop to an AUC (a fresh process)."""
    src = open(os.path.join(ROOT, "configs", "ubnormal_latent_test.yaml")).read()
    assert "conditioning_architecture: 'AE'" in src
    cfg = tmp_path / "latent_eunet.yaml"
    cfg.write_text(src.replace("conditioning_architecture: 'AE'", "conditioning_architecture: 'E_unet'"))
    cmd = [sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", str(cfg), "--synthetic", "4", "--random-init"]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    auc = float(p.stdout.rsplit("AUC:", 1)[1].split()[0])
    assert 0.0 <= auc <= 1.0, p.stdout[-500:]

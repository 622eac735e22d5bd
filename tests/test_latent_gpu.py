"""GPU: the latent model's two launches (mcd_latent_encode / the chain kernel behind mcd_latent_denoise and mcd_latent_score)
against the vectors the reference's MoCoDADlatent produced (tests/golden/gen_latent_golden.py), and the properties the pose path's
kernels are held to: perf mode == parity mode on the exported draws, bit-identical repeats / streams / batch splits / window
views, chain independence under a NaN, no read of uninitialised LDS, the driver end to end.

Gate (the project's): |got - ref| <= 1e-4 max(1, max|ref|) per compared tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import latent_ref as R
from conftest import ROOT
from helpers import make_args

pytestmark = pytest.mark.gpu

AGGRS = ["best", "worst", "mean", "median", "quantile:0.3", "mean_pose", "median_pose"]
_models = {}


def close(got, ref, what):
    ref = np.asarray(ref)
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=what)


def model(name, **over):
    """The module with the fixture's weights on cuda:0 (one per fixture and session)."""
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    key = (name, tuple(sorted(over.items())))
    if key not in _models:
        sd, _, cfg, _ = R.load_fixture(name)
        m = MoCoDADlatent(make_args(cfg, **over))
        m.load_state_dict(sd, strict=False)
        _models[key] = m.to("cuda:0")
    return _models[key]


@pytest.mark.parametrize("name", ["A_benign", "A_hostile", "B"])
def test_encode_vs_reference(name):
    """37 / 5 windows: odd counts, the last workgroup holds one window."""
    _, _, _, io = R.load_fixture(name)
    cond, z0 = model(name).scorer().encode(torch.from_numpy(io["data"]), noise_steps=int(io["sizes"][1]))
    close(cond, io["cond_emb"], "cond_emb")
    close(z0, io["z0"], "z0")


@pytest.mark.parametrize("name", ["A_benign", "A_hostile", "B"])
def test_denoiser_pass_vs_reference(name):
    """One denoiser pass at the chain's first and last step: all S*B rows (111 for (A): seven n-tiles, the last one ragged), and
    a single row."""
    _, _, _, io = R.load_fixture(name)
    D, ns, S, B = (int(v) for v in io["sizes"])
    sc = model(name).scorer()
    x = torch.from_numpy(io["noise"])[:, 0].reshape(S * B, D)
    c = torch.from_numpy(io["cond_emb"]).repeat(S, 1)
    for t in sorted({1, ns - 1}):
        close(sc.denoise(x, t, c, noise_steps=ns), io[f"eps_t{t}"], f"eps_t{t}")
        close(sc.denoise(x[-1:], t, c[-1:], noise_steps=ns), io[f"eps_t{t}"][-1:], f"eps_t{t}, one row")


@pytest.mark.parametrize("name", ["A_benign", "A_hostile", "B", "C"])
def test_score_parity_mode_vs_reference(name):
    _, _, _, io = R.load_fixture(name)
    D, ns, S, B = (int(v) for v in io["sizes"])
    m = model(name)
    data, noise = torch.from_numpy(io["data"]), torch.from_numpy(io["noise"])
    _, loss_all, lat, code = m.scorer().score(data, n_samples=S, noise_steps=ns, noise=noise, want_latents=True, want_code=True)
    close(code, io["z0"], "latent_code")
    close(lat, io["latent_all"], "latent_all")
    close(loss_all, io["loss_all"], "loss_all")
    batch = [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, 6, dtype=torch.int32)]
    out = m.forward(batch, aggr_strategy="all", return_="all", noise=noise)
    close(out[0], io["loss_all"], "forward all: loss")
    close(out[1], io["latent_all"], "forward all: latents")
    for a in AGGRS:
        tag = a.replace(":", "_")
        loss, sel = m.forward(batch, aggr_strategy=a, return_="all", noise=noise)[:2]
        close(loss, io[f"loss_{tag}"], f"forward {a}: loss")
        assert (sel is None) == (f"sel_{tag}" not in io)
        if sel is not None:
            close(sel, io[f"sel_{tag}"], f"forward {a}: selected latent")
        # the one-call form (aggregation inside the chain launch) that test_step takes
        close(m.forward(batch, aggr_strategy=a, return_="loss", noise=noise)[0], io[f"loss_{tag}"], f"forward {a}: loss only")


def test_perf_mode_is_parity_mode_with_the_exported_draws():
    sd, _, _, io = R.load_fixture("A_benign")
    sc = model("A_benign").scorer()
    for ns, S, nb in ((10, 3, 37), (2, 1, 37), (3, 2, 37), (3, 40, 5)):      # (40 samples: a window's chains take two passes of 32 columns)
        data = torch.from_numpy(io["data"])[:nb]
        kw = dict(n_samples=S, noise_steps=ns, aggregation="median", want_all=True, want_latents=True)
        perf = sc.score(data, seed=77, first_window_id=1000, **kw)
        z = sc.philox_noise(data.shape[0], n_samples=S, noise_steps=ns, seed=77, first_window_id=1000)
        par = sc.score(data, noise=z, **kw)
        for a, b in zip(perf[:3], par[:3]):
            assert torch.equal(a, b), (ns, S)
        # ... and the CPU restatement fed those draws computes the same losses: the timed mode runs the reference's algorithm
        with torch.no_grad():
            _, _, _, ref = R.score(sd, data, z.cpu(), noise_steps=ns)
        close(perf[1], ref.numpy(), f"perf-mode losses vs CPU, ns {ns} S {S}")


def test_exported_draws_are_standard_normal_and_distinct():
    from scipy import stats
    sc = model("A_benign").scorer()
    S, ns, B = 4, 10, 512
    z = sc.philox_noise(B, n_samples=S, noise_steps=ns, seed=20261017, first_window_id=4321).cpu().double()      # (S,K,B,64)
    flat = z.reshape(-1).numpy()
    n = flat.size
    assert n >= 1_000_000
    m, v = flat.mean(), flat.var()
    sk, ku = stats.skew(flat), stats.kurtosis(flat)
    print(f"n={n} mean={m:.3e} var={v:.6f} skew={sk:.3e} excess kurtosis={ku:.3e}")
    assert abs(m) < 4 / np.sqrt(n) and abs(v - 1) < 4 * np.sqrt(2 / n)
    assert abs(sk) < 4 * np.sqrt(6 / n) and abs(ku) < 4 * np.sqrt(24 / n)
    d, p = stats.kstest(flat[:1_000_000], "norm")
    assert p > 1e-3, (d, p)

    def corr(a, b):
        a, b = a.reshape(-1), b.reshape(-1)
        return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))
    lim = lambda k: 4.5 / np.sqrt(k)
    pairs = {"neighbouring elements": (z[..., :-1], z[..., 1:]), "consecutive steps": (z[:, :-1], z[:, 1:]),
             "consecutive samples": (z[:-1], z[1:]), "consecutive windows": (z[:, :, :-1], z[:, :, 1:]),
             "squares within a Philox call": (z[..., 0::4] ** 2, z[..., 1::4] ** 2)}
    for name, (a, b) in pairs.items():
        assert abs(corr(a, b)) < lim(a.numel()), name
    assert np.unique(flat).size > 0.99 * n          # distinct draws, not a repeated block
    z2 = sc.philox_noise(B, n_samples=S, noise_steps=ns, seed=20261018, first_window_id=4321).cpu().double()
    assert abs(corr(z, z2)) < lim(n)
    z3 = sc.philox_noise(B // 2, n_samples=S, noise_steps=ns, seed=20261017, first_window_id=4321 + B // 2).cpu().double()
    assert torch.equal(z3, z[:, :, B // 2:])


def test_repeats_and_overlapping_streams_are_bit_identical():
    sc = model("A_benign").scorer()
    gen = torch.Generator().manual_seed(9)
    batches = [torch.randn(333, 2, 6, 17, generator=gen).cuda() for _ in range(4)]
    kw = dict(n_samples=3, noise_steps=6, aggregation="best", want_all=True)
    ref = [[t.clone() for t in sc.score(b, seed=40 + i, **kw)[:2]] for i, b in enumerate(batches)]
    again = [sc.score(b, seed=40 + i, **kw)[:2] for i, b in enumerate(batches)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = []
    for i, b in enumerate(batches):
        with torch.cuda.stream(streams[i % 2]):
            out.append(sc.score(b, seed=40 + i, **kw)[:2])
    torch.cuda.synchronize()
    for r, a, o in zip(ref, again, out):
        assert torch.isfinite(r[1]).all()
        assert torch.equal(r[0], a[0]) and torch.equal(r[1], a[1])
        assert torch.equal(r[0], o[0]) and torch.equal(r[1], o[1])


def test_batch_split_with_window_offset_is_bit_identical():
    _, _, _, io = R.load_fixture("A_benign")
    sc = model("A_benign").scorer()
    data, noise = torch.from_numpy(io["data"]), torch.from_numpy(io["noise"])
    kw = dict(n_samples=3, noise_steps=10, aggregation="mean", want_all=True, want_latents=True)
    for parity in (False, True):
        nz = (lambda lo, hi: noise[:, :, lo:hi].contiguous()) if parity else (lambda lo, hi: None)
        whole = sc.score(data, noise=nz(0, 37), seed=5, first_window_id=100, **kw)
        a = sc.score(data[:20], noise=nz(0, 20), seed=5, first_window_id=100, **kw)
        b = sc.score(data[20:], noise=nz(20, 37), seed=5, first_window_id=120, **kw)
        for w, x, y in zip(whole[:3], a[:3], b[:3]):
            assert torch.equal(w, torch.cat([x, y])), parity


def test_window_views_score_like_materialised_windows():
    from mocodad_amd.data import synthetic
    from mocodad_amd.data.windows import TrajectoryWindows
    trajs, _ = synthetic.make_trajectories(n_clips=2, frames_per_clip=30, persons_per_clip=2)
    tw = TrajectoryWindows(trajs, seg_len=6, num_transform=5)
    dense = tw.materialize()
    sc = model("A_benign").scorer()
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


def test_a_nan_chain_changes_no_other_chain():
    _, _, _, io = R.load_fixture("A_benign")
    sc = model("A_benign").scorer()
    data, noise = torch.from_numpy(io["data"]), torch.from_numpy(io["noise"]).clone()
    kw = dict(n_samples=3, noise_steps=10, want_all=True, want_latents=True)
    ref = {a: sc.score(data, noise=noise, aggregation=a, **kw) for a in ("best", "mean")}
    noise[1, 4, 17, 5] = float("nan")          # sample 1 of window 17, the z of step 6
    for a in ("best", "mean"):
        agg, loss, lat, _ = sc.score(data, noise=noise, aggregation=a, **kw)
        assert torch.isnan(loss[17, 1]) and torch.isnan(lat[17, 1]).any()
        keep = torch.ones(37, 3, dtype=torch.bool)
        keep[17, 1] = False
        assert torch.equal(loss.cpu()[keep], ref[a][1].cpu()[keep]) and torch.equal(lat.cpu()[keep], ref[a][2].cpu()[keep])
        others = torch.arange(37) != 17
        assert torch.equal(agg.cpu()[others], ref[a][0].cpu()[others])
        if a == "best":      # the strict comparison skips the NaN sample, as aggregate_kernel and the reference do
            assert agg[17].item() == min(loss[17, 0].item(), loss[17, 2].item())
        else:
            assert torch.isnan(agg[17])


def test_no_uninitialised_lds_reads():
    from mocodad_amd import _lib
    _, _, _, io = R.load_fixture("B")
    L = _lib.lib()
    for name in ("A_benign", "B"):
        _, _, _, io = R.load_fixture(name)
        D, ns, S, B = (int(v) for v in io["sizes"])
        sc = model(name).scorer()
        data, noise = torch.from_numpy(io["data"]), torch.from_numpy(io["noise"])
        kw = dict(n_samples=S, noise_steps=ns, noise=noise, aggregation="worst", want_all=True, want_latents=True)
        ref = [t.clone() for t in sc.score(data, **kw)[:3]]
        assert L.mcd_debug_poison_lds(None) == 0
        got = sc.score(data, **kw)[:3]
        assert L.mcd_debug_poison_lds(None) == 0
        x, c = noise[:, 0].reshape(S * B, D), torch.from_numpy(io["cond_emb"]).repeat(S, 1)
        eps = sc.denoise(x, 1, c, noise_steps=ns)
        for r, g in zip(ref, got):
            assert torch.equal(r, g), name
        close(eps, io["eps_t1"], "eps_t1 after poisoning")


def test_driver_end_to_end_on_synthetic_clips():
    """eval_MoCoDAD.py picks MoCoDADlatent from the YAML and runs the test loop to an AUC (a fresh process, as a user starts it)."""
    cmd = [sys.executable, os.path.join(ROOT, "eval_MoCoDAD.py"), "-c", os.path.join(ROOT, "configs", "ubnormal_latent_test.yaml"),
           "--synthetic", "4", "--random-init"]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    auc = float(p.stdout.rsplit("AUC:", 1)[1].split()[0])
    assert 0.0 <= auc <= 1.0, p.stdout[-500:]

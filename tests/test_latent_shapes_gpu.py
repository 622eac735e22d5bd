"""GPU: latent_chain_kernel (and the D-dependent end of the encode launch) where width, depth and sample count branch: the
denoiser shapes of latent_ref.LATENT_SHAPES -- one layer, odd and even depths, the maximum of eight, m-tile counts that do not
divide over the four waves, every k-block count, a 16-wide layer between wide ones -- and sample counts around the 32 columns of
a pass, the 64 of the sort's comment and the limit of 1024.  Random-init models (latent_ref.random_latent_model).

Gates.  Hard, the project's: |got - ref64| <= 1e-4 max(1, max|ref64|) per tensor.  Sharp, for eps, latents and losses:
max|gpu - ref64| <= 4 max|cpu32 - ref64|, the right side being the error of the fp32 CPU restatement on the same inputs; two fp32
evaluation orders stay within 2 of each other (tests/test_latent_shapes_host.py), the margin is twice that.  Bit-identity
wherever the kernel's structure gives it: a column's result depends neither on its neighbours, nor on the samples sharing its
call, nor on where its draws come from.  Every compared figure is printed (`latent-shapes |` rows; the recorded run is
profiles/latent_shapes_fp64.txt)."""
import numpy as np
import pytest
import torch

import latent_ref as R

pytestmark = pytest.mark.gpu

NS = 10
IDS = R.SHAPE_IDS
ALL = range(len(R.LATENT_SHAPES))
ODD, ONE_WIDE, ONE_NARROW = 4, 1, 0        # [16,112,48]; [128]; [16]
SAMPLE_COUNTS = [1, 2, 3, 5, 7, 16, 31, 32, 33, 64, 65, 100]
_ref1024 = {}


def scorer(i, tame):
    """-> (LatentScorer on cuda:0, fp32 state_dict) of shape i; packed once per session."""
    D, hidden = R.LATENT_SHAPES[i]
    m, sd = R.random_latent_model(D, hidden, seed=100 + i, ns=NS, S=3, tame=tame)
    return m.to("cuda:0").scorer(), sd


def close(got, ref, what):
    ref = np.asarray(ref)
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=what)


def measure(test, i, what, got, ref64, cpu32):
    """Prints one row of the table -> (max|gpu - ref64|, max|cpu32 - ref64|, max|ref64|)."""
    assert ref64.dtype == torch.float64 and torch.isfinite(ref64).all(), what
    got = got.detach().cpu().double()
    err, yard, top = (got - ref64).abs().max().item(), (cpu32.double() - ref64).abs().max().item(), ref64.abs().max().item()
    print(f"latent-shapes | {test:7s} | {IDS[i]:24s} | {what:22s} | max|ref64| {top:9.3e} | gpu {err:9.3e} | cpu32 {yard:9.3e} | "
          f"ratio {err / yard if yard > 0 else float('inf'):6.2f} | rel {err / max(1.0, top):9.3e}")
    assert torch.isfinite(got).all(), what
    return err, yard, top


def gated(test, i, what, got, ref64, cpu32):
    err, yard, top = measure(test, i, what, got, ref64, cpu32)
    assert err <= 1e-4 * max(1.0, top), (what, err, top)
    assert err <= 4 * yard, (what, err, yard)


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_one_pass_vs_fp64(i):
    """mcd_latent_denoise on 70 rows (three workgroups, the last with 6 of its 32 columns) at the first, second and last step,
    untamed weights (eps of O(2)); then rows 0, 31, 32, 69 from a call of their own and rows 31 .. 63 from a 33-row call: a
    column's MFMA result does not depend on its neighbours or on its place in the workgroup, so these are bit-identical."""
    sc, sd = scorer(i, tame=False)
    sd64 = R.to_f64(sd)
    x, c = R.pass_inputs(i)
    for t in (0, 1, NS - 1):
        with torch.no_grad():
            ref, cpu = R.denoise(sd64, x.double(), t, c.double()), R.denoise(sd, x, t, c)
        eps = sc.denoise(x, t, c, noise_steps=NS)
        gated("pass", i, f"eps t={t}", eps, ref, cpu)
        for r in (0, 31, 32, 69):
            assert torch.equal(sc.denoise(x[r:r + 1], t, c[r:r + 1], noise_steps=NS), eps[r:r + 1]), (t, r)
        assert torch.equal(sc.denoise(x[31:64], t, c[31:64], noise_steps=NS), eps[31:64]), t


@pytest.mark.parametrize("i", [0, 4, 6, 3, 5, 1], ids=lambda i: f"D{R.LATENT_SHAPES[i][0]}")
def test_encode_vs_fp64(i):
    """to_time_dim's `u < D * 16` loop at D 16, 48, 80, 96, 112, 128 (5 windows: the last workgroup holds one)."""
    sc, sd = scorer(i, tame=True)
    data, _ = R.chain_inputs(i, NS, 1, 5)
    with torch.no_grad():
        ref = R.encode(R.to_f64(sd), data.double(), (0, 1, 2), (3, 4, 5))
        cpu = R.encode(sd, data, (0, 1, 2), (3, 4, 5))
    got = sc.encode(data, noise_steps=NS)
    for g, r, c, what in zip(got, ref, cpu, ("cond_emb", "z0")):
        assert tuple(g.shape) == tuple(r.shape)
        measure("encode", i, what, g, r, c)
        close(g, r.numpy(), what)


def chains_vs_fp64(test, i, sc, sd, data, noise, ns, S, loss_fn):
    """One parity-mode call; the fp64 chain is fed the GPU's own cond_emb and latent_code, so the chain launch alone is judged."""
    _, loss, lat, code = sc.score(data, n_samples=S, noise_steps=ns, noise=noise, loss_fn=loss_fn, want_all=True, want_latents=True,
                                  want_code=True)
    cond, z0 = sc.encode(data, noise_steps=ns)
    assert torch.equal(z0, code)
    cond, z0 = cond.cpu(), code.cpu()
    with torch.no_grad():
        ref = R.chain(R.to_f64(sd), cond.double(), z0.double(), noise.double(), ns)
        cpu = R.chain(sd, cond, z0, noise, ns)
        gated(test, i, f"latents ns={ns} S={S}", lat, ref, cpu)
        gated(test, i, f"{loss_fn} ns={ns} S={S}", loss, R.losses(ref, z0.double(), loss_fn), R.losses(cpu, z0, loss_fn))
    return loss, lat


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_chains_vs_fp64(i):
    """ns 10, S 3, 13 windows: 10 windows per workgroup, two workgroups, the second holding 3 windows (9 of 32 columns).  Tamed
    weights: max|latent| 550 .. 810 comes from the schedule."""
    sc, sd = scorer(i, tame=True)
    data, noise = R.chain_inputs(i, NS, 3, 13)
    for loss_fn in (("smooth_l1", "l1", "mse") if i == ODD else ("smooth_l1",)):
        chains_vs_fp64("chain", i, sc, sd, data, noise, NS, 3, loss_fn)


def calls_at_1024(i):
    """-> (scorer, state_dict, windows, 1024 samples of draws, loss_all and latent_all of the S = 1024 call) at ns 3, 13 windows."""
    if i not in _ref1024:
        sc, sd = scorer(i, tame=True)
        data, noise = R.chain_inputs(i, 3, 1024, 13)
        _, loss, lat, _ = sc.score(data, n_samples=1024, noise_steps=3, noise=noise, want_all=True, want_latents=True)
        assert torch.isfinite(loss).all() and torch.isfinite(lat).all()
        _ref1024[i] = (sc, sd, data, noise, loss.clone(), lat.clone())
    return _ref1024[i]


@pytest.mark.parametrize("i", [ODD, ONE_WIDE, ONE_NARROW], ids=lambda i: IDS[i])
def test_a_chain_does_not_depend_on_the_samples_sharing_its_call(i):
    """S = 1 .. 100 against the first S samples of the S = 1024 call (one window per workgroup, 32 passes), bit for bit: 32, 16,
    10, 6, 4, 2 and 1 windows per workgroup, ragged last workgroups, 28 / 30 / 31 of 32 columns, exactly one pass, a pass
    holding one chain, two, three and four passes.  The S = 1 call against fp64 anchors the family."""
    sc, sd, data, noise, loss_ref, lat_ref = calls_at_1024(i)
    for S in SAMPLE_COUNTS:
        _, loss, lat, _ = sc.score(data, n_samples=S, noise_steps=3, noise=noise[:S], want_all=True, want_latents=True)
        assert torch.equal(loss, loss_ref[:, :S]), S
        assert torch.equal(lat, lat_ref[:, :S]), S
    loss, lat = chains_vs_fp64("samples", i, sc, sd, data, noise[:1], 3, 1, "smooth_l1")
    assert torch.equal(loss, loss_ref[:, :1]) and torch.equal(lat, lat_ref[:, :1])


def test_in_kernel_aggregation_at_every_sample_count():
    """loss_agg of a call against the same call's loss_all: best, worst, median and the quantiles 0 and 1 pick an element (exact);
    mean is the kernel's sequential fp32 sum in sample order (exact); an interior quantile is torch.quantile's two-sided lerp at
    the same fp32 position, so the two differ by the contraction of a multiply-add: 4 ulp of the row's largest loss."""
    sc, _, data, noise, _, _ = calls_at_1024(ODD)
    for S in SAMPLE_COUNTS:
        for aggr in ("best", "worst", "mean", "median", "quantile:0", "quantile:0.3", "quantile:0.5", "quantile:1"):
            agg, loss, _, _ = sc.score(data, n_samples=S, noise_steps=3, noise=noise[:S], aggregation=aggr, want_all=True)
            agg, loss = agg.cpu(), loss.cpu()
            assert torch.isfinite(loss).all() and loss.min() >= 0 and loss.max() < 1e10
            if aggr in ("best", "quantile:0"):
                assert torch.equal(agg, loss.min(1).values), (S, aggr)
            elif aggr in ("worst", "quantile:1"):
                assert torch.equal(agg, loss.max(1).values), (S, aggr)
            elif aggr == "median":
                assert torch.equal(agg, loss.median(1).values), (S, aggr)
            elif aggr == "mean":
                acc = np.zeros(loss.shape[0], dtype=np.float32)
                for s in range(S):
                    acc = acc + loss[:, s].numpy()
                assert np.array_equal(agg.numpy(), acc / np.float32(S)), (S, aggr)
            else:
                ref = torch.quantile(loss, float(aggr.split(":")[1]), dim=1)
                np.testing.assert_allclose(agg.numpy(), ref.numpy(), rtol=0, atol=4 * 2.0 ** -23 * float(loss.max()), err_msg=f"{aggr} S={S}")


@pytest.mark.parametrize("S,bad", [(40, 35), (1024, 700)])
def test_one_nan_chain(S, bad):
    """A NaN in the x_T of one sample of window 5 -- in the second pass of 32 columns at S 40, in the 22nd at S 1024: every other
    chain is bit-identical to the clean call, median and quantile of that window are NaN, best and worst skip the sample."""
    sc, _, data, noise, _, _ = calls_at_1024(ODD)
    hit = noise[:S].clone()
    hit[bad, 0, 5, 7] = float("nan")
    keep = torch.ones(13, S, dtype=torch.bool)
    keep[5, bad] = False
    others = torch.arange(13) != 5
    for aggr in ("best", "worst", "median", "quantile:0.3"):
        kw = dict(n_samples=S, noise_steps=3, aggregation=aggr, want_all=True, want_latents=True)
        agg0, loss0, lat0 = (t.cpu() for t in sc.score(data, noise=noise[:S], **kw)[:3])
        agg, loss, lat = (t.cpu() for t in sc.score(data, noise=hit, **kw)[:3])
        assert torch.isfinite(loss0).all() and torch.isfinite(agg0).all()
        assert torch.isnan(loss[5, bad]) and torch.isnan(lat[5, bad]).any()
        assert torch.equal(loss[keep], loss0[keep]) and torch.equal(lat[keep], lat0[keep]), aggr
        assert torch.equal(agg[others], agg0[others]), aggr
        rest = loss0[5][keep[5]]
        if aggr == "best":
            assert agg[5] == rest.min()
        elif aggr == "worst":
            assert agg[5] == rest.max()
        else:
            assert torch.isnan(agg[5]), aggr


@pytest.mark.parametrize("i", [ONE_NARROW, ONE_WIDE], ids=lambda i: f"D{R.LATENT_SHAPES[i][0]}")
def test_perf_mode_is_parity_mode_on_the_exported_draws(i):
    """D 16 (4 element groups per chain) and D 128 (32), S 33 (a second pass holding one chain), ns 4."""
    sc, _ = scorer(i, tame=True)
    data, _ = R.chain_inputs(i, 4, 1, 13)
    kw = dict(n_samples=33, noise_steps=4, aggregation="median", want_all=True, want_latents=True)
    perf = sc.score(data, seed=20261018, first_window_id=4321, **kw)
    z = sc.philox_noise(13, n_samples=33, noise_steps=4, seed=20261018, first_window_id=4321)
    assert tuple(z.shape) == (33, 3, 13, R.LATENT_SHAPES[i][0])
    par = sc.score(data, noise=z, **kw)
    for a, b in zip(perf[:3], par[:3]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    groups = z.cpu().reshape(-1, 4)
    assert torch.isfinite(groups).all()
    assert torch.unique(groups, dim=0).shape[0] == groups.shape[0]      # no element group drawn twice (a wrong group index would)

"""CPU: the float64 reference and the fp32 yardstick that tests/test_latent_shapes_gpu.py measures latent_chain_kernel against,
on the shapes of latent_ref.LATENT_SHAPES and the inputs of those tests.  Nothing here runs a kernel: these tests say that the
reference is finite and that the yardstick does not depend on the summation order it happens to be evaluated in."""
import pytest
import torch

import latent_ref as R

NS = 10
IDS = R.SHAPE_IDS
_refs = {}


def references(i):
    """fp64 eps of one pass at t = 0, 1, ns - 1 (untamed weights) and fp64 cond_emb, z0, latents, losses of the chains at
    ns 10, S 3, B 13 (tamed weights): once per shape and session."""
    if i not in _refs:
        D, hidden = R.LATENT_SHAPES[i]
        with torch.no_grad():
            sd = R.random_latent_model(D, hidden, seed=100 + i, ns=NS, S=3, tame=False)[1]
            x, c = R.pass_inputs(i)
            eps = {t: R.denoise(R.to_f64(sd), x.double(), t, c.double()) for t in (0, 1, NS - 1)}
            sdt = R.random_latent_model(D, hidden, seed=100 + i, ns=NS, S=3, tame=True)[1]
            data, noise = R.chain_inputs(i, NS, 3, 13)
            cond, z0, lat, loss = R.score(R.to_f64(sdt), data.double(), noise.double(), noise_steps=NS)
        _refs[i] = dict(sd=sd, sdt=sdt, eps=eps, cond=cond, z0=z0, lat=lat, loss=loss, noise=noise)
    return _refs[i]


@pytest.mark.parametrize("i", range(len(R.LATENT_SHAPES)), ids=IDS)
def test_fp64_reference_is_finite(i):
    r = references(i)
    for t, e in r["eps"].items():
        assert e.dtype == torch.float64 and torch.isfinite(e).all(), t
    for k in ("cond", "z0", "lat", "loss"):
        assert r[k].dtype == torch.float64 and torch.isfinite(r[k]).all(), k
    assert r["lat"].shape == (13, 3, R.LATENT_SHAPES[i][0])
    # the stated condition of the chain tests: the chain's size comes from the schedule (1 / sqrt(alpha) reaches 31.6), not the weights
    assert 100 < r["lat"].abs().max() < 2000


@pytest.mark.parametrize("i", range(len(R.LATENT_SHAPES)), ids=IDS)
def test_fp32_yardstick_does_not_depend_on_the_summation_order(i):
    """The GPU tests gate |gpu - fp64| by 4 x |cpu fp32 - fp64|.  That is sound only if the right side is a property of fp32, not
    of one evaluation order: here F.linear against a sequential accumulate over k from the bias (the order of an MFMA k-chain).
    Measured with these seeds over the nine shapes: eps within 1.55 of each other, losses within 1.23, latents within 1.00 (a
    chain's error is led by the fp32 schedule coefficients, which both orders share; the same holds at ns 50).
    Asserted: within 2; the GPU margin of 4 is twice that."""
    r = references(i)
    worst = 1.0
    with torch.no_grad():
        x, c = R.pass_inputs(i)
        for t, ref in r["eps"].items():
            a = (R.denoise(r["sd"], x, t, c).double() - ref).abs().max().item()
            b = (R.denoise(r["sd"], x, t, c, linear=R.linear_k_chain).double() - ref).abs().max().item()
            print(f"{IDS[i]} eps t={t}: max|ref| {ref.abs().max():.3g}  F.linear {a:.3e}  k-chain {b:.3e}  spread {max(a, b) / min(a, b):.2f}")
            assert 0 < a < 1e-5 and 0 < b < 1e-5      # (fp32 on values of O(3) through at most 8 layers of at most 144 terms)
            worst = max(worst, max(a, b) / min(a, b))
        cond, z0 = r["cond"].float(), r["z0"].float()
        ref = R.chain(R.to_f64(r["sdt"]), cond.double(), z0.double(), r["noise"].double(), NS)
        lref = R.losses(ref, z0.double())
        la = R.chain(r["sdt"], cond, z0, r["noise"], NS)
        lb = R.chain(r["sdt"], cond, z0, r["noise"], NS, linear=R.linear_k_chain)
        for what, ea, eb in (("latents", (la.double() - ref).abs().max().item(), (lb.double() - ref).abs().max().item()),
                             ("losses", (R.losses(la, z0).double() - lref).abs().max().item(),
                              (R.losses(lb, z0).double() - lref).abs().max().item())):
            print(f"{IDS[i]} chain {what}: F.linear {ea:.3e}  k-chain {eb:.3e}  spread {max(ea, eb) / min(ea, eb):.2f}")
            assert ea > 0 and eb > 0
            worst = max(worst, max(ea, eb) / min(ea, eb))
    assert worst <= 2.0, worst

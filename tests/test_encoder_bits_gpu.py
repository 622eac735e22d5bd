"""GPU: the encoder family (cond_fast_kernel, cond_unet_kernel, latent_encode_kernel: csrc/mcd_encode_kernel.hpp) reproduces its
recorded output bits, one case per row of MCD_COND_FAST_INSTANCES, MCD_COND_UNET_INSTANCES and MCD_LATENT_ENCODE_INSTANCES.

The three kernels share their window loader, U-Net down path and flatten-Linear tail.  Every output element is one fixed
sequence of floating-point operations (the fmaf chains in c-then-i order, the 16-lane sum, the bias last), so a regrouping of
that text leaves the bits alone and a digest that moves means an operation order changed: restore the order, do not re-record.
tests/golden/encoder_bits.json holds the sha256 of the float32 output bytes per case, recorded before the kernels were regrouped,
and the toolchain line of the library that produced them; a library built by another compiler may legitimately schedule other
fused operations, so the cases then skip, naming both toolchains.

Inputs: seeded random-init models (perturbed BatchNorm statistics and PReLU slopes), B = 5 windows from the same generator -- one
full and one partial workgroup at 4, 3 and 2 windows per workgroup, five workgroups at 1 -- latent dimension 32."""
import hashlib
import json
import os

import pytest
import torch

from helpers import golden_weights, make_args
from latent_ref import _perturb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_bits.json")
B, D = 5, 32
# (kind, frames): the shipped channel list at 1 .. 20 condition frames and 'E_unet' at 1 .. 12 through HipScorer.cond_encode; the
# latent scorer's encode entry on the fused 3-frame row, on the split one (MCD_LATENT_OPT_SPLIT_ENCODE) and at 5 .. 12 corrupt frames
CASES = ([("cond_fast", t) for t in range(1, 21)] + [("cond_unet", t) for t in range(1, 13)]
         + [("latent_fused", 3), ("latent_split", 3)] + [("latent", t) for t in range(5, 13)])


def _seeded(build, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(), torch.no_grad():
        torch.manual_seed(seed + 1)
        m = build()
        _perturb(m, gen)
    return m, gen


def outputs(kind, t):
    """-> {name: float32 CPU tensor} of the case: one tiny launch (two for the split row, up to three at 5 .. 12 corrupt frames)."""
    seed = 7919 * (1 + [k for k, _ in CASES].index(kind)) + t
    if kind in ("cond_fast", "cond_unet"):
        from mocodad_amd.models.mocodad import MoCoDAD
        _, cfg = golden_weights("inject")
        arch = "AE" if kind == "cond_fast" else "E_unet"
        m, gen = _seeded(lambda: MoCoDAD(make_args(cfg, conditioning_strategy="inject", seg_len=t + 3, conditioning_indices=list(range(t)),
                                                   conditioning_architecture=arch)), seed)
        data = torch.randn(B, 2, t + 3, 17, generator=gen)
        sc = m.build_scorer(torch.device("cuda:0"))
        return {"cond_emb": sc.cond_encode(data[:, :, :t]).cpu()}
    from latent_ref import load_fixture
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    cfg = load_fixture("B")[2]
    m, gen = _seeded(lambda: MoCoDADlatent(make_args(cfg, conditioning_architecture="AE", seg_len=3 + t, conditioning_indices=[0, 1, 2],
                                                     latent_embedding_dim=D, hidden_sizes=[48, D], noise_steps=3, n_generated_samples=2)), seed)
    data = torch.randn(B, 2, 3 + t, 17, generator=gen)
    sc = m.build_scorer(torch.device("cuda:0"))
    if kind == "latent_split":
        sc.set_option("split_encode", 1)
    cond, z0 = sc.encode(data, noise_steps=3)
    return {"z0": z0.cpu()} if kind == "latent" else {"cond_emb": cond.cpu(), "z0": z0.cpu()}


def digest(x: torch.Tensor) -> str:
    assert x.dtype == torch.float32
    return hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest()


def library_toolchain():
    from mocodad_amd import _lib
    from mocodad_amd import build as build_mod
    p = build_mod.buildinfo_path(_lib.LIB_PATH)
    return json.load(open(p))["toolchain"] if os.path.exists(p) else None


@pytest.mark.parametrize("kind,t", CASES, ids=[f"{k}-{t}" for k, t in CASES])
def test_encoder_output_bits(kind, t):
    rec = json.load(open(GOLDEN))
    have = library_toolchain()
    if have != rec["toolchain"]:
        pytest.skip(f"digests recorded with {rec['toolchain']!r}; this library was built by {have!r}: output bits not compared")
    want = rec["digests"][f"{kind}-{t}"]
    got = outputs(kind, t)
    assert sorted(got) == sorted(want)
    for name, x in got.items():
        assert tuple(x.shape) == (B, D if name == "z0" else 16)
        assert torch.isfinite(x).all(), f"{kind}-{t} {name}: not finite"      # (a digest of NaNs must not pass)
        print(f"encoder-bits | {kind}-{t} {name} max|x| {x.abs().max().item():.4f} sha256 {digest(x)}")
        assert digest(x) == want[name], f"{kind}-{t} {name}: an operation order of the encoder changed (restore it; do not re-record)"

"""GPU: the autoencoder's pass (mcd_latent_reconstruct: encode, [project,] unproject, latent_decode_kernel of
csrc/mcd_encode_kernel.hpp) reproduces its recorded output bits, one case per row of MCD_LATENT_DECODE_INSTANCES plus two cases that
decode the caller's latents (z_in).

The decode launch runs the U-Net's down stem (layers 0 .. 4, down1, down2) and the step-embedding rows the encode launch runs, from
the same text.  Every output element is one fixed sequence of floating-point operations (an embedding row is one fmaf chain from
its bias in k order, the loss 16-lane sums and then the row sums in order), so a regrouping of that text leaves the bits alone and a
digest that moves means an operation order changed: restore the order, do not re-record.  tests/golden/latent_decode_bits.json
holds the sha256 of the float32 output bytes per case, recorded from the library of the commit that added stage 'pretrain', BEFORE
the two launches shared that text, and the toolchain line of the library that produced them; a library built by another compiler
may legitimately schedule other fused operations, so the cases then skip, naming both toolchains.

    python tests/test_latent_decode_bits_gpu.py --record [FILE]      # on the MI355X, with the library of that commit only

Inputs as tests/test_encoder_bits_gpu.py builds its latent cases: a seeded random-init MoCoDADlatentPretrain (perturbed BatchNorm
statistics and PReLU slopes), B = 5 windows from the same generator -- five workgroups of the decode launch, a partial one of the
3-frame encode row -- latent dimension 32, three condition frames; the z_in cases draw z (B, 32) from that generator as well."""
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN as GOLDEN_DIR  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(GOLDEN_DIR, "latent_decode_bits.json")
B, D = 5, 32
# (kind, corrupt frames): the windows' own codes on every decode row; the caller's latents on the first and the last
CASES = [("own", t) for t in (3, 5, 6, 7, 8, 9, 10, 11, 12)] + [("z_in", 3), ("z_in", 12)]
IDS = [f"{k}-{t}" for k, t in CASES]


def outputs(kind, t):
    """-> {name: float32 CPU tensor} of the case: one tiny call of mcd_latent_reconstruct."""
    from helpers import make_args
    from latent_ref import _perturb
    from latentp_ref import ae_settings
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    seed = 6007 * (1 + ["own", "z_in"].index(kind)) + t
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(), torch.no_grad():
        torch.manual_seed(seed + 1)
        m = MoCoDADlatentPretrain(make_args(ae_settings(t, 3, D)))
        _perturb(m, gen)
    data = torch.randn(B, 2, 3 + t, 17, generator=gen)
    z = torch.randn(B, D, generator=gen) if kind == "z_in" else None
    pose, loss, cond, z0 = m.build_scorer(torch.device("cuda:0")).reconstruct(data, z, want_code=True)
    return {"pose": pose.cpu(), "loss": loss.cpu(), "cond_emb": cond.cpu(), "z0": z0.cpu()}


def digest(x: torch.Tensor) -> str:
    assert x.dtype == torch.float32
    return hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest()


def library_toolchain():
    from mocodad_amd import _lib
    from mocodad_amd import build as build_mod
    p = build_mod.buildinfo_path(_lib.LIB_PATH)
    return json.load(open(p))["toolchain"] if os.path.exists(p) else None


@pytest.mark.parametrize("kind,t", CASES, ids=IDS)
def test_decode_output_bits(kind, t):
    rec = json.load(open(GOLDEN))
    have = library_toolchain()
    if have != rec["toolchain"]:
        pytest.skip(f"digests recorded with {rec['toolchain']!r}; this library was built by {have!r}: output bits not compared")
    want = rec["digests"][f"{kind}-{t}"]
    got = outputs(kind, t)
    assert sorted(got) == sorted(want)
    shapes = {"pose": (B, 2, t, 17), "loss": (B,), "cond_emb": (B, 16), "z0": (B, D)}
    moved = []
    for name, x in got.items():
        assert tuple(x.shape) == shapes[name]
        assert torch.isfinite(x).all(), f"{kind}-{t} {name}: not finite"      # (a digest of NaNs must not pass)
        print(f"decode-bits | {kind}-{t} {name} max|x| {x.abs().max().item():.4f} sha256 {digest(x)}")
        if digest(x) != want[name]:
            moved.append(name)
    assert not moved, f"{kind}-{t}: an operation order of the autoencoder's pass changed for {moved} (restore it; do not re-record)"


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    rec = {"how": "python tests/test_latent_decode_bits_gpu.py --record on the MI355X with the library of the commit that added stage "
                  "'pretrain' (latent_decode_kernel with its own down path and embedding rows); never from a later library",
           "toolchain": library_toolchain(), "digests": {}}
    for case, (kind, t) in zip(IDS, CASES):
        got = outputs(kind, t)
        assert all(torch.isfinite(x).all() for x in got.values()), case
        rec["digests"][case] = {name: digest(x) for name, x in got.items()}
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec['digests'])} cases with {rec['toolchain']}")

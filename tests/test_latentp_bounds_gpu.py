"""GPU: guard bands round every buffer of mcd_latent_reconstruct, by the method of tests/test_buffer_bounds_gpu.py (tests/guarded.py):
inside `guarded()` every device buffer engine.LatentReconstructor.reconstruct allocates -- pose (B,2,t,17), loss (B), cond_emb
(B,16), z0 (B,D) and the workspace (cond_emb, z0, H / G) -- lies between two 4096-byte bands (or one leading row, if larger) with
a poisoned interior, and the caller's windows and z_in lie between bands of all-ones NaNs, then of finite random floats.

Asserted per case: (a) no guard byte changed, (b) no output element still holds the poison, (c) the outputs are the bits of the
call outside the region, (d) whatever the input bands hold.  B = 1, 5, 33 (one window; a partial unproject tile; a second tile
holding one window) at 3 and at 12 corrupt frames, with and without z_in."""
import pytest
import torch

import latentp_ref as R
import test_buffer_bounds_gpu as BB
from guarded import guarded, guarded_copy, unwritten

pytestmark = pytest.mark.gpu
# tests/test_buffer_bounds_gpu.py ends with an audit: every declaration of include/mocodad_hip.h that writes a caller's buffer must
# be in its list of entries exercised between guard bands.  mcd_latent_reconstruct is exercised HERE, so this module adds it to
# that list when it is imported -- at collection, before any test runs -- as tests/test_error_maps_bounds_gpu.py does for its entries.
if "mcd_latent_reconstruct" not in BB.COVERED:
    BB.COVERED.append("mcd_latent_reconstruct")
DEV = "cuda:0"
_cache = {}


def _scorer(t):
    if t not in _cache:
        m, _ = R.random_ae_model(t, 3, 32, seed=900 + t)
        _cache[t] = m.to(DEV).scorer()
    return _cache[t]


def _raw(x):
    return x.detach().contiguous().view(-1).view(torch.uint8).cpu()


@pytest.mark.parametrize("with_z", [False, True], ids=["own-code", "z_in"])
@pytest.mark.parametrize("B", [1, 5, 33])
@pytest.mark.parametrize("t", [3, 12])
def test_reconstruct_buffers(t, B, with_z):
    sc = _scorer(t)
    inputs = {"data": R.windows(B, t + 3, 60 + B).to(DEV)}
    if with_z:
        inputs["z"] = torch.randn(B, 32, generator=torch.Generator().manual_seed(B)).to(DEV)
    names = ("pose_out", "loss_out", "cond_emb_out", "z0_out")
    call = lambda data, z=None: dict(zip(names, sc.reconstruct(data, z=z, want_code=True)))
    ref = {k: v.clone() for k, v in call(**inputs).items()}
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in ref.values())
    for fill in ("nan", "finite"):
        with guarded() as g:
            sc._ws.clear()          # (the scorer's cached workspace is not a guarded one)
            out = call(**{k: guarded_copy(v, fill, seed=i) for i, (k, v) in enumerate(inputs.items())})
            torch.cuda.synchronize()
            allocs = g.allocations()
            assert sum("_workspace" in a for a in allocs) == 1 and len(allocs) == 5, allocs
            g.check()                                                                                     # (a)
            for name, v in out.items():
                assert unwritten(v) == 0, f"{name} ({fill}): {unwritten(v)} of {v.numel()} elements never written"   # (b)
                assert torch.equal(_raw(v), _raw(ref[name])), f"{name}: differs from the call outside the region (bands: {fill})"   # (c), (d)
        sc._ws.clear()
    ws = int(sc.L.mcd_latent_workspace_bytes(sc._h, B))
    r256 = lambda n: (n + 255) // 256 * 256
    assert ws == r256(B * 16 * 4) + r256(B * 32 * 4) + r256(B * 640 * t * 4)

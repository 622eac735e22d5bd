"""GPU: guard bands round every buffer of mcd_latent_decode_samples, by the method of tests/test_latentp_bounds_gpu.py
(tests/guarded.py): inside `guarded()` every device buffer engine.LatentReconstructor.decode_samples allocates -- pose_all
(B,S,2,t,17), loss_all (B,S) and the workspace at the size mcd_latent_decode_workspace_bytes reports (cond_emb, G of one chunk) --
lies between two 4096-byte bands (or one leading row, if larger) with a poisoned interior, and the caller's windows, latents and
cond_emb lie between bands of all-ones NaNs, then of finite random floats.

Asserted per case: (a) no guard byte changed, (b) no output element still holds the poison, (c) the outputs are the bits of the
call outside the region, (d) whatever the input bands hold.  B x S = 5 x 3 and 11 x 3 (33 latent rows: a second unproject tile
holding one row) at 3 and at 12 corrupt frames, with cond_emb passed in and with the handle's own encoder, and once more with the
chunk forced to 2 windows -- the workspace then holds two windows' G and the last chunk is a single window."""
import pytest
import torch

import latentp_ref as R
import test_buffer_bounds_gpu as BB
from guarded import guarded, guarded_copy, unwritten

pytestmark = pytest.mark.gpu
# (the audit at the end of tests/test_buffer_bounds_gpu.py: this entry is exercised between guard bands HERE)
if "mcd_latent_decode_samples" not in BB.COVERED:
    BB.COVERED.append("mcd_latent_decode_samples")
DEV = "cuda:0"
_cache = {}


def _scorer(t):
    if t not in _cache:
        m, _ = R.random_ae_model(t, 3, 32, seed=900 + t)
        _cache[t] = m.to(DEV).scorer()
    return _cache[t]


def _raw(x):
    return x.detach().contiguous().view(-1).view(torch.uint8).cpu()


@pytest.mark.parametrize("chunk", [0, 2], ids=["bounded", "chunk=2"])
@pytest.mark.parametrize("with_cond", [True, False], ids=["cond_emb", "own-encoder"])
@pytest.mark.parametrize("B", [5, 11])
@pytest.mark.parametrize("t", [3, 12])
def test_decode_samples_buffers(t, B, with_cond, chunk):
    sc, S = _scorer(t), 3
    inputs = {"data": R.windows(B, t + 3, 60 + B).to(DEV),
              "latents": torch.randn(B, S, 32, generator=torch.Generator().manual_seed(B)).to(DEV)}
    if with_cond:
        inputs["cond_emb"] = sc.reconstruct(inputs["data"])[2].clone()
    call = lambda data, latents, cond_emb=None: dict(zip(("pose_all", "loss_all"), sc.decode_samples(data, latents, cond_emb)))
    ref = {k: v.clone() for k, v in call(**inputs).items()}
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in ref.values())
    try:
        sc.set_option("decode_chunk", chunk)
        for fill in ("nan", "finite"):
            with guarded() as g:
                sc._ws.clear()          # (the scorer's cached workspace is not a guarded one)
                out = call(**{k: guarded_copy(v, fill, seed=i) for i, (k, v) in enumerate(inputs.items())})
                torch.cuda.synchronize()
                allocs = g.allocations()
                assert sum("_workspace" in a for a in allocs) == 1 and len(allocs) == 3, allocs
                g.check()                                                                                     # (a)
                for name, v in out.items():
                    assert unwritten(v) == 0, f"{name} ({fill}): {unwritten(v)} of {v.numel()} elements never written"   # (b)
                    assert torch.equal(_raw(v), _raw(ref[name])), f"{name}: differs from the call outside the region (bands: {fill})"   # (c), (d)
            sc._ws.clear()
        ws = int(sc.L.mcd_latent_decode_workspace_bytes(sc._h, B, S))
        r256 = lambda n: (n + 255) // 256 * 256
        assert ws == r256(B * 16 * 4) + r256((min(B, chunk) if chunk else B) * S * 640 * t * 4)
    finally:
        sc.set_option("decode_chunk", 0)
        sc._ws.clear()

#!/usr/bin/env python3
"""Generate the golden vectors of the latent model's PRETRAIN stage by importing the reference's MoCoDADlatent on CPU.

Run where the reference checkout is (MOCODAD_REFERENCE, default /root/reference):   python tests/golden/gen_latentp_golden.py

Same method as gen_latentt_golden.py (whose helpers it imports): the Lightning stub, seeded random-init weights with perturbed
BatchNorm statistics and PReLU slopes ('hostile': BN gains log-uniform in 0.1x .. 10x, windows clipped to +-5) -- but stage
'pretrain': STSAE_Unet(use_bottleneck, inject_condition), one pass at t = -1 (models/mocodad_latent.py:58-64, 130-132):

  P6, P6_hostile   'AE', seg_len 6, conditioning_indices [0, 1, 2]: 3 + 3 frames, D 64
  P12              'AE', seg_len 12, conditioning_indices [0 .. 5]: 6 + 6 frames, D 32
  P24_hostile      'AE', seg_len 24, conditioning_indices 2 (the integer form: the first half): 12 + 12 frames, D 16
  P8U              'E_unet', seg_len 8, conditioning_indices [0, 1, 2]: 3 + 5 frames, D 32

Only DATA is written: latentp_<name>_w<part>.npz (state_dict without the dead AE decoder; the full sorted key / shape list; the
YAML settings) and latentp_<name>_io.npz (windows, cond_emb, z0 -- a forward hook on to_time_dim --, the reconstructed pose, the
per-window loss and the post_processing value)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import REF, _install_lightning_stub  # noqa: E402
from gen_latent_golden import make_args, perturb_  # noqa: E402
from gen_latentx_golden import save  # noqa: E402

AE = dict(conditioning_architecture="AE")
#          name           hostile  YAML overrides                                                      corrupt D   B  seed
CONFIGS = [("P6",          False, dict(AE, seg_len=6, conditioning_indices=[0, 1, 2]),                  3,  64, 5, 41),
           ("P6_hostile",  True,  dict(AE, seg_len=6, conditioning_indices=[0, 1, 2]),                  3,  64, 5, 42),
           ("P12",         False, dict(AE, seg_len=12, conditioning_indices=[0, 1, 2, 3, 4, 5]),        6,  32, 5, 43),
           ("P24_hostile", True,  dict(AE, seg_len=24, conditioning_indices=2),                         12, 16, 5, 44),
           ("P8U",         False, dict(conditioning_architecture="E_unet", seg_len=8,
                                       conditioning_indices=[0, 1, 2]),                                 5,  32, 5, 45)]


def main():
    import argparse
    _install_lightning_stub()
    sys.path.insert(0, REF)
    torch.set_grad_enabled(False)
    import models.mocodad_latent as ML
    from models.mocodad_latent import MoCoDADlatent
    # The reference's pretrain branch passes `concat_condition=` (mocodad_latent.py:62), a keyword its STSAE_Unet does not take
    # (stsae_unet.py:256-260): the stage cannot be built as the checkout stands.  The keyword is dropped here -- it is False under the
    # 'inject' strategy the class asserts -- and nothing else of the reference is touched.
    unet = ML.STSAE_Unet
    ML.STSAE_Unet = lambda *a, concat_condition=False, **k: unet(*a, **k)
    for name, hostile, over, n_corrupt, D, B, seed in CONFIGS:
        args, cfg = make_args(D, [D], 2, 1)
        over = dict(over, stage="pretrain")
        cfg.update(over)
        args = argparse.Namespace(**{**vars(args), **over})
        T = int(cfg["seg_len"])
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        m = MoCoDADlatent(args)
        m.eval()
        perturb_(m, gen, hostile)
        sd = m.state_dict()
        assert not any(k.startswith("denoiser.") for k in sd) and "model.rev_to_time_dim.weight" in sd
        keys = sorted([k, list(v.shape)] for k, v in sd.items())
        w = {k: v.numpy() for k, v in sd.items()
             if v.dtype.is_floating_point and not k.startswith(("condition_encoder.decoder.", "condition_encoder.rev_btlnk."))}
        w["__keys__"] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
        w["__cfg__"] = np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)
        parts, cur, size = [], {}, 0
        for k in sorted(w, key=lambda k: -w[k].nbytes):
            if cur and size + w[k].nbytes > 800 * 1024:
                parts.append(cur)
                cur, size = {}, 0
            cur[k] = w[k]
            size += w[k].nbytes
        parts.append(cur)
        assert len(parts) <= 10
        for i, part in enumerate(parts):
            save(f"latentp_{name}_w{i}.npz", part)
        data = torch.randn(B, 2, T, 17, generator=gen)
        if hostile:
            data = (data * 3).clamp(-5, 5)
        batch = [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, T, dtype=torch.int32)]
        codes = []
        hook = m.model.to_time_dim.register_forward_hook(lambda mod, inp, out: codes.append(out.clone()))
        out = m.forward(batch)
        hook.remove()
        pose, corrupt = out[0], out[1]
        assert len(codes) == 1 and tuple(codes[0].shape) == (B, D) and tuple(pose.shape) == (B, 2, n_corrupt, 17)
        cond_data, corrupt_data, idxs = m._select_frames(data)
        assert torch.equal(corrupt, corrupt_data)
        cond_emb, _ = m._encode_condition(cond_data)
        ci, xi = [int(i) for i in idxs[0]], [int(i) for i in idxs[1]]
        assert len(xi) == n_corrupt and sorted(ci + xi) == list(range(T))
        loss = m.loss_fn(pose, corrupt).reshape(B, -1).mean(dim=-1)
        rec = m.post_processing(pose.numpy(), corrupt.numpy(), None, None, None)
        assert abs(rec - loss.double().mean().item()) <= 1e-6 * max(1.0, abs(rec)), (rec, loss)
        rec_out = {"data": data.numpy(), "cond_emb": cond_emb.numpy(), "z0": codes[0].numpy(), "pose": pose.numpy(), "loss": loss.numpy(),
                   "rec_loss": np.array(rec, dtype=np.float64), "cond_idx": np.array(ci, dtype=np.int64),
                   "corrupt_idx": np.array(xi, dtype=np.int64), "sizes": np.array([D, B], dtype=np.int64)}
        for k, v in rec_out.items():
            assert np.isfinite(v).all(), f"{name}: recorded {k} is not finite"
        print(f"{name}: rec_loss {rec:.6e}  max|cond_emb| {cond_emb.abs().max().item():.3e}  max|z0| {codes[0].abs().max().item():.3e}  "
              f"max|pose| {pose.abs().max().item():.3e}")
        save(f"latentp_{name}_io.npz", rec_out)


if __name__ == "__main__":
    main()

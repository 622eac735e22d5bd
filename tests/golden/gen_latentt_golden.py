#!/usr/bin/env python3
"""Generate the golden vectors of the latent model at LONGER corrupt-frame counts by importing the reference's MoCoDADlatent on CPU.

Run where the reference checkout is (MOCODAD_REFERENCE, default /root/reference):   python tests/golden/gen_latentt_golden.py

Same method as gen_latentx_golden.py (whose helpers it imports): stage 'diffusion', the Lightning stub, seeded random-init weights
with perturbed BatchNorm statistics and PReLU slopes ('hostile': BN gains log-uniform in 0.1x .. 10x, windows clipped to +-5), the
draws of torch.randn / torch.randn_like captured in call order.  The configurations are the frame splits whose encode launch leaves
to_time_dim to a projection launch of its own (5 .. 12 corrupt frames):

  S12            'AE', seg_len 12, conditioning_indices [0 .. 5]: 6 condition + 6 corrupt frames
  S24, S24_hostile   'AE', seg_len 24, conditioning_indices 2 (the integer form: the first half): 12 + 12 frames
  S8U            'E_unet', seg_len 8, conditioning_indices [0, 1, 2]: 3 condition + 5 corrupt frames

Only DATA is written: latentt_<name>_w<part>.npz (state_dict without the dead AE decoder; the full sorted key / shape list; the
YAML settings) and latentt_<name>_io.npz (windows, draws, cond_emb, z0, latent_all, loss_all, the seven aggregations)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import REF, _install_lightning_stub  # noqa: E402
from gen_latent_golden import AGGRS, Capture, make_args, perturb_  # noqa: E402
from gen_latentx_golden import save  # noqa: E402

AE = dict(conditioning_architecture="AE")
#          name           hostile  YAML overrides                                                          corrupt D   hidden    ns S  B  seed
CONFIGS = [("S12",         False, dict(AE, seg_len=12, conditioning_indices=[0, 1, 2, 3, 4, 5]),            6,  32, [48, 32], 4, 2, 5, 31),
           ("S24",         False, dict(AE, seg_len=24, conditioning_indices=2),                             12, 16, [48, 16], 4, 2, 5, 32),
           ("S24_hostile", True,  dict(AE, seg_len=24, conditioning_indices=2),                             12, 16, [48, 16], 4, 2, 5, 33),
           ("S8U",         False, dict(conditioning_architecture="E_unet", seg_len=8,
                                       conditioning_indices=[0, 1, 2]),                                     5,  32, [48, 32], 4, 2, 5, 34)]


def main():
    import argparse
    _install_lightning_stub()
    sys.path.insert(0, REF)
    torch.set_grad_enabled(False)
    from models.mocodad_latent import MoCoDADlatent
    MoCoDADlatent._freeze_main_net_and_load_ckpt = lambda self: None
    for name, hostile, over, n_corrupt, D, hidden, ns, S, B, seed in CONFIGS:
        args, cfg = make_args(D, hidden, ns, S)
        cfg.update(over)
        args = argparse.Namespace(**{**vars(args), **over})
        T = int(cfg["seg_len"])
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        m = MoCoDADlatent(args)
        m.eval()
        perturb_(m, gen, hostile)
        sd = m.state_dict()
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
            save(f"latentt_{name}_w{i}.npz", part)
        data = torch.randn(B, 2, T, 17, generator=gen)
        if hostile:
            data = (data * 3).clamp(-5, 5)
        batch = [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, T, dtype=torch.int32)]
        torch.manual_seed(seed + 100)
        with Capture() as cap:
            loss_all, lat_all = m.forward(batch, aggr_strategy="all", return_="all")[:2]
        K = max(ns - 1, 1)
        assert len(cap.draws) == S * K, (len(cap.draws), S, K)
        noise = torch.stack(cap.draws).reshape(S, K, B, D)
        assert tuple(lat_all.shape) == (B, S, D) and tuple(loss_all.shape) == (B, S)
        cond_data, corrupt_data, idxs = m._select_frames(data)
        cond_emb, _ = m._encode_condition(cond_data)
        z0 = m._unet_forward(corrupt_data, t=torch.full((B,), -1, dtype=torch.long), condition_data=cond_emb, corrupt_idxs=idxs[1])
        ci, xi = [int(i) for i in idxs[0]], [int(i) for i in idxs[1]]
        assert len(xi) == n_corrupt and sorted(ci + xi) == list(range(T))
        out = {"data": data.numpy(), "noise": noise.numpy(), "cond_emb": cond_emb.numpy(), "z0": z0.numpy(),
               "latent_all": lat_all.numpy(), "loss_all": loss_all.numpy(), "cond_idx": np.array(ci, dtype=np.int64),
               "corrupt_idx": np.array(xi, dtype=np.int64),
               "sizes": np.array([D, ns, S, B], dtype=np.int64), "hidden": np.array(hidden, dtype=np.int64)}
        gens = [lat_all[:, s] for s in range(S)]
        finite = bool(torch.isfinite(loss_all).all())
        for a in AGGRS:
            sel, loss = m._aggregation_strategy(gens, z0, a)
            tag = a.replace(":", "_")
            out[f"loss_{tag}"] = loss.numpy()
            if sel is not None:
                out[f"sel_{tag}"] = sel.numpy()
            finite = finite and bool(torch.isfinite(loss).all())
        assert finite, f"{name}: a recorded loss is not finite"
        print(f"{name}: loss_all in [{loss_all.min().item():.3e}, {loss_all.max().item():.3e}]  max|cond_emb| {cond_emb.abs().max().item():.3e}  "
              f"max|z0| {z0.abs().max().item():.3e}  max|latent| {lat_all.abs().max().item():.3e}")
        save(f"latentt_{name}_io.npz", out)


if __name__ == "__main__":
    main()

"""CPU restatement of the latent path (test infrastructure; nothing under mocodad_amd/ imports it): MoCoDADlatent.forward,
stage 'diffusion' (reference models/mocodad_latent.py:93-127), from a state_dict, on top of the oracle's ST-GCN pieces.

  encode(sd, data, ci, xi)           -> cond_emb (B,16), z0 (B,D)       condition encoder; down path at t = -1; to_time_dim
  denoise(sd, x, t, cond)            -> eps (N,D)                       Denoiser.forward (components.py:265-291)
  chain(sd, cond, z0, noise, ns)     -> latent_all (B,S,D)              the reverse diffusion with the caller's draws
  aggregate(latent_all, z0, aggr)    -> (selected | None, loss)         _aggregation_strategy (mocodad.py:454-520)
"""
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle import mocodad_oracle as O

BN_EPS = 1e-5
_LOSS = {"smooth_l1": F.smooth_l1_loss, "l1": F.l1_loss, "mse": F.mse_loss}


def n_denoiser_layers(sd) -> int:
    n = 0
    while f"denoiser.cond_layers.{n}.weight" in sd:
        n += 1
    return n


def encode(sd: Dict[str, torch.Tensor], data: torch.Tensor, cond_idx: Sequence[int], corrupt_idx: Sequence[int],
           emb_dim: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    cond = O.cond_encode(sd, data[:, :, list(cond_idx)])
    x = data[:, :, list(corrupt_idx)]
    t = torch.full((data.shape[0], 1), -1.0, dtype=data.dtype)
    e = O.pos_encoding(t, emb_dim).to(data.dtype) + cond
    h = x
    for b, i in O.UNET_DOWN:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    h = O.joint_resample(sd, "model.down1", h)
    for b, i in O.UNET_MID1:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    h = O.joint_resample(sd, "model.down2", h)
    for b, i in O.UNET_MID2:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    z0 = F.linear(h.reshape(h.shape[0], -1), O._t(sd, "model.to_time_dim.weight"), O._t(sd, "model.to_time_dim.bias"))
    return cond, z0


def denoise(sd, x: torch.Tensor, t: int, cond: torch.Tensor, emb_dim: int = 16) -> torch.Tensor:
    L = n_denoiser_layers(sd)
    e = O.pos_encoding(torch.full((x.shape[0], 1), float(t)), emb_dim).to(x.dtype) + cond
    h = x
    for l in range(L):
        p = f"denoiser.net.{l}"
        if l == L - 1:
            h = F.linear(h, O._t(sd, p + ".weight"), O._t(sd, p + ".bias"))
        else:
            h = F.linear(h, O._t(sd, p + ".0.weight"), O._t(sd, p + ".0.bias"))
            h = F.batch_norm(h, O._t(sd, p + ".1.running_mean"), O._t(sd, p + ".1.running_var"), O._t(sd, p + ".1.weight"),
                             O._t(sd, p + ".1.bias"), training=False, eps=BN_EPS)
            h = F.relu(h)
        h = h + F.linear(e, O._t(sd, f"denoiser.cond_layers.{l}.weight"), O._t(sd, f"denoiser.cond_layers.{l}.bias"))
    return h


def chain(sd, cond: torch.Tensor, z0: torch.Tensor, noise: torch.Tensor, noise_steps: int) -> torch.Tensor:
    """noise (S, max(ns-1,1), B, D): slot 0 = x_T, slot k = z of step ns-k.  -> (B,S,D)"""
    beta, alpha, ah = (v.to(z0.dtype) for v in O.schedule(noise_steps))
    out = []
    for s in range(noise.shape[0]):
        x = noise[s, 0]
        for i in reversed(range(1, noise_steps)):
            eps = denoise(sd, x, i, cond)
            z = noise[s, noise_steps - i] if i > 1 else torch.zeros_like(x)
            x = (1 / torch.sqrt(alpha[i])) * (x - ((1 - alpha[i]) / torch.sqrt(1 - ah[i])) * eps) + torch.sqrt(beta[i]) * z
        out.append(x)
    return torch.stack(out, dim=1)


def losses(latents: torch.Tensor, z0: torch.Tensor, loss_fn: str = "smooth_l1") -> torch.Tensor:
    """latents (B,S,D) or (B,D) against z0 (B,D): mean over D."""
    ref = z0[:, None].expand_as(latents) if latents.dim() == 3 else z0
    return _LOSS[loss_fn](latents, ref, reduction="none").mean(dim=-1)


def aggregate(latent_all: torch.Tensor, z0: torch.Tensor, aggr: str, loss_fn: str = "smooth_l1") -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    la = losses(latent_all, z0, loss_fn)
    if aggr == "all":
        return latent_all, la
    if aggr == "mean":
        return None, la.mean(dim=1)
    if aggr == "median":
        return None, torch.median(la, dim=1).values
    if "quantile" in aggr:
        return None, torch.quantile(la, float(aggr.split(":")[-1]), dim=1)
    if aggr == "mean_pose":
        sel = latent_all.mean(dim=1)
        return sel, losses(sel, z0, loss_fn)
    if aggr == "median_pose":
        sel = torch.median(latent_all, dim=1).values
        return sel, losses(sel, z0, loss_fn)
    if aggr in ("best", "worst"):
        best = aggr == "best"
        cur = torch.full((z0.shape[0],), 1e10 if best else -1.0, dtype=la.dtype)
        sel = torch.zeros_like(z0)
        for s in range(la.shape[1]):
            m = la[:, s] < cur if best else la[:, s] > cur
            cur = torch.where(m, la[:, s], cur)
            sel = torch.where(m[:, None], latent_all[:, s], sel)
        return sel, cur
    raise ValueError(f"Unknown aggregation strategy {aggr}")


def score(sd, data, noise, *, noise_steps: int, cond_idx=(0, 1, 2), corrupt_idx=(3, 4, 5), loss_fn: str = "smooth_l1"):
    """-> cond_emb, z0, latent_all (B,S,D), loss_all (B,S)"""
    cond, z0 = encode(sd, data, cond_idx, corrupt_idx)
    lat = chain(sd, cond, z0, noise, noise_steps)
    return cond, z0, lat, losses(lat, z0, loss_fn)


# ---- fixtures of tests/golden/gen_latent_golden.py
WEIGHTS_OF = {"A_benign": "A_benign", "A_hostile": "A_hostile", "B": "B", "C": "A_hostile"}
_cache = {}


def load_fixture(name: str):
    """-> (state_dict of float tensors, sorted [key, shape] list of the reference's full state_dict, YAML settings dict for this
    configuration, dict of recorded arrays).  Loaded once per session and shared: treat as read-only."""
    if name not in _cache:
        import glob
        import json
        import os

        import numpy as np
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        w = {}
        for p in sorted(glob.glob(os.path.join(here, f"latent_{WEIGHTS_OF[name]}_w[0-9].npz"))):
            d = np.load(p)
            w.update({k: d[k] for k in d.files})
        keys = json.loads(bytes(w.pop("__keys__")).decode())
        cfg = json.loads(bytes(w.pop("__cfg__")).decode())
        d = np.load(os.path.join(here, f"latent_{name}_io.npz"))
        io = {k: d[k] for k in d.files}
        D, ns, S, B = (int(v) for v in io["sizes"])
        cfg.update(latent_embedding_dim=D, hidden_sizes=[int(h) for h in io["hidden"]], noise_steps=ns, n_generated_samples=S)
        _cache[name] = ({k: torch.from_numpy(v) for k, v in w.items()}, keys, cfg, io)
    return _cache[name]

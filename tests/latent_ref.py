"""CPU restatement of the latent path (test infrastructure; nothing under mocodad_amd/ imports it): MoCoDADlatent.forward,
stage 'diffusion' (reference models/mocodad_latent.py:93-127), from a state_dict, on top of the oracle's ST-GCN pieces.

  encode(sd, data, ci, xi)           -> cond_emb (B,16), z0 (B,D)       condition encoder; down path at t = -1; to_time_dim
  denoise(sd, x, t, cond)            -> eps (N,D)                       Denoiser.forward (components.py:265-291)
  chain(sd, cond, z0, noise, ns)     -> latent_all (B,S,D)              the reverse diffusion with the caller's draws
  aggregate(latent_all, z0, aggr)    -> (selected | None, loss)         _aggregation_strategy (mocodad.py:454-520)

Every function runs in the dtype of its inputs: given to_f64(sd) and double inputs it is the float64 reference the GPU tests of
tests/test_latent_shapes_gpu.py measure against, given the fp32 state_dict it is the yardstick of that measurement.
random_latent_model builds the random-init models of those tests.
"""
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn
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


def to_f64(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Every floating tensor of a state_dict as double (the others, e.g. num_batches_tracked, as they are)."""
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def linear_k_chain(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """F.linear in a second summation order: from the bias, one product after the other over k -- the order of an MFMA k-chain."""
    acc = b.expand(x.shape[0], -1).clone()
    for k in range(w.shape[1]):
        acc = acc + x[:, k:k + 1] * w[:, k]
    return acc


def denoise(sd, x: torch.Tensor, t: int, cond: torch.Tensor, emb_dim: int = 16, linear=F.linear) -> torch.Tensor:
    L = n_denoiser_layers(sd)
    e = O.pos_encoding(torch.full((x.shape[0], 1), float(t)), emb_dim).to(x.dtype) + cond
    h = x
    for l in range(L):
        p = f"denoiser.net.{l}"
        if l == L - 1:
            h = linear(h, O._t(sd, p + ".weight"), O._t(sd, p + ".bias"))
        else:
            h = linear(h, O._t(sd, p + ".0.weight"), O._t(sd, p + ".0.bias"))
            h = F.batch_norm(h, O._t(sd, p + ".1.running_mean"), O._t(sd, p + ".1.running_var"), O._t(sd, p + ".1.weight"),
                             O._t(sd, p + ".1.bias"), training=False, eps=BN_EPS)
            h = F.relu(h)
        h = h + linear(e, O._t(sd, f"denoiser.cond_layers.{l}.weight"), O._t(sd, f"denoiser.cond_layers.{l}.bias"))
    return h


def chain(sd, cond: torch.Tensor, z0: torch.Tensor, noise: torch.Tensor, noise_steps: int, linear=F.linear) -> torch.Tensor:
    """noise (S, max(ns-1,1), B, D): slot 0 = x_T, slot k = z of step ns-k.  -> (B,S,D)"""
    beta, alpha, ah = (v.to(z0.dtype) for v in O.schedule(noise_steps))
    out = []
    for s in range(noise.shape[0]):
        x = noise[s, 0]
        for i in reversed(range(1, noise_steps)):
            eps = denoise(sd, x, i, cond, linear=linear)
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


# ---- random-init models (tests/test_latentx_gpu.py, tests/test_latent_shapes_*.py)
def _perturb(m, gen):
    """Seeded eval-mode statistics away from the initial (0, 1, 1, 0): a folded BatchNorm that is wrong must show."""
    for mod in m.modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=gen) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=gen) + 0.5)
            mod.weight.data.copy_(torch.rand(mod.weight.shape, generator=gen) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=gen) * 0.1)
        if isinstance(mod, nn.PReLU):
            mod.weight.data.copy_(torch.rand(mod.weight.shape, generator=gen) * 0.3 + 0.1)


# (D, hidden) of tests/test_latent_shapes_*.py, each named for the branch of latent_chain_kernel it reaches: MT = out / 16 m-tiles
# over four waves, KQ = in / 16 + 1 k-blocks, activations alternating between two buffers by layer parity
LATENT_SHAPES = [
    (16, [16]),                                 # L = 1 (the layer reads a copy of x), MT 1, KQ 2, D / 4 = 4 element groups
    (128, [128]),                               # L = 1 at full width, MT 8, KQ 9
    (16, [16, 16]),                             # the smallest two-layer model
    (96, [96, 96]),                             # even L, MT 6, KQ 7
    (48, [16, 112, 48]),                        # odd L, MT 1 / 7 / 3, KQ 4 / 2 / 8
    (112, [64, 80, 112]),                       # state stride 116, MT 4 / 5 / 7, KQ 8 / 5 / 6
    (80, [96, 32, 128, 16, 80]),                # L 5, a 16-wide layer between wide ones
    (32, [128, 16, 48, 96, 64, 112, 32]),       # L 7
    (128, [128] * 8),                           # every limit at once
]
SHAPE_IDS = ["-".join(str(h) for h in hidden) if len(hidden) < 8 else "128x8" for _, hidden in LATENT_SHAPES]
_models = {}


def pass_inputs(i: int, n: int = 70):
    """Rows of one denoiser pass on shape i: x ~ N(0,1) (n,D), cond ~ 0.5 N(0,1) (n,16)."""
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randn(n, LATENT_SHAPES[i][0], generator=g), 0.5 * torch.randn(n, 16, generator=g)


def chain_inputs(i: int, ns: int, S: int, B: int):
    """Windows (B,2,6,17) and the parity-mode draws (S, max(ns-1,1), B, D) of a scoring call on shape i."""
    g = torch.Generator().manual_seed(2000 + i)
    return torch.randn(B, 2, 6, 17, generator=g), torch.randn(S, max(ns - 1, 1), B, LATENT_SHAPES[i][0], generator=g)


def random_latent_model(D: int, hidden: Sequence[int], *, seed: int, ns: int, S: int, tame: bool, **over):
    """-> (MoCoDADlatent on the CPU, cloned fp32 state_dict): fixture B's settings with latent_embedding_dim D and the denoiser
    widths `hidden`, seeded random-init weights, perturbed BatchNorm statistics and PReLU slopes.  tame: the last denoiser layer
    and its cond_layers entry scaled by 0.1, so that eps stays O(0.1) and a chain's size comes from the schedule alone.
    over: further settings replacing fixture B's (seg_len, conditioning_indices: another frame split).
    Built once per argument set and session and shared: treat the state_dict as read-only."""
    from helpers import make_args
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    key = (D, tuple(hidden), seed, ns, S, tame, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _models:
        cfg = load_fixture("B")[2]
        with torch.random.fork_rng(), torch.no_grad():
            torch.manual_seed(seed)
            m = MoCoDADlatent(make_args(cfg, latent_embedding_dim=D, hidden_sizes=list(hidden), noise_steps=ns, n_generated_samples=S, **over))
            _perturb(m, torch.Generator().manual_seed(seed + 1))
            if tame:
                last = len(hidden) - 1
                for lin in (m.denoiser.net[last], m.denoiser.cond_layers[last]):
                    lin.weight.mul_(0.1)
                    lin.bias.mul_(0.1)
        _models[key] = (m, {k: v.detach().clone() for k, v in m.state_dict().items()})
    return _models[key]


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

"""CPU restatement of the latent model's pretrain stage (test infrastructure; nothing under mocodad_amd/ imports it):
MoCoDADlatent.forward, stage 'pretrain' (reference models/mocodad_latent.py:93-100, 131 -> STSAE_Unet.forward with use_bottleneck,
models/stsae/stsae_unet.py:406-438), from a state_dict, out of the oracle's layer and resampler functions plus the two Linears.

  reconstruct(sd, data, ci, xi, z=None, loss_fn=...) -> cond_emb (B,16), z0 (B,D), pose (B,2,Tx,17), loss (B,)
  post_processing(pose, corrupt, loss_fn)            -> the reference's pretrain_rec_loss (mocodad_latent.py:218)

Every function runs in the dtype of its inputs.  three_ways evaluates it in float64 and in fp32 in the two orders of
pose_ref.ORDERS ('bn', 'folded'); X is the factor within which those two fp32 orders stay of each other, measured and asserted by
tests/test_latentp_golden.py on the inputs of the GPU test and rounded up to the next half -- the GPU gate is err <= 2 X yard
(pose_ref.gated's rule).  random_ae_model builds the seeded random-init models, load_fixture reads tests/golden/latentp_*.
"""
import functools
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

import pose_ref as P
from latent_ref import _perturb
from oracle import mocodad_oracle as O

_LOSS = {"smooth_l1": F.smooth_l1_loss, "l1": F.l1_loss, "mse": F.mse_loss}
# measured by tests/test_latentp_golden.py::test_fp32_orders_factor (its docstring has the figures), rounded up to the next half
X = {"pose": 1.5, "loss": 1.5}
FRAME_COUNTS = (3, 5, 6, 7, 8, 9, 10, 11, 12)
FP64_CASE = dict(t=12, D=128, B=5, seed=77)      # the longest shape: 12 + 12 frames, D 128


def reconstruct(sd: Dict[str, torch.Tensor], data: torch.Tensor, cond_idx: Sequence[int], corrupt_idx: Sequence[int],
                z: Optional[torch.Tensor] = None, loss_fn: str = "smooth_l1", emb_dim: int = 16):
    cond = O.cond_encode(sd, data[:, :, list(cond_idx)])
    x = data[:, :, list(corrupt_idx)]
    t = torch.full((data.shape[0], 1), -1.0, dtype=data.dtype)
    e = O.pos_encoding(t, emb_dim).to(data.dtype) + cond
    h = x
    for b, i in O.UNET_DOWN:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    d1 = h
    h = O.joint_resample(sd, "model.down1", h)
    for b, i in O.UNET_MID1:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    d2 = h
    h = O.joint_resample(sd, "model.down2", h)
    for b, i in O.UNET_MID2:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    shape = h.shape
    z0 = F.linear(h.reshape(shape[0], -1), O._t(sd, "model.to_time_dim.weight"), O._t(sd, "model.to_time_dim.bias"))
    g = F.linear(z0 if z is None else z, O._t(sd, "model.rev_to_time_dim.weight"), O._t(sd, "model.rev_to_time_dim.bias"))
    h = O.joint_resample(sd, "model.up3", g.reshape(shape)) + d2
    for b, i in O.UNET_UP4:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    h = O.joint_resample(sd, "model.up2", h) + d1
    for b, i in O.UNET_UP3:
        h = O.st_gcnn_layer(sd, f"model.{b}.{i}", h, e)
    pose = h + x
    loss = _LOSS[loss_fn](pose, x, reduction="none").reshape(x.shape[0], -1).mean(dim=-1)
    return cond, z0, pose, loss


def post_processing(pose: torch.Tensor, corrupt: torch.Tensor, loss_fn: str = "smooth_l1") -> float:
    return torch.mean(_LOSS[loss_fn](pose, corrupt, reduction="none")).item()


def three_ways(sd, data, ci, xi, z=None, loss_fn="smooth_l1"):
    """-> (ref64, {order: fp32}), each the (cond_emb, z0, pose, loss) of reconstruct"""
    fn = (lambda s, d: reconstruct(s, d, ci, xi, None, loss_fn)) if z is None else (lambda s, d, z_: reconstruct(s, d, ci, xi, z_, loss_fn))
    return P.three_ways(fn, sd, *((data,) if z is None else (data, z)))


def gated(test: str, case: str, what: str, kind: str, got, ref64, cpu32) -> None:
    """pose_ref.gated's rule with this module's factors: the hard 1e-4 max(1, max|ref64|) gate, and err <= 2 X yard on max and rms."""
    err, rms, ymax, yrms, top = P.measure(test, case, what, got, ref64, cpu32)
    assert err <= 1e-4 * max(1.0, top), (case, what, err, top)
    assert err <= 2 * X[kind] * ymax, (case, what, "max", err, ymax, 2 * X[kind])
    assert rms <= 2 * X[kind] * yrms, (case, what, "rms", rms, yrms, 2 * X[kind])


# ---- random-init models
_models = {}


def ae_settings(t_corrupt: int, t_cond: int, D: int, arch: str = "AE") -> dict:
    """The YAML settings of fixture P6 with another frame split, latent size and condition encoder."""
    cfg = dict(load_fixture("P6")[2])
    cfg.update(seg_len=t_cond + t_corrupt, conditioning_indices=list(range(t_cond)), latent_embedding_dim=D, conditioning_architecture=arch,
               stage="pretrain")
    return cfg


def random_ae_model(t_corrupt: int, t_cond: int, D: int, *, seed: int, arch: str = "AE"):
    """-> (MoCoDADlatentPretrain on the CPU, cloned fp32 state_dict): seeded random-init weights, perturbed BatchNorm statistics and
    PReLU slopes.  Built once per argument set and session and shared: treat the state_dict as read-only."""
    from helpers import make_args
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    key = (t_corrupt, t_cond, D, seed, arch)
    if key not in _models:
        with torch.random.fork_rng(), torch.no_grad():
            torch.manual_seed(seed)
            m = MoCoDADlatentPretrain(make_args(ae_settings(t_corrupt, t_cond, D, arch)))
            _perturb(m, torch.Generator().manual_seed(seed + 1))
        _models[key] = (m, {k: v.detach().clone() for k, v in m.state_dict().items()})
    return _models[key]


def windows(B: int, seg_len: int, seed: int) -> torch.Tensor:
    return torch.randn(B, 2, seg_len, 17, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def fp64_case():
    """-> dict(m, sd, data, ci, xi, ref=(cond, z0, pose, loss) in float64, out={order: the same in fp32}) of FP64_CASE"""
    c = FP64_CASE
    m, sd = random_ae_model(c["t"], c["t"], c["D"], seed=c["seed"])
    data = windows(c["B"], 2 * c["t"], c["seed"] + 2)
    ci, xi = list(range(c["t"])), list(range(c["t"], 2 * c["t"]))
    ref, out = three_ways(sd, data, ci, xi)
    return dict(m=m, sd=sd, data=data, ci=ci, xi=xi, ref=ref, out=out)


# ---- fixtures of tests/golden/gen_latentp_golden.py
FIXTURES = ("P6", "P6_hostile", "P12", "P24_hostile", "P8U")
_cache = {}


def load_fixture(name: str):
    """-> (state_dict of float tensors, sorted [key, shape] list of the reference's full state_dict, YAML settings, recorded arrays).
    Loaded once per session and shared: treat as read-only."""
    if name not in _cache:
        import glob
        import json
        import os

        import numpy as np
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        w = {}
        for p in sorted(glob.glob(os.path.join(here, f"latentp_{name}_w[0-9].npz"))):
            d = np.load(p)
            w.update({k: d[k] for k in d.files})
        keys = json.loads(bytes(w.pop("__keys__")).decode())
        cfg = json.loads(bytes(w.pop("__cfg__")).decode())
        d = np.load(os.path.join(here, f"latentp_{name}_io.npz"))
        _cache[name] = ({k: torch.from_numpy(v) for k, v in w.items()}, keys, cfg, {k: d[k] for k in d.files})
    return _cache[name]

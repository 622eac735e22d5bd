"""CPU restatement of the latent model's pretrain stage (test infrastructure; nothing under mocodad_amd/ imports it):
MoCoDADlatent.forward, stage 'pretrain' (reference models/mocodad_latent.py:93-100, 131 -> STSAE_Unet.forward with use_bottleneck,
models/stsae/stsae_unet.py:406-438), from a state_dict, out of the oracle's layer and resampler functions plus the two Linears.

  reconstruct(sd, data, ci, xi, z=None, loss_fn=..., linear=...) -> cond_emb (B,16), z0 (B,D), pose (B,2,Tx,17), loss (B,)
  post_processing(pose, corrupt, loss_fn)            -> the reference's pretrain_rec_loss (mocodad_latent.py:218)

Every function runs in the dtype of its inputs.  three_ways evaluates it in float64 and in fp32 in the two orders of
pose_ref.ORDERS ('bn', 'folded'), on one thread.  FP64_CASES is the table of models and inputs that tests/test_latentp_fp64_host.py
(CPU) and tests/test_latentp_gpu.py::test_rows_vs_fp64 (GPU) both run on; fp64_case(name) evaluates a case once per session.  z0
has a third fp32 evaluation, to_time_dim as latent_ref.linear_k_chain (one sequential chain over K = 640 t, up to 7 680): its
yardstick is the largest error of the three.  X[kind] is the factor within which the two fp32 orders stay of each other over all
cases, measured and asserted by the host test (its docstring has the figures) and by
tests/test_latentp_golden.py::test_fp32_orders_factor, rounded up to the next half -- the GPU gate is err <= 2 X yard
(pose_ref.gated's rule).  random_ae_model builds the seeded random-init models, load_fixture reads tests/golden/latentp_*.
"""
import functools
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

import pose_ref as P
from latent_ref import _perturb, linear_k_chain
from oracle import mocodad_oracle as O

_LOSS = {"smooth_l1": F.smooth_l1_loss, "l1": F.l1_loss, "mse": F.mse_loss}
# per compared kind of tensor: the worst spread of the two fp32 orders over FP64_CASES on two CPUs, rounded up to the next half
# (tests/test_latentp_fp64_host.py has the figures and asserts it; no entry may exceed pose_ref.X)
X = {"cond": 2.0, "z0": 1.5, "pose": 2.0, "loss": 2.5}
KINDS = ("cond", "z0", "pose", "loss")           # of the four results of reconstruct, in their order
WHAT = ("cond_emb", "z0", "pose", "loss")
FRAME_COUNTS = (3, 5, 6, 7, 8, 9, 10, 11, 12)
LATENT_DIMS = (16, 32, 48, 64, 80, 96, 112, 128)
# windows per case: one full 32-row tile of the projection and unprojection launches plus a 13-row one; odd, for the 3-frame encode
# row's two windows per workgroup.  A case whose tensors are too small for a stable max-spread gets 77, then 109: X does not go up.
WINDOWS = 45
Z_GAIN = 31.6                                    # 1 / sqrt(alpha_9): the schedule's gain at 10 steps, the scale generated latents reach


def _case(t, tc, D, *, arch="AE", channels=None, h_dim=None, seed=None, B=WINDOWS, z=None, loss_fn="smooth_l1", weights=None):
    """t corrupt + tc condition frames, latent size D.  z: None = the windows' own code, else the scale of the caller's N(0,1)
    latents (the decode launch alone).  weights: a fixture of FIXTURES whose state_dict the case runs on (t, tc, D are its own)."""
    return dict(t=t, tc=tc, D=D, arch=arch, channels=channels, h_dim=h_dim, seed=seed, B=B, z=z, loss_fn=loss_fn, weights=weights)


FP64_CASES = {
    # rows: every frame count with 3 condition frames of 'AE', D walking through every legal size
    **{f"{t}+3 D{D}": _case(t, 3, D) for t, D in zip(FRAME_COUNTS, LATENT_DIMS + LATENT_DIMS[:1])},
    # the corners of test_every_frame_count_vs_cpu_restatement ('3+3 D16' is the first row above); 12 + 12 at D 128 under its old seed
    "3+3 D128": _case(3, 3, 128), "12+12 D16": _case(12, 12, 16), "12+12 D128": _case(12, 12, 128, seed=77),
    # cond, at 6 corrupt frames: both ends of cond_fast_kernel in front of this encode launch, 'E_unet', and the runtime channel
    # list of pose_ref.COND_E_CASE (the gather and cond_encode_kernel)
    "6+1 D32": _case(6, 1, 32), "6+12 D32": _case(6, 12, 32), "6+6 D32 E_unet": _case(6, 6, 32, arch="E_unet"),
    f"6+{P.COND_E_CASE[0]} D32 E": _case(6, P.COND_E_CASE[0], 32, arch="E", channels=P.COND_E_CASE[1], h_dim=P.COND_E_CASE[2]),
    # weights: the hostile fixtures' state_dicts on 45 seeded windows
    "P6_hostile": _case(3, 3, 64, weights="P6_hostile"), "P24_hostile": _case(12, 12, 16, weights="P24_hostile"),
    # decode alone: the caller's latents at unit scale and at the scale generated latents reach
    **{f"{t}+3 D{D} z x{g:g}": _case(t, 3, D, z=g) for t, D in ((3, 32), (7, 64), (12, 128)) for g in (1.0, Z_GAIN)},
    # loss: the pose of a corner, the other two loss functions
    **{f"{t}+{t} D{D} {fn}": _case(t, t, D, seed=s, loss_fn=fn) for t, D, s in ((3, 16, None), (12, 128, 77)) for fn in ("l1", "mse")},
}


def reconstruct(sd: Dict[str, torch.Tensor], data: torch.Tensor, cond_idx: Sequence[int], corrupt_idx: Sequence[int],
                z: Optional[torch.Tensor] = None, loss_fn: str = "smooth_l1", emb_dim: int = 16, linear=F.linear):
    """linear: to_time_dim as F.linear or as latent_ref.linear_k_chain (a second fp32 summation order of z0)."""
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
    z0 = linear(h.reshape(shape[0], -1), O._t(sd, "model.to_time_dim.weight"), O._t(sd, "model.to_time_dim.bias"))
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


def z0_k_chain(sd, data, ci, xi) -> torch.Tensor:
    """z0 of the fp32 restatement (the oracle's own order, one thread) with to_time_dim as one sequential chain over K"""
    with P.evaluation(torch.float32), P.one_thread():
        return reconstruct(sd, data, ci, xi, linear=linear_k_chain)[1]


def gated(test: str, case: str, what: str, kind: str, got, ref64, cpu32) -> None:
    """pose_ref.gated's rule with this module's factors: the hard 1e-4 max(1, max|ref64|) gate, and err <= 2 X yard on max and rms."""
    err, rms, ymax, yrms, top = P.measure(test, case, what, got, ref64, cpu32)
    assert err <= 1e-4 * max(1.0, top), (case, what, err, top)
    assert err <= 2 * X[kind] * ymax, (case, what, "max", err, ymax, 2 * X[kind])
    assert rms <= 2 * X[kind] * yrms, (case, what, "rms", rms, yrms, 2 * X[kind])


# ---- random-init models
_models = {}


def ae_settings(t_corrupt: int, t_cond: int, D: int, arch: str = "AE", channels=None, h_dim=None) -> dict:
    """The YAML settings of fixture P6 with another frame split, latent size and condition encoder (channels, h_dim: of 'E' / 'AE')."""
    cfg = dict(load_fixture("P6")[2])
    cfg.update(seg_len=t_cond + t_corrupt, conditioning_indices=list(range(t_cond)), latent_embedding_dim=D, conditioning_architecture=arch,
               stage="pretrain")
    if channels is not None:
        cfg.update(channels=list(channels), h_dim=h_dim)
    return cfg


def random_ae_model(t_corrupt: int, t_cond: int, D: int, *, seed: int, arch: str = "AE", channels=None, h_dim=None):
    """-> (MoCoDADlatentPretrain on the CPU, cloned fp32 state_dict): seeded random-init weights, perturbed BatchNorm statistics and
    PReLU slopes.  Built once per argument set and session and shared: treat the state_dict as read-only."""
    from helpers import make_args
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    key = (t_corrupt, t_cond, D, seed, arch, None if channels is None else tuple(channels), h_dim)
    if key not in _models:
        with torch.random.fork_rng(), torch.no_grad():
            torch.manual_seed(seed)
            m = MoCoDADlatentPretrain(make_args(ae_settings(t_corrupt, t_cond, D, arch, channels, h_dim)))
            _perturb(m, torch.Generator().manual_seed(seed + 1))
        _models[key] = (m, {k: v.detach().clone() for k, v in m.state_dict().items()})
    return _models[key]


def fixture_model(name: str):
    """-> (MoCoDADlatentPretrain on the CPU with the fixture's weights, the fixture's state_dict), once per fixture and session"""
    from helpers import make_args
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    if ("fixture", name) not in _models:
        sd, _, cfg, _ = load_fixture(name)
        m = MoCoDADlatentPretrain(make_args(cfg))
        m.load_state_dict(sd, strict=False)
        _models["fixture", name] = (m, sd)
    return _models["fixture", name]


def windows(B: int, seg_len: int, seed: int) -> torch.Tensor:
    return torch.randn(B, 2, seg_len, 17, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def fp64_case(name: str):
    """-> dict(m, sd, data, ci, xi, z (the caller's latents or None), loss_fn, ref=(cond, z0, pose, loss) in float64,
    out={order: the same in fp32}, z0_chain (z0 with to_time_dim as linear_k_chain, fp32; None where z is given)) of
    FP64_CASES[name].  Evaluated once per name and session and shared: treat every tensor as read-only."""
    c = FP64_CASES[name]
    seed = c["seed"] if c["seed"] is not None else P._seed_of("latentp", c["weights"], c["t"], c["tc"], c["D"], c["arch"])
    if c["weights"] is not None:
        m, sd = fixture_model(c["weights"])
    else:
        m, sd = random_ae_model(c["t"], c["tc"], c["D"], seed=seed, arch=c["arch"], channels=c["channels"], h_dim=c["h_dim"])
    ci, xi = m._frame_split()
    assert (len(xi), len(ci), m.latent_embedding_dim) == (c["t"], c["tc"], c["D"]), name
    data = windows(c["B"], c["t"] + c["tc"], seed + 2)
    z = None if c["z"] is None else c["z"] * torch.randn(c["B"], c["D"], generator=torch.Generator().manual_seed(seed + 3))
    ref, out = three_ways(sd, data, ci, xi, z, c["loss_fn"])
    return dict(m=m, sd=sd, data=data, ci=ci, xi=xi, z=z, loss_fn=c["loss_fn"], ref=ref, out=out,
                z0_chain=None if z is not None else z0_k_chain(sd, data, ci, xi))


def compared(name: str):
    """-> [(index into reconstruct's results, what, kind)] of the tensors a case is compared on: the decode-alone cases leave out
    cond_emb and z0, which the caller's latents do not change"""
    return [(i, WHAT[i], KINDS[i]) for i in range(4) if FP64_CASES[name]["z"] is None or i >= 2]


def yard_of(c: dict, i: int) -> Dict[str, torch.Tensor]:
    """The fp32 evaluations of result i of fp64_case's dict c that make its yardstick: the two orders, for z0 also the k-chain."""
    y = {o: c["out"][o][i] for o in c["out"]}
    if i == 1 and c["z0_chain"] is not None:
        y["k_chain"] = c["z0_chain"]
    return y


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

"""The float64 reference and the fp32 yardstick of the pose model, stated once (test infrastructure; nothing under mocodad_amd/
imports it).  tests/test_pose_fp64_host.py (CPU) and tests/test_pose_fp64_gpu.py (GPU) run on exactly these models and inputs.

Reference.  The oracle (oracle/mocodad_oracle.py) as it stands, run in float64: state dict, windows and draws cast (to_f64),
inside `oracle_dtype(torch.float64)`, which hands the oracle's fp32 sinusoid table on in that dtype -- the table is part of the
model, so every run shares its values.  schedule() stays fp32 for the same reason: the three update coefficients are model
constants (utils/diffusion_utils.step_table computes them with the same fp32 torch operations), nobody's error.

Yardstick.  The fp32 error of the same algorithm on the same inputs, in two evaluation orders:
  'bn'      the oracle as written: conv, then F.batch_norm;
  'folded'  BatchNorm folded into the conv weights and bias first (what the weight packer does), then one conv.
yard = the larger of the two errors against float64, on max and on rms separately.  X[kind] is the factor within which the two
orders stay of each other (measured and asserted by the host test, rounded up to the next half); the GPU gate is
err_gpu <= 2 X yard.  Nothing of it comes from the code under test.

random_pose_model builds the seeded random-init models; pass_inputs / chain_inputs / cond_inputs the seeded inputs;
pass_reference / chain_reference / cond_reference evaluate (float64, 'bn', 'folded') once per case and session and share the
result: treat every returned tensor as read-only.
"""
import contextlib
import functools
import zlib
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import mocodad_oracle as O

NS = 10                 # noise steps of the pass tests and of the short chains
ROWS = 45               # rows of a single pass / an encoder call: odd (a partial last workgroup at 4 and at 2 chains per workgroup)
PASS_STEPS = (1, 5, NS - 1)
# the factor two fp32 evaluation orders stay within of each other, per kind of tensor: measured by tests/test_pose_fp64_host.py on
# these inputs and rounded up to the next half (its docstring has the figures)
X = {"pass": 2.0, "cond": 2.0, "pose": 2.0, "loss": 3.0}
ORDERS = ("bn", "folded")


# --------------------------------------------------------------------------- dtype and evaluation order
def to_f64(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Every floating tensor of a state_dict as double (the others, e.g. num_batches_tracked, as they are)."""
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


@contextlib.contextmanager
def oracle_dtype(dtype):
    """Inside: O.pos_encoding returns its fp32 table cast to `dtype`.  The original is back on exit, whatever happened."""
    orig = O.pos_encoding
    O.pos_encoding = lambda t, ch: orig(t, ch).to(dtype)
    try:
        yield
    finally:
        O.pos_encoding = orig


def conv_bn_folded(sd, conv, bn, x):
    """O._conv_bn in the packer's order: g = gamma / sqrt(var + eps); W' = g W, b' = (b - mean) g + beta; one conv."""
    w, b = O._t(sd, conv + ".weight"), O._t(sd, conv + ".bias")
    g = O._t(sd, bn + ".weight") / torch.sqrt(O._t(sd, bn + ".running_var") + O.BN_EPS)
    return F.conv2d(x, w * g[:, None, None, None], (b - O._t(sd, bn + ".running_mean")) * g + O._t(sd, bn + ".bias"))


@contextlib.contextmanager
def folded_conv_bn(on: bool = True):
    """Inside (on=True): every conv + BatchNorm of the oracle is evaluated folded.  The oracle's own order is back on exit."""
    orig = O._conv_bn
    if on:
        O._conv_bn = conv_bn_folded
    try:
        yield
    finally:
        O._conv_bn = orig


@contextlib.contextmanager
def evaluation(dtype, order: str = "bn"):
    assert order in ORDERS, order
    with torch.no_grad(), oracle_dtype(dtype), folded_conv_bn(order == "folded"):
        yield


@contextlib.contextmanager
def one_thread():
    """The fp32 CPU kernels sum in an order that depends on how many threads share a convolution, and the max error of a small
    tensor moves with it (measured: a 15-element loss tensor's spread 2.26 at 8 threads, 2.68 at 16, 2.36 at 1).  The yardstick is
    evaluated on one thread, so that it is one thing wherever the tests run."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def three_ways(fn, sd, *tensors):
    """fn(sd, *tensors) -> tensor or tuple of tensors, evaluated in float64 and in fp32 in both orders -> (ref64, {order: fp32})."""
    cast = lambda ts, d: [t.to(d) if torch.is_tensor(t) and t.is_floating_point() else t for t in ts]
    with evaluation(torch.float64):
        ref = fn(to_f64(sd), *cast(tensors, torch.float64))
    out = {}
    for order in ORDERS:
        with evaluation(torch.float32, order), one_thread():
            out[order] = fn(sd, *cast(tensors, torch.float32))
    return ref, out


# --------------------------------------------------------------------------- models
def _perturb_benign(m, gen) -> None:
    """The perturbation of tests/test_random_configs_gpu.py: eval-mode BatchNorm statistics and PReLU slopes away from their
    initial values (a folded BatchNorm that drops a term must show), the last layer's convs x 0.25 (eps stays O(1))."""
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=gen) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=gen) + 0.5)
            mod.weight.copy_(torch.rand(mod.weight.shape, generator=gen) + 0.5)
            mod.bias.copy_(torch.randn(mod.bias.shape, generator=gen) * 0.1)
        if isinstance(mod, torch.nn.PReLU):
            mod.weight.copy_(torch.rand(mod.weight.shape, generator=gen) * 0.3 + 0.1)
    last = m.model.st_gcnnsu3[-1]
    last.tcn[0].weight.mul_(0.25)
    last.residual[0].weight.mul_(0.25)


def trained_scale(sd, cfg, seed):
    """BatchNorm gains x 10^U(-1,1), PReLU slopes alternating 0.01 / 1.5; the last layer rescaled so that the U-Net's
    eps-prediction stays O(1) (otherwise the 200x..1000x gain of the reverse chain overflows, with any arithmetic).
    cfg: 'seg_len', 'conditioning_strategy', 'conditioning_indices'.  (Windows x 2.5 clamped to +-5 go with it: *_inputs.)"""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    i = 0
    for k in sorted(out):
        if k.endswith(".tcn.1.weight") or k.endswith(".residual.1.weight") or k.endswith(".block.1.weight"):
            out[k] = out[k] * 10 ** (torch.rand(out[k].shape, generator=g) * 2 - 1)
        if k.endswith(".prelu.weight"):
            out[k] = torch.full_like(out[k], 0.01 if i % 2 == 0 else 1.5)
            i += 1
    Tu = cfg["seg_len"] if cfg["conditioning_strategy"] != "inject" else len(O.split_indices(cfg["seg_len"], cfg["conditioning_indices"], "inject")[1])
    for _ in range(3):
        x = torch.randn(16, 2, Tu, 17, generator=g)
        cond = torch.randn(16, 16, generator=g) * 0.5 if cfg["conditioning_strategy"] == "inject" else None
        with torch.no_grad():
            eps = O.unet_forward(out, x, torch.full((16,), 5, dtype=torch.long), cond) - x
        s = float(eps.std())
        for n in ("tcn.0.weight", "tcn.0.bias", "residual.0.weight", "residual.0.bias", "tcn.1.bias", "residual.1.bias",
                  "tcn.1.running_mean", "residual.1.running_mean"):
            k = "model.st_gcnnsu3.1." + n
            out[k] = out[k] * (0.5 / s)
    return out


def _seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def _model(strategy, seg_len, ci, arch, channels, h_dim, seed, scale):
    from helpers import golden_weights, make_args
    from mocodad_amd.models.mocodad import MoCoDAD
    assert scale in ("benign", "trained"), scale
    _, cfg = golden_weights("inject")
    ci = list(ci) if isinstance(ci, tuple) else ci
    with torch.random.fork_rng(), torch.no_grad():
        torch.manual_seed(seed)
        m = MoCoDAD(make_args(cfg, conditioning_strategy=strategy, seg_len=seg_len, conditioning_indices=ci,
                              conditioning_architecture=arch, channels=list(channels), h_dim=h_dim, noise_steps=NS, n_generated_samples=1))
        _perturb_benign(m, torch.Generator().manual_seed(seed + 1))
        if scale == "trained":
            sd = trained_scale({k: v.detach().clone() for k, v in m.state_dict().items()},
                               dict(seg_len=seg_len, conditioning_strategy=m.conditioning_strategy, conditioning_indices=ci), seed + 2)
            m.load_state_dict(sd)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def random_pose_model(strategy, seg_len, conditioning_indices, arch="AE", channels=(32, 16, 32), h_dim=32, seed=0, scale="benign"):
    """-> (MoCoDAD on the CPU, cloned fp32 state_dict): seeded random-init weights.  scale 'benign' = the perturbation of
    tests/test_random_configs_gpu.py; 'trained' = trained_scale on top of it.  Built once per argument set and session and
    shared: treat both as read-only (module.build_scorer(device) packs the weights without moving the module)."""
    ci = tuple(conditioning_indices) if isinstance(conditioning_indices, (list, tuple, range)) else conditioning_indices
    return _model(strategy, int(seg_len), ci, arch, tuple(channels), int(h_dim), int(seed), scale)


# --------------------------------------------------------------------------- inputs
def _windows(shape, gen, scale):
    w = torch.randn(*shape, generator=gen)
    return (w * 2.5).clamp_(-5, 5) if scale == "trained" else w.clamp_(-3, 3)


def pass_inputs(t_unet: int, seed: int, rows: int = ROWS, scale: str = "benign"):
    """Rows of one U-Net pass: x (rows,2,t_unet,17), cond ~ 0.5 N(0,1) (rows,16) (for the models that take one)."""
    g = torch.Generator().manual_seed(seed)
    return _windows((rows, 2, t_unet, 17), g, scale), 0.5 * torch.randn(rows, 16, generator=g)


def cond_inputs(t_cond: int, seed: int, rows: int = ROWS, scale: str = "benign"):
    """Condition frames of `rows` windows: (rows,2,t_cond,17)."""
    return _windows((rows, 2, t_cond, 17), torch.Generator().manual_seed(seed), scale)


def chain_inputs(seg_len: int, n_corrupt: int, ns: int, S: int, B: int, seed: int, scale: str = "benign"):
    """Windows (B,2,seg_len,17) and the parity-mode draws (S, max(ns-1,1), B, 2, n_corrupt, 17) of a scoring call."""
    g = torch.Generator().manual_seed(seed)
    return _windows((B, 2, seg_len, 17), g, scale), torch.randn(S, max(ns - 1, 1), B, 2, n_corrupt, 17, generator=g)


def mask32(sets) -> torch.Tensor:
    """per-window condition frame sets -> (B,) int32 bitmasks (bit 31 is the sign bit)"""
    m = torch.tensor([sum(1 << f for f in fs) for fs in sets], dtype=torch.int64)
    return torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)


# --------------------------------------------------------------------------- the cases
# single passes (HipScorer.unet_forward): (kind, U-Net frames, scale)
PASS_FRAMES = list(range(1, 33))                # 'no_condition', benign: every score_kernel row, every slab-tiled frame count
PASS_INJECT_FRAMES = [3, 6, 12, 24]             # with a condition embedding: 'inject', 3 condition frames + these
PASS_TRAINED_FRAMES = [3, 7, 12, 16, 32]
PASS_CASES = ([("none", t) for t in PASS_FRAMES] + [("inject", t) for t in PASS_INJECT_FRAMES] + [("trained", t) for t in PASS_TRAINED_FRAMES])
# condition encoders alone (HipScorer.cond_encode): condition frames.  mcd_cond_encode has no workspace argument and answers
# MCD_EUNSUPPORTED where the encoder needs global scratch -- 'E_unet' at 13 .. 32 condition frames (the COND form of the slab-tiled
# kernel) and the plain encoder at 25 and more -- so those run where the library runs them, in a scoring call (the enc_* chains
# below: one corrupt frame behind the condition, the smallest U-Net); 32 condition frames cannot occur there (n_cond < seg_len
# <= 32), 31 is the far end of the padded size 32.
COND_AE_FRAMES = list(range(1, 21)) + [21, 24]            # cond_fast_kernel rows; the plain encoder with its buffers in LDS
COND_UNET_FRAMES = list(range(1, 13))                     # cond_unet_kernel rows
COND_E_CASE = (5, (8, 24), 16)                  # 'E' with a runtime channel list: condition frames, channels, h_dim
COND_CASES = ([("AE", t, "benign") for t in COND_AE_FRAMES] + [("E_unet", t, "benign") for t in COND_UNET_FRAMES]
              + [("E", COND_E_CASE[0], "benign")] + [("AE", t, "trained") for t in (3, 12, 16)] + [("E_unet", t, "trained") for t in (3, 12)])
ENC_CHAIN_UNET_FRAMES = [13, 16, 17, 24, 25, 31]          # 'E_unet' in a scoring call: both ends of the padded sizes 16, 24, 32
ENC_CHAIN_AE_FRAMES = [25, 31]                            # the plain encoder with its third buffer in global scratch


def _chain(strategy, seg_len, ci, *, arch="AE", channels=(32, 16, 32), h_dim=32, ns=NS, S=3, B=5, scale="benign",
           losses=("smooth_l1",), sets=None, generic=False):
    return dict(strategy=strategy, seg_len=seg_len, ci=ci, arch=arch, channels=channels, h_dim=h_dim, ns=ns, S=S, B=B, scale=scale,
                losses=losses, sets=sets, generic=generic)


def _r(a, b=None):
    return list(range(a)) if b is None else list(range(a, b))


ALL_LOSSES = ("smooth_l1", "l1", "mse")
# whole chains (parity mode, 15 chains: odd, and 3 mod 4).  generic=True: ALSO run with the 'generic_unet' option.
CHAINS = {
    "inject_3+3": _chain("inject", 6, _r(3), losses=ALL_LOSSES),
    "inject_6+6": _chain("inject", 12, _r(6)),
    "inject_12+12": _chain("inject", 24, _r(12)),
    "inject_4+20": _chain("inject", 24, _r(4)),
    "concat_front6": _chain("concat", 6, _r(3), generic=True),
    "concat_end6": _chain("concat", 6, _r(3, 6), generic=True, losses=ALL_LOSSES),
    "concat_front13": _chain("concat", 13, _r(4), generic=True, losses=ALL_LOSSES),
    "concat_end13": _chain("concat", 13, _r(9, 13), generic=True),
    "concat_front20": _chain("concat", 20, _r(5)),
    "concat_end20": _chain("concat", 20, _r(15, 20)),
    "concat_front32": _chain("concat", 32, _r(8)),
    "concat_end32": _chain("concat", 32, _r(24, 32)),
    "inbetween6": _chain("inbetween_imp", 6, 2),
    "inbetween24": _chain("inbetween_imp", 24, 3),
    "random6": _chain("random_imp", 6, 3, sets=[[0, 1, 2], [1, 3, 5], [0, 4, 5], [2, 3, 4], [0, 2, 5]]),
    "random32": _chain("random_imp", 32, 5, sets=[[31, 0, 7, 16, 30], [3, 31, 12, 13, 14], [1, 2, 4, 8, 31], [0, 1, 2, 3, 4], [5, 11, 17, 23, 29]]),
    **{f"none{t}": _chain("no_condition", t, None) for t in (1, 2, 5, 7, 9, 10, 11, 17)},
    "inject_E_3+3": _chain("inject", 6, _r(3), arch="E", channels=(8, 24), h_dim=16),
    "inject_Eunet_4+4": _chain("inject", 8, _r(4), arch="E_unet"),
    "long_inject_3+3": _chain("inject", 6, _r(3), ns=50, S=2, B=3),
    "long_inject_12+12": _chain("inject", 24, _r(12), ns=50, S=2, B=3),
    "long_none24": _chain("no_condition", 24, None, ns=50, S=2, B=3),
    "trained_inject_3+3": _chain("inject", 6, _r(3), scale="trained", B=37),
    "trained_concat6": _chain("concat", 6, _r(3), scale="trained", B=37),
    "trained_inject_12+12": _chain("inject", 24, _r(12), scale="trained", B=37),
    **{f"enc_Eunet_{t}+1": _chain("inject", t + 1, _r(t), arch="E_unet") for t in ENC_CHAIN_UNET_FRAMES},
    **{f"enc_AE_{t}+1": _chain("inject", t + 1, _r(t)) for t in ENC_CHAIN_AE_FRAMES},
    "enc_trained_Eunet_16+1": _chain("inject", 17, _r(16), arch="E_unet", scale="trained", B=37),
}


def chain_frames(name):
    """-> (U-Net frames, condition-encoder frames) of a chain case"""
    c = CHAINS[name]
    n_cond = 0 if c["ci"] is None else c["ci"] if c["strategy"] == "random_imp" else \
        len(O.split_indices(c["seg_len"], c["ci"], c["strategy"])[0])
    return (c["seg_len"] - n_cond, n_cond) if c["strategy"] == "inject" else (c["seg_len"], 0)


# --------------------------------------------------------------------------- references, once per case and session
def pass_model(kind: str, t_unet: int):
    """kind 'none' | 'trained' ('no_condition' over t_unet frames) | 'inject' (3 condition frames + t_unet) -> (module, state_dict)"""
    if kind == "inject":
        return random_pose_model("inject", t_unet + 3, [0, 1, 2], seed=_seed_of("pass", kind, t_unet))
    return random_pose_model("no_condition", t_unet, None, seed=_seed_of("pass", kind, t_unet), scale="trained" if kind == "trained" else "benign")


@functools.lru_cache(maxsize=None)
def pass_reference(kind: str, t_unet: int):
    """-> dict(x, cond | None, out={t: (ref64, {order: fp32})}) of the passes at PASS_STEPS, each (ROWS,2,t_unet,17)"""
    _, sd = pass_model(kind, t_unet)
    x, cond = pass_inputs(t_unet, _seed_of("pass-in", kind, t_unet), scale="trained" if kind == "trained" else "benign")
    if kind != "inject":
        cond = None
    out = {}
    for t in PASS_STEPS:
        fn = lambda s, x_, c_=None: O.unet_forward(s, x_, torch.full((x_.shape[0],), t, dtype=torch.long), c_)
        out[t] = three_ways(fn, sd, *((x,) if cond is None else (x, cond)))
    return dict(x=x, cond=cond, out=out)


def cond_model(arch: str, t_cond: int, scale: str = "benign"):
    channels, h_dim = (COND_E_CASE[1], COND_E_CASE[2]) if arch == "E" else ((32, 16, 32), 32)
    return random_pose_model("inject", t_cond + 1, list(range(t_cond)), arch=arch, channels=channels, h_dim=h_dim,
                             seed=_seed_of("cond", arch, t_cond, scale), scale=scale)


@functools.lru_cache(maxsize=None)
def cond_reference(arch: str, t_cond: int, scale: str = "benign"):
    """-> dict(x, out=(ref64, {order: fp32})): the condition embedding (ROWS,16)"""
    _, sd = cond_model(arch, t_cond, scale)
    x = cond_inputs(t_cond, _seed_of("cond-in", arch, t_cond, scale), scale=scale)
    return dict(x=x, out=three_ways(O.cond_encode, sd, x))


def chain_model(name: str):
    c = CHAINS[name]
    return random_pose_model(c["strategy"], c["seg_len"], c["ci"], arch=c["arch"], channels=c["channels"], h_dim=c["h_dim"],
                             seed=_seed_of("chain", name), scale=c["scale"])


@functools.lru_cache(maxsize=None)
def chain_reference(name: str):
    """-> dict(data, noise, mask | None, poses=(ref64, {order: fp32}) each (B,S,2,Tx,17), loss={loss_fn: (ref64, {order: fp32})}
    each (B,S)): the layout of HipScorer.score."""
    c = CHAINS[name]
    m, sd = chain_model(name)
    data, noise = chain_inputs(c["seg_len"], m.n_frames_corrupt, c["ns"], c["S"], c["B"], _seed_of("chain-in", name), scale=c["scale"])
    mask = None if c["sets"] is None else mask32(c["sets"])
    assert mask is None or len(c["sets"]) == c["B"]

    def run(s, d, z):
        poses, corrupt = O.reverse_diffusion(s, d, z, noise_steps=c["ns"], strategy=c["strategy"], conditioning_indices=c["ci"], cond_mask=mask)
        return (poses.transpose(0, 1).contiguous(),) + tuple(O.window_losses(poses, corrupt, fn).t().contiguous() for fn in c["losses"])

    ref, out = three_ways(run, sd, data, noise)
    loss = {fn: (ref[1 + i], {o: out[o][1 + i] for o in ORDERS}) for i, fn in enumerate(c["losses"])}
    return dict(data=data, noise=noise, mask=mask, poses=(ref[0], {o: out[o][0] for o in ORDERS}), loss=loss)


# --------------------------------------------------------------------------- measuring
def errors(got: torch.Tensor, ref64: torch.Tensor):
    """-> (max |got - ref64|, rms of got - ref64, max |ref64|)"""
    assert ref64.dtype == torch.float64 and tuple(got.shape) == tuple(ref64.shape), (ref64.dtype, got.shape, ref64.shape)
    d = got.detach().cpu().double() - ref64
    return d.abs().max().item(), d.pow(2).mean().sqrt().item(), ref64.abs().max().item()


def yardstick(ref64, cpu32):
    """-> (max, rms) of the yardstick: per figure the larger of the errors of the evaluation orders against ref64"""
    e = [errors(cpu32[o], ref64) for o in cpu32]
    return max(v[0] for v in e), max(v[1] for v in e)


def spread(ref64, cpu32):
    """-> (max-error spread, rms-error spread) between the evaluation orders: largest / smallest, >= 1"""
    e = [errors(cpu32[o], ref64) for o in cpu32]
    assert all(v[0] > 0 and v[1] > 0 for v in e), "an fp32 evaluation without any error is not fp32"
    return max(v[0] for v in e) / min(v[0] for v in e), max(v[1] for v in e) / min(v[1] for v in e)


def measure(test: str, case: str, what: str, got, ref64, cpu32):
    """Prints one `pose-fp64 |` row -> (gpu max, gpu rms, yard max, yard rms, max|ref64|)."""
    assert torch.isfinite(ref64).all(), (case, what)
    err, rms, top = errors(got, ref64)
    ymax, yrms = yardstick(ref64, cpu32)
    print(f"pose-fp64 | {test:5s} | {case:22s} | {what:16s} | max|ref64| {top:9.3e} | gpu max {err:9.3e} rms {rms:9.3e} | "
          f"yard max {ymax:9.3e} rms {yrms:9.3e} | ratio max {err / ymax:5.2f} rms {rms / yrms:5.2f} | rel {err / max(1.0, top):9.3e}")
    assert torch.isfinite(got).all(), (case, what)
    return err, rms, ymax, yrms, top


def gated(test: str, case: str, what: str, kind: str, got, ref64, cpu32) -> None:
    """The hard gate, the project's: |got - ref64| <= 1e-4 max(1, max|ref64|); the sharp gate, on max and on rms:
    err <= 2 X[kind] yard."""
    err, rms, ymax, yrms, top = measure(test, case, what, got, ref64, cpu32)
    assert err <= 1e-4 * max(1.0, top), (case, what, err, top)
    assert err <= 2 * X[kind] * ymax, (case, what, "max", err, ymax, 2 * X[kind])
    assert rms <= 2 * X[kind] * yrms, (case, what, "rms", rms, yrms, 2 * X[kind])

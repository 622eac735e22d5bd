"""GPU: what a chain is -- its x_T draw, its per-step draws, its frame maps, its update and its loss (csrc/mcd_chain.hpp) -- holds
its recorded bits in every kernel that runs one: score_kernel, score_tiled_kernel, score_generic_kernel, latent_chain_kernel and
the exported draw kernels (philox_noise_kernel, latent_philox_kernel, random_imp_masks_kernel).

The chain contract is stated once and used by several kernels; score_kernel and score_tiled_kernel keep some statements of their
own (their code objects must not move).  tests/golden/chain_bits.json holds the sha256 of the output bytes per case, recorded before the statements were
gathered, and the toolchain line of the library that produced them; a library built by another compiler may legitimately fuse
other operations, so the recorded cases then skip, naming both toolchains.  A digest that moves means a key, a frame map or an
operation order changed: restore it, do not re-record.

Every case: B = 3 windows (a partial workgroup with a clamped slot at two windows per workgroup), 2 samples, noise_steps = 3 (x_T
and one noise step are drawn, the last step is taken without noise), perf mode (in-kernel Philox), first_window_id = 5.  Seeded
random-init models (perturbed BatchNorm statistics and PReLU slopes) and windows from the same generator.

Invariants that need no recording: per kernel family the perf mode is bit for bit the parity mode fed with philox_noise(...) of
the same keys; and score_kernel / score_tiled_kernel -- whose own statements of the draws stay beside the shared ones -- and
score_generic_kernel consume the same x_T: with the exported slot-0 tensor each reproduces its own perf-mode bits, and their poses after
noise_steps = 2 agree within the kernels' cross-check bound (1e-4 relative to max(1, largest value), tests/test_extra6_gpu.py)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import golden_weights, make_args
from latent_ref import _perturb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_bits.json")
B, S, NS, D = 3, 2, 3, 32
SEED, FIRST = 20261019, 5


def _mask32(sets):
    """frame sets -> (B,) int32 bitmasks (bit 31 is the sign bit)"""
    m = torch.tensor([sum(1 << f for f in fs) for fs in sets], dtype=torch.int64)
    return torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)


# name -> (strategy, seg_len, conditioning_indices, condition encoder, generic_unet, per-window condition sets | None)
POSE = {
    "sk_inject6": ("inject", 6, [0, 1, 2], "AE", 0, None),                 # 3 frames, two chains per workgroup
    "sk_concat_end6": ("concat", 6, [3, 4, 5], "AE", 0, None),             # upd_shift: a prediction drives another frame
    "sk_inbetween6": ("inbetween_imp", 6, 2, "AE", 0, None),               # every second frame
    "sk_random6": ("random_imp", 6, 3, "AE", 0, [[0, 1, 2], [1, 3, 5], [0, 4, 5]]),
    "tl_concat13": ("concat", 13, [0, 1, 2, 3], "AE", 0, None),            # pads to 16, two workgroups per CU
    "tl_concat_end20": ("concat", 20, [15, 16, 17, 18, 19], "AE", 0, None),    # pads to 24, twelve waves
    "tl_random32": ("random_imp", 32, 5, "AE", 0, [[31, 0, 7, 16, 30], [3, 31, 12, 13, 14], [1, 2, 4, 8, 31]]),
    "tl_cond_unet16": ("inject", 16, list(range(13)), "E_unet", 0, None),  # the COND form: 13 condition + 3 corrupt frames
    "gen_concat_end6": ("concat", 6, [3, 4, 5], "AE", 1, None),
    "gen_concat13": ("concat", 13, [0, 1, 2, 3], "AE", 1, None),
}
DRAWS = ["draw_pose3", "draw_pose13", "draw_latent32", "draw_masks32"]
CASES = list(POSE) + DRAWS + ["latent3"]
POSE["gen_random6"] = POSE["sk_random6"][:4] + (1,) + POSE["sk_random6"][5:]     # cross-check only: no recorded digest


def _seeded(build, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(), torch.no_grad():
        torch.manual_seed(seed + 1)
        m = build()
        _perturb(m, gen)
    return m, gen


@functools.lru_cache(maxsize=None)
def _pose_model(strategy, seg_len, ci, arch):
    """-> (module on the CPU, its windows): one model per configuration, whichever kernel runs it"""
    from mocodad_amd.models.mocodad import MoCoDAD
    _, cfg = golden_weights("inject")
    ci = list(ci) if isinstance(ci, tuple) else ci
    seed = 6007 + 31 * seg_len + 7 * sorted(["inject", "concat", "inbetween_imp", "random_imp", "no_condition"]).index(strategy) + (100 if arch == "E_unet" else 0)
    m, gen = _seeded(lambda: MoCoDAD(make_args(cfg, conditioning_strategy=strategy, seg_len=seg_len, conditioning_indices=ci,
                                               conditioning_architecture=arch, noise_steps=NS, n_generated_samples=S)), seed)
    return m, torch.randn(B, 2, seg_len, 17, generator=gen)


def _pose(name):
    strategy, seg_len, ci, arch, generic, sets = POSE[name]
    m, data = _pose_model(strategy, seg_len, tuple(ci) if isinstance(ci, list) else ci, arch)
    sc = m.build_scorer(torch.device("cuda:0"))
    if generic:
        sc.set_option("generic_unet", 1)
    return sc, data, (None if sets is None else _mask32(sets))


@functools.lru_cache(maxsize=None)
def _latent_model():
    from latent_ref import load_fixture
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    cfg = load_fixture("B")[2]
    m, gen = _seeded(lambda: MoCoDADlatent(make_args(cfg, conditioning_architecture="AE", seg_len=6, conditioning_indices=[0, 1, 2],
                                                     latent_embedding_dim=D, hidden_sizes=[48, D], noise_steps=NS, n_generated_samples=S)), 6203)
    return m, torch.randn(B, 2, 6, 17, generator=gen)


def _latent():
    m, data = _latent_model()
    return m.build_scorer(torch.device("cuda:0")), data


def _pose_score(name, ns=NS, noise=None):
    sc, data, mask = _pose(name)
    loss, poses = sc.score(data, n_samples=S, noise_steps=ns, noise=noise, seed=SEED, first_window_id=FIRST, want_poses=True, cond_mask=mask)
    return {"loss": loss.cpu(), "poses": poses.cpu()}


def _pose_noise(name, ns=NS):
    return _pose(name)[0].philox_noise(B, n_samples=S, noise_steps=ns, seed=SEED, first_window_id=FIRST)


def _latent_score(noise=None):
    sc, data = _latent()
    _, loss, lat, _ = sc.score(data, n_samples=S, noise_steps=NS, aggregation="all", noise=noise, seed=SEED, first_window_id=FIRST, want_latents=True)
    return {"loss": loss.cpu(), "latents": lat.cpu()}


def _latent_noise():
    return _latent()[0].philox_noise(B, n_samples=S, noise_steps=NS, seed=SEED, first_window_id=FIRST)


def outputs(name):
    """-> {output name: CPU tensor} of the case: one or two tiny launches"""
    if name in POSE:
        return _pose_score(name)
    if name == "latent3":
        return _latent_score()
    if name == "draw_pose3":
        return {"noise": _pose_noise("sk_inject6").cpu()}
    if name == "draw_pose13":
        from mocodad_amd.models.mocodad import MoCoDAD
        _, cfg = golden_weights("inject")
        m = MoCoDAD(make_args(cfg, conditioning_strategy="no_condition", seg_len=13, conditioning_indices=None, noise_steps=NS, n_generated_samples=S))
        sc = m.build_scorer(torch.device("cuda:0"))
        return {"noise": sc.philox_noise(B, n_samples=S, noise_steps=NS, seed=SEED, first_window_id=FIRST).cpu()}
    if name == "draw_latent32":
        return {"noise": _latent_noise().cpu()}
    assert name == "draw_masks32"
    from mocodad_amd.models.mocodad import MoCoDAD
    _, cfg = golden_weights("inject")
    m = MoCoDAD(make_args(cfg, conditioning_strategy="random_imp", seg_len=32, conditioning_indices=16, noise_steps=NS, n_generated_samples=S))
    return {"masks": m.build_scorer(torch.device("cuda:0")).random_imp_masks(B, seed=SEED, first_window_id=FIRST).cpu()}


def shape_of(name, out):
    if name in POSE:
        strategy, seg_len, ci, _, _, _ = POSE[name]
        n_cond = ci if strategy == "random_imp" else (len(range(0, seg_len, ci)) if isinstance(ci, int) else len(ci))
        return {"loss": (B, S), "poses": (B, S, 2, seg_len - n_cond, 17)}[out]
    return {"latent3": {"loss": (B, S), "latents": (B, S, D)}, "draw_pose3": {"noise": (S, NS - 1, B, 2, 3, 17)},
            "draw_pose13": {"noise": (S, NS - 1, B, 2, 13, 17)}, "draw_latent32": {"noise": (S, NS - 1, B, D)},
            "draw_masks32": {"masks": (B,)}}[name][out]


def digest(x: torch.Tensor) -> str:
    assert x.dtype in (torch.float32, torch.int32)
    return hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest()


def library_toolchain():
    from mocodad_amd import _lib
    from mocodad_amd import build as build_mod
    p = build_mod.buildinfo_path(_lib.LIB_PATH)
    return json.load(open(p))["toolchain"] if os.path.exists(p) else None


@pytest.mark.parametrize("name", CASES)
def test_chain_output_bits(name):
    rec = json.load(open(GOLDEN))
    have = library_toolchain()
    if have != rec["toolchain"]:
        pytest.skip(f"digests recorded with {rec['toolchain']!r}; this library was built by {have!r}: output bits not compared")
    want = rec["digests"][name]
    got = outputs(name)
    assert sorted(got) == sorted(want)
    for out, x in got.items():
        assert tuple(x.shape) == shape_of(name, out)
        if x.dtype == torch.float32:
            assert torch.isfinite(x).all(), f"{name} {out}: not finite"      # (a digest of NaNs must not pass)
            assert x.abs().max() > 0
        else:
            assert all(bin(int(v) & 0xFFFFFFFF).count("1") == 16 for v in x), f"{name}: a mask without 16 condition frames"
        print(f"chain-bits | {name} {out} max|x| {x.abs().max().item():.4f} sha256 {digest(x)}")
        assert digest(x) == want[out], f"{name} {out}: a key, a frame map or an operation order of the chain changed (restore the order; do not re-record)"


@pytest.mark.parametrize("name", ["sk_inject6", "tl_concat13", "tl_concat_end20", "gen_concat_end6", "latent3"])
def test_perf_mode_is_parity_mode_on_the_exported_draws(name):
    """One case per kernel family: in-kernel draws == the caller's tensor holding philox_noise(...) of the same keys, bit for bit."""
    perf = outputs(name)
    par = _latent_score(_latent_noise()) if name == "latent3" else _pose_score(name, noise=_pose_noise(name))
    for out in perf:
        assert torch.isfinite(perf[out]).all(), f"{name} {out}: not finite"
        assert torch.equal(perf[out], par[out]), f"{name} {out}: the exported draw is not the kernel's"


@pytest.mark.parametrize("sk, gen", [("sk_concat_end6", "gen_concat_end6"), ("sk_random6", "gen_random6"), ("tl_concat13", "gen_concat13")])
def test_score_kernel_and_generic_kernel_consume_the_same_xT(sk, gen):
    """score_kernel and score_tiled_kernel state their draws and (per-window masks) their corrupt-frame loop themselves, beside the
    shared statements the generic kernel and the export use.  noise_steps = 2 draws x_T alone: each kernel reproduces its perf-mode bits from the exported
    slot-0 tensor (so that tensor is what both consumed), and the two kernels' poses agree within the cross-check bound."""
    z = _pose_noise(sk, ns=2)
    assert tuple(z.shape) == (S, 1, B) + shape_of(sk, "poses")[2:] and torch.isfinite(z).all()
    res = {}
    for name in (sk, gen):
        perf, par = _pose_score(name, ns=2), _pose_score(name, ns=2, noise=z)
        assert torch.isfinite(perf["poses"]).all()
        assert torch.equal(perf["poses"], par["poses"]) and torch.equal(perf["loss"], par["loss"]), f"{name}: x_T is not the exported slot 0"
        res[name] = perf["poses"].numpy()
    a, b = res[sk], res[gen]
    scale = max(1.0, float(np.abs(b).max()))
    print(f"chain-bits | {sk}: own statement vs generic after noise_steps = 2: max |diff| {np.abs(a - b).max():.3e} (bound {1e-4 * scale:.1e})")
    np.testing.assert_allclose(a, b, atol=1e-4 * scale, rtol=0, err_msg=f"{sk} vs score_generic_kernel poses")

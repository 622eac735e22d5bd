"""GPU: which numbers a chain draws for itself.  bench.py, eval_MoCoDAD.py and the stream paths score in perf mode (noise == NULL):
every chain draws its x_T and its step noise inside the kernel, Philox4x32-10 + Box-Muller.  The float64 gates run in parity mode
and say nothing about those draws; here they are pinned in two steps.

  export   mcd_philox_noise / mcd_latent_philox_noise against the NumPy restatement of the key layout (tests/draws_ref.py, checked
           on the CPU by tests/test_draws_host.py): pose Tx 1, 2, 3, 7, 12, 13, 17, 32 and latent D 16 .. 128, each at
           first_window_id 0, 2^32 - 2 (wraps inside the batch), -3 and 2^40 + 5, plus noise_steps 2 and 3 at Tx 3 / D 16.
           Gate: the project's hard gate on every element, |gpu - ref64| <= 1e-4 max(1, max|ref64|) (draws_ref.close_draws; the
           host test shows that it rejects every single-field mistake of a key).
  kernels  perf mode == parity mode fed with the exported tensor, bit for bit (per-sample losses and poses / latents), at every
           row: score_kernel at 1 .. 12 U-Net frames under 'inject' (two condition frames in front, 'AE') and at 2 .. 12 under
           'random_imp' (per-window masks from random_imp_masks, one window's set by hand with frame 0 and, where the count allows,
           the last frame), each with `split` 0, 1 and S, rows 3, 7 and 12 also through the fused call ('median', want_all); the
           slab-tiled kernel at 13, 16, 17, 24, 25, 32 frames under 'concat' and at 16, 24, 32 under 'random_imp', and its COND form
           (13 condition frames, 'E_unet'); the runtime-shape kernel at 1, 7, 12, 13, 32 frames; the latent chain at D 16 .. 128 and,
           at D 32, at 6 and 12 corrupt frames (the four-launch path); one case per family at first_window_id 2^32 - 2.
  last     per case one more parity call with 0.5 added to ONE element of the tensor, the last of everything (s = S - 1, slot
           K - 1, b = B - 1, c = 1, tx = Tx - 1, v = 16; the last d): chain (B - 1, S - 1) changes, every other chain keeps its
           bits -- the equality above is not two kernels ignoring the same slot.

Every call: S 3, noise_steps 4 (slots 0, 1, 2: slot 2 is read), B 5 (the last workgroup is partial at 4, 2 and 1 chains per
workgroup), seed 0xFEDCBA9876543210 (a key with a high word).  The parity calls pass seed 0 and first_window_id 0: nothing of a
parity call depends on either.  Every compared figure is printed (`draws |` rows; the recorded run is profiles/draws_fp64.txt).
The 64-bit index decomposition of philox_noise_kernel past 2^31 elements is not reached (a tensor of over 8 GB).

Found (MI355X, 68 cases, the module alone 4.3 s): no case misses, no kernel was changed.  Export: the largest |gpu - ref64| over the 68
compared tensors is 2.0e-6 (pose Tx 12 .. 32 at first_window_id 2^40 + 5), 4.8e-7 relative to max(1, max|ref64|) at the most, where
NumPy's own fp32 evaluation of the same formula is 8.5e-7 off on that case: the hardware log2 / sin / cos cost a factor of two to three,
fifty times inside the gate.  Kernels: every row is bit-identical to the parity call on the exported tensor, with every `split`; the poked element moves
chain (B - 1, S - 1) alone (its poses or latents by 0.22 .. 0.55, its loss by 2.7e-5 .. 3.4e-2) in every case.  Same keys give the pose and the latent export the
same words wherever their counters coincide (Tx 1 and D 16 share their largest value): the two models never share a call."""
import functools

import numpy as np
import pytest
import torch

import draws_ref as D
import latent_ref as LR
import pose_ref as R

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
S, NS, B = 3, 4, 5
K = D.n_slots(NS)
SEED = 0xFEDCBA9876543210
FIRST, WRAP = 5, 2 ** 32 - 2
FIRSTS = [0, WRAP, -3, 2 ** 40 + 5]
EXPORT_POSE = [1, 2, 3, 7, 12, 13, 17, 32]
EXPORT_LATENT = list(range(16, 129, 16))
HAND = 1                    # the window whose 'random_imp' frame set is written by hand


def _case(family, strategy, seg_len, ci, *, t_unet, t_cond=0, arch="AE", generic=False, splits=(0,), fused=False, first=FIRST, D=None):
    return dict(family=family, strategy=strategy, seg_len=seg_len, ci=ci, t_unet=t_unet, t_cond=t_cond, arch=arch, generic=generic,
                splits=tuple(splits), fused=fused, first=first, D=D)


def _sk(strategy, t, **kw):
    """score_kernel at t U-Net frames: 'inject' behind two condition frames, or 'random_imp' over a window of t frames"""
    kw = dict(t_unet=t, splits=(0, 1, S), fused=t in (3, 7, 12), **kw)
    if strategy == "inject":
        return _case("score_kernel", "inject", t + 2, (0, 1), t_cond=2, **kw)
    return _case("score_kernel", "random_imp", t, max(1, t // 3), **kw)


CASES = {
    **{f"sk_inject{t}": _sk("inject", t) for t in range(1, 13)},
    **{f"sk_random{t}": _sk("random_imp", t) for t in range(2, 13)},
    **{f"tl_concat{t}": _case("tiled", "concat", t, (0, 1, 2), t_unet=t) for t in (13, 16, 17, 24, 25, 32)},
    **{f"tl_random{t}": _case("tiled", "random_imp", t, t // 3, t_unet=t) for t in (16, 24, 32)},
    "tl_cond_unet13+3": _case("tiled_cond", "inject", 16, tuple(range(13)), t_unet=3, t_cond=13, arch="E_unet"),
    "gen_none1": _case("generic", "no_condition", 1, None, t_unet=1, generic=True),
    "gen_concat7": _case("generic", "concat", 7, (0, 1, 2), t_unet=7, generic=True),
    "gen_none12": _case("generic", "no_condition", 12, None, t_unet=12, generic=True),
    "gen_concat13": _case("generic", "concat", 13, (0, 1, 2), t_unet=13, generic=True),
    "gen_none32": _case("generic", "no_condition", 32, None, t_unet=32, generic=True),
    **{f"lat_D{d}": _case("latent", "inject", 6, (0, 1, 2), t_unet=3, t_cond=3, D=d) for d in EXPORT_LATENT},
    "lat_D32_tx6": _case("latent", "inject", 9, (0, 1, 2), t_unet=6, t_cond=3, D=32),
    "lat_D32_tx12": _case("latent", "inject", 15, (0, 1, 2), t_unet=12, t_cond=3, D=32),
    "sk_inject3_wrap": _sk("inject", 3, first=WRAP),
    "tl_concat13_wrap": _case("tiled", "concat", 13, (0, 1, 2), t_unet=13, first=WRAP),
    "gen_concat7_wrap": _case("generic", "concat", 7, (0, 1, 2), t_unet=7, generic=True, first=WRAP),
    "lat_D32_wrap": _case("latent", "inject", 6, (0, 1, 2), t_unet=3, t_cond=3, D=32, first=WRAP),
}


# --------------------------------------------------------------------------- models, scorers, inputs: once per session
@functools.lru_cache(maxsize=None)
def _pose_scorer(strategy, seg_len, ci, arch="AE"):
    """-> (HipScorer, corrupt frames) of the seeded random model of the configuration"""
    m, _ = R.random_pose_model(strategy, seg_len, ci, arch=arch, seed=R._seed_of("draws", strategy, seg_len, ci, arch))
    return m.build_scorer(torch.device(DEVICE)), m.n_frames_corrupt


@functools.lru_cache(maxsize=None)
def _latent_scorer(dim, seg_len=6):
    over = {} if seg_len == 6 else dict(seg_len=seg_len, conditioning_indices=[0, 1, 2])
    m, _ = LR.random_latent_model(dim, [48, dim], seed=700 + dim + seg_len, ns=NS, S=S, tame=True, **over)
    assert m.n_frames_corrupt == seg_len - 3
    return m.build_scorer(torch.device(DEVICE))


def _hand_set(seg_len, n_cond):
    """frame 0, the last frame, then frames 2, 4, ...: as many as the model conditions on"""
    return ([0, seg_len - 1] + list(range(2, seg_len - 1, 2)))[:n_cond]


def _masks(sc, seg_len, n_cond, first):
    m = sc.random_imp_masks(B, seed=SEED, first_window_id=first).cpu()
    m[HAND] = R.mask32([_hand_set(seg_len, n_cond)])[0]
    assert all(bin(int(v) & 0xFFFFFFFF).count("1") == n_cond for v in m), m
    assert int(m[HAND]) & 1
    return m


def row(test, case, what, **figures):
    print(f"draws | {test:7s} | {case:18s} | {what:26s} | " + " | ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


def live(x, what):
    """every compared tensor is finite and not all zero"""
    assert torch.isfinite(x).all(), f"{what}: not finite"
    assert x.abs().max() > 0, f"{what}: all zero"


# --------------------------------------------------------------------------- a. export against the restatement
def _export_gate(kind, size, exporter, ns, first):
    ref = (D.pose_noise if kind == "pose" else D.latent_noise)(SEED, first, B, S, ns, size)
    z = exporter(B, n_samples=S, noise_steps=ns, seed=SEED, first_window_id=first)
    assert tuple(z.shape) == ref.shape, (tuple(z.shape), ref.shape)
    live(z, f"{kind} {size} export")
    got = z.cpu().double().numpy()
    ok, err, idx = D.close_draws(got, ref)
    top = float(np.abs(ref).max())
    row("export", f"{kind} {size}", f"ns {ns} first {first}", **{"max|ref64|": top, "max|gpu-ref64|": err, "rel": err / max(1.0, top),
                                                                "elements": ref.size})
    if not ok:      # the element and the uniforms it was computed from
        u1, u2 = (D.pose_uniforms if kind == "pose" else D.latent_uniforms)(SEED, first, B, S, ns, size)
        print(f"draws | export  | {kind} {size}: element {idx} gpu {got[idx]!r} ref64 {ref[idx]!r} u1 {u1[idx]!r} u2 {u2[idx]!r}")
    assert ok, (kind, size, ns, first, idx, got[idx], ref[idx], err)
    return err


@pytest.mark.parametrize("tx", EXPORT_POSE)
def test_pose_export_is_the_restatement(tx):
    sc, n = _pose_scorer("no_condition", tx, None, "AE")
    assert n == tx
    for first in FIRSTS:
        _export_gate("pose", tx, sc.philox_noise, NS, first)
    if tx == 3:
        for ns in (2, 3):
            _export_gate("pose", tx, sc.philox_noise, ns, FIRST)


@pytest.mark.parametrize("dim", EXPORT_LATENT)
def test_latent_export_is_the_restatement(dim):
    sc = _latent_scorer(dim)
    for first in FIRSTS:
        _export_gate("latent", dim, sc.philox_noise, NS, first)
    if dim == 16:
        for ns in (2, 3):
            _export_gate("latent", dim, sc.philox_noise, ns, FIRST)


# --------------------------------------------------------------------------- b, c. the kernels' own draws
def _pose_call(sc, data, mask, *, fused, noise=None, seed=0, first=0):
    kw = dict(n_samples=S, noise_steps=NS, noise=noise, seed=seed, first_window_id=first, want_poses=True, cond_mask=mask)
    if fused:
        agg, loss, poses = sc.score_fused(data, aggregation="median", want_all=True, **kw)
        return {"agg": agg.cpu(), "loss": loss.cpu(), "poses": poses.cpu()}
    loss, poses = sc.score(data, **kw)
    return {"loss": loss.cpu(), "poses": poses.cpu()}


def _latent_call(sc, data, *, noise=None, seed=0, first=0):
    _, loss, lat, _ = sc.score(data, n_samples=S, noise_steps=NS, aggregation="all", noise=noise, seed=seed, first_window_id=first,
                               want_latents=True)
    return {"loss": loss.cpu(), "latents": lat.cpu()}


def _compare(name, tag, call, z, chain_out):
    """perf == parity on z, bit for bit; then the last element of z + 0.5: chain (B-1, S-1) alone moves.  chain_out: the outputs
    with a (B, S, ...) layout."""
    perf = call(seed=SEED, first=CASES[name]["first"])
    par = call(noise=z)
    assert sorted(perf) == sorted(par)
    for out, x in perf.items():
        live(x, f"{name} {tag} {out}")
        same = torch.equal(x, par[out])
        row("kernels", name, f"{tag} {out}", **{"max|x|": float(x.abs().max()), "perf==parity": same,
                                                "max|diff|": float((x - par[out]).abs().max())})
        assert same, f"{name} {tag} {out}: the kernel's own draw is not the exported one"
    hit = z.clone()
    hit.view(-1)[-1] += 0.5
    assert hit[(S - 1, K - 1, B - 1) + (-1,) * (z.dim() - 3)] == z.view(-1)[-1] + 0.5
    moved = call(noise=hit)
    others = torch.ones(B, S, dtype=torch.bool)
    others[B - 1, S - 1] = False
    for out in chain_out:
        a, b = par[out], moved[out]
        kept = torch.equal(a[others], b[others])
        changed = not torch.equal(a[B - 1, S - 1], b[B - 1, S - 1])
        row("last", name, f"{tag} {out}", **{"others keep bits": kept, "chain (B-1,S-1) moved": changed,
                                             "by": float((a[B - 1, S - 1] - b[B - 1, S - 1]).abs().max())})
        assert kept, f"{name} {tag} {out}: another chain read the last element of the tensor"
        assert changed, f"{name} {tag} {out}: the last slot of the last chain is not read"
    if "agg" in par:
        assert torch.equal(par["agg"][:B - 1], moved["agg"][:B - 1]), f"{name} {tag}: another window's aggregated loss moved"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["family"] != "latent"])
def test_pose_kernel_draws_are_the_exported_ones(name):
    c = CASES[name]
    sc, tx = _pose_scorer(c["strategy"], c["seg_len"], c["ci"], c["arch"])
    assert sc.t_unet == c["t_unet"] and sc.t_cond == c["t_cond"]
    data = R.chain_inputs(c["seg_len"], tx, NS, S, B, R._seed_of("draws-in", name))[0]
    mask = _masks(sc, c["seg_len"], c["ci"], c["first"]) if c["strategy"] == "random_imp" else None
    z = sc.philox_noise(B, n_samples=S, noise_steps=NS, seed=SEED, first_window_id=c["first"])
    assert tuple(z.shape) == (S, K, B, 2, tx, 17)
    ok, err, idx = D.close_draws(z.cpu().double().numpy(), D.pose_noise(SEED, c["first"], B, S, NS, tx))
    assert ok, (name, err, idx)             # (the tensor the kernels are held to is the restatement's)
    try:
        sc.set_option("generic_unet", int(c["generic"]))
        for split in c["splits"]:
            sc.set_option("split", split)
            plan = sc.plan_split(B, S, NS)          # the kernel family the call runs on, and how it is cut
            if c["family"] in ("tiled", "generic"):
                assert plan == 0, (name, plan)
            else:
                assert plan == split if split else plan in (1, S), (name, split, plan)
            for fused in ((False, True) if c["fused"] else (False,)):
                _compare(name, f"split {split}" + (" fused" if fused else ""), functools.partial(_pose_call, sc, data, mask, fused=fused), z,
                         ("loss", "poses"))
    finally:
        sc.set_option("split", 0)
        sc.set_option("generic_unet", 0)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["family"] == "latent"])
def test_latent_chain_draws_are_the_exported_ones(name):
    c = CASES[name]
    sc = _latent_scorer(c["D"], c["seg_len"])
    data = torch.randn(B, 2, c["seg_len"], 17, generator=torch.Generator().manual_seed(R._seed_of("draws-in", name)))
    z = sc.philox_noise(B, n_samples=S, noise_steps=NS, seed=SEED, first_window_id=c["first"])
    assert tuple(z.shape) == (S, K, B, c["D"])
    ok, err, idx = D.close_draws(z.cpu().double().numpy(), D.latent_noise(SEED, c["first"], B, S, NS, c["D"]))
    assert ok, (name, err, idx)
    _compare(name, f"{c['t_unet']} frames", functools.partial(_latent_call, sc, data), z, ("loss", "latents"))

#!/usr/bin/env python3
"""Times the latent model's launches (mcd_latent_encode, the chain launch of mcd_latent_score) on one GPU.

    python tools/latent_bench.py [--out profiles/latent_bench.json] [--reps 30] [--fill-batch 12288]
    python tools/latent_bench.py --cond-arch E_unet            # the three-launch form: cond_unet_kernel + encode + chain
    python tools/latent_bench.py --cond-frames 12              # ... cond_fast_kernel<12,1> + encode + chain (seg_len 15)
    python tools/latent_bench.py --split-encode                # the shipped configuration through the three-launch form
    python tools/latent_bench.py --corrupt-frames 12 --cond-frames 12     # seg_len 24: cond_fast_kernel + encode + projection + chain
                                                               # (default output: profiles/latent_bench_tx12.json)
    python tools/latent_bench.py --stage pretrain --corrupt-frames 12 --cond-frames 12      # the autoencoder's call, mcd_latent_reconstruct
                                                               # (default output: profiles/latent_recon_bench_tx12.json)
    python tools/latent_bench.py --stage forecast --corrupt-frames 12 --cond-frames 12 --batches 1024 96   # generated latents -> poses
                                                               # (default output: profiles/latent_forecast_bench_tx12.json)

Shipped configuration (configs/ubnormal_latent_test.yaml: D 64, hidden [64,128,128,64], noise_steps 10, 10 samples), seeded
random-init weights, perf mode (in-kernel Philox), batch 1024 and a batch that fills the device.  Per batch, three legs alternate
inside one timed loop, each bracketed by device events:
  encode        mcd_latent_encode (5 .. 12 corrupt frames: condition encoder + encode + projection launches)
  score         mcd_latent_score (encode + chain; the chain launch's time is score - encode: the two run back to back on one stream)
  pose_onepass  the yardstick of the encode launch: the pose model's one-pass scoring call (score_fused, noise_steps 2, 1 sample,
                same windows) -- the condition encoder and all 11 U-Net layers, against 7 here
FLOPs are counted from the shapes (functions below), never copied.  Yardsticks of the chain launch: the MFMAs it issues at 32 cycles
per SIMD each (v_mfma_f32_16x16x4_f32) on 256 CUs x 4 SIMDs at --clock-ghz, and the CPU restatement tests/latent_ref.py on 16 threads.
--stage pretrain times mcd_latent_reconstruct (MoCoDADlatentPretrain) instead: the legs `reconstruct` (the whole call), `encode` (the
diffusion stage's mcd_latent_encode on a model of the same frame split and latent size: the launches the two stages share, the
yardstick) and their difference, the unproject + decode launches; the per-launch kernel averages come from a kernel trace of this
command (rocprofv3 --kernel-trace --stats -- python tools/latent_bench.py --stage pretrain ...), not from this script.
--stage forecast times the pose-space scoring of the diffusion stage: the chain call (mcd_latent_score with latent_all) and
mcd_latent_decode_samples on its latents and cond_emb, against the only way there was before that call: the chain call followed by
S calls of mcd_latent_reconstruct(z_in = latents[:, s]).  Legs: `chain`, `decode_samples`, `decode_samples_one_wg_per_window`
(MCD_LATENT_OPT_DECODE_SPW = S: no split of a window's samples), `reconstruct_loop` (the S calls), and the two whole sequences
`forecast` and `baseline`; kernel averages again from a kernel trace of this command.
No GPU: fails (a CPU run says nothing about these times)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mocodad_amd.models.mocodad import MoCoDAD  # noqa: E402
from mocodad_amd.models.mocodad_latent import MoCoDADlatent  # noqa: E402
from mocodad_amd.utils.argparser import load_config  # noqa: E402

DOWN = [(2, 16, 17), (16, 32, 17), (32, 32, 17), (32, 64, 12), (64, 64, 12), (64, 128, 10), (128, 64, 10)]      # (cin, cout, V)
UP = [(64, 64, 12), (64, 32, 12), (32, 32, 17), (32, 2, 17)]


def stgcn_flops(cin, cout, V, T, emb=True):
    """one ST_GCNN_layer (stsgcn.py:94-116): time mix, joint mix, 1x1 conv, residual conv when cin != cout, embedding Linear"""
    f = 2 * cin * V * T * T + 2 * cin * T * V * V + 2 * cin * cout * T * V
    if cin != cout:
        f += 2 * cin * cout * T * V
    return f + (2 * 16 * cout if emb else 0)


def encoder_flops(T, D):
    down = sum(stgcn_flops(a, b, v, T) for a, b, v in DOWN) + 2 * 32 * T * 17 * 12 + 2 * 64 * T * 12 * 10
    return down, 2 * 64 * T * 10 * D


def cond_flops(T, channels=(32, 16, 32, 32), unet=False):
    if unet:      # 'E_unet': the down path without embeddings, ending in 6 channels, + to_time_dim onto 16
        down = DOWN[:-1] + [(128, 6, 10)]
        return (sum(stgcn_flops(a, b, v, T, emb=False) for a, b, v in down) + 2 * 32 * T * 17 * 12 + 2 * 64 * T * 12 * 10
                + 2 * 6 * T * 10 * 16)
    f, cin = 0, 2
    for c in channels:
        f += stgcn_flops(cin, c, 17, T, emb=False)
        cin = c
    return f + 2 * cin * T * 17 * 16


def pose_pass_flops(T):
    layers = sum(stgcn_flops(a, b, v, T) for a, b, v in DOWN + UP)
    return layers + 2 * T * (32 * 17 * 12 + 64 * 12 * 10 + 64 * 10 * 12 + 32 * 12 * 17)


def denoiser_flops(D, hidden):
    ins = [D] + list(hidden[:-1])
    return 2 * sum((i + 16) * o for i, o in zip(ins, hidden))


def chain_mfmas_per_wg_step(D, hidden, n_tiles=2):
    """v_mfma_f32_16x16x4_f32 issued by one workgroup in one denoiser pass: per m-tile and n-tile, in/4 + 4 (the conditioning product)"""
    ins = [D] + list(hidden[:-1])
    return sum((o // 16) * n_tiles * (i // 4 + 4) for i, o in zip(ins, hidden))


def timed(legs, reps, warmup):
    """legs: {name: callable}; alternates them `reps` times -> {name: [ms, ...]}"""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in legs}
    for r in range(reps):
        for k, fn in legs.items():
            ev[k][r][0].record()
            fn()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}


def decoder_flops(T, D):
    """rev_to_time_dim; the up path (layers 7 .. 10, up3, up2); the layers 0 .. 4 and down1 the decode launch runs again for the skips"""
    up = sum(stgcn_flops(a, b, v, T) for a, b, v in UP) + 2 * 64 * T * 10 * 12 + 2 * 32 * T * 12 * 17
    again = sum(stgcn_flops(a, b, v, T) for a, b, v in DOWN[:5]) + 2 * 32 * T * 17 * 12 + 2 * 64 * T * 12 * 10
    return 2 * 64 * T * 10 * D, up, again


def main_pretrain(a):
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    dev = torch.device("cuda:0")
    Tc, Tx = int(a.cond_frames), int(a.corrupt_frames)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", f"latent_recon_bench_tx{Tx}.json")
    cfgs = []
    for name in ("ubnormal_latent_pretrain.yaml", "ubnormal_latent_test.yaml"):
        cfg = load_config(os.path.join(ROOT, "configs", name))
        if a.cond_arch:
            cfg.conditioning_architecture = a.cond_arch
        cfg.seg_len, cfg.conditioning_indices = Tc + Tx, list(range(Tc))
        cfgs.append(cfg)
    torch.manual_seed(0)
    ae, lat = MoCoDADlatentPretrain(cfgs[0]).to(dev), MoCoDADlatent(cfgs[1]).to(dev)
    sa, sl = ae.scorer(), lat.scorer()
    D, T, ns = ae.latent_embedding_dim, ae.n_frames_corrupt, lat.noise_steps
    assert D == lat.latent_embedding_dim
    down_f, ttd_f = encoder_flops(T, D)
    rev_f, up_f, again_f = decoder_flops(T, D)
    cond_f = cond_flops(Tc, unet=cfgs[0].conditioning_architecture == "E_unet")
    res = {"config": {"stage": "pretrain", "latent_dim": D, "frames": [T, Tc], "cond_arch": cfgs[0].conditioning_architecture,
                      "launches_per_call": "[condition encoder] encode [project] unproject decode"},
           "flops_per_window": {"condition_encoder": cond_f, "down_path": down_f, "to_time_dim": ttd_f, "rev_to_time_dim": rev_f,
                                "up_path": up_f, "layers_0_4_again_for_the_skips": again_f,
                                "total": cond_f + down_f + ttd_f + rev_f + up_f + again_f},
           "bytes_per_window": {"H": 4 * 640 * T, "G": 4 * 640 * T, "skips_if_they_crossed_the_launch": 4 * (32 * T * 17 + 64 * T * 12)},
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "batches": {}}
    gen = torch.Generator().manual_seed(1)
    for B in (a.batches or (1024,)):
        data = torch.randn(B, 2, Tc + Tx, 17, generator=gen).clamp_(-3, 3).to(dev)
        legs = {"reconstruct": lambda: sa.reconstruct(data), "reconstruct_loss_only": lambda: sa.reconstruct(data, want_pose=False),
                "encode": lambda: sl.encode(data, noise_steps=ns)}
        t = timed(legs, a.reps, a.warmup)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        res["batches"][str(B)] = {
            "ms_median": med, "ms_min": {k: v[0] for k, v in t.items()}, "ms_max": {k: v[-1] for k, v in t.items()},
            "unproject_plus_decode_ms_derived": med["reconstruct"] - med["encode"], "windows_per_s": B / (med["reconstruct"] * 1e-3),
            "reconstruct_gflops": B * res["flops_per_window"]["total"] / (med["reconstruct"] * 1e-3) / 1e9,
            "reconstruct_over_encode": med["reconstruct"] / med["encode"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def main_forecast(a):
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    dev = torch.device("cuda:0")
    Tc, Tx = int(a.cond_frames), int(a.corrupt_frames)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", f"latent_forecast_bench_tx{Tx}.json")
    cfgs = []
    for name in ("ubnormal_latent_pretrain.yaml", "ubnormal_latent_test.yaml"):
        cfg = load_config(os.path.join(ROOT, "configs", name))
        if a.cond_arch:
            cfg.conditioning_architecture = a.cond_arch
        cfg.seg_len, cfg.conditioning_indices = Tc + Tx, list(range(Tc))
        cfgs.append(cfg)
    torch.manual_seed(0)
    ae, lat = MoCoDADlatentPretrain(cfgs[0]), MoCoDADlatent(cfgs[1]).to(dev)
    sd = ae.state_dict()
    sd.update({k: v.detach().cpu() for k, v in lat.state_dict().items() if k in sd})      # the tensors the two stages share
    lat.load_decoder(sd)
    sl, sa = lat.scorer(), lat.decoder()
    D, T, ns, S = lat.latent_embedding_dim, lat.n_frames_corrupt, lat.noise_steps, lat.n_generated_samples
    rev_f, up_f, again_f = decoder_flops(T, D)
    res = {"config": {"stage": "forecast", "latent_dim": D, "frames": [T, Tc], "noise_steps": ns, "n_samples": S,
                      "cond_arch": cfgs[0].conditioning_architecture,
                      "launches": {"decode_samples": "per chunk of windows: unproject, decode", "reconstruct_loop": f"{S} x ([condition encoder] encode [project] unproject decode)"}},
           "flops_per_window": {"rev_to_time_dim_per_sample": rev_f, "up_path_per_sample": up_f, "stem_for_the_skips": again_f,
                                "decode_samples": S * (rev_f + up_f) + again_f, "decode_launches_of_the_loop": S * (rev_f + up_f + again_f)},
           "bytes_per_window": {"G": 4 * 640 * T * S, "latents": 4 * D * S, "pose_all": 4 * 2 * T * 17 * S},
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "batches": {}}
    gen = torch.Generator().manual_seed(1)
    for B in (a.batches or (1024, 96)):
        data = torch.randn(B, 2, Tc + Tx, 17, generator=gen).clamp_(-3, 3).to(dev)
        chain = lambda: sl.score(data, n_samples=S, noise_steps=ns, aggregation="all", want_latents=True, want_cond=True, seed=1)
        _, _, z, _, cond = chain()
        z, cond = z.clone(), cond.clone()

        def one_wg_per_window():
            sa.set_option("decode_spw", S)
            sa.decode_samples(data, z, cond)
            sa.set_option("decode_spw", 0)

        def loop(lat_all=z):
            for s in range(S):
                sa.reconstruct(data, z=lat_all[:, s])

        def forecast():
            _, _, l, _, c = chain()
            return sa.decode_samples(data, l, c)

        def baseline():
            loop(chain()[2])
        # the new call and the loop it replaces must agree bit for bit at the size that is timed
        p, lo = sa.decode_samples(data, z, cond)
        for s in (0, S - 1):
            p1, l1, _, _ = sa.reconstruct(data, z=z[:, s])
            assert torch.equal(p[:, s], p1) and torch.equal(lo[:, s], l1)
        legs = {"chain": chain, "decode_samples": lambda: sa.decode_samples(data, z, cond), "decode_samples_one_wg_per_window": one_wg_per_window,
                "reconstruct_loop": loop, "forecast": forecast, "baseline": baseline}
        t = timed(legs, a.reps, a.warmup)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        res["batches"][str(B)] = {
            "ms_median": med, "ms_min": {k: v[0] for k, v in t.items()}, "ms_max": {k: v[-1] for k, v in t.items()},
            "decode_samples_over_reconstruct_loop": med["decode_samples"] / med["reconstruct_loop"],
            "forecast_over_baseline": med["forecast"] / med["baseline"],
            "split_over_one_wg_per_window": med["decode_samples"] / med["decode_samples_one_wg_per_window"],
            "windows_per_s_forecast": B / (med["forecast"] * 1e-3),
            "decode_samples_gflops": B * res["flops_per_window"]["decode_samples"] / (med["decode_samples"] * 1e-3) / 1e9}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default: profiles/latent_bench.json, profiles/latent_bench_tx<N>.json with --corrupt-frames N")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fill-batch", type=int, default=12288)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--cond-arch", choices=["AE", "E", "E_unet"], default=None, help="conditioning_architecture (default: the YAML's 'AE')")
    ap.add_argument("--cond-frames", type=int, default=3, help="condition frames, 1 .. 12 (seg_len = this + the corrupt frames)")
    ap.add_argument("--corrupt-frames", type=int, default=3, help="corrupt frames: 3 or 5 .. 12")
    ap.add_argument("--batches", type=int, nargs="+", default=None, help="window counts to time (default: 1024 and --fill-batch)")
    ap.add_argument("--split-encode", action="store_true", help="MCD_LATENT_OPT_SPLIT_ENCODE: the shipped configuration in three launches")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement of the chain")
    ap.add_argument("--stage", choices=["diffusion", "pretrain", "forecast"], default="diffusion",
                    help="pretrain: time mcd_latent_reconstruct; forecast: the chain call + mcd_latent_decode_samples against the loop of reconstruct calls")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_bench.py needs an MI355X: nothing about these launches can be timed on a CPU")
    if a.stage == "pretrain":
        return main_pretrain(a)
    if a.stage == "forecast":
        return main_forecast(a)
    import latent_ref as R
    dev = torch.device("cuda:0")
    cfg = load_config(os.path.join(ROOT, "configs", "ubnormal_latent_test.yaml"))
    Tc, Tx = int(a.cond_frames), int(a.corrupt_frames)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "latent_bench.json" if Tx == 3 else f"latent_bench_tx{Tx}.json")
    if a.cond_arch:
        cfg.conditioning_architecture = a.cond_arch
    if Tc != 3 or Tx != 3:
        cfg.seg_len, cfg.conditioning_indices = Tc + Tx, list(range(Tc))
    unet = cfg.conditioning_architecture == "E_unet"
    torch.manual_seed(0)
    lat = MoCoDADlatent(cfg).to(dev)
    if a.split_encode:
        lat.scorer().set_option("split_encode", 1)
    # 3 corrupt frames: the fused form, or the condition encoder in front; 5 .. 12: condition encoder, encode, projection, chain
    launches = 4 if Tx != 3 else 2 if (not unet and Tc == 3 and not a.split_encode) else 3
    pose = MoCoDAD(load_config(os.path.join(ROOT, "configs", "hr_avenue_test.yaml"))).to(dev)
    sl, sp = lat.scorer(), pose.scorer()
    D, hidden, ns, S, T = lat.latent_embedding_dim, lat.hidden_sizes, lat.noise_steps, lat.n_generated_samples, lat.n_frames_corrupt
    down_f, ttd_f = encoder_flops(T, D)
    cond_f = cond_flops(Tc, unet=unet)
    enc_f = down_f + ttd_f + cond_f
    step_f = denoiser_flops(D, hidden)
    chain_f = step_f * S * (ns - 1)
    res = {"config": {"latent_dim": D, "hidden_sizes": hidden, "noise_steps": ns, "n_samples": S, "frames": [T, Tc],
                      "cond_arch": cfg.conditioning_architecture, "launches_per_score": launches},
           "flops_per_window": {"down_path": down_f, "to_time_dim": ttd_f, "condition_encoder": cond_f, "denoiser_per_chain_step": step_f,
                                "chain": chain_f, "total": enc_f + chain_f, "pose_one_pass_call": pose_pass_flops(3) + cond_flops(3)},      # (the yardstick stays 3 + 3 frames)
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "clock_ghz_assumed": a.clock_ghz, "batches": {}}
    gen = torch.Generator().manual_seed(1)
    for B in (a.batches or (1024, a.fill_batch)):
        data = torch.randn(B, 2, Tc + Tx, 17, generator=gen).clamp_(-3, 3).to(dev)
        data6 = data if Tc + Tx == 6 else torch.randn(B, 2, 6, 17, generator=gen).clamp_(-3, 3).to(dev)      # (the pose yardstick stays 3 + 3)
        legs = {"encode": lambda: sl.encode(data, noise_steps=ns),
                "score": lambda: sl.score(data, n_samples=S, noise_steps=ns, aggregation="best", seed=1),
                "pose_onepass": lambda: sp.score_fused(data6, n_samples=1, noise_steps=2, aggregation="best", seed=1)}
        t = timed(legs, a.reps, a.warmup)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        chain_ms = med["score"] - med["encode"]
        wpg = 1 if S >= 32 else 32 // S
        wgs = (B + wpg - 1) // wpg
        mfma_ms = wgs * (ns - 1) * chain_mfmas_per_wg_step(D, hidden) * 32 / (256 * 4) / (a.clock_ghz * 1e6)
        res["batches"][str(B)] = {
            "ms_median": med, "ms_min": {k: v[0] for k, v in t.items()}, "ms_max": {k: v[-1] for k, v in t.items()},
            "chain_ms_derived": chain_ms, "clips_per_s": B / (med["score"] * 1e-3),
            "encode_gflops": B * enc_f / (med["encode"] * 1e-3) / 1e9, "chain_gflops": B * chain_f / (chain_ms * 1e-3) / 1e9,
            "encode_over_pose_onepass": med["encode"] / med["pose_onepass"],
            "chain_workgroups": wgs, "chain_mfma_issue_bound_ms": mfma_ms, "chain_over_mfma_issue_bound": chain_ms / mfma_ms}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.no_cpu:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res, indent=1))
        return
    # the CPU restatement of the chain on 16 threads, batch 1024 (fp32 torch ops: 4 GEMMs + BN + ReLU per step, as the reference runs it)
    torch.set_num_threads(16)
    sd = {k: v.detach().cpu() for k, v in lat.state_dict().items()}
    B = 1024
    if "1024" not in res["batches"]:
        raise SystemExit("the CPU comparison is made at batch 1024: add it to --batches or pass --no-cpu")
    cond, z0 = torch.randn(B, 16), torch.randn(B, D)
    noise = torch.randn(S, ns - 1, B, D)
    with torch.no_grad():
        R.chain(sd, cond, z0, noise, ns)
        t0 = time.perf_counter()
        for _ in range(3):
            R.chain(sd, cond, z0, noise, ns)
        cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    res["cpu_chain_ms_1024_16_threads"] = cpu_ms
    res["cpu_over_gpu_chain_1024"] = cpu_ms / res["batches"]["1024"]["chain_ms_derived"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

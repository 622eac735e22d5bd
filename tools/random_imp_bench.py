#!/usr/bin/env python3
"""'random_imp': what a batch costs with the frame sets drawn on the host (random_imp_draw='host': one torch.randperm per window,
the reference's draw) against drawn on the device (random_imp_draw='device': mcd_random_imp_masks), on one GPU.

    python tools/random_imp_bench.py [--out profiles/random_imp_draw.json]

One process.  seg_len 6, 3 condition frames, noise_steps 10, 5 samples, 1024 windows per batch (configs/hr_avenue_test.yaml with the
strategy swapped), seeded random-init weights, perf-mode noise, the windows resident on the device, the loss-only 'best' call
(one trajectory launch per batch).  After a warm-up of both modes, blocks of --calls forward calls alternate between the two modules;
a block is timed by a host clock from its first call to the return of ONE device synchronise behind its last, and its figure is
that time over the number of calls.  --blocks blocks each: the median over the blocks and their range are reported per mode.
Separately, bracketed by device events and alternating too: the mask launch alone and the scoring call alone (masks given).
No GPU: fails (a CPU run says nothing about these times)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mocodad_amd.models.mocodad import MoCoDAD  # noqa: E402
from mocodad_amd.utils.argparser import load_config  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_imp_draw.json"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10, help="forward calls per mode before the timed blocks")
    ap.add_argument("--event-reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("random_imp_bench.py needs an MI355X: nothing about these times can be measured on a CPU")
    dev = torch.device("cuda:0")
    cfg = load_config(os.path.join(ROOT, "configs", "hr_avenue_test.yaml"))
    cfg.conditioning_strategy, cfg.conditioning_indices = "random_imp", 3
    B, S, ns = int(cfg.batch_size), int(cfg.n_generated_samples), int(cfg.noise_steps)
    mods = {}
    for mode in ("host", "device"):
        cfg.random_imp_draw = mode
        torch.manual_seed(0)              # the same weights in both
        mods[mode] = MoCoDAD(cfg).to(dev)
    data = torch.randn(B, 2, cfg.seg_len, 17, generator=torch.Generator().manual_seed(1)).clamp_(-3, 3).to(dev)
    batch = [data, torch.zeros(B), torch.zeros(B, 4), torch.zeros(B, cfg.seg_len)]
    torch.manual_seed(2)                  # the host draw's generator

    def block(m, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            m.forward(batch, window_offset=i * B)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for m in mods.values():
        block(m, a.warmup)
    per_block = {k: [] for k in mods}
    for _ in range(a.blocks):
        for k, m in mods.items():
            per_block[k].append(block(m, a.calls))

    # the launches alone, device events: the mask launch, and the scoring call with the masks given
    sc = mods["device"].scorer()
    masks = sc.random_imp_masks(B, cfg.seed, 0)
    legs = {"mask_launch": lambda: sc.random_imp_masks(B, cfg.seed, 0),
            "scoring_call": lambda: sc.score_fused(data, n_samples=S, noise_steps=ns, aggregation="best", seed=cfg.seed, cond_mask=masks)}
    for _ in range(5):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.event_reps)] for k in legs}
    for r in range(a.event_reps):
        for k, fn in legs.items():
            ev[k][r][0].record()
            fn()
            ev[k][r][1].record()
        torch.cuda.synchronize()          # (each pair on an idle device: the event pair brackets this launch only)
    ev_ms = {k: sorted(x.elapsed_time(y) for x, y in v) for k, v in ev.items()}

    # host time of the reference's draw alone (no GPU work in it)
    t0 = time.perf_counter()
    for _ in range(3):
        mods["host"].draw_random_imp_mask(B)
    host_draw_ms = (time.perf_counter() - t0) * 1e3 / 3

    med = {k: median(v) for k, v in per_block.items()}
    spread_host = max(per_block["host"]) - min(per_block["host"])
    res = {"config": {"seg_len": int(cfg.seg_len), "n_cond": 3, "noise_steps": ns, "n_samples": S, "windows_per_batch": B,
                      "aggregation": cfg.aggregation_strategy, "weights": "seeded random init"},
           "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls_per_block": a.calls, "warmup_calls_per_mode": a.warmup,
           "per_batch_ms_by_block": per_block,
           "per_batch_ms_median": med,
           "per_batch_ms_range": {k: [min(v), max(v)] for k, v in per_block.items()},
           "host_minus_device_ms": med["host"] - med["device"],
           "host_block_spread_ms": spread_host,
           "device_below_host_by_more_than_host_spread": bool(med["host"] - med["device"] > spread_host),
           "clips_per_s": {k: B / (v * 1e-3) for k, v in med.items()},
           "event_ms_median": {k: median(v) for k, v in ev_ms.items()},
           "event_ms_range": {k: [v[0], v[-1]] for k, v in ev_ms.items()},
           "mask_launch_over_scoring_call": median(ev_ms["mask_launch"]) / median(ev_ms["scoring_call"]),
           "host_draw_alone_ms": host_draw_ms}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

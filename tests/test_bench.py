"""bench.py's command line: a plain run prints the headline line alone (the informational legs need --full), and
--dump-outputs writes what the timed path returned in its last step -- the same scores a direct HipScorer call on the
benchmark's fixed inputs and noise seed gives, run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("cpu_baseline", "auc", "sustained", "e2e", "value_incl_h2d")


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    import torch
    import bench
    from mocodad_amd.engine import HipScorer

    steps, B = 3, 256
    lines, dumps = [], []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--steps", str(steps), "--warmup", "1", "--batch", str(B),
                            "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
        dumps.append(np.load(tmp_path / run / "window_scores.npy"))
    d = lines[0]
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "clips/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and "roofline" in d
    assert all(d.get(k) is None for k in FULL_ONLY + ("gpu_after_timed_region",))
    s = dumps[0]
    assert s.dtype == np.float32 and s.shape == (B,) and np.isfinite(s).all()
    np.testing.assert_allclose(dumps[1], s, atol=1e-6, rtol=0)
    # the last timed step, recomputed: avenue workload, windows of seed 1000, Philox seed 100 + (steps - 1)
    variant, _, ns, S, _ = bench.CONFIGS["avenue"]
    sd, cfg = bench.load_weights(variant)
    ci, xi = bench.frame_split(cfg["seg_len"], cfg["conditioning_indices"], cfg["conditioning_strategy"])
    sc = HipScorer(sd, strategy=cfg["conditioning_strategy"], seg_len=cfg["seg_len"], cond_idx=ci, corrupt_idx=xi,
                   cond_channels=list(cfg["channels"]) + [cfg["h_dim"]], device="cuda:0", options=dict(split=0, phase=0, variant=0))
    data = bench.synth_windows(B, cfg["seg_len"], 1000).to("cuda:0")
    best, _, _ = sc.score_fused(data, n_samples=S, noise_steps=ns, aggregation="best", seed=100 + steps - 1, first_window_id=0)
    torch.cuda.synchronize()
    np.testing.assert_allclose(s, best.cpu().numpy(), atol=1e-6, rtol=0)

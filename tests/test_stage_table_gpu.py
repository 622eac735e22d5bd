"""GPU: the per-wave stage table of the 3-frame trajectory kernel (csrc/mcd_stage_table.hpp) addresses exactly what the scalar
arithmetic it replaces addressed.

score_kernel<3, 2, 4> and its layer-test twin read the LDS bases of a wave's mix and resampler units from a table row instead of
deriving them from the wave index in every stage; the table is checked entry by entry at compile time.  Here the outputs of the
kernels are compared with what the library computed BEFORE the table existed: tests/golden/stage_table_bits.json holds the sha256
of the output bytes per case and the toolchain line of the library that produced them (a library built by another compiler may
legitimately fuse other operations: the recorded cases then skip, naming both toolchains, as in test_chain_bits_gpu.py).  A digest
that moves means an address or an operation order changed: restore it, do not re-record.

Shapes: 2 samples x noise_steps 3 (every stage row of every wave and both rounds of the 12-unit stages are used in each of the two
passes of a trajectory); 1 and 3 windows leave the clamped duplicate chain slot of a workgroup in use.

    python tests/test_stage_table_gpu.py out.json        # records the digests of the library in use"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_table_bits.json")
S, NS = 2, 3
SEED, FIRST = 20261019, 5
STAGES = [(i, f"L{i}") for i in range(11)] + [(11, "down1"), (12, "down2"), (13, "up3"), (14, "up2")]


@functools.lru_cache(maxsize=None)
def _inject():
    from test_hip_parity import _scorer
    return _scorer("inject")


@functools.lru_cache(maxsize=None)
def _windows(B):
    return torch.randn(B, 2, 6, 17, generator=torch.Generator().manual_seed(4100 + B))


def digest(x: torch.Tensor) -> str:
    assert x.dtype == torch.float32
    return hashlib.sha256(x.contiguous().cpu().numpy().tobytes()).hexdigest()


def fused_perf(B, split):
    """-> (per-sample losses (B, S), best score per window (B,)) of the inject model in perf mode"""
    sc = _inject()[0]
    sc.set_option("split", split)
    try:
        agg, all_, _ = sc.score_fused(_windows(B), n_samples=S, noise_steps=NS, aggregation="best", seed=SEED, first_window_id=FIRST, want_all=True)
    finally:
        sc.set_option("split", 0)
    return all_.cpu(), agg.cpu()


def stage_output(sid, name):
    """stage `sid` alone (mcd_layer_forward: the layer-test twin of the kernel) on the first 2 windows of the reference's layer input"""
    from conftest import load_golden
    from mocodad_amd import _lib
    g = load_golden("layers_inject.npz")
    assert _lib.lib().mcd_debug_poison_lds(None) == 0
    return _inject()[0].layer_forward(sid, torch.from_numpy(g[f"{name}_in"][:2]), torch.from_numpy(g["emb_in"][:2])).cpu()


def record():
    from test_chain_bits_gpu import library_toolchain
    d = {}
    for B in (1, 3):
        all_, agg = fused_perf(B, 1)
        d[f"fused_B{B}"] = {"loss": digest(all_), "best": digest(agg)}
    for sid, name in STAGES:
        d[f"stage_{sid}"] = {"out": digest(stage_output(sid, name))}
    return {"toolchain": library_toolchain(), "digests": d}


def _recorded(case):
    from test_chain_bits_gpu import library_toolchain
    rec = json.load(open(GOLDEN))
    have = library_toolchain()
    if have != rec["toolchain"]:
        pytest.skip(f"digests recorded with {rec['toolchain']!r}; this library was built by {have!r}: output bits not compared")
    return rec["digests"][case]


@pytest.mark.parametrize("B", [1, 3])
def test_fused_perf_mode_bits_window_major_and_chain_major(B):
    want = _recorded(f"fused_B{B}")
    ref = None
    for split in (1, S):
        all_, agg = fused_perf(B, split)
        assert tuple(all_.shape) == (B, S) and tuple(agg.shape) == (B,)
        assert torch.isfinite(all_).all() and all_.abs().max() > 0          # (a digest of NaNs must not pass)
        print(f"stage-table | B {B} split {split}: loss sha256 {digest(all_)} best sha256 {digest(agg)}")
        assert digest(all_) == want["loss"], f"B {B} split {split}: per-sample losses moved"
        assert digest(agg) == want["best"], f"B {B} split {split}: best scores moved"
        ref = all_ if ref is None else ref
        assert torch.equal(all_, ref), f"B {B}: split {split} differs from split 1"


def test_parity_mode_vs_oracle():
    """3 windows (the second workgroup's second chain slot is the clamped duplicate), the caller's noise tensor: poses and losses
    against the oracle at the suite's bound (1e-4 absolute, tests/test_hip_parity.py)."""
    from oracle import mocodad_oracle as O
    from test_hip_parity import ATOL
    sc, sd, _ = _inject()
    B = 3
    gen = torch.Generator().manual_seed(4203)
    data = torch.randn(B, 2, 6, 17, generator=gen)
    noise = torch.randn(S, NS - 1, B, 2, 3, 17, generator=gen)
    loss, poses = sc.score(data, n_samples=S, noise_steps=NS, noise=noise, want_poses=True)
    with torch.no_grad():
        p_ref, corrupt = O.reverse_diffusion(sd, data, noise, noise_steps=NS, strategy="inject", conditioning_indices=[0, 1, 2])
        l_ref = O.window_losses(p_ref, corrupt)
    np.testing.assert_allclose(poses.cpu().numpy(), p_ref.transpose(0, 1).numpy(), atol=ATOL, rtol=1e-5)
    np.testing.assert_allclose(loss.cpu().numpy(), l_ref.t().numpy(), atol=ATOL, rtol=0)


@pytest.mark.parametrize("sid, name", STAGES)
def test_layer_test_twin_stage_bits(sid, name):
    want = _recorded(f"stage_{sid}")
    out = stage_output(sid, name)
    assert out.shape[0] == 2 and torch.isfinite(out).all() and out.abs().max() > 0
    print(f"stage-table | stage {sid} ({name}): sha256 {digest(out)}")
    assert digest(out) == want["out"], f"stage {sid} ({name}): the layer-test twin's output moved"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    with open(sys.argv[1], "w") as fh:
        json.dump(record(), fh, indent=1)
        fh.write("\n")

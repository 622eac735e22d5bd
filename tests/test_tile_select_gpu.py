"""GPU: the 3-frame trajectory kernel picks a GEMM tile's embedding row (which of the workgroup's two chains a column belongs to)
per tile SLOT at compile time and per lane only in the one tile that holds columns of both chains (mcd_device.hpp, TSEL).  What
can go wrong is a column that carries the OTHER chain's embedding, so:
  - a whole scoring call in parity mode on an odd window count (the last workgroup's second chain slot is a clamped duplicate)
    against the oracle, repeated, and cut into workgroups both ways;
  - stages 3 and 5 alone (mcd_layer_forward) on two windows with DIFFERENT embeddings: the columns on both sides of the chain
    boundary (0-based 35 | 36, 37 at 12 joints, 29 | 30, 31 at 10: all inside the straddling tile) against the reference's layer
    I/O, and each window's output independent of the other window's embedding."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
ATOL = 1e-4         # tests/test_hip_parity.py


@pytest.fixture(scope="module")
def scorer():
    from mocodad_amd.engine import HipScorer
    w = load_golden("weights_inject.npz")
    cfg = json.loads(bytes(w.pop("__cfg__")).decode())
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sc = HipScorer(sd, strategy="inject", seg_len=6, cond_idx=[0, 1, 2], corrupt_idx=[3, 4, 5],
                   cond_channels=list(cfg["channels"]) + [cfg["h_dim"]], device="cuda:0")
    return sc, sd


def test_odd_window_count_parity_and_bit_identity(scorer):
    from oracle import mocodad_oracle as O
    sc, sd = scorer
    gen = torch.Generator().manual_seed(31)
    B, S, ns = 3, 2, 3          # ns = 3: one pass that adds noise, one that does not
    data = torch.randn(B, 2, 6, 17, generator=gen)
    noise = torch.randn(S, ns - 1, B, 2, 3, 17, generator=gen)
    with torch.no_grad():
        _, ref = O.score(sd, data, noise, noise_steps=ns, strategy="inject", conditioning_indices=[0, 1, 2], aggregation="best")
    out = {}
    try:
        for split in (1, S):
            sc.set_option("split", split)
            best, all_, _ = sc.score_fused(data, n_samples=S, noise_steps=ns, aggregation="best", noise=noise, want_all=True)
            again, all2, _ = sc.score_fused(data, n_samples=S, noise_steps=ns, aggregation="best", noise=noise, want_all=True)
            assert torch.equal(best, again) and torch.equal(all_, all2), f"split={split}: the same call twice"
            out[split] = (best.clone(), all_.clone())
    finally:
        sc.set_option("split", 0)
    err = float((out[1][0].cpu() - ref).abs().max())
    print(f"B = 3, S = 2, ns = 3: max |hip - oracle| on the window scores = {err:.3e}")
    np.testing.assert_allclose(out[1][0].cpu().numpy(), ref.numpy(), atol=ATOL, rtol=0)
    assert torch.equal(out[1][0], out[S][0]) and torch.equal(out[1][1], out[S][1]), "split=1 against split=S"
    assert torch.equal(out[1][1].min(1)[0], out[1][0])


# (stage, joints, channels checked): the chain boundary lies at column 3 V, inside a 16-column tile at both joint counts
@pytest.mark.parametrize("stage,V", [(3, 12), (5, 10)])
def test_straddling_tile_carries_each_chains_embedding(scorer, stage, V):
    sc, _ = scorer
    g = load_golden("layers_inject.npz")
    x = torch.from_numpy(g[f"L{stage}_in"][:2])
    e = torch.from_numpy(g["emb_in"][:2])
    assert float((e[0] - e[1]).abs().max()) > 0.1, "the two windows' embeddings differ"
    ref = g[f"L{stage}_out"][:2]
    out = sc.layer_forward(stage, x, e).cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(out, ref, atol=2e-5 * scale, rtol=1e-5, err_msg=f"layer {stage}")      # tests/test_layers_gpu.py's bound
    # the two columns at the chain boundary: (window 0, frame 2, joint V - 1) = column 3 V - 1, (window 1, frame 0, joint 0) = column 3 V
    assert 3 * V - 1 == {12: 35, 10: 29}[V] and (3 * V) // 16 == (3 * V - 1) // 16, "both in the tile that straddles"
    np.testing.assert_allclose(out[0, :, 2, V - 1], ref[0, :, 2, V - 1], atol=2e-5 * scale, rtol=1e-5, err_msg=f"layer {stage} column {3 * V - 1}")
    np.testing.assert_allclose(out[1, :, 0, 0], ref[1, :, 0, 0], atol=2e-5 * scale, rtol=1e-5, err_msg=f"layer {stage} column {3 * V}")
    np.testing.assert_allclose(out[1, :, 0, 1], ref[1, :, 0, 1], atol=2e-5 * scale, rtol=1e-5, err_msg=f"layer {stage} column {3 * V + 1}")
    # a window's output depends on its own embedding alone: swapping in another row for window 1 leaves window 0 bit-identical
    # (every column of chain 0, the straddling tile's included) and moves window 1 everywhere
    e2 = e.clone()
    e2[1] = torch.from_numpy(g["emb_in"][2])
    out2 = sc.layer_forward(stage, x, e2).cpu().numpy()
    assert np.array_equal(out2[0], out[0])
    assert (np.abs(out2[1] - out[1]).max(axis=0) > 0).all(), "every (frame, joint) column of window 1 carries window 1's embedding"
    e3 = e.clone()
    e3[0] = torch.from_numpy(g["emb_in"][3])
    out3 = sc.layer_forward(stage, x, e3).cpu().numpy()
    assert np.array_equal(out3[1], out[1])
    assert (np.abs(out3[0] - out[0]).max(axis=0) > 0).all(), "every (frame, joint) column of window 0 carries window 0's embedding"

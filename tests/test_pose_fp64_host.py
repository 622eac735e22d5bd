"""CPU: the float64 reference and the fp32 yardstick that tests/test_pose_fp64_gpu.py measures the trajectory kernels and the
condition encoders against, on exactly the models and inputs of those tests (tests/pose_ref.py).  Nothing here runs a kernel:
these tests say that the reference is finite, of the stated size and of a size that comes from the inputs and the schedule, and
that the yardstick is a property of fp32, not of the order it happens to be evaluated in.

Two fp32 evaluation orders against float64: 'bn' (conv, then F.batch_norm: the oracle as written) and 'folded' (BatchNorm folded
into the conv first, as the weight packer does), both on one CPU thread (pose_ref.one_thread).  Spread = larger error / smaller
error, on max and on rms; every pair is printed (`pose-orders |` rows).

Measured, worst spread max / rms per kind of tensor, on two CPUs (the yardstick is fp32 arithmetic of the CPU at hand: its
convolution kernels differ with the instruction set, and before the thread count was pinned also with the number of threads;
every such evaluation is a valid fp32 order, so X covers the worst of all of them):
                                 passes        encoders      poses         losses
  8-core x86 host, 1 thread      1.83 / 1.89   1.66 / 1.46   1.39 / 1.39   2.36 / 2.03
  8-core x86 host, 8 threads     1.83 / 1.89   1.59 / 1.46   1.46 / 1.25   2.26 / 1.88
  MI355X host's CPU, 1 thread    1.79 / 1.79   1.32 / 1.46   1.62 / 1.31   2.09 / 1.96
  MI355X host's CPU, 16 threads  1.79 / 1.79   1.32 / 1.46   1.62 / 1.28   2.68 / 1.67
(the rows at 8 and 16 threads: before the pin, benign chains)
Asserted: X = the worst rounded up to the next half: passes 2, encoders 2, poses 2, losses 3 (pose_ref.X); the GPU margin is
2 X.  A loss tensor has 15 elements (6 in the long chains), which is why its max moves most.  A tensor whose max-spread needs
more than 3 has too few elements for its max to be stable; its row count goes up, X does not: single passes and encoders run on
45 rows (9 rows gave spreads above 2), and the trained-scale chains on B = 37 windows (their poses reach 100 .. 670 through the
condition embedding of a trained-scale encoder, and at B = 5 / B = 13 the max-spread of 'trained_inject_3+3' was 3.20 / 3.06)."""
import pytest
import torch

import pose_ref as R
from oracle import mocodad_oracle as O

PASSES, CONDS = R.PASS_CASES, R.COND_CASES
# max |pose| of a benign chain: the windows are clamped to +-3, x_T ~ N(0,1) over up to 5 x 3 x 2 x 32 x 17 draws (|z| < 5), and the
# chain's last step divides by sqrt(alpha_1) ~ 1: measured 2.1 .. 7.4 at ns 10, 1.4 .. 2.3 at ns 50.  A model whose random
# eps-prediction blows the chain up tests the schedule, not the kernel.
BENIGN_POSE_BOUND = 16.0
# 'concat' with the condition at the END is the exception, by the algorithm and with any weights: the prediction is read at the
# corrupt frames' original indices, where the U-Net's input holds condition frames (oracle reverse_diffusion, "reproduced as
# is"), so it does not track x, nothing cancels in x - c pred, and x grows by 1 / sqrt(alpha_t) per step: the schedule's gain
# (1 / sqrt(alpha_9) = 31.6 at ns 10), as in the latent chains.  Measured 1.1e3 .. 8.2e3; the gates are relative to it.
SHIFTED_POSE_RANGE = (100.0, 2e4)


def report(case, what, kind, ref64, cpu32):
    assert ref64.dtype == torch.float64 and torch.isfinite(ref64).all(), (case, what)
    for o in R.ORDERS:
        assert cpu32[o].dtype == torch.float32 and torch.isfinite(cpu32[o]).all(), (case, what, o)
    e = {o: R.errors(cpu32[o], ref64) for o in R.ORDERS}
    smax, srms = R.spread(ref64, cpu32)
    print(f"pose-orders | {case:22s} | {what:16s} | max|ref64| {e['bn'][2]:9.3e} | bn max {e['bn'][0]:9.3e} rms {e['bn'][1]:9.3e} | "
          f"folded max {e['folded'][0]:9.3e} rms {e['folded'][1]:9.3e} | spread max {smax:5.2f} rms {srms:5.2f}")
    # fp32 through at most 11 layers on values of O(10): an evaluation order further off than this is not fp32
    assert max(e[o][0] for o in R.ORDERS) <= 2e-5 * max(1.0, e["bn"][2]), (case, what, e)
    assert smax <= R.X[kind] and srms <= R.X[kind], (case, what, kind, smax, srms, R.X[kind])


@pytest.mark.parametrize("kind,t", PASSES, ids=[f"{k}-{t}" for k, t in PASSES])
def test_single_pass(kind, t):
    r = R.pass_reference(kind, t)
    assert tuple(r["x"].shape) == (R.ROWS, 2, t, 17) and R.ROWS % 4 != 0 and R.ROWS % 2 == 1
    assert (r["cond"] is not None) == (kind == "inject")
    for step, (ref, cpu) in r["out"].items():
        assert tuple(ref.shape) == (R.ROWS, 2, t, 17)
        report(f"{kind} T={t}", f"eps t={step}", "pass", ref, cpu)


@pytest.mark.parametrize("arch,t,scale", CONDS, ids=[f"{a}-{t}-{s}" for a, t, s in CONDS])
def test_condition_encoder(arch, t, scale):
    r = R.cond_reference(arch, t, scale)
    ref, cpu = r["out"]
    assert tuple(r["x"].shape) == (R.ROWS, 2, t, 17) and tuple(ref.shape) == (R.ROWS, 16)
    report(f"{arch} Tc={t} {scale}", "cond_emb", "cond", ref, cpu)


@pytest.mark.parametrize("name", list(R.CHAINS))
def test_chain(name):
    c = R.CHAINS[name]
    r = R.chain_reference(name)
    tu, tc = R.chain_frames(name)
    m, _ = R.chain_model(name)
    assert m.input_n_frames == tu and (m.n_frames_condition if c["strategy"] == "inject" else 0) == tc
    ref, cpu = r["poses"]
    assert tuple(ref.shape) == (c["B"], c["S"], 2, m.n_frames_corrupt, 17)
    if c["ns"] == R.NS:
        assert (c["B"] * c["S"]) % 4 == 3       # the short chains: an odd number, 3 mod 4
    if c["scale"] == "benign":
        shifted = c["strategy"] == "concat" and c["ci"][0] != 0
        lo, hi = SHIFTED_POSE_RANGE if shifted else (1.0, BENIGN_POSE_BOUND)
        assert lo < ref.abs().max() < hi, ref.abs().max()
    report(name, "poses", "pose", ref, cpu)
    assert list(r["loss"]) == list(c["losses"])
    for fn, (lref, lcpu) in r["loss"].items():
        assert tuple(lref.shape) == (c["B"], c["S"]) and lref.min() > 0
        report(name, f"loss {fn}", "loss", lref, lcpu)
    if c["sets"] is not None:
        assert all(len(s) == c["ci"] for s in c["sets"]) and (c["seg_len"] < 32 or any(31 in s for s in c["sets"]))


def test_contexts_leave_the_oracle_as_it_was():
    """oracle_dtype and folded_conv_bn patch the oracle module other test modules import: the originals are back on exit, also
    after an exception, and the oracle's default behaviour is the one of its source."""
    pe, cb = O.pos_encoding, O._conv_bn
    t = torch.full((3, 1), 4.0)
    with R.oracle_dtype(torch.float64):
        assert O.pos_encoding(t, 16).dtype == torch.float64
        assert torch.equal(O.pos_encoding(t, 16), pe(t, 16).double())      # the fp32 table's values, not a float64 sinusoid
        with R.folded_conv_bn():
            assert O._conv_bn is R.conv_bn_folded
        assert O._conv_bn is cb
    assert O.pos_encoding is pe and O._conv_bn is cb
    with pytest.raises(RuntimeError):
        with R.evaluation(torch.float64, "folded"):
            raise RuntimeError("inside")
    assert O.pos_encoding is pe and O._conv_bn is cb and O.pos_encoding(t, 16).dtype == torch.float32
    with R.folded_conv_bn(False):
        assert O._conv_bn is cb


def test_frame_counts_cover_the_kernel_tables():
    """Every frame count that has a kernel of its own appears in a parametrisation of the GPU module.  The counts below restate
    the rows of csrc/mcd_instances.hpp (non-LT): a row added there is added here, and then to pose_ref's lists."""
    import test_pose_fp64_gpu as G
    score_kernel = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]                   # MCD_SCORE_INSTANCES
    tiled = {16: range(13, 17), 24: range(17, 25), 32: range(25, 33)}        # MCD_TILED_INSTANCES: padded size -> frame counts
    cond_fast = list(range(1, 21))                                           # MCD_COND_FAST_INSTANCES
    cond_unet = list(range(1, 13))                                           # MCD_COND_UNET_INSTANCES
    # MCD_TILED_COND_INSTANCES: both ends of each padded size that a scoring call can reach (n_cond < seg_len <= 32); these
    # encoders have no entry of their own, they run in the enc_* chains
    tiled_cond = {16: (13, 16), 24: (17, 24), 32: (25, 31)}
    passes = {t for k, t in G.PASSES if k == "none"}
    assert set(score_kernel) <= passes
    for tp, frames in tiled.items():
        assert set(frames) <= passes, tp
    assert passes == set(range(1, 33))
    assert set(cond_fast) <= {t for a, t, s in G.CONDS if a == "AE" and s == "benign"}
    unet = {t for a, t, s in G.CONDS if a == "E_unet" and s == "benign"}
    assert set(cond_unet) <= unet
    enc = {R.chain_frames(n)[1] for n in G.CHAINS if R.CHAINS[n]["arch"] == "E_unet" and R.CHAINS[n]["scale"] == "benign"}
    for tp, ends in tiled_cond.items():
        assert set(ends) <= enc, tp
    plain_scratch = {R.chain_frames(n)[1] for n in G.CHAINS if R.CHAINS[n]["arch"] == "AE"}
    assert {25, 31} <= plain_scratch and {21, 24} <= {t for a, t, s in G.CONDS if a == "AE"}      # the plain encoder, both buffer modes
    # whole chains: each kernel family, and the frame counts the issue names
    chain_tu = {R.chain_frames(n)[0] for n in G.CHAINS}
    assert {1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 17, 20, 24, 32} <= chain_tu
    assert any(o.get("generic_unet") for n in G.CHAINS for o in G.options_of(n))
    assert all({0, 1} <= {o["split"] for o in G.options_of(n)} for n in G.CHAINS)

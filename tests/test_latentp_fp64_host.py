"""CPU: the float64 reference and the fp32 yardstick that tests/test_latentp_gpu.py::test_rows_vs_fp64 measures the latent
autoencoder's launches against -- [condition encoder] -> encode -> [project] -> unproject -> decode -- on exactly the models and
inputs of that test (latentp_ref.FP64_CASES).  Nothing here runs a kernel: these tests say that each reference is float64, finite
and of the stated shape, that each fp32 evaluation is fp32 (within 2e-5 max(1, max|ref64|) of it), that the yardstick is a property
of fp32 and not of the order it happens to be evaluated in, that the cases reach every row of the three latent instance tables and
every legal latent size, and that the gate built on all this fires on a fault of the size it is there for.

Two fp32 evaluation orders against float64, as in tests/test_pose_fp64_host.py: 'bn' (conv, then F.batch_norm) and 'folded'
(BatchNorm folded into the conv first), both on one CPU thread.  Spread = larger error / smaller error, on max and on rms; every
pair is printed (`pose-orders |` rows).  z0 has a third evaluation, to_time_dim as latent_ref.linear_k_chain (one sequential chain
over K = 640 t): it is part of z0's yardstick (printed as `k-chain`), not of the spread.

Measured, worst spread max / rms per kind of tensor over the 28 cases, each on 45 windows:
                                 cond_emb      z0            pose          loss
  x86 build host, 1 thread       1.44 / 1.25   1.49 / 1.08   1.54 / 1.25   2.05 / 1.49
  MI355X host's CPU, 1 thread    1.70 / 1.30   1.33 / 1.18   1.40 / 1.21   1.76 / 1.50
(the worst cases: cond_emb '6+6 D32 E_unet' on both; loss '6+1 D32' on the first, '6+6 D32 E_unet' on the second)
Asserted: X = the worst rounded up to the next half: cond_emb 2, z0 1.5, pose 2, loss 2.5 (latentp_ref.X); the GPU margin is
2 X.  No entry may exceed pose_ref.X (2, 2, 2, 3): a case that needs more has too few elements for its max to be stable, and its
window count goes up (77, then 109: odd), X does not.  At 45 windows no case needs it: a loss tensor has 45 elements (the 5 of the
earlier single case gave a loss spread of 2.73 at 5 + 3 frames, and made the factor fail on the MI355X host's CPU).

The instrument (test_the_sharp_gate_fires, case '6+3 D48'): the fp32 restatement with one element of model.to_time_dim.bias moved
by 1e-5 passes the hard 1e-4 gate on all four tensors and misses the sharp one on z0 (error 1.0e-5, 8.0 x the yardstick of 1.3e-6;
pose and loss move by less than their own fp32 error: one latent of 48 off by 1e-5 is not visible behind the decoder); with the
PReLU slope of model.st_gcnnsd1.0 (a layer of the down path) moved by 1e-3 relative it passes the hard gate (pose error 1.9e-4 of
max|ref| 5.2: 3.6e-5 relative) and misses the sharp one on pose (344 x the yardstick), loss (82 x) and z0 (3.7 x).  Neither
needed a larger perturbation than the one first tried."""
import pytest
import torch

import latentp_ref as R
import pose_ref as P

CASES = list(R.FP64_CASES)


@pytest.mark.parametrize("name", CASES)
def test_case(name):
    s = R.FP64_CASES[name]
    c = R.fp64_case(name)
    B, t, tc, D = s["B"], s["t"], s["tc"], s["D"]
    assert B % 2 == 1 and B > 32 and B % 32 != 0      # odd; one full 32-row tile and a partial one
    assert tuple(c["data"].shape) == (B, 2, t + tc, 17) and len(c["xi"]) == t and len(c["ci"]) == tc
    assert (c["z"] is None) == (s["z"] is None) and (c["z"] is None or tuple(c["z"].shape) == (B, D))
    shapes, over = ((B, 16), (B, D), (B, 2, t, 17), (B,)), []
    for i, what, kind in R.compared(name):
        ref, cpu = c["ref"][i], {o: c["out"][o][i] for o in P.ORDERS}
        assert ref.dtype == torch.float64 and torch.isfinite(ref).all() and tuple(ref.shape) == shapes[i], (name, what)
        yard = R.yard_of(c, i)
        assert len(yard) == (3 if what == "z0" else 2), (name, what)
        e = {o: P.errors(v, ref) for o, v in yard.items()}
        for o, v in yard.items():
            assert v.dtype == torch.float32 and torch.isfinite(v).all(), (name, what, o)
            assert e[o][0] <= 2e-5 * max(1.0, e[o][2]), (name, what, o, e[o])
        smax, srms = P.spread(ref, cpu)
        print(f"pose-orders | {name:22s} | {what:16s} | max|ref64| {e['bn'][2]:9.3e} | bn max {e['bn'][0]:9.3e} rms {e['bn'][1]:9.3e} | "
              f"folded max {e['folded'][0]:9.3e} rms {e['folded'][1]:9.3e} | spread max {smax:5.2f} rms {srms:5.2f}"
              + (f" | k-chain max {e['k_chain'][0]:9.3e} rms {e['k_chain'][1]:9.3e}" if "k_chain" in e else ""))
        if not (smax <= R.X[kind] and srms <= R.X[kind]):
            over.append((name, what, kind, smax, srms, R.X[kind]))
    assert not over, over      # (after every row of the case is printed)
    assert c["ref"][3].min() > 0


def test_factors_stay_inside_the_pose_model_s():
    assert set(R.X) == set(R.KINDS)
    assert R.X["cond"] <= P.X["cond"] and R.X["z0"] <= P.X["cond"] and R.X["pose"] <= P.X["pose"] and R.X["loss"] <= P.X["loss"]
    assert all(2 * x == int(2 * x) for x in R.X.values())      # halves


def test_cases_cover_the_kernel_tables():
    """Every corrupt frame count with a row in one of the three latent instance tables, and every latent size the packer takes,
    appears among the cases.  The counts below restate the rows of mocodad_amd/csrc/mcd_instances.hpp: a row added there is added
    here, and then to latentp_ref.FP64_CASES."""
    encode = [3, 3, 5, 12, 6, 11, 7, 10, 8, 9]                      # MCD_LATENT_ENCODE_INSTANCES (3 frames: condition in and out of the kernel)
    decode = [3, 5, 6, 7, 8, 9, 10, 11, 12]                         # MCD_LATENT_DECODE_INSTANCES
    decode_samples = [3, 5, 6, 7, 8, 9, 10, 11, 12]                 # MCD_LATENT_DECODE_SAMPLES_INSTANCES
    assert len(encode) + len(decode) + len(decode_samples) == 28
    own = {s["t"] for s in R.FP64_CASES.values() if s["z"] is None and s["weights"] is None}
    assert set(encode) | set(decode) | set(decode_samples) <= own and set(R.FRAME_COUNTS) == own
    assert {s["D"] for s in R.FP64_CASES.values()} == set(range(16, 129, 16)) == set(R.LATENT_DIMS)
    # the condition lengths and encoders in front of the encode launch, the decode launch alone, every loss function
    conds = {(s["arch"], s["tc"]) for s in R.FP64_CASES.values() if s["t"] == 6}
    assert {("AE", 1), ("AE", 3), ("AE", 12), ("E_unet", 6), ("E", P.COND_E_CASE[0])} <= conds
    assert {(s["t"], s["z"]) for s in R.FP64_CASES.values() if s["z"] is not None} == {(t, g) for t in (3, 7, 12) for g in (1.0, R.Z_GAIN)}
    assert {s["loss_fn"] for s in R.FP64_CASES.values()} == {"smooth_l1", "l1", "mse"}
    assert {s["weights"] for s in R.FP64_CASES.values()} == {None, "P6_hostile", "P24_hostile"}


def _sharp_misses(c, got):
    """R.gated on each of the four tensors -> the names of those that miss the sharp gate; a miss of the hard gate propagates"""
    missed = []
    for i, what, kind in R.compared("6+3 D48"):
        try:
            R.gated("fires", "6+3 D48", what, kind, got[i], c["ref"][i], R.yard_of(c, i))
        except AssertionError as e:
            assert len(e.args[0]) == 6 and e.args[0][2] in ("max", "rms"), e      # the sharp gate's tuple, not the hard gate's
            missed.append(what)
    return missed


@pytest.mark.parametrize("fault", ["bias", "slope"])
def test_the_sharp_gate_fires(fault):
    """A dropped-term sized fault in the restatement's own weights: invisible to the hard 1e-4 gate, caught by err <= 2 X yard."""
    c = R.fp64_case("6+3 D48")
    sd = dict(c["sd"])
    if fault == "bias":
        k, delta = "model.to_time_dim.bias", torch.zeros_like(sd["model.to_time_dim.bias"])
        delta[5] = 1e-5
    else:
        k = "model.st_gcnnsd1.0.prelu.weight"
        delta = 1e-3 * sd[k]
    sd[k] = sd[k] + delta
    with P.evaluation(torch.float32), P.one_thread():
        got = R.reconstruct(sd, c["data"], c["ci"], c["xi"])
    with P.evaluation(torch.float32), P.one_thread():      # the instrument is silent on the unperturbed restatement
        assert _sharp_misses(c, R.reconstruct(c["sd"], c["data"], c["ci"], c["xi"])) == []
    missed = _sharp_misses(c, got)
    print(f"latentp-fires | {fault} | sharp gate missed on {missed}")
    # measured ratios to the yardstick, max / rms: bias -> z0 8.0 / 6.1 (gate 3); slope -> pose 344 / 308 (gate 4), loss 82 / 90 (gate 5)
    assert set({"bias": ["z0"], "slope": ["pose", "loss"]}[fault]) <= set(missed) and "cond_emb" not in missed, missed

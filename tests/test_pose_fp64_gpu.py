"""GPU: every trajectory kernel and condition encoder of the pose model against the oracle in float64, gated by the error fp32
itself shows on the same inputs (tests/pose_ref.py; tests/test_pose_fp64_host.py states the yardstick's side).

  passes   HipScorer.unet_forward at every frame count 1 .. 32 ('no_condition': each score_kernel row, the slab-tiled kernel at
           both ends of each padded size and between), at t = 1, 5, 9 of 10 steps, on 45 rows (odd: the last workgroup is
           partial at 4 and at 2 chains per workgroup); with a condition embedding at 3, 6, 12, 24 frames; trained-scale weights
           at 3, 7, 12, 16, 32.  Rows 0, 23 | 24 (a workgroup boundary at 1, 2 and 4 chains per workgroup) and 44, each from a
           one-row call, equal the batch call bit for bit: a window changes no bit of any other however the batch is cut.
  chains   parity mode with the caller's draws, ns 10, S 3, B 5 (15 chains: odd, 3 mod 4), poses and per-sample losses, each
           case with `split` 0 and 1, the concat cases at 6 and 13 frames also on the runtime-shape kernel ('generic_unet');
           l1 and mse on one case per kernel family; ns 50, S 2, B 3 at 3, 12 and 24 corrupt frames; trained-scale weights (B 37:
           at fewer chains the max error of these ill-conditioned chains is not a stable figure, pose_ref.CHAINS).
  encoders HipScorer.cond_encode on 45 rows: 'AE' at 1 .. 20 condition frames (cond_fast_kernel) and at 21 and 24 (the plain
           encoder), 'E_unet' at 1 .. 12 (cond_unet_kernel), one 'E' with a runtime channel list; trained-scale weights at 3, 12,
           16.  mcd_cond_encode takes no workspace and answers MCD_EUNSUPPORTED for the encoders that need global scratch, so
           those are measured where the library runs them, in a scoring call (the enc_* chains: one corrupt frame behind the
           condition): 'E_unet' at 13, 16, 17, 24, 25, 31 condition frames (the COND form of the slab-tiled kernel, both ends of
           each padded size; 32 cannot occur in a call, n_cond < seg_len <= 32) and 'AE' at 25 and 31.

Gates, the same for every compared tensor.  Hard, the project's: |gpu - ref64| <= 1e-4 max(1, max|ref64|).  Sharp, on max and on
rms: err_gpu <= 2 X yard, yard = the larger of the errors of the two fp32 CPU evaluation orders against float64, X = the factor
those orders stay within of each other (pose_ref.X: passes 2, encoders 2, poses 2, losses 3).  Every compared figure is printed
(`pose-fp64 |` rows; the recorded run is profiles/pose_kernels_fp64.txt).

Found (MI355X, 351 rows): no kernel misses a gate, none was changed, and no third evaluation order was needed.  Worst ratio to
the yardstick, max / rms: passes 1.49 / 1.70 (gate 4), encoders 2.20 / 1.64 (gate 4), poses 1.81 / 1.09 (gate 4), losses 2.18 /
2.04 (gate 6); worst error relative to max(1, max|ref64|) 2.2e-6 (trained-scale poses of 100), 9.4e-7 otherwise.  `split` 0 and 1
give the same error figures in every case.  The yardstick itself depends on the CPU that evaluates it (the ratios above are against the
CPU of the MI355X host), which is why X is taken over every CPU configuration seen (tests/test_pose_fp64_host.py).
Run time: the module alone 41 s for 121 of its 133 cases on one MI355X with 16 CPU threads, most of it the CPU references (shared
with the host test's within a session); the slowest case (ns 50 at 24 frames) 2.5 s."""
import functools

import pytest
import torch

import pose_ref as R

pytestmark = pytest.mark.gpu

PASSES, CONDS = R.PASS_CASES, R.COND_CASES
CHAINS = list(R.CHAINS)
DEVICE = "cuda:0"
BOUNDARY_ROWS = (0, 23, 24, R.ROWS - 1)


def options_of(name):
    """The hip_options a chain case runs under."""
    return [{"split": 0}, {"split": 1}] + ([{"split": 0, "generic_unet": 1}] if R.CHAINS[name]["generic"] else [])


@functools.lru_cache(maxsize=None)
def _scorer(build, *key):
    return build(*key)[0].build_scorer(torch.device(DEVICE))


@pytest.mark.parametrize("kind,t", PASSES, ids=[f"{k}-{t}" for k, t in PASSES])
def test_single_pass_vs_fp64(kind, t):
    sc = _scorer(R.pass_model, kind, t)
    r = R.pass_reference(kind, t)
    x, cond = r["x"], r["cond"]
    for step, (ref, cpu) in r["out"].items():
        eps = sc.unet_forward(x, step, cond, noise_steps=R.NS)
        R.gated("pass", f"{kind} T={t}", f"eps t={step}", "pass", eps, ref, cpu)
        for row in BOUNDARY_ROWS:
            one = sc.unet_forward(x[row:row + 1], step, None if cond is None else cond[row:row + 1], noise_steps=R.NS)
            assert torch.equal(one, eps[row:row + 1]), (kind, t, step, row)


@pytest.mark.parametrize("arch,t,scale", CONDS, ids=[f"{a}-{t}-{s}" for a, t, s in CONDS])
def test_condition_encoder_vs_fp64(arch, t, scale):
    sc = _scorer(R.cond_model, arch, t, scale)
    r = R.cond_reference(arch, t, scale)
    ref, cpu = r["out"]
    R.gated("cond", f"{arch} Tc={t} {scale}", "cond_emb", "cond", sc.cond_encode(r["x"]), ref, cpu)


@pytest.mark.parametrize("name", CHAINS)
def test_chain_vs_fp64(name):
    c = R.CHAINS[name]
    r = R.chain_reference(name)
    sc = _scorer(R.chain_model, name)
    try:
        for opt in options_of(name):
            for k in ("split", "generic_unet"):
                sc.set_option(k, opt.get(k, 0))
            tag = f"{name} s{opt['split']}" + (" gen" if opt.get("generic_unet") else "")
            for i, fn in enumerate(c["losses"]):
                loss, poses = sc.score(r["data"], n_samples=c["S"], noise_steps=c["ns"], noise=r["noise"], loss_fn=fn, want_poses=True,
                                       cond_mask=r["mask"])
                if i == 0:
                    R.gated("chain", tag, "poses", "pose", poses, *r["poses"])
                    first = poses.clone()
                else:
                    assert torch.equal(poses, first), (tag, fn)       # the loss function does not touch the chain
                R.gated("chain", tag, f"loss {fn}", "loss", loss, *r["loss"][fn])
    finally:
        sc.set_option("split", 0)
        sc.set_option("generic_unet", 0)

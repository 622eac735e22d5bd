"""GPU: 'random_imp' with the frame sets drawn on the device (mcd_random_imp_masks, random_imp_draw='device') and the
mean_pose / median_pose aggregations with per-window frame sets (mcd_aggregate_view).
The kernel's masks are held to the NumPy restatement (tests/rndimp_ref.py) bit for bit; scores and poses to the oracle within
the project's gate, |got - ref| <= 1e-4 * max(1, max|ref|)."""
import ctypes

import numpy as np
import pytest
import torch

import rndimp_ref as R
from conftest import load_golden
from helpers import golden_weights, make_args

pytestmark = pytest.mark.gpu
ATOL = 1e-4
DEV = "cuda:0"


def _gate(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = ATOL * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(f"{what}: max|got-ref| = {err:.3e}, gate {tol:.3e}")
    np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg=what)


def _batch(data):
    B, T = data.shape[0], data.shape[2]
    return [data, torch.zeros(B), torch.zeros(B, 4), torch.zeros(B, T)]


# ---------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("T,k", [(2, 1), (6, 2), (6, 3), (7, 6), (32, 5), (32, 31)])
def test_masks_equal_the_restatement_bit_for_bit(T, k):
    from mocodad_amd import _lib
    L = _lib.lib()
    n = 1000            # four workgroups, the last one partly filled
    for seed in (999, 0xDEADBEEF12345678):
        for first in (0, 2 ** 32 - 3):
            out = torch.full((n + 8,), 0x55AA55AA, device=DEV, dtype=torch.int32)       # (8 guard words behind the masks)
            _lib.check(L.mcd_random_imp_masks(ctypes.c_uint64(seed), ctypes.c_int64(first), n, T, k, ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            got = out.cpu().numpy()
            assert np.array_equal(got[:n], R.masks(seed, first, n, T, k)), (T, k, seed, first)
            assert (got[n:] == 0x55AA55AA).all(), "wrote behind n_windows"


# ---------------------------------------------------------------- the module: replay, oracle, batch cuts
@pytest.fixture(scope="module")
def rndimp():
    from mocodad_amd.models.mocodad import MoCoDAD
    sd, cfg = golden_weights("rndimp")
    mk = lambda **over: MoCoDAD(make_args(cfg, noise_steps=4, n_generated_samples=2, seed=4242, **over)).to(DEV)
    dev, host = mk(random_imp_draw="device"), mk()
    dev.load_state_dict(sd)
    host.load_state_dict(sd)
    data = torch.randn(10, 2, 6, 17, generator=torch.Generator().manual_seed(606)).clamp_(-3, 3)
    return dev, host, sd, data


def test_device_draw_replays_from_the_exported_masks_and_matches_the_oracle(rndimp):
    from oracle import mocodad_oracle as O
    m, host, sd, data = rndimp
    B, S, ns, off = 10, 2, 4, 1234
    live = m.forward(_batch(data), aggr_strategy="all", return_="all", window_offset=off)
    masks = m.random_imp_masks(B, off)
    assert masks.dtype == torch.int32 and masks.shape == (B,) and masks.is_cuda
    assert np.array_equal(masks.cpu().numpy(), R.masks(m.seed, off, B, 6, 2))
    assert len(set(masks.tolist())) > 1                  # (per-window sets, not one set for the batch)
    replay = m.forward(_batch(data), aggr_strategy="all", return_="all", window_offset=off, cond_mask=masks)
    assert torch.equal(live[0], replay[0]) and torch.equal(live[1], replay[1])
    # an explicit cond_mask always wins, and the host module scores the same sets the same way
    other = host.forward(_batch(data), aggr_strategy="all", return_="all", window_offset=off, cond_mask=masks.cpu())
    assert torch.equal(live[0], other[0])
    # the oracle, fed with the exported masks and the exported noise
    noise = m.scorer().philox_noise(B, n_samples=S, noise_steps=ns, seed=m.seed, first_window_id=off)
    explicit = m.forward(_batch(data), aggr_strategy="all", return_="all", noise=noise, cond_mask=masks)
    assert torch.equal(live[0], explicit[0])
    with torch.no_grad():
        poses, corrupt = O.reverse_diffusion(sd, data, noise.cpu(), noise_steps=ns, strategy="random_imp", conditioning_indices=2,
                                             cond_mask=masks.cpu())
        loss = O.window_losses(poses, corrupt)
    _gate(live[0].cpu(), loss.t(), "loss (B,S)")
    _gate(live[1].cpu(), poses.transpose(0, 1), "poses (B,S,C,Tx,V)")
    # the fused, loss-only call draws the same sets
    best = m.forward(_batch(data), aggr_strategy="best", return_="loss", window_offset=off)[0]
    _gate(best.cpu(), loss.min(0)[0], "fused best loss")


def test_masks_and_losses_do_not_depend_on_how_windows_are_cut_into_batches(rndimp):
    m, _, _, data = rndimp
    whole = m.forward(_batch(data), aggr_strategy="all", return_="loss", window_offset=0)[0]
    lo = m.forward(_batch(data[:5]), aggr_strategy="all", return_="loss", window_offset=0)[0]
    hi = m.forward(_batch(data[5:]), aggr_strategy="all", return_="loss", window_offset=5)[0]
    assert torch.equal(torch.cat([lo, hi]), whole)
    assert torch.equal(torch.cat([m.random_imp_masks(5, 0), m.random_imp_masks(5, 5)]), m.random_imp_masks(10, 0))
    # without window_offset the module counts the windows itself, as for the noise
    m._calls = 0
    a = m.forward(_batch(data[:5]), aggr_strategy="all", return_="loss")[0]
    b = m.forward(_batch(data[5:]), aggr_strategy="all", return_="loss")[0]
    assert torch.equal(torch.cat([a, b]), whole)


def test_host_draw_is_still_the_default(rndimp):
    _, host, _, data = rndimp
    g = load_golden("traj_rndimp_ns4_S2.npz")
    assert host.random_imp_draw == "host"
    noise = torch.from_numpy(g["noise"].astype(np.float32))
    torch.manual_seed(int(g["rng_seed"][0]))
    out = host.forward(_batch(torch.from_numpy(g["data"])), aggr_strategy="all", return_="loss", noise=noise)
    _gate(out[0].cpu(), g["loss_all"], "host draw, fixture losses")


# ---------------------------------------------------------------- mean_pose / median_pose with per-window frame sets
@pytest.fixture(scope="module")
def pose_cases():
    """(module, state dict, data, cond_mask, k, noise (3, ns-1, B, C, Tx, V)) per case; the oracle's chains are run once per case
    for the three samples and shared by the S = 1, 2, 3 tests (a chain depends on its own noise only)."""
    from mocodad_amd.models.mocodad import MoCoDAD
    from oracle import mocodad_oracle as O
    cases = {}
    # the reference-generated fixture with its own frame sets (its noise holds two samples: a third is drawn here)
    sd, cfg = golden_weights("rndimp")
    g = load_golden("traj_rndimp_ns4_S2.npz")
    m = MoCoDAD(make_args(cfg, noise_steps=4)).to(DEV)
    m.load_state_dict(sd)
    noise = torch.from_numpy(g["noise"].astype(np.float32))
    extra = torch.randn(1, *noise.shape[1:], generator=torch.Generator().manual_seed(77))
    cases["fixture"] = [m, sd, torch.from_numpy(g["data"]), torch.from_numpy(g["cond_mask"]), 2, 4, torch.cat([noise, extra])]
    # 32 frames, 5 of them conditioning, frame 31 among them: the slab-tiled kernel, bit 31 of the mask
    _, cfg = golden_weights("inject")
    torch.manual_seed(31)
    m = MoCoDAD(make_args(cfg, conditioning_strategy="random_imp", seg_len=32, conditioning_indices=5, noise_steps=3, n_generated_samples=2))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    gen = torch.Generator().manual_seed(3131)
    data = torch.randn(3, 2, 32, 17, generator=gen).clamp_(-3, 3)
    noise = torch.randn(3, 2, 3, 2, m.n_frames_corrupt, 17, generator=gen)
    sets = [[31, 0, 7, 16, 30], [3, 5, 12, 13, 14], [1, 2, 4, 8, 31]]
    mask64 = torch.tensor([sum(1 << f for f in fs) for fs in sets], dtype=torch.int64)
    mask = torch.where(mask64 >= 2 ** 31, mask64 - 2 ** 32, mask64).to(torch.int32)
    assert (mask < 0).any() and (mask > 0).any()
    cases["T32"] = [m, sd, data, mask, 5, 3, noise]
    for c in cases.values():
        m, sd, data, mask, k, ns, noise = c
        with torch.no_grad():
            poses, corrupt = O.reverse_diffusion(sd, data, noise, noise_steps=ns, strategy="random_imp", conditioning_indices=k, cond_mask=mask)
        c += [poses, corrupt]
    return cases


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("aggr", ["mean_pose", "median_pose"])
@pytest.mark.parametrize("case", ["fixture", "T32"])
def test_pose_aggregations_under_random_imp_vs_oracle(pose_cases, case, aggr, S):
    from oracle import mocodad_oracle as O
    m, sd, data, mask, k, ns, noise, poses, corrupt = pose_cases[case]
    m.n_generated_samples = S
    out = m.forward(_batch(data), aggr_strategy=aggr, return_="all", noise=noise[:S], cond_mask=mask)
    sel, loss = O.aggregate(poses[:S], corrupt, aggr)
    assert out[1].shape == sel.shape == (data.shape[0], 2, data.shape[2] - k, 17)
    _gate(out[0].cpu(), loss, f"{case} {aggr} S={S} loss")
    _gate(out[1].cpu(), sel, f"{case} {aggr} S={S} pose")


def test_pose_aggregations_with_device_drawn_masks(rndimp):
    """the mask the module drew itself reaches the aggregation: equal to the replay with the exported masks"""
    m, _, _, data = rndimp
    for aggr in ("mean_pose", "median_pose"):
        live = m.forward(_batch(data), aggr_strategy=aggr, return_="all", window_offset=40)
        replay = m.forward(_batch(data), aggr_strategy=aggr, return_="all", window_offset=40, cond_mask=m.random_imp_masks(10, 40))
        assert torch.equal(live[0], replay[0]) and torch.equal(live[1], replay[1])
        assert torch.isfinite(live[0]).all()


# ---------------------------------------------------------------- mcd_aggregate is what it was
@pytest.mark.parametrize("aggr", ["best", "median", "mean_pose", "median_pose"])
def test_aggregate_and_aggregate_view_without_a_mask_are_bit_identical(aggr):
    from mocodad_amd import _lib
    L = _lib.lib()
    g = load_golden("traj_inject_ns10_S5.npz")
    loss_all = torch.from_numpy(g["loss_all"]).to(DEV).contiguous()
    poses = torch.from_numpy(g["poses_all"]).to(DEV).contiguous()
    data = torch.from_numpy(g["data"]).to(DEV).contiguous()
    B, S = loss_all.shape
    cfg = _lib.ScoreCfg(n_windows=B, n_samples=S, noise_steps=10, seg_len=6, n_cond=3, n_corrupt=3, loss_fn=_lib.LOSS["smooth_l1"])
    for i in range(3):
        cfg.cond_idx[i], cfg.corrupt_idx[i] = i, 3 + i
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    no_mask = _lib.WindowView(base=None, stride_c=0, stride_t=0, trans=None, affine=None, cond_mask=None)
    for view in ("plain", None, no_mask):
        la = torch.full((B,), float("nan"), device=DEV)
        pa = torch.full((B, 2, 3, 17), float("nan"), device=DEV)
        head = (ctypes.byref(cfg), 2, 17, _lib.AGGR[aggr], ctypes.c_float(0.0), p(loss_all), p(poses), p(data))
        if view == "plain":
            _lib.check(L.mcd_aggregate(*head, p(la), p(pa), st))
        else:
            _lib.check(L.mcd_aggregate_view(*head, ctypes.byref(view) if view is not None else None, p(la), p(pa), st))
        outs.append((la.cpu(), None if aggr == "median" else pa.cpu()))
    for la, pa in outs[1:]:
        assert torch.equal(la, outs[0][0])
        if pa is not None:
            assert torch.equal(pa, outs[0][1])
    # ... and what the reference computed
    _gate(outs[0][0], g[f"loss_{aggr}"], f"{aggr} loss vs the reference's")
    if f"pose_{aggr}" in g:
        _gate(outs[0][1], g[f"pose_{aggr}"], f"{aggr} pose vs the reference's")

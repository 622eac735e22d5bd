"""GPU: the error maps through the module surface -- MoCoDAD.forward(..., return_maps=True) -- on the shipped 3 + 3 'inject'
configuration, one 'concat' and one 'random_imp' configuration, B = 5 windows, S = 5 samples, ns = 3, with given noise.

Consistency: |mean_{t,v} M[b] - loss_agg[b]| <= 2 (C Tx V + 16) 2^-24 loss_agg[b] -- both sides are sums over the same C Tx V
per-element losses of the same fp32 poses and ground truth, in different orders: the worst case of two such summations (+ the
aggregation's few operations), not a measured figure.
Parity: against the CPU oracle on the same noise, the maps formed in float64 from the ORACLE's generated poses with the selection
made on the oracle's losses (tests/maps_ref.py); the project's tolerance, 1e-4 relative to max(1, |ref|)."""
import numpy as np
import pytest
import torch

from helpers import golden_weights, make_args
from maps_ref import reference_maps

pytestmark = pytest.mark.gpu
B, S, NS = 5, 5, 3
AGGRS = ("best", "worst", "mean", "median", "mean_pose", "median_pose", "quantile:0.3", "all")
VARIANTS = ("inject", "concat", "rndimp")
MASKS = [0b000011, 0b010100, 0b100001, 0b001010, 0b110000]        # rndimp: two condition frames per window, mostly not the head


def _model(variant, **over):
    from mocodad_amd.models.mocodad import MoCoDAD
    sd, cfg = golden_weights(variant)
    m = MoCoDAD(make_args(cfg, **over)).to("cuda:0")
    m.load_state_dict(sd)
    return m, sd, cfg


_CACHE = {}


def case(variant):
    """Module, batch, noise, masks and the oracle's (poses (S,B,C,Tx,V), ground truth (B,C,Tx,V), losses (B,S)) -- once per variant."""
    if variant not in _CACHE:
        from oracle import mocodad_oracle as O
        m, sd, cfg = _model(variant, noise_steps=NS, n_generated_samples=S, model_return_value="loss", aggregation_strategy="best")
        T, Tx = cfg["seg_len"], m.n_frames_corrupt
        gen = torch.Generator().manual_seed(41)
        data = torch.randn(B, 2, T, 17, generator=gen)
        noise = torch.randn(S, NS - 1, B, 2, Tx, 17, generator=gen)
        mask = torch.tensor(MASKS, dtype=torch.int32) if variant == "rndimp" else None
        batch = [data, torch.zeros(B), torch.zeros(B, 4), torch.zeros(B, T)]
        with torch.no_grad():
            poses, gt = O.reverse_diffusion(sd, data, noise, noise_steps=NS, strategy=cfg["conditioning_strategy"],
                                            conditioning_indices=cfg["conditioning_indices"], cond_mask=MASKS if mask is not None else None)
            losses = O.window_losses(poses, gt, "smooth_l1").t().contiguous()
        _CACHE[variant] = (m, batch, noise, mask, poses.transpose(0, 1).contiguous().numpy(), gt.numpy(), losses.numpy())
    return _CACHE[variant]


def forward(m, batch, noise, mask, aggr, ret="all", maps=True):
    kw = dict(cond_mask=mask) if mask is not None else {}
    if maps:
        kw["return_maps"] = True
    return m.forward(batch, aggr_strategy=aggr, return_=ret, noise=noise, **kw)


@pytest.mark.parametrize("variant", VARIANTS)
def test_maps_mean_is_the_window_loss(variant):
    m, batch, noise, mask, *_ = case(variant)
    Tx = m.n_frames_corrupt
    lim = 2 * (2 * Tx * 17 + 16) * 2.0 ** -24
    for aggr in AGGRS:
        for ret in ("loss", "all"):          # (loss-only: the fused call; all: mcd_score + mcd_aggregate)
            out = forward(m, batch, noise, mask, aggr, ret)
            loss, maps, frames = out[0].cpu().numpy().astype(np.float64), out[-2].cpu().numpy().astype(np.float64), out[-1].cpu().numpy()
            assert maps.shape == ((B, S, Tx, 17) if aggr == "all" else (B, Tx, 17)) and frames.shape == (B, Tx)
            assert np.isfinite(maps).all() and (maps >= 0).all()
            mean = maps.mean(axis=(-2, -1))
            rel = np.abs(mean - loss) / loss
            print(f"{variant} {aggr} ({ret}): largest |mean M - loss| / loss = {rel.max():.3e} (bound {lim:.3e})")
            assert (rel <= lim).all(), (variant, aggr, ret, rel.max(), lim)


@pytest.mark.parametrize("variant", VARIANTS)
def test_map_frames(variant):
    m, batch, noise, mask, *_ = case(variant)
    frames = forward(m, batch, noise, mask, "best", "loss")[-1].cpu().numpy()
    if variant == "rndimp":
        assert frames.tolist() == [[t for t in range(6) if not (k >> t) & 1] for k in MASKS]
    else:
        assert frames.tolist() == [[3, 4, 5]] * B


@pytest.mark.parametrize("variant", VARIANTS)
def test_maps_against_the_oracle(variant):
    m, batch, noise, mask, poses, gt, losses = case(variant)
    for aggr in AGGRS:
        got = forward(m, batch, noise, mask, aggr, "loss")[-2].cpu().numpy().astype(np.float64)
        pagg = None
        if aggr.endswith("_pose"):            # the oracle's own aggregate pose
            p = torch.from_numpy(poses)
            pagg = (p.mean(1) if aggr == "mean_pose" else p.median(1)[0]).numpy()
        ref = reference_maps(losses, poses, gt, "smooth_l1", aggr, pagg)
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        print(f"{variant} {aggr}: largest |map - oracle| / max(1, |ref|) = {err.max():.3e}")
        assert err.max() <= 1e-4, (variant, aggr, err.max())


@pytest.mark.parametrize("variant", VARIANTS)
def test_return_maps_off_is_todays_list(variant):
    m, batch, noise, mask, *_ = case(variant)
    for aggr in ("best", "mean_pose", "all"):
        for ret in ("loss", "all"):
            off = forward(m, batch, noise, mask, aggr, ret, maps=False)
            on = forward(m, batch, noise, mask, aggr, ret)
            assert len(off) == (5 if ret == "loss" else 6) and len(on) == len(off) + 2
            for a, b in zip(off, on[:-2]):
                assert (a is None and b is None) or (a is b) or torch.equal(a.to("cuda:0"), b.to("cuda:0"))
    kw = dict(cond_mask=mask) if mask is not None else {}
    with pytest.raises(TypeError):
        m.forward(batch, "best", "loss", noise, None, None, True)          # keyword only
    with pytest.raises(ValueError, match="random"):
        m.forward(batch, aggr_strategy="random", return_="all", noise=noise, return_maps=True, **kw)


def test_slab_tiled_route():
    """24 U-Net frames ('concat', 12 + 12): the slab-tiled kernel's poses, the same maps launch."""
    from oracle import mocodad_oracle as O
    m, sd, cfg = _model("cat24", noise_steps=NS, n_generated_samples=2, model_return_value="loss", aggregation_strategy="best")
    assert m.scorer().plan_split(2, 2, NS) == 0            # not score_kernel: the slab-tiled route
    T, Tx = cfg["seg_len"], m.n_frames_corrupt
    gen = torch.Generator().manual_seed(43)
    data = torch.randn(2, 2, T, 17, generator=gen)
    noise = torch.randn(2, NS - 1, 2, 2, Tx, 17, generator=gen)
    batch = [data, torch.zeros(2), torch.zeros(2, 4), torch.zeros(2, T)]
    with torch.no_grad():
        poses, gt = O.reverse_diffusion(sd, data, noise, noise_steps=NS, strategy="concat", conditioning_indices=cfg["conditioning_indices"])
        losses = O.window_losses(poses, gt, "smooth_l1").t().contiguous().numpy()
    lim = 2 * (2 * Tx * 17 + 16) * 2.0 ** -24
    for aggr in ("best", "mean", "all"):
        out = m.forward(batch, aggr_strategy=aggr, return_="loss", noise=noise, return_maps=True)
        loss, maps = out[0].cpu().numpy().astype(np.float64), out[-2].cpu().numpy().astype(np.float64)
        assert out[-1].tolist() == [list(range(T - Tx, T))] * 2
        assert (np.abs(maps.mean(axis=(-2, -1)) - loss) / loss <= lim).all(), aggr
        ref = reference_maps(losses, poses.transpose(0, 1).contiguous().numpy(), gt.numpy(), "smooth_l1", aggr)
        assert (np.abs(maps - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-4, aggr


def test_maps_do_not_depend_on_the_route():
    """MCD_OPT_SPLIT = S (one trajectory per workgroup, encoder and aggregation as launches of their own) against the window-major
    single launch: the maps are a function of pose_out, loss_all and the windows alone -- bit-identical whenever those are."""
    m, batch, noise, mask, *_ = case("inject")
    sc = m.scorer()
    res = {}
    for split in (1, S):
        sc.set_option("split", split)
        try:
            assert sc.plan_split(B, S, NS) == split
            res[split] = sc.score_fused(batch[0], n_samples=S, noise_steps=NS, aggregation="best", noise=noise, want_all=True,
                                        want_poses=True, want_maps=True)
        finally:
            sc.set_option("split", 0)
    (a_agg, a_loss, a_pose, a_maps), (b_agg, b_loss, b_pose, b_maps) = res[1], res[S]
    same = torch.equal(a_pose, b_pose) and torch.equal(a_loss, b_loss)
    print(f"poses and losses bit-identical between the routes: {same}")
    if same:
        assert torch.equal(a_maps, b_maps)
    else:       # routes that round differently: the maps follow the poses within the parity tolerance
        assert ((a_maps - b_maps).abs() / b_maps.abs().clamp_min(1.0)).max().item() <= 1e-4
    # and the maps of a call are those of the entry alone on what the call returned
    assert torch.equal(a_maps, sc.error_maps(batch[0], a_loss, a_pose, "best"))
    assert torch.equal(b_maps, sc.error_maps(batch[0], b_loss, b_pose, "best"))


def test_dataset_joint_scores_rows(tmp_path):
    """utils.eval_utils.joint_score_rows (eval_MoCoDAD.py --joint-scores): the maps averaged over the transforms and scatter-maxed
    per (scene, clip, person) -- against np.maximum.at on the same maps; a frame no window forecasts stays 0.  (The synthetic
    dataset is person-major, not transform-major: the windows are matched by their meta rows.)"""
    from mocodad_amd.data import synthetic
    from mocodad_amd.utils.eval_utils import joint_score_rows
    nt = 2
    data, trans, meta, frames, gts = synthetic.make_dataset(n_clips=2, frames_per_clip=30, persons_per_clip=2, num_transform=nt)
    m, _, _ = _model("inject", noise_steps=NS, n_generated_samples=2, model_return_value="loss", aggregation_strategy="best", num_transform=nt)
    out = m.forward([data, trans, meta, frames], return_maps=True, window_offset=0)
    maps, mf = out[-2], out[-1]
    fids = torch.gather(frames.to(mf.device).long(), 1, mf).cpu().numpy()
    js, rows = joint_score_rows(maps, trans.numpy(), meta.numpy(), fids, gts, nt, m.scorer().joint_scatter_max)
    keys = [tuple(int(v) for v in r) for r in rows]
    mt = [tuple(int(v) for v in r) for r in meta.numpy()]
    assert keys == sorted({k[:3] for k in mt}) and js.shape == (len(keys), max(len(g) for g in gts.values()), 17)
    ref = np.zeros_like(js)
    at = {(k, int(t)): i for i, (k, t) in enumerate(zip(mt, trans.numpy()))}
    for k in sorted(set(mt)):
        i0, i1 = at[(k, 0)], at[(k, 1)]
        mean = torch.stack([maps[i0], maps[i1]]).mean(0).cpu().numpy()
        for r in range(3):
            cell = ref[keys.index(k[:3]), fids[i0, r] - 1]
            np.maximum(cell, np.fmax(mean[r], np.float32(0)), out=cell)
    assert np.array_equal(js.view(np.int32), ref.view(np.int32)) and (js > 0).any() and (js == 0).any()
    with pytest.raises(ValueError, match="every transform"):
        joint_score_rows(maps[:-1], trans.numpy()[:-1], meta.numpy()[:-1], fids[:-1], gts, nt, m.scorer().joint_scatter_max)

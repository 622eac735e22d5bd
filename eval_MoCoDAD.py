#!/usr/bin/env python3
"""eval_MoCoDAD.py — Trainer-free counterpart of the reference's eval_MoCoDAD.py (same `-c config.yaml` interface,
same YAML keys) running the MI355X path.

  python eval_MoCoDAD.py -c config.yaml                       # dataset + checkpoint from the YAML paths
  python eval_MoCoDAD.py -c config.yaml --synthetic 8         # 8 synthetic clips (no dataset files needed)
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 eval_MoCoDAD.py -c cfg.yaml --synthetic 64

With more than one process the window index range is sharded contiguously over the ranks (one GPU each) and the
per-window scores are reassembled by a single RCCL all-gather before the (rank-0) AUC computation."""
import argparse
import os
import sys
import tempfile
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC for RCCL across processes (see bench.py); before HIP loads

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from mocodad_amd.data import synthetic  # noqa: E402
from mocodad_amd.data.trajectories import check_supported, load_dataset  # noqa: E402
from mocodad_amd.models.mocodad import MoCoDAD  # noqa: E402
from mocodad_amd.parallel import WindowShard  # noqa: E402
from mocodad_amd.utils.argparser import load_config  # noqa: E402


def model_class(args):
    """MoCoDADlatent when the YAML says `diffusion_on_latent: true` (the reference's eval_MoCoDAD.py:45-46) -- its pretrain stage,
    MoCoDADlatentPretrain, with `stage: 'pretrain'` -- else MoCoDAD."""
    if getattr(args, "diffusion_on_latent", False):
        if getattr(args, "stage", "diffusion") == "pretrain":
            from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
            return MoCoDADlatentPretrain
        from mocodad_amd.models.mocodad_latent import MoCoDADlatent
        return MoCoDADlatent
    return MoCoDAD


def load_latent_decoder(model, args, random_init: bool) -> None:
    """latent_score_space 'pose': the stage-1 decoder from pretrained_model_ckpt_path; with --random-init and no such file, from a
    seeded MoCoDADlatentPretrain whose shared tensors (down path, to_time_dim, condition encoder) are copied from the diffusion module."""
    path = getattr(args, "pretrained_model_ckpt_path", None)
    if path and os.path.exists(path):
        model.load_decoder(path)
        return
    if not random_init:
        raise SystemExit(f"stage-1 checkpoint {path} not found: latent_score_space 'pose' decodes with it (pass --random-init to decode "
                         "with seeded random-init weights)")
    import copy
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    a = copy.copy(args)
    a.stage = "pretrain"
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(getattr(args, "seed", 0)) + 1)
        sd = MoCoDADlatentPretrain(a).state_dict()
    sd.update({k: v.detach().cpu() for k, v in model.state_dict().items() if k in sd})
    model.load_decoder(sd)


def main():
    ap = argparse.ArgumentParser(description="MoCoDAD (MI355X)")
    ap.add_argument("-c", "--config", type=str, required=True)
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate on N synthetic clips instead of dataset files")
    ap.add_argument("--frames-per-clip", type=int, default=200)
    ap.add_argument("--device-windows", action="store_true",
                    help="upload per-person trajectories once and let the kernels window + transform them on load "
                         "(instead of materialising seg_len x num_transform copies on the host)")
    ap.add_argument("--device-masks", action="store_true",
                    help="'random_imp' only: draw the per-window condition-frame sets on the device from (seed, window id) "
                         "(random_imp_draw: device) instead of one torch.randperm per window on the host")
    ap.add_argument("--random-init", action="store_true", help="score with seeded random-init weights when the checkpoint "
                    "is missing (otherwise a missing checkpoint is an error)")
    ap.add_argument("--dist-backend", default="nccl", help="'nccl' (= RCCL over xGMI) or 'gloo' (tests with several ranks on one GPU)")
    ap.add_argument("--dump-scores", type=str, default=None, help="rank 0 writes the gathered window scores + AUC to this .npz")
    ap.add_argument("--joint-scores", type=str, default=None, metavar="OUT.npz",
                    help="pose model, or the latent model scoring in pose space; one process: also write, per (scene, clip, person) row, the (n_frames, 17) per-joint frame "
                         "scores -- the scatter-max of the windows' error maps (which joints and forecast frames a score comes "
                         "from), averaged over the transforms -- with the row table and the joint names")
    ap.add_argument("--forecast-tracks", type=str, default=None, metavar="OUT.npz",
                    help="pose model, or the latent model scoring in pose space; one process: also write, per trajectory row (tracked "
                         "person and video frame), the expected pose -- the forecasts of the windows covering the row collapsed into "
                         "one, in image pixels next to the observed row -- with how many windows forecast it and how much they disagree")
    ap.add_argument("--forecast-method", choices=("unique", "mean", "median"), default="median",
                    help="--forecast-tracks: the pose of a row from its covering windows (extract_single_pose's `method`)")
    ap.add_argument("--forecast-spread", choices=("mean", "median"), default="mean",
                    help="--forecast-tracks: how the 34 per-feature standard deviations become one spread (its `std_method`)")
    ap.add_argument("--forecast-transforms", choices=("identity", "all"), default="identity",
                    help="--forecast-tracks / --forecast-fan: which windows forecast a row -- those of transform 0 only, or those of every test-time "
                         "transform, each forecast mapped back through the inverse of its transform (more forecasts per row: larger "
                         "counts, nothing else changes in the output)")
    ap.add_argument("--forecast-fan", type=str, default=None, metavar="OUT.npz",
                    help="pose model, or the latent model scoring in pose space; one process: also write, per trajectory row, the "
                         "distribution of ALL generated futures covering the row (every sample of every covering window) -- quantile "
                         "bands in image pixels and in normalised coordinates, mean, standard deviation, and where the observed "
                         "coordinate falls among them (mid-rank in [0, 1]); works with every aggregation strategy but 'random'")
    ap.add_argument("--forecast-levels", type=str, default="0.1,0.5,0.9", metavar="Q,Q,...",
                    help="--forecast-fan: 1 .. 8 quantile levels in [0, 1], strictly ascending")
    ap.add_argument("--latent-score-space", choices=("latent", "pose"), default=None,
                    help="latent model, stage 'diffusion' (overrides the YAML's latent_score_space): 'pose' decodes the generated "
                         "latents with the stage-1 decoder of pretrained_model_ckpt_path and scores the forecasts as the pose model does")
    cli = ap.parse_args()
    args = load_config(cli.config)
    model_cls = model_class(args)
    if cli.latent_score_space is not None:
        args.latent_score_space = cli.latent_score_space
    pose_space = getattr(model_cls, "is_latent", False) and not getattr(model_cls, "is_pretrain", False) \
        and getattr(args, "latent_score_space", None) == "pose"
    if cli.joint_scores:
        if model_cls is not MoCoDAD and not pose_space:
            raise SystemExit("eval_MoCoDAD.py: --joint-scores needs the pose model, or the latent model with latent_score_space: 'pose' "
                             "(a latent has no joints)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("eval_MoCoDAD.py: --joint-scores runs in one process (the maps are not gathered across ranks)")
        if getattr(args, "aggregation_strategy", "best") in ("all", "random") or "random" in str(args.conditioning_strategy):
            raise SystemExit("eval_MoCoDAD.py: --joint-scores needs one map per window with the same forecast frames under every "
                             "transform: not aggregation_strategy all / random, not the random_imp strategy")
    if cli.forecast_tracks and cli.forecast_fan:
        raise SystemExit("eval_MoCoDAD.py: --forecast-tracks and --forecast-fan are separate runs")
    if cli.forecast_tracks:      # (refusals by name, before any GPU call)
        aggr = str(getattr(args, "aggregation_strategy", "best"))
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("eval_MoCoDAD.py: --forecast-tracks runs in one process (the forecasts are not gathered across ranks)")
        if model_cls is not MoCoDAD and not pose_space:
            raise SystemExit("eval_MoCoDAD.py: --forecast-tracks needs the pose model, or the latent model with latent_score_space: 'pose' "
                             "(in latent space the model forecasts a latent code, not a pose)")
        if aggr in ("mean", "median") or "quantile" in aggr:
            raise SystemExit(f"eval_MoCoDAD.py: --forecast-tracks needs an aggregation that selects a pose (best, worst, mean_pose, "
                             f"median_pose): aggregation_strategy {aggr!r} aggregates losses and selects none")
        if aggr in ("all", "random"):
            raise SystemExit(f"eval_MoCoDAD.py: --forecast-tracks needs one forecast per window: not aggregation_strategy {aggr!r}")
        if cli.joint_scores:
            raise SystemExit("eval_MoCoDAD.py: --forecast-tracks and --joint-scores are separate runs")
        forecast_cover = 32
        if cli.forecast_transforms == "all":      # the forecasts a row can collect: per transform one per forecast frame of a window
            from types import SimpleNamespace
            from mocodad_amd.utils.eval_utils import forecast_max_cover
            split = SimpleNamespace(n_frames=args.seg_len, conditioning_indices=args.conditioning_indices,
                                    conditioning_strategy=MoCoDAD.conditioning_strategies.get(args.conditioning_strategy, args.conditioning_strategy))
            per_window = args.seg_len if split.conditioning_strategy == "random_imp" else len(MoCoDAD._frame_split(split)[1])
            try:
                forecast_cover = forecast_max_cover(args.num_transform, per_window, "all")
            except ValueError as e:
                raise SystemExit(f"eval_MoCoDAD.py: --forecast-transforms all: {e}") from None
    elif cli.forecast_fan:      # (refusals by name, before any GPU call)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("eval_MoCoDAD.py: --forecast-fan runs in one process (the forecasts are not gathered across ranks)")
        if model_cls is not MoCoDAD and not pose_space:
            raise SystemExit("eval_MoCoDAD.py: --forecast-fan needs the pose model, or the latent model with latent_score_space: 'pose' "
                             "(in latent space the model forecasts a latent code, not a pose)")
        if cli.joint_scores:
            raise SystemExit("eval_MoCoDAD.py: --forecast-fan and --joint-scores are separate runs")
        if str(getattr(args, "aggregation_strategy", "best")) == "random":
            raise SystemExit("eval_MoCoDAD.py: --forecast-fan: not aggregation_strategy 'random' (it keeps no record of the sample it drew)")
        from types import SimpleNamespace
        from mocodad_amd.engine import forecast_levels
        from mocodad_amd.utils.eval_utils import forecast_fan_cover, forecast_max_cover
        try:
            fan_levels = forecast_levels([float(q) for q in cli.forecast_levels.split(",") if q.strip()], "--forecast-levels")
            split = SimpleNamespace(n_frames=args.seg_len, conditioning_indices=args.conditioning_indices,
                                    conditioning_strategy=MoCoDAD.conditioning_strategies.get(args.conditioning_strategy, args.conditioning_strategy))
            per_window = args.seg_len if split.conditioning_strategy == "random_imp" else len(MoCoDAD._frame_split(split)[1])
            forecast_cover = forecast_fan_cover(args.n_generated_samples, forecast_max_cover(args.num_transform, per_window, cli.forecast_transforms))
        except ValueError as e:
            raise SystemExit(f"eval_MoCoDAD.py: --forecast-fan: {e}") from None
    elif cli.forecast_transforms != "identity":
        raise SystemExit("eval_MoCoDAD.py: --forecast-transforms goes with --forecast-tracks or --forecast-fan")
    pretrain = bool(getattr(model_cls, "is_pretrain", False))
    if pretrain and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("eval_MoCoDAD.py: stage 'pretrain' runs in one process (its result is one mean over all windows, not gathered scores)")
    if cli.device_masks:
        args.random_imp_draw = "device"
    if not cli.synthetic:
        try:
            check_supported(args)        # (before any GPU call)
        except ValueError as e:
            raise SystemExit(f"eval_MoCoDAD.py: {e}") from None

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    # ranks on THIS node (torchrun exports LOCAL_WORLD_SIZE; a multi-node job has world > ndev with one GPU per rank)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if local_world > ndev and cli.dist_backend == "nccl":
        # RCCL refuses two ranks on one GPU (and would otherwise hang in its bootstrap)
        raise SystemExit(f"eval_MoCoDAD.py: {local_world} ranks on this node but {ndev} GPU(s) visible; the nccl backend needs one "
                         "rank per GPU (--dist-backend gloo is for tests that share a GPU)")
    local = local % ndev   # (several ranks per GPU only in the 1-GPU tests, with --dist-backend gloo)
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    use_dist = world > 1 or "LOCAL_RANK" in os.environ     # under torch.distributed.run: RCCL path even with one rank
    if use_dist:
        import torch.distributed as dist
        if cli.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(cli.dist_backend)

    tw = None
    if cli.synthetic and cli.device_windows:
        from mocodad_amd.data.windows import TrajectoryWindows
        trajs, gts = synthetic.make_trajectories(n_clips=cli.synthetic, frames_per_clip=cli.frames_per_clip, seed=args.seed)
        tw = TrajectoryWindows(trajs, args.seg_len, args.num_transform).to(dev)
        data, trans, meta, frames = tw, tw.trans.long(), tw.meta, tw.frames
        gt_dir = tempfile.mkdtemp(prefix="mocodad_gt_")
        synthetic.write_gt(gt_dir, gts)
        args.gt_path = gt_dir
    elif cli.synthetic:
        data, trans, meta, frames, gts = synthetic.make_dataset(n_clips=cli.synthetic, frames_per_clip=cli.frames_per_clip,
                                                                seg_len=args.seg_len, num_transform=args.num_transform,
                                                                seed=args.seed)
        gt_dir = tempfile.mkdtemp(prefix="mocodad_gt_")
        synthetic.write_gt(gt_dir, gts)
        args.gt_path = gt_dir
    else:
        # the dataset of the YAML paths: CSVs parsed on the host, normalised into the trajectory buffer on the device
        tw, load_t = load_dataset(args, dev)
        data, trans, meta, frames = tw, tw.trans.long(), tw.meta, tw.frames
        if rank == 0:
            print(f"dataset: {tw.n_samples} windows x {tw.num_transform} transforms from {args.data_dir}  load: parse "
                  f"{load_t['parse']:.3f}s  upload+normalise {load_t['normalise']:.3f}s")

    torch.manual_seed(int(getattr(args, "seed", 0)))      # without a checkpoint every rank must draw the same weights
    model = model_cls(args).to(dev)
    if cli.synthetic:
        model.dataset_name = "synthetic"      # synthetic clips have their own lengths: no HR-Avenue / UBnormal frame masks
    ckpt = os.path.join(args.ckpt_dir, args.load_ckpt)
    if os.path.exists(ckpt):
        model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"])
    elif not cli.random_init:
        raise SystemExit(f"checkpoint {ckpt} not found (pass --random-init to score with seeded random-init weights)")
    if pose_space:
        load_latent_decoder(model, args, cli.random_init)

    n = len(tw) if tw is not None else data.shape[0]
    shard = WindowShard(n, rank, world)
    if use_dist and not pretrain:
        shard.host_meta = (trans.numpy(), meta.numpy(), frames.numpy())
        model.shard = shard
    model.save_tensors = False
    import sklearn.metrics  # noqa: F401  (imported here, not inside the timed region: ~0.3 s on first use)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    model.on_test_epoch_start()
    with torch.no_grad():
        batches = tw.batches(args.batch_size, shard.lo, shard.hi) if tw is not None else \
            synthetic.batches((data, trans, meta, frames), args.batch_size, shard.lo, shard.hi)
        maps, map_frames = [], []
        forecasts, forecast_frames = [], []
        for i, batch in enumerate(batches):
            model._calls = shard.lo + i * args.batch_size     # global window id keys the noise stream
            if cli.forecast_tracks:   # test_step with the selected forecast of the batch's windows beside its output
                n_b, kw = int(batch[1].shape[0]), {}
                if model.conditioning_strategy == "random_imp":      # the frame sets forward would draw, drawn here: they say which frames a window forecasts
                    kw["cond_mask"] = model.random_imp_masks(n_b, model._calls) if model.random_imp_draw == "device" \
                        else model.draw_random_imp_mask(n_b)
                out = model.forward(batch, return_="all", **kw)
                model._test_output_list.append(out[:1] + out[2:])
                forecasts.append(out[1])
                forecast_frames.append(model.map_frames(kw.get("cond_mask"), n_b))
            elif cli.forecast_fan:      # test_step with EVERY sample of the batch's windows beside its output
                n_b, kw = int(batch[1].shape[0]), {}
                if model.conditioning_strategy == "random_imp":      # drawn here, as for --forecast-tracks
                    kw["cond_mask"] = model.random_imp_masks(n_b, model._calls) if model.random_imp_draw == "device" \
                        else model.draw_random_imp_mask(n_b)
                out = model.forward(batch, return_samples=True, **kw)
                model._test_output_list.append(out[:-2])
                forecasts.append(out[-2])
                forecast_frames.append(out[-1])
            elif cli.joint_scores:      # test_step with the error maps of the batch's windows beside its output
                out = model.forward(batch, return_maps=True)
                model._test_output_list.append(out[:-2])
                maps.append(out[-2])
                map_frames.append(torch.gather(batch[3].to(dev).long(), 1, out[-1]))      # frame ids of the map rows
            else:
                model.test_step(batch, i)
    ev1.record()                             # (no synchronisation here: the epoch end's host work runs under the queued batches)
    auc = model.on_test_epoch_end()          # gather of the scores + frame-score assembly (device) + roc_auc_score (host)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    t1 = t0 + ev0.elapsed_time(ev1) * 1e-3   # the scoring loop alone: device time from the first launch to the last batch's end
    if rank == 0:
        # end to end (test_step loop + gather + frame-score assembly + AUC) beside the scoring loop alone (the kernels)
        print(f"windows: {n}  gpus: {world}  time: {dt:.3f}s  ({n / dt:.0f} clips/s end to end; scoring loop {t1 - t0:.3f}s = {n / (t1 - t0):.0f} clips/s "
              f"+ epoch end {dt - (t1 - t0):.3f}s)  batch: {args.batch_size}  noise_steps: {args.noise_steps}  samples: {args.n_generated_samples}  "
              + (f"pretrain_rec_loss: {auc:.6f}" if pretrain else f"AUC: {auc:.6f}"))
        if cli.dump_scores:
            import numpy as np
            np.savez(cli.dump_scores, scores=model.last_scores, auc=np.float64(auc))
        if cli.joint_scores:
            import numpy as np
            from mocodad_amd._lib import JOINT_NAMES
            from mocodad_amd.utils.eval_utils import joint_score_rows
            gts, _ = model._gt_and_masks()
            js, rows = joint_score_rows(torch.cat(maps), trans.numpy(), meta.numpy(), torch.cat(map_frames).cpu().numpy(), gts,
                                        args.num_transform, model.scorer().joint_scatter_max)
            np.savez(cli.joint_scores, joint_scores=js, rows=rows, row_columns=np.asarray(["scene", "clip", "person"]),
                     joint_names=np.asarray(JOINT_NAMES))
            print(f"joint scores: {js.shape[0]} (scene, clip, person) rows x {js.shape[1]} frames x {js.shape[2]} joints -> {cli.joint_scores}")
        if cli.forecast_tracks:
            import numpy as np
            from mocodad_amd._lib import JOINT_NAMES
            from mocodad_amd.engine import denormalize_poses, forecast_assemble
            from mocodad_amd.utils.eval_utils import forecast_track_rows
            t2 = time.perf_counter()
            src = dict(windows=tw) if tw is not None else dict(meta=meta.numpy(), frames=frames.numpy())
            pose, count, spread, rows, frame_ids = forecast_track_rows(
                torch.cat(forecasts), trans.numpy(), torch.cat(forecast_frames).cpu().numpy(), forecast_assemble,
                method=cli.forecast_method, spread_method=cli.forecast_spread, max_cover=forecast_cover,
                transforms=cli.forecast_transforms, num_transform=args.num_transform, **src)
            res = dict(rows=rows, row_columns=np.asarray(["scene", "clip", "person"]), frames=frame_ids,
                       expected_norm=pose.cpu().numpy(), count=count.cpu().numpy(), spread=spread.cpu().numpy(),
                       joint_names=np.asarray(JOINT_NAMES), method=np.asarray(cli.forecast_method), spread_method=np.asarray(cli.forecast_spread))
            if getattr(tw, "raw", None) is not None:      # a dataset: row r of the buffer is CSV row r, back to its pixels
                res["observed"] = tw.raw.poses
                res["expected"] = denormalize_poses(pose, tw.raw.poses, tw.vid_res, *tw.scaler, count=count).cpu().numpy()
            np.savez(cli.forecast_tracks, **res)
            print(f"forecast tracks: {len(rows)} trajectory rows, {int((res['count'] > 0).sum())} with a forecast ({cli.forecast_method}, spread "
                  f"{cli.forecast_spread}) -> {cli.forecast_tracks}  {time.perf_counter() - t2:.3f}s"
                  + ("" if "expected" in res else "  (synthetic clips have no pixel rows: expected_norm only, no observed / expected)"))
        if cli.forecast_fan:
            import numpy as np
            from mocodad_amd._lib import JOINT_NAMES
            from mocodad_amd.engine import denormalize_poses, forecast_fan
            from mocodad_amd.utils.eval_utils import forecast_fan_rows, forecast_observed_rows
            t2 = time.perf_counter()
            src = dict(windows=tw) if tw is not None else dict(meta=meta.numpy(), frames=frames.numpy(), data=data)
            poses_all = torch.cat(forecasts)
            quant, mean, std, rank, count, rows, frame_ids = forecast_fan_rows(
                poses_all, trans.numpy(), torch.cat(forecast_frames).cpu().numpy(), forecast_fan, levels=fan_levels,
                max_cover=forecast_cover, transforms=cli.forecast_transforms, num_transform=args.num_transform, **src)
            observed = forecast_observed_rows(trans.numpy(), **src)      # (R,2,17) as the fan was given them
            obs_norm = observed.reshape(len(rows), 2, 17).transpose(1, 2).reshape(len(rows), 34).cpu().numpy()      # interleaved x1,y1,...
            res = dict(rows=rows, row_columns=np.asarray(["scene", "clip", "person"]), frames=frame_ids, levels=np.asarray(fan_levels),
                       observed_norm=obs_norm, bands_norm=quant.cpu().numpy(), mean_norm=mean.cpu().numpy(), std_norm=std.cpu().numpy(),
                       rank=rank.cpu().numpy(), count=count.cpu().numpy(), n_samples=np.int64(poses_all.shape[1]),
                       joint_names=np.asarray(JOINT_NAMES))
            if getattr(tw, "raw", None) is not None:      # a dataset: row r of the buffer is CSV row r, each level back to its pixels
                res["observed"] = tw.raw.poses
                res["bands"] = np.stack([denormalize_poses(quant[l], tw.raw.poses, tw.vid_res, *tw.scaler, count=count).cpu().numpy()
                                         for l in range(len(fan_levels))])
            np.savez(cli.forecast_fan, **res)
            has = res["count"] > 0
            lo, hi, ob = res["bands_norm"][0][has], res["bands_norm"][-1][has], obs_norm[has]
            outside = ((ob < lo) | (ob > hi)).any(axis=1)
            print(f"forecast fan: {len(rows)} trajectory rows, {int(has.sum())} with a forecast, "
                  f"{100.0 * float(outside.mean()) if len(outside) else 0.0:.1f}% of those with a coordinate outside "
                  f"[{fan_levels[0]:g}, {fan_levels[-1]:g}]; {poses_all.shape[1]} samples per window, "
                  f"{poses_all.numel() * poses_all.element_size()} device bytes held for poses_all -> {cli.forecast_fan}  "
                  f"{time.perf_counter() - t2:.3f}s"
                  + ("" if "bands" in res else "  (synthetic clips have no pixel rows: the _norm outputs only, no observed / bands)"))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Replay recorded pose tracks through a PoseStream (mocodad_amd/stream.py) as a live feed and time the ticks.

    python tools/stream_replay.py -c configs/hr_avenue_test.yaml --random-init               # the split of the YAML paths
    python tools/stream_replay.py -c configs/hr_avenue_test.yaml --random-init --data-dir tests/golden/dataset \\
           --dataset-choice HR-STC --no-scaler                                                # the test fixture
    python tools/stream_replay.py -c configs/hr_avenue_test.yaml --random-init --synthetic-tracks 256 --rows 120
    python tools/stream_replay.py -c configs/ubnormal_latent_test.yaml --random-init --synthetic-tracks 64    # the latent model
    python tools/stream_replay.py -c configs/hr_avenue_test.yaml --random-init --synthetic-tracks 64 --ticks-per-call 8
    python tools/stream_replay.py -c configs/ubnormal_latent_test.yaml --random-init --synthetic-tracks 64 \\
           --latent-score-space pose --joint-scores --forecasts                               # the latent model in pose space

On-disk split: the trajectory CSVs are replayed in frame order, one tick = one frame id across all clips; a track is closed
after its last row.  The window scores, put back into dataset order, go through the model's own post_processing: the AUC is
printed.  --synthetic-tracks N: N tracks that all receive a row on every tick (no AUC) -- the load of N tracked people.

Timing (host clock around work that ends in a device synchronise, one warm-up replay, then --reps replays):
  tick      PoseStream.push of one tick (a launch group of one): host table + one H2D copy + mcd_stream_push_group + the scoring
            call + mcd_stream_frame_scores_group
  baseline  ONE score_fused call (a YAML with diffusion_on_latent: true: ONE LatentScorer.score call) on a pre-built WindowBatch of the tick's window count over a trajectory buffer already on the
            device (what a caller of the dataset path would pay for the same windows if the buffer and the window list cost
            nothing), timed the same way in the same process, alternating with the stream replay.
--ticks-per-call K (default 1 = the path above through `push`): K ticks per PoseStream.push_many call, ring_len = seg_len + K - 1
unless --ring-len says otherwise (then a call may be cut into several launch groups); tracks are closed after the call that held
their last row.  "tick" is then one CALL (K ticks: one copy, one mcd_stream_push_group, ONE scoring call on the windows of all K
ticks, one mcd_stream_frame_scores_group per group), the baseline ONE scoring call on a pre-built batch of the call's window count,
and rows_per_s = pose rows pushed / time in push or push_many over a whole replay (every call, also those without a window).
--clip-scores [--sigma S]: the online per-clip frame scores (PoseStream(clip_scores=...)) ride in every tick, so
"tick" includes mcd_stream_clip_update + mcd_stream_clip_emit; every clip is ended with close_clip after the last call (not timed).
On an on-disk split the AUC of the ONLINE scores against the ground-truth masks is printed next to the offline AUC (frames of the
masks without an emitted score are excluded and counted).  The two differ by definition -- online, a frame's persons are those
with a score at that frame, not the clip's whole roster, and neither pad_size nor the HR masks are applied -- so neither is
asserted against the other.
--joint-scores: per-joint frame scores in every tick (PoseStream(joint_scores=True)): "tick" then includes the error
maps launch behind the scoring call and mcd_stream_joint_scores_group; the pose model, or a latent config in pose space.
--forecasts [--forecast-method M] [--forecast-spread S]: the expected pose of every row in every tick (PoseStream(forecasts=
ForecastCfg(M, S))): "tick" then includes the scoring call writing its per-sample losses and poses and the two launches
of mcd_stream_forecast_group (closes: mcd_stream_forecast_flush); a best / worst aggregation only; the pose model, or a latent config
in pose space.  --forecast-transforms all: the windows of every transform forecast a row, each mapped back through the inverse of
its transform (ForecastCfg(M, S, 'all'): mcd_stream_forecast_group_tta, one store wave per window of every transform).
--latent-score-space pose (a latent config): the stage-1 decoder is loaded as eval_MoCoDAD.py loads it (--random-init: a seeded one
sharing the module's frozen tensors), the tick's scoring call is LatentPoseScorer.score (mcd_latent_score_pose: + the unproject,
decode, aggregate and maps launches), and the baseline is that call alone, asked for the same outputs.
--forecasts-out OUT.npz: the rows of the warm-up replay in the layout of eval_MoCoDAD.py --forecast-tracks (rows, frames, observed,
expected, expected_norm, count, spread, joint_names), sorted by (scene, clip, person, frame); not timed.
Prints one JSON line and writes it to --out (default profiles/stream_replay.json): median and p99 over all timed ticks that
emitted windows, the range of the per-replay medians (the spread), and the same for the baseline."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mocodad_amd.data import trajectories as T  # noqa: E402
from mocodad_amd.data.windows import TrajectoryWindows, WindowBatch  # noqa: E402
from mocodad_amd.engine import normalize_poses  # noqa: E402
from mocodad_amd.models.mocodad import MoCoDAD  # noqa: E402
from mocodad_amd.models.mocodad_latent import MoCoDADlatent  # noqa: E402
from mocodad_amd.stream import ClipScoreCfg, ForecastCfg, PoseStream, ticks_by_frame  # noqa: E402
from mocodad_amd.utils.argparser import load_config  # noqa: E402


def synthetic_tracks(n_tracks, rows, vid_res, seed=0):
    """n_tracks people walking through the frame for `rows` frames: [((scene, clip, person), frames, poses (rows, 34))]."""
    rng = np.random.default_rng(seed)
    W, H = vid_res
    skel = rng.normal(0, 1, (n_tracks, 1, 17, 2)) * np.array([12.0, 30.0])
    centre = np.stack([rng.uniform(60, W - 60, n_tracks), rng.uniform(60, H - 60, n_tracks)], 1)[:, None, None, :]
    walk = np.cumsum(rng.normal(0, 1.5, (n_tracks, rows, 1, 2)), axis=1)
    p = (centre + walk + skel + rng.normal(0, 0.8, (n_tracks, rows, 17, 2))).clip(1, None).astype(np.float32)
    fr = np.arange(1, rows + 1, dtype=np.int32)
    return [((1, 1 + i // 16, i), fr, p[i].reshape(rows, 34)) for i in range(n_tracks)]


def stats(per_rep):
    """per_rep: one array of tick times (s) per replay -> microseconds."""
    allt = np.concatenate(per_rep) * 1e6
    med = [float(np.median(r) * 1e6) for r in per_rep]
    return {"median_us": round(float(np.median(allt)), 1), "p99_us": round(float(np.percentile(allt, 99)), 1),
            "max_us": round(float(allt.max()), 1), "replay_median_us_min": round(min(med), 1), "replay_median_us_max": round(max(med), 1),
            "ticks_timed": int(allt.size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--data-dir", default=None, help="overrides data_dir (and test_path = <data-dir>/testing/test_frame_mask)")
    ap.add_argument("--dataset-choice", default=None)
    ap.add_argument("--no-scaler", action="store_true", help="bounding-box normalisation only (no fitted RobustScaler at hand)")
    ap.add_argument("--random-init", action="store_true", help="seeded random-init weights when the checkpoint is missing")
    ap.add_argument("--synthetic-tracks", type=int, default=0)
    ap.add_argument("--rows", type=int, default=120, help="rows per synthetic track")
    ap.add_argument("--ring-len", type=int, default=None)
    ap.add_argument("--ticks-per-call", type=int, default=1, help="K > 1: K ticks per push_many call (1: one push per tick)")
    ap.add_argument("--clip-scores", action="store_true", help="online per-clip frame scores in every tick (Tick.clip)")
    ap.add_argument("--sigma", type=float, default=None, help="Gaussian sigma of the clip scores (default: the model's filter_kernel_size)")
    ap.add_argument("--joint-scores", action="store_true", help="per-joint frame scores in every tick (Tick.joint_final)")
    ap.add_argument("--forecasts", action="store_true", help="expected poses in every tick (Tick.forecast)")
    ap.add_argument("--forecast-method", choices=("unique", "mean", "median"), default="median")
    ap.add_argument("--forecast-spread", choices=("mean", "median"), default="mean")
    ap.add_argument("--forecast-transforms", choices=("identity", "all"), default="identity",
                    help="--forecasts: forecasts of transform 0 only, or of every transform mapped back (ForecastCfg(transforms=...))")
    ap.add_argument("--forecasts-out", default=None, metavar="OUT.npz", help="--forecasts: write the rows of the warm-up replay")
    ap.add_argument("--latent-score-space", choices=("latent", "pose"), default=None,
                    help="latent model (overrides the YAML's latent_score_space): 'pose' loads the stage-1 decoder as eval_MoCoDAD.py "
                         "does and scores the decoded forecasts (then --joint-scores and --forecasts work)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_replay.json"))
    cli = ap.parse_args()
    args = load_config(cli.config)
    if cli.latent_score_space is not None:
        args.latent_score_space = cli.latent_score_space
    if cli.data_dir:
        args.data_dir = cli.data_dir
        args.test_path = args.gt_path = os.path.join(cli.data_dir, "testing", "test_frame_mask")
    if cli.dataset_choice:
        args.dataset_choice = cli.dataset_choice
    if not torch.cuda.is_available():
        raise SystemExit("stream_replay.py measures on an MI355X: no GPU found (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    seg_len, nt, vid_res = int(args.seg_len), int(args.num_transform), tuple(args.vid_res)

    torch.manual_seed(int(getattr(args, "seed", 0)))
    latent = bool(getattr(args, "diffusion_on_latent", False))      # (the class choice of eval_MoCoDAD.py)
    model = (MoCoDADlatent if latent else MoCoDAD)(args).to(dev)
    model.save_tensors = False
    ckpt = os.path.join(args.ckpt_dir, args.load_ckpt)
    if os.path.exists(ckpt):
        model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"])
    elif not cli.random_init:
        raise SystemExit(f"checkpoint {ckpt} not found (pass --random-init to score with seeded random-init weights)")
    pose_space = latent and model.latent_score_space == "pose"
    if cli.latent_score_space is not None and not latent:
        raise SystemExit("--latent-score-space is for a latent config (diffusion_on_latent: true)")
    if pose_space:                                  # the stage-1 decoder, as eval_MoCoDAD.py loads it (--random-init included)
        from eval_MoCoDAD import load_latent_decoder
        load_latent_decoder(model, args, cli.random_init)
    elif latent and (cli.joint_scores or cli.forecasts):
        raise SystemExit("--joint-scores / --forecasts with a latent config need --latent-score-space pose (a latent has no joints)")
    center, scale = (None, None) if cli.no_scaler or cli.synthetic_tracks else T.load_scaler_stats(args.ckpt_dir)

    if cli.synthetic_tracks:
        tracks = synthetic_tracks(cli.synthetic_tracks, cli.rows, vid_res, seed=int(getattr(args, "seed", 0)))
        source = f"synthetic: {cli.synthetic_tracks} tracks x {cli.rows} rows"
    else:
        split = str(getattr(args, "split", "test"))
        files = T.list_trajectory_files(T.trajectories_root(args.data_dir, split))
        tracks = [(key,) + T.read_trajectory_csv(path) for key, path in files]
        source = f"{args.data_dir} ({split}): {len(tracks)} track files"
    K = cli.ticks_per_call
    if K < 1:
        raise SystemExit("--ticks-per-call must be at least 1")
    ring_len = cli.ring_len if cli.ring_len is not None or K == 1 else seg_len + K - 1
    size = {k: len(f) for k, f, _ in tracks}
    calls, left, n_open, peak = [], dict(size), 0, 0
    for i, (_, keys, fids, poses) in enumerate(ticks_by_frame(tracks)):
        if i % K == 0:
            calls.append(([], []))
        n_open += sum(left[k] == size[k] for k in keys)
        peak = max(peak, n_open)
        for k in keys:
            left[k] -= 1
        calls[-1][0].append((keys, fids, poses))
        calls[-1][1].extend(k for k in keys if left[k] == 0)
        if i % K == K - 1:                              # closed right after the call that held their last row
            n_open -= len(calls[-1][1])
    n_ticks = sum(len(c[0]) for c in calls)
    # the dataset path on the same rows: the trajectory buffer + window list the baseline scores from (and the AUC needs)
    kept = sorted(((k, f, p) for k, f, p in tracks if len(f) >= seg_len), key=lambda t: t[0])
    off = np.zeros(len(kept) + 1, np.int64)
    off[1:] = np.cumsum([len(f) for _, f, _ in kept])
    buf = normalize_poses(np.concatenate([p for _, _, p in kept]), vid_res, center, scale, device=dev)
    tw = TrajectoryWindows.from_buffer(buf.reshape(-1), off, np.concatenate([f for _, f, _ in kept]), [k for k, _, _ in kept],
                                       seg_len, nt)
    n = tw.n_samples
    sample_of = {tuple(int(v) for v in r): i for i, r in enumerate(tw.meta[:n].numpy())}
    base_d, trans_d = tw.base.to(dev), tw.trans.to(dev)
    sc = model.pose_scorer() if pose_space else model.scorer()
    kw = dict(n_samples=model.n_generated_samples, noise_steps=model.noise_steps, aggregation=model.aggregation_strategy,
              seed=model.seed, loss_fn=model.loss_name)

    clip_keys = sorted({k[:2] for k, _, _ in tracks})
    clip_cfg = ClipScoreCfg(sigma=cli.sigma, max_clips=len(clip_keys)) if cli.clip_scores else None
    if cli.forecasts_out and not cli.forecasts:
        raise SystemExit("--forecasts-out needs --forecasts")
    extra = {"joint_scores": True} if cli.joint_scores else {}
    if cli.forecasts:
        extra["forecasts"] = ForecastCfg(cli.forecast_method, cli.forecast_spread, cli.forecast_transforms)
    # the baseline asks its scoring call for what the tick's asks (PoseStream._run_group): maps, per-sample losses and poses
    base_extra = {}
    if pose_space:
        base_extra = dict(**({"want_maps": True} if cli.joint_scores else {}), **({"want_all": True, "want_poses": True} if cli.forecasts else {}))
    FIELDS = ("observed", "expected", "expected_norm", "count", "spread")

    def replay(collect=None, online=None, forecast_rows=None):
        stream = PoseStream(model, vid_res=vid_res, center=center, scale=scale, max_tracks=peak, ring_len=ring_len,
                            num_transform=nt, clip_scores=clip_cfg, **extra)

        def keep(fs):       # (the warm-up replay only: copies to the host, outside the timed region)
            if forecast_rows is not None and len(fs):
                forecast_rows.append((np.asarray(fs.keys, np.int64).reshape(-1, 3), np.asarray(fs.frames, np.int64))
                                     + tuple(getattr(fs.forecast, name).cpu().numpy() for name in FIELDS))
        times, counts, rows, spent = [], [], 0, 0.0
        for call, done in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = [stream.push(*call[0])] if K == 1 else stream.push_many(call)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rows += sum(len(keys) for keys, _, _ in call)
            spent += dt
            nw = sum(len(tick.final) for tick in out) * nt
            if nw:
                times.append(dt)
                counts.append(nw)
                for tick in out if collect is not None else ():
                    ne = len(tick.final)
                    if ne:
                        idx = np.asarray([t * n + sample_of[tuple(int(v) for v in m)] for t in range(nt) for m in tick.meta[:ne]])
                        collect[idx] = tick.scores.cpu().numpy()
            if online is not None:
                online += [tick.clip for tick in out]
            for tick in out if forecast_rows is not None else ():
                keep(tick.closed)
                keep(tick.final)
            if done:
                keep(stream.close(done))
        if clip_cfg is not None:
            for clip in clip_keys:
                _, tail = stream.close_clip(clip)
                if online is not None:
                    online.append(tail)
        return np.asarray(times), counts, rows / spent

    def baseline(counts):
        times = []
        out = torch.empty(max(counts), device=dev, dtype=torch.float32)
        for i, c in enumerate(counts):
            lo = (i * 7) % max(1, len(tw) - c + 1) if c <= len(tw) else 0
            wb = WindowBatch(tw.buffer, base_d[lo:lo + c], trans_d[lo:lo + c], tw.affine, seg_len)
            if wb.base.shape[0] != c:                      # (more windows in a tick than the split has: not with these replays)
                raise SystemExit("baseline: the tick holds more windows than the dataset path built")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (sc.score if latent else sc.score_fused)(wb, first_window_id=lo, out=out[:c], **kw, **base_extra)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return np.asarray(times)

    scores = np.full(nt * n, np.nan, np.float32)
    online = [] if cli.clip_scores else None
    frows = [] if cli.forecasts_out else None
    _, counts, _ = replay(scores, online, frows)        # warm-up replay (code objects, allocator pools); also the scores for the AUC
    if frows is not None:
        from mocodad_amd._lib import JOINT_NAMES
        cols = [np.concatenate([r[i] for r in frows]) for i in range(2 + len(FIELDS))]
        order = np.lexsort((cols[1], cols[0][:, 2], cols[0][:, 1], cols[0][:, 0]))
        np.savez(cli.forecasts_out, rows=cols[0][order], row_columns=np.asarray(["scene", "clip", "person"]), frames=cols[1][order],
                 joint_names=np.asarray(JOINT_NAMES), method=np.asarray(cli.forecast_method), spread_method=np.asarray(cli.forecast_spread),
                 **{name: cols[2 + i][order] for i, name in enumerate(FIELDS)})
        print(f"forecasts: {len(order)} track rows, {int((cols[2 + FIELDS.index('count')] > 0).sum())} with a forecast -> {cli.forecasts_out}")
    baseline(counts)
    assert not np.isnan(scores).any() and sum(counts) == nt * n, "the replay did not emit every window of the dataset path"
    auc = None
    if not cli.synthetic_tracks:
        auc = float(model.post_processing(scores, None, tw.trans.long().numpy(), tw.meta.numpy(), tw.frames.numpy()))
    clip_res = None
    if online is not None:
        n_scores = sum(len(cf) for cf in online)
        clip_res = {"sigma": float(model.anomaly_score_filter_kernel_size if cli.sigma is None else cli.sigma),
                    "shift": int(model.anomaly_score_frames_shift), "frames_scored": n_scores,
                    "dropped_rows": sum(cf.dropped_rows for cf in online)}
        if not cli.synthetic_tracks:
            from sklearn.metrics import roc_auc_score
            gts, _ = model._gt_and_masks()
            score_of = {(clip, int(f)): float(v) for cf in online for clip, f, v in zip(cf.clips, cf.frames, cf.values.cpu().numpy())}
            y, p, missing = [], [], 0
            for clip, gt in gts.items():
                for i, label in enumerate(np.asarray(gt).reshape(-1)):
                    v = score_of.get((tuple(int(c) for c in clip), i + 1))        # frame ids are 1-based
                    if v is None:
                        missing += 1
                    else:
                        y.append(int(label))
                        p.append(v)
            clip_res.update(gt_frames=len(y) + missing, gt_frames_without_score=missing,
                            auc_online=float(roc_auc_score(y, p)) if len(set(y)) == 2 else None)
    t_stream, t_base, rate = [], [], []
    for _ in range(cli.reps):                   # alternating: both legs see the same machine state
        t, _, r = replay()
        t_stream.append(t)
        rate.append(r)
        t_base.append(baseline(counts))
    res = {"source": source, "ticks": n_ticks, "ticks_per_call": K, "calls": len(calls), "ticks_with_windows": len(counts),
           "peak_open_tracks": peak, "rows_per_s": {"median": round(float(np.median(rate))), "min": round(min(rate)), "max": round(max(rate))},
           "windows_per_tick_median": int(np.median(counts)), "windows_per_tick_max": int(max(counts)),
           "windows_total": int(sum(counts)), "seg_len": seg_len, "num_transform": nt, "noise_steps": int(model.noise_steps),
           "n_samples": int(model.n_generated_samples), "ring_len": ring_len or seg_len, "reps": cli.reps, "auc": auc,
           "model": "MoCoDADlatent" if latent else "MoCoDAD", "score_space": model.latent_score_space if latent else None, "clip_scores": clip_res, "joint_scores": bool(cli.joint_scores),
           "forecasts": {"method": cli.forecast_method, "spread": cli.forecast_spread, "transforms": cli.forecast_transforms} if cli.forecasts else None,
           "tick": stats(t_stream), "baseline_score_fused": stats(t_base), "device": torch.cuda.get_device_name(0)}
    if auc is not None:
        print(f"AUC: {auc:.6f}")
    if clip_res is not None and clip_res.get("auc_online") is not None:
        print(f"AUC of the online clip scores: {clip_res['auc_online']:.6f} ({clip_res['gt_frames_without_score']} of "
              f"{clip_res['gt_frames']} ground-truth frames without an emitted score excluded; a different definition: not comparable bit for bit)")
    print(f"{K} tick(s) per call, {res['rows_per_s']['median']} rows/s | tick: median {res['tick']['median_us']} us, p99 {res['tick']['p99_us']} us | baseline score_fused alone: median "
          f"{res['baseline_score_fused']['median_us']} us, p99 {res['baseline_score_fused']['p99_us']} us")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

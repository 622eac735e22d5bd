"""CPU: calls the library rejects before it touches a device, on the entries that take no handle -- each must keep its return
code and its mcd_last_error() text.  The expected pairs are tests/golden/call_errors.json["host"], recorded from the library
before the call front end (mcd_call.hpp) existed:

    python tests/test_call_errors_host.py --record      # rewrites the "host" key; see the file's "how" entry

(the stream_push_group / stream_frame_scores_group pairs: from the library of the last commit that also had per-tick stream
entries, whose state and argument rules they took over one to one; the pairs of mcd_denormalize_poses, mcd_forecast_assemble, the
joint and forecast ring entries and the clip entries, with the pairs that fix the ORDER of two checks failing together: from the
library of the last commit whose stream entry points stood in mcd_api.hip, each check written out per entry -- `--record FILE`
writes a copy of the JSON elsewhere)

Pointers that a rejected call never reads are the dummy address P."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402

from mocodad_amd import _lib  # noqa: E402

JSON = os.path.join(GOLDEN, "call_errors.json")
P = C.c_void_p(0x1000)        # non-null, 16-byte aligned, never dereferenced
ODD = C.c_void_p(0x1004)      # ... and not 16-byte aligned
INF, NAN = float("inf"), float("nan")


def score_cfg(B=3, S=2, ns=4, seg_len=6, n_cond=3, n_corrupt=3, loss_fn=0):
    c = _lib.ScoreCfg()
    c.n_windows, c.n_samples, c.noise_steps, c.seg_len, c.n_cond, c.n_corrupt, c.loss_fn = B, S, ns, seg_len, n_cond, n_corrupt, loss_fn
    for i in range(n_cond):
        c.cond_idx[i] = i
    for i in range(n_corrupt):
        c.corrupt_idx[i] = n_cond + i
    return c


def view(base=None, trans=None, affine=None, cond_mask=None):
    return _lib.WindowView(base=base, stride_c=0, stride_t=0, trans=trans, affine=affine, cond_mask=cond_mask)


def state(ring=0x1000, fs=0x1000, n_slots=4, ring_len=12, seg_len=6, nt=2):
    return _lib.StreamState(ring=ring, frame_scores=fs, n_slots=n_slots, ring_len=ring_len, seg_len=seg_len, num_transform=nt)


def frame_cfg(**over):
    d = dict(n_clips=1, num_transform=1, n_persons=1, max_frames=16, pad_size=-1, frames_shift=1, gauss_radius=0,
             clip_keys=0x1000, clip_n_frames=0x1000, frame_dst=0x1000, clip_out_len=0x1000, clip_out_off=0x1000, gauss_weights=0x1000)
    d.update(over)
    return _lib.FrameCfg(**d)


def _agg(L, cfg, strategy=1, q=0.0, loss_all=P, pose_all=None, data=None, v=None, loss_agg=P, pose_agg=None):
    return L.mcd_aggregate_view(C.byref(cfg) if cfg is not None else None, 2, 17, strategy, C.c_float(q), loss_all, pose_all, data,
                                C.byref(v) if v is not None else None, loss_agg, pose_agg, None)


def _agg_dense(L, cfg, strategy=1, q=0.0, loss_all=P, loss_agg=P):
    return L.mcd_aggregate(C.byref(cfg), 2, 17, strategy, C.c_float(q), loss_all, None, None, loss_agg, None, None)


def _push(L, s, raw=P, desc=P, n=2, n_windows=1, w=640.0, h=360.0, center=None, scale=None, base=P, trans=P):
    return L.mcd_stream_push_group(C.byref(s) if s is not None else None, raw, desc, n, n_windows, w, h, center, scale, base, trans, None)


def _frames(L, c, scores=P, trans=P, meta=P, frames=P, n=4, ws=P, out=P):
    return L.mcd_frame_scores(C.byref(c) if c is not None else None, scores, trans, meta, frames, n, 6, ws, out, None)


def _scatter(L, scores=P, frames=P, row=P, n=2, seg_len=3, n_rows=2, n_frames=4, out=P):
    return L.mcd_scatter_max(scores, frames, row, n, seg_len, n_rows, n_frames, out, None)


def _denorm(L, norm=P, raw=P, count=None, n=4, w=640.0, h=360.0, center=None, scale=None, out=P):
    return L.mcd_denormalize_poses(norm, raw, count, n, w, h, center, scale, out, None)


def _assemble(L, poses=P, cell=P, n=4, n_corrupt=3, n_cells=5, method=1, spread=1, max_cover=3, ws=P, pose=P, count=P, spread_out=P):
    return L.mcd_forecast_assemble(poses, cell, n, n_corrupt, n_cells, method, spread, max_cover, ws, pose, count, spread_out, None)


def jstate(js=0x1000):
    return _lib.StreamJointState(joint_scores=js)


def fstate(fc=0x1000, obs=0x1000, n_corrupt=3):
    return _lib.StreamForecastState(forecast=fc, observed=obs, n_corrupt=n_corrupt)


def cfg_idx(corrupt_idx, **kw):
    """score_cfg with the corrupt frame list replaced"""
    c = score_cfg(**kw)
    for i, v in enumerate(corrupt_idx):
        c.corrupt_idx[i] = v
    return c


BIG_JOINT = dict(n_slots=1 << 19, ring_len=32, nt=16)      # pose and score rings below 2^31 elements, 17 per score cell above
BIG_FORECAST = dict(n_slots=1 << 19, ring_len=48)           # 2^19 * 48 * 3 * 34 forecast elements


def _joint(L, s="state", js="jstate", maps=P, win=P, n_windows=1, cfg="cfg", final=P):
    s, js, cfg = state() if s == "state" else s, jstate() if js == "jstate" else js, score_cfg() if cfg == "cfg" else cfg
    return L.mcd_stream_joint_scores_group(C.byref(s) if s is not None else None, C.byref(js) if js is not None else None, maps, win,
                                           n_windows, C.byref(cfg) if cfg is not None else None, final, None)


def _jflush(L, s="state", js="jstate", win=P, n=1, out=P):
    s, js = state() if s == "state" else s, jstate() if js == "jstate" else js
    return L.mcd_stream_joint_flush(C.byref(s) if s is not None else None, C.byref(js) if js is not None else None, win, n, out, None)


def _fgroup(L, s="state", fs="fstate", raw=P, desc=P, n=2, loss_all=P, poses_all=P, win=P, n_windows=1, cfg="cfg", aggregation=1,
            method=1, spread=1, w=640.0, h=360.0, center=None, scale=None, expected=P, norm=P, observed=P, count=P, spread_out=P):
    s, fs, cfg = state() if s == "state" else s, fstate() if fs == "fstate" else fs, score_cfg() if cfg == "cfg" else cfg
    return L.mcd_stream_forecast_group(C.byref(s) if s is not None else None, C.byref(fs) if fs is not None else None, raw, desc, n,
                                       loss_all, poses_all, win, n_windows, C.byref(cfg) if cfg is not None else None, aggregation,
                                       method, spread, w, h, center, scale, expected, norm, observed, count, spread_out, None)


def _fflush(L, s="state", fs="fstate", win=P, n=1, cfg="cfg", method=1, spread=1, w=640.0, h=360.0, center=None, scale=None,
            expected=P, norm=P, observed=P, count=P, spread_out=P):
    s, fs, cfg = state() if s == "state" else s, fstate() if fs == "fstate" else fs, score_cfg() if cfg == "cfg" else cfg
    return L.mcd_stream_forecast_flush(C.byref(s) if s is not None else None, C.byref(fs) if fs is not None else None, win, n,
                                       C.byref(cfg) if cfg is not None else None, method, spread, w, h, center, scale, expected, norm,
                                       observed, count, spread_out, None)


def clip(**over):
    d = dict(sum=0x1000, lmax=0x1000, lmin=0x1000, n=0x1000, n_clips=2, clip_ring_len=8, num_transform=2)
    d.update(over)
    return _lib.ClipState(**d)


def _cupdate(L, c="clip", runs=P, n_runs=1, contrib=P, n_contrib=1, finals=P, n_finals=1, tails=P, n_tails=1):
    c = clip() if c == "clip" else c
    return L.mcd_stream_clip_update(C.byref(c) if c is not None else None, runs, n_runs, contrib, n_contrib, finals, n_finals, tails,
                                    n_tails, None)


def _cemit(L, c="clip", outs=P, n_out=1, gauss=P, radius=2, shift=1, out=P):
    c = clip() if c == "clip" else c
    return L.mcd_stream_clip_emit(C.byref(c) if c is not None else None, outs, n_out, gauss, radius, shift, out, None)


CASES = {
    # ---- mcd_aggregate / mcd_aggregate_view
    "aggregate_view: null cfg": lambda L: _agg(L, None),
    "aggregate_view: null loss_all": lambda L: _agg(L, score_cfg(), loss_all=None),
    "aggregate_view: null loss_agg": lambda L: _agg(L, score_cfg(), loss_agg=None),
    "aggregate_view: n_samples 0": lambda L: _agg(L, score_cfg(S=0)),
    "aggregate_view: strategy all": lambda L: _agg(L, score_cfg(), strategy=0),
    "aggregate_view: strategy 8": lambda L: _agg(L, score_cfg(), strategy=8),
    "aggregate_view: quantile 1.5": lambda L: _agg(L, score_cfg(), strategy=7, q=1.5),
    "aggregate_view: quantile -0.1": lambda L: _agg(L, score_cfg(), strategy=7, q=-0.1),
    "aggregate_view: quantile nan": lambda L: _agg(L, score_cfg(), strategy=7, q=NAN),
    "aggregate_view: mean_pose without pose_all": lambda L: _agg(L, score_cfg(), strategy=5, data=P),
    "aggregate_view: median_pose without data": lambda L: _agg(L, score_cfg(), strategy=6, pose_all=P),
    "aggregate_view: pose_agg without pose_all": lambda L: _agg(L, score_cfg(), pose_agg=P),
    "aggregate_view: view with base": lambda L: _agg(L, score_cfg(), v=view(base=0x1000)),
    "aggregate_view: cond_mask, seg_len 33": lambda L: _agg(L, score_cfg(seg_len=33), v=view(cond_mask=0x1000)),
    "aggregate_view: cond_mask, n_corrupt 0": lambda L: _agg(L, score_cfg(n_cond=6, n_corrupt=0), v=view(cond_mask=0x1000)),
    "aggregate_view: cond_mask, n_corrupt > seg_len": lambda L: _agg(L, score_cfg(seg_len=2), v=view(cond_mask=0x1000)),
    "aggregate: null loss_all": lambda L: _agg_dense(L, score_cfg(), loss_all=None),
    "aggregate: n_samples 0": lambda L: _agg_dense(L, score_cfg(S=0)),
    "aggregate: strategy 9": lambda L: _agg_dense(L, score_cfg(), strategy=9),
    "aggregate: quantile 1.5": lambda L: _agg_dense(L, score_cfg(), strategy=7, q=1.5),
    # ---- mcd_philox_noise / mcd_latent_philox_noise
    "philox_noise: null out": lambda L: L.mcd_philox_noise(1, 0, 3, 2, 4, 3, None, None),
    "philox_noise: n_samples 0": lambda L: L.mcd_philox_noise(1, 0, 3, 0, 4, 3, P, None),
    "philox_noise: noise_steps 1": lambda L: L.mcd_philox_noise(1, 0, 3, 2, 1, 3, P, None),
    "philox_noise: n_corrupt 0": lambda L: L.mcd_philox_noise(1, 0, 3, 2, 4, 0, P, None),
    "philox_noise: n_corrupt 33": lambda L: L.mcd_philox_noise(1, 0, 3, 2, 4, 33, P, None),
    "latent_philox_noise: null out": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 2, 4, 32, None, None),
    "latent_philox_noise: n_samples 0": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 0, 4, 32, P, None),
    "latent_philox_noise: noise_steps 1": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 2, 1, 32, P, None),
    "latent_philox_noise: latent_dim 0": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 2, 4, 0, P, None),
    "latent_philox_noise: latent_dim 24": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 2, 4, 24, P, None),
    "latent_philox_noise: latent_dim 144": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 2, 4, 144, P, None),
    "latent_philox_noise: misaligned out": lambda L: L.mcd_latent_philox_noise(1, 0, 3, 2, 4, 32, ODD, None),
    # ---- mcd_random_imp_masks
    "random_imp_masks: seg_len 1": lambda L: L.mcd_random_imp_masks(1, 0, 3, 1, 1, P, None),
    "random_imp_masks: seg_len 33": lambda L: L.mcd_random_imp_masks(1, 0, 3, 33, 2, P, None),
    "random_imp_masks: n_cond 0": lambda L: L.mcd_random_imp_masks(1, 0, 3, 6, 0, P, None),
    "random_imp_masks: n_cond = seg_len": lambda L: L.mcd_random_imp_masks(1, 0, 3, 6, 6, P, None),
    "random_imp_masks: n_windows -1": lambda L: L.mcd_random_imp_masks(1, 0, -1, 6, 2, P, None),
    "random_imp_masks: null out": lambda L: L.mcd_random_imp_masks(1, 0, 3, 6, 2, None, None),
    # ---- mcd_normalize_poses
    "normalize_poses: n_frames -1": lambda L: L.mcd_normalize_poses(P, -1, 640.0, 360.0, None, None, P, None),
    "normalize_poses: vid_w inf": lambda L: L.mcd_normalize_poses(P, 4, INF, 360.0, None, None, P, None),
    "normalize_poses: vid_h nan": lambda L: L.mcd_normalize_poses(P, 4, 640.0, NAN, None, None, P, None),
    "normalize_poses: center without scale": lambda L: L.mcd_normalize_poses(P, 4, 640.0, 360.0, P, None, P, None),
    "normalize_poses: scale without center": lambda L: L.mcd_normalize_poses(P, 4, 640.0, 360.0, None, P, P, None),
    "normalize_poses: null raw": lambda L: L.mcd_normalize_poses(None, 4, 640.0, 360.0, None, None, P, None),
    "normalize_poses: null out": lambda L: L.mcd_normalize_poses(P, 4, 640.0, 360.0, None, None, None, None),
    "normalize_poses: 2^40 frames": lambda L: L.mcd_normalize_poses(P, 1 << 40, 640.0, 360.0, None, None, P, None),
    # ---- mcd_scatter_max (the checks of mcd_joint_scatter_max, recorded when the two became one host function)
    "scatter_max: null out": lambda L: _scatter(L, out=None),
    "scatter_max: null scores": lambda L: _scatter(L, scores=None),
    "scatter_max: null frames": lambda L: _scatter(L, frames=None),
    "scatter_max: null row": lambda L: _scatter(L, row=None),
    "scatter_max: n -1": lambda L: _scatter(L, n=-1),
    "scatter_max: seg_len 0": lambda L: _scatter(L, seg_len=0),
    "scatter_max: n_rows -1": lambda L: _scatter(L, n_rows=-1),
    "scatter_max: n_frames -2": lambda L: _scatter(L, n_frames=-2),
    "scatter_max: 2^40 windows": lambda L: _scatter(L, n=1 << 40),
    # ---- mcd_stream_*
    "stream_push_group: null state": lambda L: _push(L, None),
    "stream_push_group: null ring": lambda L: _push(L, state(ring=None)),
    "stream_push_group: null frame_scores": lambda L: _push(L, state(fs=None)),
    "stream_push_group: n_slots 0": lambda L: _push(L, state(n_slots=0)),
    "stream_push_group: num_transform 0": lambda L: _push(L, state(nt=0)),
    "stream_push_group: seg_len 33": lambda L: _push(L, state(seg_len=33, ring_len=40)),
    "stream_push_group: ring_len < seg_len": lambda L: _push(L, state(ring_len=5)),
    "stream_push_group: rings over 2^31": lambda L: _push(L, state(n_slots=1 << 26, ring_len=32)),
    "stream_push_group: score ring over 2^31": lambda L: _push(L, state(n_slots=1 << 19, ring_len=32, nt=1 << 8)),
    "stream_push_group: n_windows > n": lambda L: _push(L, state(), n=1, n_windows=2),
    "stream_push_group: n -1": lambda L: _push(L, state(), n=-1, n_windows=0),
    "stream_push_group: n = 29": lambda L: _push(L, state(), n=29),       # (state(): 4 * (12 - 6 + 1) = 28 rows per group)
    # (n_windows <= n <= n_slots * (ring_len - seg_len + 1) <= n_slots * ring_len: the product reaches 2^31 only where the score
    # ring does, so the state is what the entry refuses -- here the smallest such call, seg_len 1 and a window per cell)
    "stream_push_group: n_windows * num_transform over 2^31": lambda L: _push(L, state(n_slots=1 << 19, ring_len=16, seg_len=1, nt=1 << 8),
                                                                              n=1 << 23, n_windows=1 << 23),
    "stream_push_group: vid_w inf": lambda L: _push(L, state(), w=INF),
    "stream_push_group: center without scale": lambda L: _push(L, state(), center=P),
    "stream_push_group: null raw": lambda L: _push(L, state(), raw=None),
    "stream_push_group: null desc": lambda L: _push(L, state(), desc=None),
    "stream_push_group: null base_out": lambda L: _push(L, state(), base=None),
    "stream_frame_scores_group: null state": lambda L: L.mcd_stream_frame_scores_group(None, P, P, 1, P, None),
    "stream_frame_scores_group: seg_len 0": lambda L: L.mcd_stream_frame_scores_group(C.byref(state(seg_len=0)), P, P, 1, P, None),
    "stream_frame_scores_group: n_windows -1": lambda L: L.mcd_stream_frame_scores_group(C.byref(state()), P, P, -1, P, None),
    "stream_frame_scores_group: n_windows = 29": lambda L: L.mcd_stream_frame_scores_group(C.byref(state()), P, P, 29, P, None),
    "stream_frame_scores_group: null scores": lambda L: L.mcd_stream_frame_scores_group(C.byref(state()), None, P, 1, P, None),
    "stream_frame_scores_group: null final_out": lambda L: L.mcd_stream_frame_scores_group(C.byref(state()), P, P, 1, None, None),
    "stream_flush: null state": lambda L: L.mcd_stream_flush(None, P, 1, P, None),
    "stream_flush: ring_len < seg_len": lambda L: L.mcd_stream_flush(C.byref(state(ring_len=3)), P, 1, P, None),
    "stream_flush: n > n_slots": lambda L: L.mcd_stream_flush(C.byref(state()), P, 5, P, None),
    "stream_flush: n -1": lambda L: L.mcd_stream_flush(C.byref(state()), P, -1, P, None),
    "stream_flush: null win": lambda L: L.mcd_stream_flush(C.byref(state()), None, 1, P, None),
    "stream_flush: null out": lambda L: L.mcd_stream_flush(C.byref(state()), P, 1, None, None),
    # (order of the checks: the counts before the bound on a group)
    "stream_push_group: n_windows > n, n = 29": lambda L: _push(L, state(), n=29, n_windows=30),
    # ---- mcd_denormalize_poses
    "denormalize_poses: n -1": lambda L: _denorm(L, n=-1),
    "denormalize_poses: vid_w inf": lambda L: _denorm(L, w=INF),
    "denormalize_poses: vid_h nan": lambda L: _denorm(L, h=NAN),
    "denormalize_poses: center without scale": lambda L: _denorm(L, center=P),
    "denormalize_poses: scale without center": lambda L: _denorm(L, scale=P),
    "denormalize_poses: vid_w inf, center without scale": lambda L: _denorm(L, w=INF, center=P),
    "denormalize_poses: null norm": lambda L: _denorm(L, norm=None),
    "denormalize_poses: null raw": lambda L: _denorm(L, raw=None),
    "denormalize_poses: null out": lambda L: _denorm(L, out=None),
    "denormalize_poses: 2^40 rows": lambda L: _denorm(L, n=1 << 40),
    # ---- mcd_forecast_assemble
    "forecast_assemble: n -1": lambda L: _assemble(L, n=-1),
    "forecast_assemble: n_cells -1": lambda L: _assemble(L, n_cells=-1),
    "forecast_assemble: n_corrupt 0": lambda L: _assemble(L, n_corrupt=0),
    "forecast_assemble: n_corrupt 33": lambda L: _assemble(L, n_corrupt=33),
    "forecast_assemble: max_cover 0": lambda L: _assemble(L, max_cover=0),
    "forecast_assemble: max_cover 33": lambda L: _assemble(L, max_cover=33),
    "forecast_assemble: method 3": lambda L: _assemble(L, method=3),
    "forecast_assemble: method -1": lambda L: _assemble(L, method=-1),
    "forecast_assemble: spread unique": lambda L: _assemble(L, spread=0),
    "forecast_assemble: spread 3": lambda L: _assemble(L, spread=3),
    "forecast_assemble: method 3, spread 3": lambda L: _assemble(L, method=3, spread=3),
    "forecast_assemble: n x n_corrupt over 2^31": lambda L: _assemble(L, n=1 << 30),
    "forecast_assemble: null workspace": lambda L: _assemble(L, ws=None),
    "forecast_assemble: null pose_out": lambda L: _assemble(L, pose=None),
    "forecast_assemble: null count_out": lambda L: _assemble(L, count=None),
    "forecast_assemble: null spread_out": lambda L: _assemble(L, spread_out=None),
    "forecast_assemble: null poses": lambda L: _assemble(L, poses=None),
    "forecast_assemble: null cell": lambda L: _assemble(L, cell=None),
    # ---- mcd_stream_joint_scores_group / mcd_stream_joint_flush
    "stream_joint_scores_group: null state": lambda L: _joint(L, s=None),
    "stream_joint_scores_group: ring_len < seg_len": lambda L: _joint(L, s=state(ring_len=5)),
    "stream_joint_scores_group: null joint state": lambda L: _joint(L, js=None),
    "stream_joint_scores_group: null joint_scores": lambda L: _joint(L, js=jstate(None)),
    "stream_joint_scores_group: joint ring over 2^31": lambda L: _joint(L, s=state(**BIG_JOINT)),
    "stream_joint_scores_group: null joint state, joint ring over 2^31": lambda L: _joint(L, s=state(**BIG_JOINT), js=None),
    "stream_joint_scores_group: null cfg": lambda L: _joint(L, cfg=None),
    "stream_joint_scores_group: cfg seg_len 5": lambda L: _joint(L, cfg=score_cfg(seg_len=5, n_cond=2)),
    "stream_joint_scores_group: n_cond + n_corrupt != seg_len": lambda L: _joint(L, cfg=score_cfg(n_cond=2)),
    "stream_joint_scores_group: n_corrupt 0": lambda L: _joint(L, cfg=score_cfg(n_cond=6, n_corrupt=0)),
    "stream_joint_scores_group: corrupt_idx 6": lambda L: _joint(L, cfg=cfg_idx([3, 4, 6])),
    "stream_joint_scores_group: corrupt_idx -1": lambda L: _joint(L, cfg=cfg_idx([-1, 4, 5])),
    "stream_joint_scores_group: corrupt_idx twice": lambda L: _joint(L, cfg=cfg_idx([3, 4, 4])),
    "stream_joint_scores_group: cfg seg_len 5, corrupt_idx descending": lambda L: _joint(L, cfg=cfg_idx([4, 3, 2], seg_len=5, n_cond=2)),
    "stream_joint_scores_group: n_windows -1": lambda L: _joint(L, n_windows=-1),
    "stream_joint_scores_group: n_windows = 29": lambda L: _joint(L, n_windows=29),
    "stream_joint_scores_group: null maps": lambda L: _joint(L, maps=None),
    "stream_joint_scores_group: null win": lambda L: _joint(L, win=None),
    "stream_joint_scores_group: null final_out": lambda L: _joint(L, final=None),
    "stream_joint_flush: null state": lambda L: _jflush(L, s=None),
    "stream_joint_flush: null joint state": lambda L: _jflush(L, js=None),
    "stream_joint_flush: null joint_scores": lambda L: _jflush(L, js=jstate(None)),
    "stream_joint_flush: joint ring over 2^31": lambda L: _jflush(L, s=state(**BIG_JOINT)),
    "stream_joint_flush: null joint state, joint ring over 2^31": lambda L: _jflush(L, s=state(**BIG_JOINT), js=None),
    "stream_joint_flush: n -1": lambda L: _jflush(L, n=-1),
    "stream_joint_flush: n > n_slots": lambda L: _jflush(L, n=5),
    "stream_joint_flush: null win": lambda L: _jflush(L, win=None),
    "stream_joint_flush: null out": lambda L: _jflush(L, out=None),
    # ---- mcd_stream_forecast_group / mcd_stream_forecast_flush
    "stream_forecast_group: null state": lambda L: _fgroup(L, s=None),
    "stream_forecast_group: seg_len 33": lambda L: _fgroup(L, s=state(seg_len=33, ring_len=40)),
    "stream_forecast_group: null forecast state": lambda L: _fgroup(L, fs=None),
    "stream_forecast_group: null forecast": lambda L: _fgroup(L, fs=fstate(fc=None)),
    "stream_forecast_group: null observed": lambda L: _fgroup(L, fs=fstate(obs=None)),
    "stream_forecast_group: null forecast state, method 3": lambda L: _fgroup(L, fs=None, method=3),
    "stream_forecast_group: state n_corrupt 0": lambda L: _fgroup(L, fs=fstate(n_corrupt=0)),
    "stream_forecast_group: state n_corrupt 33": lambda L: _fgroup(L, fs=fstate(n_corrupt=33)),
    "stream_forecast_group: null cfg": lambda L: _fgroup(L, cfg=None),
    "stream_forecast_group: cfg seg_len 5": lambda L: _fgroup(L, cfg=score_cfg(seg_len=5, n_cond=2)),
    "stream_forecast_group: cfg n_corrupt 2": lambda L: _fgroup(L, cfg=score_cfg(n_cond=4, n_corrupt=2)),
    "stream_forecast_group: n_cond + n_corrupt != seg_len": lambda L: _fgroup(L, cfg=score_cfg(n_cond=2)),
    "stream_forecast_group: corrupt_idx descending": lambda L: _fgroup(L, cfg=cfg_idx([5, 4, 3])),
    "stream_forecast_group: corrupt_idx twice": lambda L: _fgroup(L, cfg=cfg_idx([3, 4, 4])),
    "stream_forecast_group: corrupt_idx 6": lambda L: _fgroup(L, cfg=cfg_idx([3, 4, 6])),
    "stream_forecast_group: corrupt_idx -1": lambda L: _fgroup(L, cfg=cfg_idx([-1, 4, 5])),
    "stream_forecast_group: cfg seg_len 5, corrupt_idx descending": lambda L: _fgroup(L, cfg=cfg_idx([4, 3, 2], seg_len=5, n_cond=2)),
    "stream_forecast_group: method 3": lambda L: _fgroup(L, method=3),
    "stream_forecast_group: spread unique": lambda L: _fgroup(L, spread=0),
    "stream_forecast_group: method -1, spread 3": lambda L: _fgroup(L, method=-1, spread=3),
    "stream_forecast_group: corrupt_idx descending, method 3": lambda L: _fgroup(L, cfg=cfg_idx([5, 4, 3]), method=3),
    "stream_forecast_group: spread 3, vid_h nan": lambda L: _fgroup(L, spread=3, h=NAN),
    "stream_forecast_group: vid_w inf": lambda L: _fgroup(L, w=INF),
    "stream_forecast_group: vid_h nan": lambda L: _fgroup(L, h=NAN),
    "stream_forecast_group: center without scale": lambda L: _fgroup(L, center=P),
    "stream_forecast_group: scale without center": lambda L: _fgroup(L, scale=P),
    "stream_forecast_group: vid_w inf, center without scale": lambda L: _fgroup(L, w=INF, center=P),
    "stream_forecast_group: forecast ring over 2^31": lambda L: _fgroup(L, s=state(**BIG_FORECAST)),
    "stream_forecast_group: center without scale, forecast ring over 2^31": lambda L: _fgroup(L, s=state(**BIG_FORECAST), center=P),
    "stream_forecast_group: aggregation mean": lambda L: _fgroup(L, aggregation=3),
    "stream_forecast_group: aggregation all": lambda L: _fgroup(L, aggregation=0),
    "stream_forecast_group: aggregation mean, n -1": lambda L: _fgroup(L, aggregation=3, n=-1, n_windows=0),
    "stream_forecast_group: n -1": lambda L: _fgroup(L, n=-1, n_windows=0),
    "stream_forecast_group: n_windows -1": lambda L: _fgroup(L, n_windows=-1),
    "stream_forecast_group: n_windows > n": lambda L: _fgroup(L, n=1, n_windows=2),
    "stream_forecast_group: n = 29": lambda L: _fgroup(L, n=29),
    "stream_forecast_group: n_windows > n, n = 29": lambda L: _fgroup(L, n=29, n_windows=30),
    "stream_forecast_group: n_samples 0": lambda L: _fgroup(L, cfg=score_cfg(S=0)),
    "stream_forecast_group: n = 29, n_samples 0": lambda L: _fgroup(L, n=29, cfg=score_cfg(S=0)),
    "stream_forecast_group: null raw": lambda L: _fgroup(L, raw=None),
    "stream_forecast_group: null desc": lambda L: _fgroup(L, desc=None),
    "stream_forecast_group: null loss_all": lambda L: _fgroup(L, loss_all=None),
    "stream_forecast_group: null poses_all": lambda L: _fgroup(L, poses_all=None),
    "stream_forecast_group: null win": lambda L: _fgroup(L, win=None),
    "stream_forecast_group: null expected_out": lambda L: _fgroup(L, expected=None),
    "stream_forecast_group: null spread_out": lambda L: _fgroup(L, spread_out=None),
    "stream_forecast_flush: null state": lambda L: _fflush(L, s=None),
    "stream_forecast_flush: null forecast state": lambda L: _fflush(L, fs=None),
    "stream_forecast_flush: null forecast state, method 3": lambda L: _fflush(L, fs=None, method=3),
    "stream_forecast_flush: state n_corrupt 33": lambda L: _fflush(L, fs=fstate(n_corrupt=33)),
    "stream_forecast_flush: null cfg": lambda L: _fflush(L, cfg=None),
    "stream_forecast_flush: cfg seg_len 5": lambda L: _fflush(L, cfg=score_cfg(seg_len=5, n_cond=2)),
    "stream_forecast_flush: cfg n_corrupt 2": lambda L: _fflush(L, cfg=score_cfg(n_cond=4, n_corrupt=2)),
    "stream_forecast_flush: n_cond + n_corrupt != seg_len": lambda L: _fflush(L, cfg=score_cfg(n_cond=2)),
    "stream_forecast_flush: corrupt_idx descending": lambda L: _fflush(L, cfg=cfg_idx([5, 4, 3])),
    "stream_forecast_flush: cfg seg_len 5, corrupt_idx descending": lambda L: _fflush(L, cfg=cfg_idx([4, 3, 2], seg_len=5, n_cond=2)),
    "stream_forecast_flush: method 3": lambda L: _fflush(L, method=3),
    "stream_forecast_flush: spread unique": lambda L: _fflush(L, spread=0),
    "stream_forecast_flush: vid_w inf": lambda L: _fflush(L, w=INF),
    "stream_forecast_flush: center without scale": lambda L: _fflush(L, center=P),
    "stream_forecast_flush: vid_w inf, center without scale": lambda L: _fflush(L, w=INF, center=P),
    "stream_forecast_flush: forecast ring over 2^31": lambda L: _fflush(L, s=state(**BIG_FORECAST)),
    "stream_forecast_flush: n -1": lambda L: _fflush(L, n=-1),
    "stream_forecast_flush: n > n_slots": lambda L: _fflush(L, n=5),
    "stream_forecast_flush: null win": lambda L: _fflush(L, win=None),
    "stream_forecast_flush: null norm_out": lambda L: _fflush(L, norm=None),
    "stream_forecast_flush: null count_out": lambda L: _fflush(L, count=None),
    # ---- mcd_stream_clip_update / mcd_stream_clip_emit
    "stream_clip_update: null state": lambda L: _cupdate(L, c=None),
    "stream_clip_update: null sum": lambda L: _cupdate(L, c=clip(sum=None)),
    "stream_clip_update: null lmax": lambda L: _cupdate(L, c=clip(lmax=None)),
    "stream_clip_update: null lmin": lambda L: _cupdate(L, c=clip(lmin=None)),
    "stream_clip_update: null n": lambda L: _cupdate(L, c=clip(n=None)),
    "stream_clip_update: n_clips 0": lambda L: _cupdate(L, c=clip(n_clips=0)),
    "stream_clip_update: num_transform 0": lambda L: _cupdate(L, c=clip(num_transform=0)),
    "stream_clip_update: clip_ring_len 0": lambda L: _cupdate(L, c=clip(clip_ring_len=0)),
    "stream_clip_update: 257 transforms": lambda L: _cupdate(L, c=clip(num_transform=257)),
    "stream_clip_update: cells over 2^31": lambda L: _cupdate(L, c=clip(n_clips=1 << 16, clip_ring_len=1 << 15)),
    "stream_clip_update: n_runs -1": lambda L: _cupdate(L, n_runs=-1),
    "stream_clip_update: n_runs = 17": lambda L: _cupdate(L, n_runs=17),        # (clip(): 2 * 8 = 16 cells)
    "stream_clip_update: n_runs = 17, null runs": lambda L: _cupdate(L, n_runs=17, runs=None),
    "stream_clip_update: n_runs = 17, n_contrib -1": lambda L: _cupdate(L, n_runs=17, n_contrib=-1),
    "stream_clip_update: n_contrib -1": lambda L: _cupdate(L, n_contrib=-1),
    "stream_clip_update: n_finals -1": lambda L: _cupdate(L, n_finals=-1),
    "stream_clip_update: n_tails -1": lambda L: _cupdate(L, n_tails=-1),
    "stream_clip_update: null runs": lambda L: _cupdate(L, runs=None),
    "stream_clip_update: null contrib": lambda L: _cupdate(L, contrib=None),
    "stream_clip_update: null finals": lambda L: _cupdate(L, finals=None),
    "stream_clip_update: null tails": lambda L: _cupdate(L, tails=None),
    "stream_clip_emit: null state": lambda L: _cemit(L, c=None),
    "stream_clip_emit: 257 transforms": lambda L: _cemit(L, c=clip(num_transform=257)),
    "stream_clip_emit: n_out -1": lambda L: _cemit(L, n_out=-1),
    "stream_clip_emit: n_out = 17": lambda L: _cemit(L, n_out=17),
    "stream_clip_emit: radius -1": lambda L: _cemit(L, radius=-1),
    "stream_clip_emit: radius 2^24 + 1": lambda L: _cemit(L, radius=(1 << 24) + 1),
    "stream_clip_emit: shift -1": lambda L: _cemit(L, shift=-1),
    "stream_clip_emit: n_out = 17, radius -1": lambda L: _cemit(L, n_out=17, radius=-1),
    "stream_clip_emit: null outs": lambda L: _cemit(L, outs=None),
    "stream_clip_emit: null gauss": lambda L: _cemit(L, gauss=None),
    "stream_clip_emit: null out": lambda L: _cemit(L, out=None),
    # ---- mcd_frame_scores
    "frame_scores: null cfg": lambda L: _frames(L, None),
    "frame_scores: null workspace": lambda L: _frames(L, frame_cfg(), ws=None),
    "frame_scores: null out": lambda L: _frames(L, frame_cfg(), out=None),
    "frame_scores: n_clips 0": lambda L: _frames(L, frame_cfg(n_clips=0)),
    "frame_scores: max_frames 0": lambda L: _frames(L, frame_cfg(max_frames=0)),
    "frame_scores: null clip_keys": lambda L: _frames(L, frame_cfg(clip_keys=None)),
    "frame_scores: null gauss_weights": lambda L: _frames(L, frame_cfg(gauss_weights=None)),
    "frame_scores: null scores": lambda L: _frames(L, frame_cfg(), scores=None),
    "frame_scores: null frames": lambda L: _frames(L, frame_cfg(), frames=None),
    "frame_scores: frames_shift 0": lambda L: _frames(L, frame_cfg(frames_shift=0)),
    "frame_scores: gauss_radius -1": lambda L: _frames(L, frame_cfg(gauss_radius=-1)),
    "frame_scores: 10000 frames": lambda L: _frames(L, frame_cfg(max_frames=10000)),
}


def run_case(L, fn):
    rc = int(fn(L))
    return [rc, L.mcd_last_error().decode() if rc != 0 else ""]


def expected(key):
    with open(JSON) as f:
        return json.load(f)[key]


@pytest.mark.parametrize("name", list(CASES))
def test_rejected_before_any_device_call(name):
    code, msg = run_case(_lib.lib(), CASES[name])
    assert code < 0, "the case must be a rejected call"
    assert [code, msg] == expected("host")[name]


def test_scatter_max_empty_output_is_ok_without_a_device_call():
    L = _lib.lib()      # (there is no GPU here: a memset of zero bytes or a launch would not come back as MCD_OK)
    assert _scatter(L, n_rows=0) == 0 and _scatter(L, n_frames=0) == 0
    assert _scatter(L, scores=None, frames=None, row=None, n=0, n_rows=0) == 0      # the inputs may be null when n == 0


def test_table_and_recording_agree():
    assert sorted(expected("host")) == sorted(CASES)


def record(key, results, path=JSON):
    d = {}
    if os.path.exists(path):
        with open(path) as f:
            d = json.load(f)
    # (an existing "how" stays: it also says where the later pairs came from)
    d.setdefault("how", "host: `python tests/test_call_errors_host.py --record` on a machine without a GPU; "
                        "gpu: `python tests/test_call_errors_gpu.py --record` on the MI355X; both with the library built from the commit "
                        "before the call front end (mcd_call.hpp), so the pairs are what callers saw until then")
    d[key] = results
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    L = _lib.lib()
    res = {name: run_case(L, fn) for name, fn in CASES.items()}
    bad = [n for n, (c, _) in res.items() if c >= 0]
    assert not bad, f"not rejected: {bad}"
    record("host", res, sys.argv[2] if len(sys.argv) > 2 else JSON)
    print(f"recorded {len(res)} cases")

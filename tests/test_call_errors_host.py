"""CPU: calls the library rejects before it touches a device, on the entries that take no handle -- each must keep its return
code and its mcd_last_error() text.  The expected pairs are tests/golden/call_errors.json["host"], recorded from the library
before the call front end (mcd_call.hpp) existed:

    python tests/test_call_errors_host.py --record      # rewrites the "host" key; see the file's "how" entry

(the stream_push_group / stream_frame_scores_group pairs: from the library of the last commit that also had per-tick stream
entries, whose state and argument rules they took over one to one -- `--record FILE` writes a copy of the JSON elsewhere)

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
    d["how"] = ("host: `python tests/test_call_errors_host.py --record` on a machine without a GPU; "
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

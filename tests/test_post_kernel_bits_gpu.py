"""GPU: aggregate_kernel and error_maps_kernel (csrc/mcd_post_kernel.hpp) reproduce their recorded output bits.

The two kernels share one statement of which samples a window's score comes from (SelectParams, corrupt_frame, wave_select,
wave_pose_stat).  Every output element is one fixed sequence of floating-point operations -- the rank counting, the sequential sums
in sample order, lerp_two_sided, loss_elem, map_cell's (l0 + l1) / C -- so a regrouping of that text leaves the bits alone and a
digest that moves means an operation order changed: restore the order, do not re-record.  tests/golden/post_kernel_bits.json holds
the sha256 of the float32 output bytes per case, recorded from the library of the commit BEFORE the selection was stated once
(through mcd_aggregate_view and mcd_error_maps, which that commit has unchanged), the sha256 of each case's inputs, and the toolchain
line of the library that produced them; a library built by another compiler may legitimately schedule other fused operations, so the
cases then skip, naming both toolchains.

    python tests/test_post_kernel_bits_gpu.py --record [FILE]      # on the MI355X, with the library of that commit only

Inputs are seeded NumPy arrays (no model): B = 3 windows; the losses of window 1 hold one NaN sample (S = 1: its only one); wherever
S >= 4 samples 0, 1 are copied onto samples 2, 3, losses and poses -- exact ties in every order statistic and in best / worst.
Frames: seg_len 6 with corrupt (3,4,5), 51 cells = a partial wave, and seg_len 8 with corrupt (1,2,4,5,7), 85 cells = a second lap
of the 64 lanes over non-tail frames.  S in {1, 2, 5, 64, 65}; smooth_l1 throughout, l1 and mse at S = 5; at S = 5 also the
cond_mask variant (three different non-tail sets) and, for the maps, the base / trans / affine view of
test_error_maps_gpu.test_view_with_base_trans_affine; S = 8193, one past AGG_LDS_MAX (samples read in place), with B = 2 and
the loss-based strategies only (median_pose is O(S^2) per element).  Digested: loss_agg, pose_agg where the strategy gives one, the
maps.  NaNs: only where the definition puts them (window 1: loss_agg under mean / median / quantile, the map under median /
quantile, and under best / worst when no sample is left)."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402

pytestmark = pytest.mark.gpu

JSON = os.path.join(GOLDEN, "post_kernel_bits.json")
LOSS_STRATEGIES = ("best", "worst", "mean", "median", "quantile:0.3", "quantile:1.0")
STRATEGIES = LOSS_STRATEGIES + ("mean_pose", "median_pose")
FRAMES = {"t6": (6, (3, 4, 5)), "t8": (8, (1, 2, 4, 5, 7))}
MASK_SETS = ([0, 2, 4], [1, 3, 5], [0, 4, 5])      # the corrupt frames of the three windows under cond_mask
# (frames, S, loss_fn, variant)
CASES = ([(f, S, "smooth_l1", "plain") for f in FRAMES for S in (1, 2, 5, 64, 65)]
         + [(f, 5, fn, "plain") for f in FRAMES for fn in ("l1", "mse")]
         + [("t6", 5, "smooth_l1", "mask"), ("t6", 5, "smooth_l1", "view"), ("t6", 8193, "smooth_l1", "plain")])
IDS = [f"{f}-S{S}-{fn}-{v}" for f, S, fn, v in CASES]


def inputs(frames, S, variant):
    """-> dict(loss (B,S), pose (B,S,2,Tx,17), data = dense (B,2,T,17) windows, T, corrupt, mask | None, view | None)."""
    T, corrupt = FRAMES[frames]
    B, Tx = (2 if S > 8192 else 3), len(corrupt)
    rng = np.random.default_rng(100003 * S + 17 * T + {"plain": 0, "mask": 1, "view": 2}[variant])
    loss = np.abs(rng.standard_normal((B, S))).astype(np.float32)
    pose = (rng.standard_normal((B, S, 2, Tx, 17)) * rng.choice([0.05, 0.7, 2.5], (B, S, 1, 1, 1))).astype(np.float32)
    if S >= 4:
        loss[:, 2:4], pose[:, 2:4] = loss[:, 0:2], pose[:, 0:2]
    loss[1, S // 2] = np.nan
    d = dict(loss=loss, pose=pose, T=T, corrupt=list(corrupt), mask=None, view=None, buf=None)
    if variant == "view":      # a frame-major trajectory buffer, exact transforms (multiples of 1/64 and 1/4)
        buf = (np.round(rng.standard_normal((40, 2, 17)) * 64) / 64).astype(np.float32)
        first, trans = np.asarray([0, 7, 34], np.int64), np.asarray([1, 3, 2], np.int32)
        affine = np.asarray([[1, 0, 0, 0, 1, 0], [-1, 0, 0, 0, 1, 0], [0, -1, 0.25, 1, 0, -0.5], [0.5, 0.25, 1, -0.25, 0.5, 2]], np.float32)
        d.update(buf=buf.reshape(-1), view=dict(base=first * 34, trans=trans, affine=affine), data=None)
    else:
        d["data"] = rng.standard_normal((B, 2, T, 17)).astype(np.float32)
    if variant == "mask":
        d["mask"] = np.asarray([sum(1 << t for t in range(T) if t not in s) for s in MASK_SETS], np.int32)
    return d


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(str((a.dtype.str, a.shape)).encode() + a.tobytes())
    return h.hexdigest()


def input_digest(d):
    v = d["view"] or {}
    return _sha(d["loss"], d["pose"], d["data"], d["buf"], d["mask"], v.get("base"), v.get("trans"), v.get("affine"))


def device_aggregate(d, loss_fn, strategy):
    """mcd_aggregate_view on device copies -> (loss_agg (B,), pose_agg (B,2,Tx,17) | None)."""
    import torch
    from maps_ref import _split
    from test_error_maps_gpu import DEV, _cfg, _lib, _ptr, _stream
    L = _lib()
    name, q = _split(strategy)
    B, S, _, Tx, V = d["pose"].shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lo, po, da = dev(d["loss"]), dev(d["pose"]), dev(d["data"])
    agg = torch.full((B,), -7.0, device=DEV)
    pagg = torch.full((B, 2, Tx, V), -7.0, device=DEV) if name in ("best", "worst", "mean_pose", "median_pose") else None
    cfg = _cfg(B, S, d["T"], d["corrupt"], loss_fn)
    view = None
    if d["mask"] is not None:
        m = dev(d["mask"])
        view = L.WindowView(base=None, stride_c=0, stride_t=0, trans=None, affine=None, cond_mask=m.data_ptr())
    L.check(L.lib().mcd_aggregate_view(C.byref(cfg), 2, V, L.AGGR[name], C.c_float(q), _ptr(lo), _ptr(po), _ptr(da),
                                       C.byref(view) if view is not None else None, _ptr(agg), _ptr(pagg), _stream()))
    return agg.cpu().numpy(), None if pagg is None else pagg.cpu().numpy()


def outputs(frames, S, loss_fn, variant):
    """-> {"<strategy>.<output>": float32 array} of the case, and for each the boolean array of the NaNs its definition puts there."""
    from test_error_maps_gpu import device_maps
    d = inputs(frames, S, variant)
    out, nans = {}, {}
    big = S > 8192
    no_sample = S == 1           # window 1's only loss is the NaN: best / worst keep no sample
    win1 = lambda a, on: np.broadcast_to((np.arange(a.shape[0]) == 1).reshape((-1,) + (1,) * (a.ndim - 1)) & on, a.shape)
    if variant != "view":        # (mcd_aggregate_view reads dense windows)
        for s in (LOSS_STRATEGIES if big else STRATEGIES):
            agg, pagg = device_aggregate(d, loss_fn, s)
            out[f"{s}.loss_agg"], nans[f"{s}.loss_agg"] = agg, win1(agg, s in ("mean", "median") or s.startswith("quantile"))
            if pagg is not None:
                out[f"{s}.pose_agg"], nans[f"{s}.pose_agg"] = pagg, win1(pagg, False)
    view = d["view"] if variant == "view" else (dict(cond_mask=d["mask"]) if variant == "mask" else None)
    for s in (LOSS_STRATEGIES if big else STRATEGIES + ("all",)):
        m = device_maps(d["loss"], d["pose"], d["buf"] if variant == "view" else d["data"], d["T"], d["corrupt"], loss_fn, s, view=view)
        out[f"{s}.maps"] = m
        nans[f"{s}.maps"] = win1(m, s == "median" or s.startswith("quantile") or (s in ("best", "worst") and no_sample))
    return d, out, nans


def digest(x):
    assert x.dtype == np.float32
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def library_toolchain():
    from mocodad_amd import _lib
    from mocodad_amd import build as build_mod
    p = build_mod.buildinfo_path(_lib.LIB_PATH)
    return json.load(open(p))["toolchain"] if os.path.exists(p) else None


@pytest.mark.parametrize("frames,S,loss_fn,variant", CASES, ids=IDS)
def test_post_kernel_output_bits(frames, S, loss_fn, variant):
    rec = json.load(open(JSON))
    have = library_toolchain()
    if have != rec["toolchain"]:
        pytest.skip(f"digests recorded with {rec['toolchain']!r}; this library was built by {have!r}: output bits not compared")
    case = IDS[CASES.index((frames, S, loss_fn, variant))]
    d, got, nans = outputs(frames, S, loss_fn, variant)
    assert input_digest(d) == rec["inputs"][case], f"{case}: the seeded inputs are not the recorded ones (the NumPy generator changed?)"
    want = rec["digests"][case]
    assert sorted(got) == sorted(want)
    moved = []
    for name, x in got.items():
        assert np.array_equal(np.isnan(x), nans[name]), f"{case} {name}: NaNs other than the expected ones"      # (a digest of NaNs must not pass)
        assert np.isfinite(x[~nans[name]]).all(), f"{case} {name}: not finite"
        print(f"post-bits | {case} {name} max|x| {np.nanmax(np.abs(x)):.4f} sha256 {digest(x)}")
        if digest(x) != want[name]:
            moved.append(name)
    assert not moved, f"{case}: an operation order of the selection changed for {moved} (restore it; do not re-record)"


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    rec = {"how": "python tests/test_post_kernel_bits_gpu.py --record on the MI355X with the library of the commit before "
                  "aggregate_kernel and error_maps_kernel shared one selection; never from a later library",
           "toolchain": library_toolchain(), "inputs": {}, "digests": {}}
    for case, args in zip(IDS, CASES):
        d, got, nans = outputs(*args)
        for name, x in got.items():
            assert np.array_equal(np.isnan(x), nans[name]), (case, name)
        rec["inputs"][case] = input_digest(d)
        rec["digests"][case] = {name: digest(x) for name, x in got.items()}
        print(f"{case}: {len(got)} outputs", flush=True)
    path = sys.argv[2] if len(sys.argv) > 2 else JSON
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec['digests'])} cases with {rec['toolchain']}")

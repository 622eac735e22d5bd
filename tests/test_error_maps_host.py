"""CPU: the host side of the error maps (ABI 15) -- every argument error of mcd_error_maps, mcd_joint_scatter_max and the two
stream entries comes back as MCD_EINVAL before any device call (the buffers here are HOST memory: a call that got as far as a
launch could not return MCD_EINVAL), the latent module's refusal, and a NumPy model of the joint ring's walk
(stream_joint_scores_group_kernel / stream_flush_kernel<17>, restated below) held to a brute-force per-row maximum over seeded
random interleavings with slot reuse, ring wrap and groups of K ticks.  The GPU tests (test_stream_joint_gpu.py) hold the kernels
to the dataset path bit for bit."""
import ctypes

import numpy as np
import pytest

from helpers import make_args
from mocodad_amd import _lib
from mocodad_amd.stream import TrackTable, pack_ticks

EINVAL = -1
BUF = (ctypes.c_float * 64)()
P = ctypes.cast(BUF, ctypes.c_void_p)


def _L():
    return _lib.lib()


def _cfg(B=2, S=2, T=6, n_cond=3, n_corrupt=3, corrupt=None):
    c = _lib.ScoreCfg(n_windows=B, n_samples=S, noise_steps=2, seg_len=T, n_cond=n_cond, n_corrupt=n_corrupt, loss_fn=0)
    for i, v in enumerate(range(T - n_corrupt, T) if corrupt is None else corrupt):
        if i < 32:
            c.corrupt_idx[i] = v
    return c


def test_abi_version_is_15():
    assert _lib.ABI_VERSION == 15
    L = _L()
    assert L.mcd_abi_version() == 15
    for name in ("mcd_error_maps", "mcd_joint_scatter_max", "mcd_stream_joint_scores_group", "mcd_stream_joint_flush"):
        assert name in _lib.EXPORTS and hasattr(L, name)


# ---------------------------------------------------------------- mcd_error_maps
def _maps(cfg, strategy="best", q=0.0, loss=P, pose=P, data=P, view=None, out=P, C=2, V=17):
    L = _L()
    rc = L.mcd_error_maps(ctypes.byref(cfg) if cfg is not None else None, C, V, _lib.AGGR[strategy] if isinstance(strategy, str) else strategy,
                          ctypes.c_float(q), loss, pose, data, ctypes.byref(view) if view is not None else None, out, None)
    return rc, L.mcd_last_error()


def _view(mask=None, trans=None, affine=None, base=None):
    return _lib.WindowView(base=base, stride_c=17, stride_t=34, trans=trans, affine=affine, cond_mask=mask)


@pytest.mark.parametrize("kw,word", [
    (dict(out=None), b"null"), (dict(pose=None), b"null"), (dict(data=None), b"null"), (dict(loss=None), b"null"),
    (dict(loss=None, strategy="median"), b"null"), (dict(loss=None, strategy="quantile", q=0.5), b"null"),
    (dict(cfg=None), b"null"),
    (dict(cfg=_cfg(S=0)), b"n_samples"), (dict(cfg=_cfg(S=-3)), b"n_samples"),
    (dict(cfg=_cfg(B=-1)), b"n_windows"),
    (dict(strategy=8), b"aggregation"), (dict(strategy=-1), b"aggregation"),
    (dict(strategy="quantile", q=1.5), b"quantile"), (dict(strategy="quantile", q=float("nan")), b"quantile"),
    (dict(cfg=_cfg(T=33, n_cond=30, n_corrupt=3)), b"seg_len"), (dict(cfg=_cfg(n_corrupt=0, n_cond=6)), b"n_corrupt"),
    (dict(cfg=_cfg(n_corrupt=7, n_cond=0)), b"n_corrupt"),
    (dict(cfg=_cfg(corrupt=[3, 4, 6])), b"corrupt_idx"), (dict(cfg=_cfg(corrupt=[-1, 4, 5])), b"corrupt_idx"),
    (dict(C=3), b"num_coords"), (dict(V=18), b"n_joints"),
    # a mask carries n_cond = seg_len - n_corrupt set bits: a call whose two counts do not add up to seg_len names another bit count
    (dict(cfg=_cfg(n_cond=2, n_corrupt=3), view=_view(mask=P)), b"mask"),
    (dict(cfg=_cfg(n_cond=4, n_corrupt=3), view=_view(mask=P)), b"mask"),
    (dict(view=_view(trans=P)), b"affine"),
])
def test_error_maps_rejects_before_any_device_call(kw, word):
    kw = dict(kw)
    cfg = kw.pop("cfg", _cfg())
    rc, msg = _maps(cfg, **kw)
    assert rc == EINVAL, (rc, msg)
    assert word in msg, msg


def test_error_maps_optional_loss_and_zero_windows():
    # zero windows: MCD_OK, nothing launched (there is no GPU here: a launch would be MCD_EDEVICE), whatever the pointers say
    for strat in ("all", "best", "mean", "median_pose"):
        assert _maps(_cfg(B=0), strategy=strat)[0] == 0
    # a view with a base is accepted (unlike mcd_aggregate_view): with zero windows the call is MCD_OK
    assert _maps(_cfg(B=0), view=_view(base=P, trans=P, affine=P))[0] == 0
    assert _maps(_cfg(B=0, n_cond=3, n_corrupt=3), view=_view(mask=P))[0] == 0


# ---------------------------------------------------------------- mcd_joint_scatter_max
@pytest.mark.parametrize("kw,word", [
    (dict(out=None), b"null"), (dict(maps=None), b"null"), (dict(frames=None), b"null"), (dict(row=None), b"null"),
    (dict(n=-1), b"n"), (dict(Tx=0), b"n_corrupt"), (dict(Tx=33), b"n_corrupt"), (dict(n_rows=-1), b"n_rows"), (dict(n_frames=-2), b"n_frames")])
def test_joint_scatter_max_rejects_before_any_device_call(kw, word):
    a = dict(maps=P, frames=P, row=P, n=2, Tx=3, n_rows=2, n_frames=4, out=P)
    a.update(kw)
    L = _L()
    rc = L.mcd_joint_scatter_max(a["maps"], a["frames"], a["row"], a["n"], a["Tx"], a["n_rows"], a["n_frames"], a["out"], None)
    assert rc == EINVAL and word in L.mcd_last_error(), (rc, L.mcd_last_error())


# ---------------------------------------------------------------- the stream entries
def _state(n_slots=4, L=8, T=6, nt=2, ring=P, fs=P):
    return _lib.StreamState(ring=ring, frame_scores=fs, n_slots=n_slots, ring_len=L, seg_len=T, num_transform=nt)


JS = _lib.StreamJointState(joint_scores=P)


@pytest.mark.parametrize("kw,word", [
    (dict(maps=None), b"null"), (dict(win=None), b"null"), (dict(out=None), b"null"), (dict(cfg=None), b"null"),
    (dict(js=None), b"joint"), (dict(js=_lib.StreamJointState(joint_scores=None)), b"joint"),
    (dict(st=None), b"stream state"), (dict(st=_state(ring=None)), b"stream state"),
    (dict(st=_state(T=33, L=40), cfg=_cfg(T=33, n_cond=30)), b"seg_len"),
    (dict(st=_state(L=5)), b"ring_len"),
    (dict(cfg=_cfg(T=7, n_cond=4)), b"seg_len"),
    (dict(cfg=_cfg(n_cond=2)), b"partition"), (dict(cfg=_cfg(corrupt=[3, 4, 4])), b"corrupt_idx"), (dict(cfg=_cfg(corrupt=[3, 4, 9])), b"corrupt_idx"),
    (dict(n=-1), b"n_windows"),
    (dict(n=4 * (8 - 6 + 1) + 1), b"ring_len - seg_len + 1"),      # beyond n_slots * (ring_len - seg_len + 1)
])
def test_stream_joint_scores_group_rejects_before_any_device_call(kw, word):
    a = dict(st=_state(), js=JS, maps=P, win=P, n=2, cfg=_cfg(), out=P)
    a.update(kw)
    L = _L()
    by = lambda x: ctypes.byref(x) if x is not None else None
    rc = L.mcd_stream_joint_scores_group(by(a["st"]), by(a["js"]), a["maps"], a["win"], a["n"], by(a["cfg"]), a["out"], None)
    assert rc == EINVAL and word in L.mcd_last_error(), (rc, L.mcd_last_error())


@pytest.mark.parametrize("kw,word", [
    (dict(win=None), b"null"), (dict(out=None), b"null"), (dict(js=None), b"joint"), (dict(st=None), b"stream state"),
    (dict(st=_state(T=33, L=40)), b"seg_len"), (dict(n=-1), b"n_slots"), (dict(n=5), b"n_slots")])
def test_stream_joint_flush_rejects_before_any_device_call(kw, word):
    a = dict(st=_state(), js=JS, win=P, n=2, out=P)
    a.update(kw)
    L = _L()
    by = lambda x: ctypes.byref(x) if x is not None else None
    rc = L.mcd_stream_joint_flush(by(a["st"]), by(a["js"]), a["win"], a["n"], a["out"], None)
    assert rc == EINVAL and word in L.mcd_last_error(), (rc, L.mcd_last_error())


def test_stream_joint_entries_accept_empty_calls():
    L = _L()
    st, cfg = _state(), _cfg()
    assert L.mcd_stream_joint_scores_group(ctypes.byref(st), ctypes.byref(JS), None, None, 0, ctypes.byref(cfg), None, None) == 0
    assert L.mcd_stream_joint_flush(ctypes.byref(st), ctypes.byref(JS), None, 0, None, None) == 0


# ---------------------------------------------------------------- the latent module
def test_latent_module_names_the_reason():
    import latent_ref as R
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    _, _, cfg, _ = R.load_fixture("A_benign")
    m = MoCoDADlatent(make_args(cfg))
    with pytest.raises(NotImplementedError, match="a latent has no joints"):
        m.forward([None, None, None, None], return_maps=True)      # (refused before the inputs, the device or a scorer are touched)


def test_return_maps_is_keyword_only():
    import inspect
    from mocodad_amd.models.mocodad import MoCoDAD
    p = inspect.signature(MoCoDAD.forward).parameters["return_maps"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


# ---------------------------------------------------------------- NumPy model of the joint ring's walk
def walk_group(ring, win, maps, tx_of, T, nt):
    """stream_joint_scores_group_kernel: ring (n_slots, nt, L, 17) updated in place, win (n, 5) sorted by slot then row, maps
    (nt * n, Tx, 17) -> finals (n, nt, 17)."""
    n, L = len(win), ring.shape[2]
    final = np.full((n, nt, 17), np.nan, np.float32)
    for q in range(n):
        slot, r_last, pos0, ne, w = (int(x) for x in win[q])
        first = r_last - T + 1
        for t in range(nt):
            m = maps[pos0 + t * ne]
            for k in range(T - 1, -1, -1):
                tx = tx_of[k]
                val = np.fmax(m[tx], np.float32(0)) if tx >= 0 else np.zeros(17, np.float32)
                c = (first + k) % L
                ring[slot, t, c] = val if (first == 0 or k == T - 1) else np.fmax(ring[slot, t, c], val)
                if k == 0:
                    final[w, t] = ring[slot, t, c]
    return final


def flush_model(ring, win, T):
    """stream_flush_kernel<17>: win (n, 2) [slot, r_last] -> (n, T - 1, nt, 17)."""
    L = ring.shape[2]
    return np.stack([np.stack([ring[s, :, (r - T + 2 + k) % L] for k in range(T - 1)]) for s, r in win.tolist()]) if len(win) else \
        np.zeros((0, T - 1, ring.shape[1], 17), np.float32)


@pytest.mark.parametrize("seed,K,max_tracks,tx_of", [
    (0, 1, 3, [-1, -1, -1, 0, 1, 2]),          # ring_len = seg_len: one tick per group; tail forecast
    (1, 3, 3, [-1, -1, -1, 0, 1, 2]),          # groups of up to 3 ticks, ring wrap every 8 rows
    (2, 3, 2, [-1, 0, -1, 1, -1, 2]),          # in-between forecast frames
    (3, 4, 4, [0, 1, 2, 3, 4, 5]),             # every row forecast (no_condition)
    (4, 2, 3, [0, 1, 2, -1, -1, -1]),          # head forecast: the window ending at a row never forecasts it
])
def test_walk_model_matches_the_per_row_maximum(seed, K, max_tracks, tx_of):
    rng = np.random.default_rng(seed)
    T, nt, Tx = 6, 2, sum(t >= 0 for t in tx_of)
    L = T + K - 1
    table = TrackTable(max_tracks, T, L, max_idle=2)
    ring = rng.standard_normal((max_tracks, nt, L, 17)).astype(np.float32)      # (garbage: a cell must be initialised before it is read)
    persons = list(range(max_tracks))          # (as many keys as slots: a call always fits; a key that pauses for two ticks is
    #                                            closed by max_idle and comes back as a new track, on whatever slot is free)
    inst = {}                  # slot -> instance id of the track that owns it
    rows = {}                  # instance -> {row: running maximum (nt, 17)}
    n_inst = checked = reused = wrapped = 0
    seen_slots = set()
    frame = 0
    for _ in range(120):
        ticks = []
        for _k in range(int(rng.integers(1, K + 2))):
            frame += 1
            live = [p for p in persons if rng.random() < 0.75]
            ticks.append(([(1, 1, p) for p in live], [frame] * len(live)))
        groups, planned = pack_ticks(table, ticks, nt)
        table.adopt(planned)
        for g in groups:
            # 1. the idle closures of the group come first (PoseStream._run_group): their pending rows
            tails = flush_model(ring, g.closed.win, T)
            for (slot, r_last), tail in zip(g.closed.win.tolist(), tails):
                i = inst[slot]
                for k in range(T - 1):
                    np.testing.assert_array_equal(tail[k], rows[i][r_last - T + 2 + k])
                    checked += 1
            # 2. the brute force: every window of the group into every row it forecasts
            maps = rng.standard_normal((nt * g.n_windows, Tx, 17)).astype(np.float32) * 2
            maps[rng.random(maps.shape) < 0.02] = np.nan
            expect = {}
            for ti, plan in enumerate(g.plans):
                for slot, r, j in plan.desc.tolist():
                    if r == 0:
                        reused += slot in seen_slots
                        seen_slots.add(slot)
                        inst[slot] = n_inst
                        rows[n_inst] = {}
                        n_inst += 1
                    rows[inst[slot]][r] = np.zeros((nt, 17), np.float32)
                    if j < 0:
                        continue
                    w0, ne = int(g.offsets[ti]), plan.n_emit
                    for t in range(nt):
                        m = maps[nt * w0 + t * ne + j]
                        for k in range(T):
                            if tx_of[k] >= 0:
                                cell = rows[inst[slot]][r - T + 1 + k]
                                cell[t] = np.fmax(cell[t], np.fmax(m[tx_of[k]], np.float32(0)))
                    expect[w0 + j] = rows[inst[slot]][r - T + 1].copy()      # final: no later window covers the oldest row
                    wrapped += r >= L
            final = walk_group(ring, g.win, maps, tx_of, T, nt)
            assert len(expect) == g.n_windows
            for w, e in expect.items():
                np.testing.assert_array_equal(final[w], e)
                checked += 1
    assert checked > 200 and reused > 0 and wrapped > 0, (checked, reused, wrapped)

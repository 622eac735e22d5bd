"""GPU: table rows "the host table cannot produce" touch nothing.  The stream's group and flush entries are called through the C
ABI with hand-built tables -- no model, no trajectory kernel -- on a small state (n_slots 3, seg_len 4, ring_len 6: three rows per
track and group; num_transform 2; condition frames (0, 2), corrupt frames (1, 3); S = 3 samples; aggregation best, forecast method
median, spread mean).  Every ring and output comes from tests/guarded.py: between guard bands, its interior the all-ones pattern.

  call A: a well-formed group.  Track 0 (slot 0) receives rows 3, 4, 5 -- three ticks, three windows, so the walk over a track's
          windows has more than one -- and track 1 (slot 1) row 3 in the first of those ticks.  Slot 2 never holds a track.
  call B: the same rows plus malformed ones, one violated condition per malformed row.  A group of this state holds at most nine
          rows (n_windows <= n <= n_slots * (ring_len - seg_len + 1)), so the conditions are spread over two B calls, and the
          flushes (n <= n_slots) take one malformed closed-track row at a time.

Asserted: the rings after B equal the rings after A bit for bit, the output rows of the well-formed windows are equal, every
output row owned by a malformed row still holds the sentinel, and no guard byte changed.

Each malformed row is checked against the kernels' own predicates (restated below) BEFORE it runs: it must be skipped by every
thread that reads it.  Two consequences of those predicates shape the tables:
  * a pushed-row descriptor whose slot and row are valid always writes its pose row (and zeroes its frame-score cells); only its
    WINDOW part can be malformed.  Such descriptors here repeat the (slot, row, raw values) of a row the call writes anyway, so the
    rings stay A's, and what is asserted is that no base / transform descriptor appears at their batch position.
  * the walk over a track's windows tests the batch position per transform, pos0 + t * ne < n_win, and the forecast kernels read
    transform 0 only: a window row with pos0 + (nt - 1) * ne = n_win is a VALID row for transform 0.  That condition is therefore
    given to the descriptors, whose predicate has exactly this form, and the window tables get the bound every transform refuses,
    pos0 = n_win."""
import ctypes as C

import pytest
import torch

from guarded import GuardedTorch, unwritten
from mocodad_amd import _lib

pytestmark = pytest.mark.gpu

N_SLOTS, SEG, L, NT, TX, S = 3, 4, 6, 2, 2, 3
COND, CORRUPT = (0, 2), (1, 3)
AGGR_BEST, METHOD_MEDIAN, SPREAD_MEAN = 1, 2, 1
VID_W, VID_H = 640.0, 360.0
PEND = SEG - 1
DEV = "cuda:0"

# the well-formed group: descriptors [slot, r, pos0, ne], windows [slot, r_last, pos0, ne, w] sorted by slot, then row.  Ticks:
# (slot 0 row 3, slot 1 row 3) -> batch positions 0, 1 (+ ne = 2 per transform), then slot 0 row 4 at 4, then slot 0 row 5 at 6
DESC_A = [[0, 3, 0, 2], [0, 4, 4, 1], [0, 5, 6, 1], [1, 3, 1, 2]]
WIN_A = [[0, 3, 0, 2, 0], [0, 4, 4, 1, 2], [0, 5, 6, 1, 3], [1, 3, 1, 2, 1]]
CLOSED_A = [[0, 5], [1, 3]]
SETUP = [[s, r, -1, 0] for s in (0, 1) for r in range(SEG - 1)]      # rows 0 .. 2 of both tracks: no window yet


# ---- the kernels' predicates, restated
def desc_touches_nothing(d):
    return d[0] < 0 or d[0] >= N_SLOTS or d[1] < 0


def desc_has_no_window(d, n_win):
    return d[2] < 0 or d[3] < 1 or d[1] < SEG - 1 or d[2] + (NT - 1) * d[3] >= n_win


def win_skipped(w, t, n_win, n_windows):
    slot, r_last, pos0, ne, row = w
    return (slot < 0 or slot >= N_SLOTS or r_last < SEG - 1 or pos0 < 0 or ne < 1 or pos0 + t * ne >= n_win or row < 0
            or row >= n_windows)


def closed_skipped(c):
    return c[0] < 0 or c[0] >= N_SLOTS or c[1] < SEG - 1


def tables_b(which):
    """-> (desc, malformed descriptor indices that keep a pose, windows, malformed window indices) of B call `which`"""
    if which == 1:
        n_win = 9 * NT
        desc = [[-1, 3, 8, 1],                      # slot -1
                [0, 3, 0, 2],
                [0, 4, 4, 1],
                [0, 4, 16, 0],                      # ne 0            (the pose of slot 0 row 4 once more)
                [0, 5, 6, 1],
                [0, 5, n_win - 1, 1],               # pos0 + (nt - 1) ne = n_win   (the pose of slot 0 row 5 once more)
                [1, 3, 1, 2],
                [2, -1, 9, 1],                      # r -1
                [N_SLOTS, 3, 10, 1]]                # slot = n_slots
        keeps_pose = [3, 5]
        win = [[-1, 3, 8, 1, 4],                    # slot -1
               [0, 3, 0, 2, 0], [0, 4, 4, 1, 2], [0, 5, 6, 1, 3], [1, 3, 1, 2, 1],
               [2, SEG - 2, 9, 1, 5],               # r_last = seg_len - 2
               [2, 3, -1, 1, 6],                    # pos0 -1
               [2, 3, 10, 0, 7],                    # ne 0
               [N_SLOTS, 3, 11, 1, 8]]              # slot = n_slots
    else:
        n_win = 8 * NT
        desc = [[-1, 3, 8, 1],                      # slot -1
                [0, SEG - 2, 9, 1],                 # r = seg_len - 2 with a batch position   (the pose of slot 0 row 2 once more)
                [0, 3, 0, 2],
                [0, 3, -1, 2],                      # pos0 -1         (the pose of slot 0 row 3 once more)
                [0, 4, 4, 1], [0, 5, 6, 1], [1, 3, 1, 2],
                [2, -1, 10, 1],                     # r -1
                [N_SLOTS, 3, 11, 1]]                # slot = n_slots
        keeps_pose = [1, 3]
        win = [[0, 3, 0, 2, 0],
               [0, 4, 8, 0, 5],                     # a malformed row (ne 0) with a valid track's slot, between that track's rows
               [0, 4, 4, 1, 2], [0, 5, 6, 1, 3], [1, 3, 1, 2, 1],
               [2, 3, n_win, 1, 4],                 # pos0 = n_win
               [2, 3, 9, 1, -1],                    # w -1
               [2, 3, 10, 1, 8]]                    # w = n_windows
    bad_win = [i for i, w in enumerate(win) if w not in WIN_A]
    return desc, keeps_pose, win, bad_win


def check_tables(desc, keeps_pose, win, bad_win):
    n, n_windows = len(desc), len(win)
    n_win = n_windows * NT
    assert n_windows <= n <= N_SLOTS * (L - SEG + 1)
    assert [w[0] for w in win] == sorted(w[0] for w in win) and [d[0] for d in desc] == sorted(d[0] for d in desc)
    for i, d in enumerate(desc):
        if d in DESC_A:
            assert not desc_touches_nothing(d) and not desc_has_no_window(d, n_win)
        elif i in keeps_pose:
            assert not desc_touches_nothing(d) and desc_has_no_window(d, n_win)
            assert 0 <= d[1] < L and any(e[:2] == d[:2] for e in DESC_A + SETUP)
        else:
            assert desc_touches_nothing(d)
    for i, w in enumerate(win):
        for t in range(NT):
            assert win_skipped(w, t, n_win, n_windows) == (i in bad_win), (w, t)
        if i not in bad_win:      # what a valid row indexes lies inside the rings and the batch
            assert w[1] - SEG + 1 >= 0 and w[2] + (NT - 1) * w[3] < n_win
    assert sorted(w[4] for i, w in enumerate(win) if i not in bad_win) == list(range(len(WIN_A)))


def _i32(rows, width):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(-1, width).contiguous()


def _cfg():
    c = _lib.ScoreCfg()
    c.n_windows, c.n_samples, c.noise_steps, c.seg_len, c.n_cond, c.n_corrupt, c.loss_fn = 0, S, 2, SEG, len(COND), TX, 0
    for i, v in enumerate(COND):
        c.cond_idx[i] = v
    for i, v in enumerate(CORRUPT):
        c.corrupt_idx[i] = v
    return c


def _inputs():
    """The values the group reads, by (slot, row) and by batch position, so that A and B hand the well-formed rows the same ones."""
    gen = torch.Generator().manual_seed(11)
    n_pos = N_SLOTS * (L - SEG + 1) * NT
    return {"raw": torch.rand(N_SLOTS + 2, L, 34, generator=gen) * 280 + 20,      # [slot + 1, r]: slot -1 .. n_slots
            "scores": torch.rand(n_pos, generator=gen) + 0.1,
            "maps": torch.rand(n_pos, TX, 17, generator=gen) + 0.1,
            "loss_all": torch.rand(n_pos, S, generator=gen) + 0.1,
            "poses_all": torch.randn(n_pos, S, 2, TX, 17, generator=gen)}


def run_group(desc, win, closed_list):
    """One state from nothing: the setup rows, the group, the flushes of every entry of closed_list -> every ring and output."""
    L_ = _lib.lib()
    g = GuardedTorch()
    new = lambda *shape, dtype=torch.float32: g.empty(*shape, dtype=dtype, device=DEV)
    inp = _inputs()
    ring, fs, js = new(N_SLOTS, 2 * L, 34), new(N_SLOTS, NT, L), new(N_SLOTS, NT, L, 17)
    fc, obs = new(N_SLOTS, L, TX, 34), new(N_SLOTS, L, 34)
    st = _lib.StreamState(ring=ring.data_ptr(), frame_scores=fs.data_ptr(), n_slots=N_SLOTS, ring_len=L, seg_len=SEG, num_transform=NT)
    jst = _lib.StreamJointState(joint_scores=js.data_ptr())
    fst = _lib.StreamForecastState(forecast=fc.data_ptr(), observed=obs.data_ptr(), n_corrupt=TX)
    cfg = _cfg()
    raw_of = lambda rows: torch.stack([inp["raw"][d[0] + 1, d[1] % L] for d in rows]).to(DEV).contiguous()
    out = {}

    def forecast_outs(rows, prefix):
        o = {"expected": new(rows, 34), "norm": new(rows, 34), "observed": new(rows, 34), "count": new(rows, dtype=torch.int32),
             "spread": new(rows)}
        out.update({prefix + k: v for k, v in o.items()})
        return [o[k].data_ptr() for k in ("expected", "norm", "observed", "count", "spread")]

    # rows 0 .. 2 of both tracks: poses and raw rows only
    d0, r0 = _i32(SETUP, 4), raw_of(SETUP)
    _lib.check(L_.mcd_stream_push_group(C.byref(st), r0.data_ptr(), d0.data_ptr(), len(SETUP), 0, VID_W, VID_H, None, None, None, None, None))
    _lib.check(L_.mcd_stream_forecast_group(C.byref(st), C.byref(fst), r0.data_ptr(), d0.data_ptr(), len(SETUP), None, None, None, 0,
                                            C.byref(cfg), AGGR_BEST, METHOD_MEDIAN, SPREAD_MEAN, VID_W, VID_H, None, None, None, None,
                                            None, None, None, None))
    # the group
    n, n_windows = len(desc), len(win)
    n_win = n_windows * NT
    d, w, raw = _i32(desc, 4), _i32(win, 5), raw_of(desc)
    dev_in = {k: inp[k][:n_win].to(DEV).contiguous() for k in ("scores", "maps", "loss_all", "poses_all")}
    out["base"], out["trans"] = new(n_win, dtype=torch.int64), new(n_win, dtype=torch.int32)
    out["final"], out["joint_final"] = new(n_windows, NT), new(n_windows, NT, 17)
    _lib.check(L_.mcd_stream_push_group(C.byref(st), raw.data_ptr(), d.data_ptr(), n, n_windows, VID_W, VID_H, None, None,
                                        out["base"].data_ptr(), out["trans"].data_ptr(), None))
    _lib.check(L_.mcd_stream_frame_scores_group(C.byref(st), dev_in["scores"].data_ptr(), w.data_ptr(), n_windows,
                                                out["final"].data_ptr(), None))
    _lib.check(L_.mcd_stream_joint_scores_group(C.byref(st), C.byref(jst), dev_in["maps"].data_ptr(), w.data_ptr(), n_windows,
                                                C.byref(cfg), out["joint_final"].data_ptr(), None))
    _lib.check(L_.mcd_stream_forecast_group(C.byref(st), C.byref(fst), raw.data_ptr(), d.data_ptr(), n, dev_in["loss_all"].data_ptr(),
                                            dev_in["poses_all"].data_ptr(), w.data_ptr(), n_windows, C.byref(cfg), AGGR_BEST,
                                            METHOD_MEDIAN, SPREAD_MEAN, VID_W, VID_H, None, None, *forecast_outs(n_windows, "fc_"), None))
    # the flushes
    for i, closed in enumerate(closed_list):
        c, nc = _i32(closed, 2), len(closed)
        out[f"tails{i}"], out[f"joint_tails{i}"] = new(nc, PEND, NT), new(nc, PEND, NT, 17)
        _lib.check(L_.mcd_stream_flush(C.byref(st), c.data_ptr(), nc, out[f"tails{i}"].data_ptr(), None))
        _lib.check(L_.mcd_stream_joint_flush(C.byref(st), C.byref(jst), c.data_ptr(), nc, out[f"joint_tails{i}"].data_ptr(), None))
        _lib.check(L_.mcd_stream_forecast_flush(C.byref(st), C.byref(fst), c.data_ptr(), nc, C.byref(cfg), METHOD_MEDIAN, SPREAD_MEAN,
                                                VID_W, VID_H, None, None, *forecast_outs(nc * PEND, f"fct{i}_"), None))
    torch.cuda.synchronize()
    g.check()
    out.update(ring=ring, fs=fs, js=js, fc=fc, obs=obs)
    return out


RINGS = ("ring", "fs", "js", "fc", "obs")
FC = ("expected", "norm", "observed", "count", "spread")


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def untouched(t):
    return unwritten(t) == t.numel()


@pytest.fixture(scope="module")
def call_a():
    check_tables(DESC_A, [], WIN_A, [])
    assert not any(closed_skipped(c) for c in CLOSED_A)
    a = run_group(DESC_A, WIN_A, [CLOSED_A])
    # the well-formed call itself: every output written, the rings written where the two tracks live and nowhere in slot 2
    for k in ("base", "trans", "final", "joint_final", "tails0", "joint_tails0") + tuple("fc_" + f for f in FC) + tuple("fct0_" + f for f in FC):
        assert unwritten(a[k]) == 0, k
    assert a["trans"].tolist() == [0, 0, 1, 1, 0, 1, 0, 1]
    # windows that forecast the row, corrupt frames (1, 3): final rows 0, 0, 1, 2 of the windows; pending rows 3 .. 5 and 1 .. 3
    assert a["fc_count"].tolist() == [0, 0, 1, 1] and a["fct0_count"].tolist() == [2, 1, 1, 1, 0, 1]
    for k in RINGS:
        assert untouched(a[k][2]) and not untouched(a[k][:2]), k
    return a


@pytest.mark.parametrize("which", [1, 2])
def test_malformed_group_rows_touch_nothing(call_a, which):
    desc, keeps_pose, win, bad_win = tables_b(which)
    check_tables(desc, keeps_pose, win, bad_win)
    b = run_group(desc, win, [])
    for k in RINGS:
        assert same(call_a[k], b[k]), k
    n_win_a = len(WIN_A) * NT
    for k in ("base", "trans"):      # batch positions: the well-formed rows' are A's, nothing appears behind them
        assert same(call_a[k], b[k][:n_win_a]) and untouched(b[k][n_win_a:]), k
    good = [w[4] for i, w in enumerate(win) if i not in bad_win]
    rest = [r for r in range(len(win)) if r not in good]
    for k in ("final", "joint_final") + tuple("fc_" + f for f in FC):
        assert same(call_a[k], b[k][:len(WIN_A)]), k
        assert untouched(b[k][rest]), k


@pytest.mark.parametrize("row", [[-1, 5], [N_SLOTS, 5], [2, SEG - 2]], ids=["slot -1", "slot = n_slots", "r_last = seg_len - 2"])
def test_malformed_closed_track_rows_touch_nothing(call_a, row):
    assert closed_skipped(row)
    b = run_group(DESC_A, WIN_A, [CLOSED_A + [row]])
    for k in RINGS:
        assert same(call_a[k], b[k]), k
    nc = len(CLOSED_A)
    for k in ("tails0", "joint_tails0"):
        assert same(call_a[k], b[k][:nc]) and untouched(b[k][nc:]), k
    for f in FC:
        k = "fct0_" + f
        assert same(call_a[k], b[k][:nc * PEND]) and untouched(b[k][nc * PEND:]), k

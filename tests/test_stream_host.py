"""Host half of the live pose stream (mocodad_amd/stream.py: TrackTable) without a GPU: replaying the fixture's trajectory files
in frame order emits exactly the reference's windows (tests/golden/dataset_golden.npz: meta / frames of utils/preprocessing.py),
short tracks emit nothing, misuse is rejected by name, and the ring offsets address the right rows of a NumPy model of the
mirrored ring."""
import collections

import numpy as np
import pytest

from dataset_spec import DATASET, load_dataset_golden
from mocodad_amd.data import trajectories as T
from mocodad_amd.stream import ROW, TrackTable, ticks_by_frame

SEG_LEN = 6


def _split_tracks(split):
    files = T.list_trajectory_files(T.trajectories_root(DATASET, split))
    return [(key,) + T.read_trajectory_csv(path) for key, path in files]


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("split, meta_name, frames_name, n_windows", [("test", "meta", "frames", 283),
                                                                      ("validation", "meta_val", "frames_val", 76)])
def test_replay_emits_exactly_the_reference_windows(split, meta_name, frames_name, n_windows, per_clip):
    g = load_dataset_golden()
    tracks = _split_tracks(split)
    if split == "test":
        assert len(tracks) == 22 and sum(len(f) >= SEG_LEN for _, f, _ in tracks) == 14
    table = TrackTable(max_tracks=len(tracks), seg_len=SEG_LEN)
    got, emitted = {}, []
    n_ticks = 0
    for _, keys, fids, _ in ticks_by_frame(tracks, per_clip):
        plan = table.push(keys, fids)
        n_ticks += 1
        assert plan.desc.shape == (len(keys), 3) and plan.n_emit <= len(keys)
        assert sorted(j for j in plan.desc[:, 2] if j >= 0) == list(range(plan.n_emit))
        for m, f in zip(plan.meta, plan.frames):
            m = tuple(int(v) for v in m)
            emitted.append(m)
            got[m] = f
    groups = {((k[:2] if per_clip else ()), int(x)) for k, f, _ in tracks for x in f}
    assert n_ticks == len(groups)
    if split == "test" and per_clip:
        assert n_ticks == 146
    want = {tuple(int(v) for v in m): f for m, f in zip(g[meta_name], g[frames_name])}
    assert len(emitted) == n_windows == len(g[meta_name])
    assert collections.Counter(emitted) == collections.Counter(tuple(int(v) for v in m) for m in g[meta_name])     # as a multiset
    for m, f in want.items():
        assert np.array_equal(got[m], f), m
    if split == "test":
        assert any((np.diff(f) > 1).any() for f in got.values())         # frame gaps reach the windows
    # closing: the kept tracks hand back their seg_len - 1 pending rows, the short ones nothing; every slot comes back
    lens = {k: len(f) for k, f, _ in tracks}
    last = {k: f[-(SEG_LEN - 1):] for k, f, _ in tracks}
    plan = table.close([k for k, _, _ in tracks])
    assert sorted(plan.keys) == sorted(k for k, n in lens.items() if n >= SEG_LEN)
    for k, f in zip(plan.keys, plan.frames):
        assert np.array_equal(f, last[k])
    assert len(table) == 0 and table.free_slots == len(tracks)


def test_short_tracks_emit_nothing_and_free_their_slot():
    table = TrackTable(max_tracks=2, seg_len=SEG_LEN)
    for f in range(1, SEG_LEN):
        plan = table.push([(1, 1, 7)], [f])
        assert plan.n_emit == 0 and plan.desc[0].tolist() == [0, f - 1, -1]
    assert table.free_slots == 1
    closed = table.close([(1, 1, 7)])
    assert len(closed) == 0 and closed.win.shape == (0, 2) and closed.frames.shape == (0, SEG_LEN - 1)
    assert table.free_slots == 2 and (1, 1, 7) not in table


def test_misuse_is_rejected_with_the_key_in_the_message():
    table = TrackTable(max_tracks=2, seg_len=SEG_LEN)
    table.push([(1, 1, 1), (1, 1, 2)], [1, 1])
    with pytest.raises(RuntimeError, match=r"max_tracks = 2 exhausted.*\(1, 2, 3\)"):
        table.push([(1, 1, 1), (1, 2, 3)], [2, 2])
    assert table.rows[:2].tolist() == [1, 1] and table.tick == 1           # a rejected tick changes nothing
    with pytest.raises(ValueError, match=r"\(1, 1, 2\) has two rows in one tick"):
        table.push([(1, 1, 2), (1, 1, 1), (1, 1, 2)], [2, 2, 3])
    assert table.rows[:2].tolist() == [1, 1]
    table.close([(1, 1, 2)])
    with pytest.raises(ValueError, match=r"\(1, 1, 2\) was closed"):
        table.push([(1, 1, 2)], [3])
    with pytest.raises(KeyError, match=r"\(1, 1, 2\) is not open"):
        table.close([(1, 1, 2)])
    table.reopen([(1, 1, 2)])
    plan = table.push([(1, 1, 2)], [3])
    assert plan.desc[0].tolist() == [1, 0, -1]                              # a new track: row 0 again
    with pytest.raises(ValueError, match="ring_len"):
        TrackTable(max_tracks=2, seg_len=SEG_LEN, ring_len=SEG_LEN - 1)


def test_max_idle_closes_idle_tracks_at_the_start_of_the_next_push():
    table = TrackTable(max_tracks=2, seg_len=3, max_idle=2)
    a, b, c = (1, 1, 1), (1, 1, 2), (1, 1, 3)
    for f in (1, 2, 3):
        plan = table.push([a, b], [f, f])
    assert plan.n_emit == 2
    assert len(table.push([a], [4]).closed) == 0          # b idle for 1 tick
    assert len(table.push([a], [5]).closed) == 0          # 2 ticks: closed at the start of the NEXT push
    plan = table.push([a, c], [6, 6])                     # ... whose new track takes the slot b leaves
    assert plan.closed.keys == [b] and plan.closed.win.tolist() == [[1, 2]] and plan.closed.frames.tolist() == [[2, 3]]
    assert b not in table and plan.desc.tolist() == [[0, 5, 0], [1, 0, -1]]
    # an idle-closed key may come back: it starts a new track (explicitly closed keys need reopen)
    table.close([c])
    assert table.push([b], [9]).desc.tolist() == [[1, 0, -1]]


def test_a_reused_slot_starts_at_row_0():
    table = TrackTable(max_tracks=1, seg_len=2)
    assert table.push([(1, 1, 1)], [5]).n_emit == 0
    p = table.push([(1, 1, 1)], [6])
    assert p.desc.tolist() == [[0, 1, 0]] and p.meta.tolist() == [[1, 1, 1, 5]] and p.frames.tolist() == [[5, 6]]
    assert table.close([(1, 1, 1)]).frames.tolist() == [[6]]
    p = table.push([(2, 1, 1)], [40])
    assert p.desc.tolist() == [[0, 0, -1]] and p.n_emit == 0
    p = table.push([(2, 1, 1)], [43])
    assert p.meta.tolist() == [[2, 1, 1, 40]] and p.frames.tolist() == [[40, 43]]


@pytest.mark.parametrize("ring_len", [SEG_LEN, SEG_LEN + 3, 16])
def test_base_offsets_address_the_right_rows_of_a_mirrored_ring(ring_len):
    """NumPy model of the pose ring: row r of a track at positions r % L and r % L + L (what mcd_stream_push_group writes)."""
    tracks = _split_tracks("test")
    L, n_slots = ring_len, 18                                 # fewer slots than the 22 tracks: reused through close()
    table = TrackTable(max_tracks=n_slots, seg_len=SEG_LEN, ring_len=L)
    ring = np.full((n_slots, 2 * L, ROW), np.nan, np.float32)
    rows = {k: p for k, _, p in tracks}
    left = {k: len(f) for k, f, _ in tracks}
    n_checked = 0
    for _, keys, fids, poses in ticks_by_frame(tracks):
        plan = table.push(keys, fids)
        for (slot, r, j), row in zip(plan.desc, poses):
            ring[slot, r % L] = ring[slot, r % L + L] = row
        assert plan.base.dtype == np.int64 and plan.base.shape == (plan.n_emit,)
        flat = ring.reshape(-1)
        for (slot, r_last), base, k in zip(plan.win, plan.base, plan.keys):
            assert base == table.base_offset(int(slot), int(r_last) - SEG_LEN + 1)
            assert slot * 2 * L * ROW <= base and base + SEG_LEN * ROW <= (slot + 1) * 2 * L * ROW
            want = rows[k][r_last - SEG_LEN + 1:r_last + 1]
            assert np.array_equal(flat[base:base + SEG_LEN * ROW].reshape(SEG_LEN, ROW), want)
            n_checked += 1
        done = []
        for k in keys:
            left[k] -= 1
            if left[k] == 0:
                done.append(k)
        table.close(done)
    assert n_checked == 283 and len(table) == 0

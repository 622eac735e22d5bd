"""Host half of PoseStream.push_many (mocodad_amd/stream.py: pack_ticks) without a GPU: the groups of a call concatenate to exactly
the plans of sequential TrackTable.push calls, every group respects the three cutting rules and is as long as they allow, the
merged descriptors follow the tick-major formula, a NumPy model of the two group launches leaves the frame-score ring and the
finals that tick-by-tick launches leave, a one-plan group (what PoseStream.push builds) is the group pack_ticks returns for
that tick, and a rejected call names its tick and changes nothing."""
import numpy as np
import pytest

from dataset_spec import DATASET
from mocodad_amd.data import trajectories as T
from mocodad_amd.stream import TrackTable, _group, pack_ticks, ticks_by_frame

SEG_LEN = 6
NT = 5


def _interleaving(seed, n_keys=7, n_ticks=48):
    """Seeded random ticks: track i starts at a random tick (mid-call), pauses at random (so max_idle closes it and its key
    comes back as a new track), frame ids with gaps."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, n_ticks // 2, n_keys)
    start[0] = 0
    pause = [(int(a), int(a) + int(rng.integers(1, 6))) for a in rng.integers(3, n_ticks, n_keys)]
    ticks = []
    for i in range(n_ticks):
        live = [k for k in range(n_keys) if i >= start[k] and not pause[k][0] <= i < pause[k][1] and rng.random() < 0.85]
        live = [live[j] for j in rng.permutation(len(live))]
        ticks.append(([(1, 1 + k % 2, k) for k in live], [3 * i + 1 + int(rng.integers(0, 2))] * len(live)))
    return ticks


def _same_plan(a, b):
    for name in ("desc", "win", "base", "meta", "frames"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert a.keys == b.keys and a.closed.keys == b.closed.keys and a.closed.slots == b.closed.slots
    assert np.array_equal(a.closed.win, b.closed.win) and np.array_equal(a.closed.frames, b.closed.frames)


def _check_rules(table, groups, cap):
    """The three cutting rules hold inside every group, and each cut was forced: the next tick would have broken one."""
    per_track = table.ring_len - table.seg_len + 1
    for gi, g in enumerate(groups):
        count = {}
        for p in g.plans:
            assert not set(p.closed.slots) & set(count), "a slot with a row in the group was freed inside it"
            for s in p.desc[:, 0].tolist():
                count[s] = count.get(s, 0) + 1
        assert max(count.values(), default=0) <= per_track
        assert g.n_rows == sum(count.values()) <= cap
        if gi + 1 < len(groups):
            nxt = groups[gi + 1].plans[0]
            slots = nxt.desc[:, 0].tolist()
            assert (per_track == 1 or g.n_rows + len(slots) > cap or any(count.get(s, 0) >= per_track for s in slots)
                    or set(nxt.closed.slots) & set(count)), f"group {gi} was cut although tick {groups[gi + 1].first_tick} fits"


def _check_descriptors(g, nt, seg_len):
    ne = [p.n_emit for p in g.plans]
    assert g.offsets.tolist() == [0] + np.cumsum(ne).tolist() and g.n_windows == sum(ne)
    assert g.desc.dtype == np.int32 and g.desc.shape == (sum(len(p.desc) for p in g.plans), 4)
    assert g.win.dtype == np.int32 and g.win.shape == (g.n_windows, 5)
    # per row, tick after tick: [slot, r, pos0, n_emit]: pos0 = nt * (windows of the earlier ticks) + j
    row = 0
    slot_r_of_pos = {}
    for i, p in enumerate(g.plans):
        for slot, r, j in p.desc.tolist():
            want = [slot, r, nt * int(g.offsets[i]) + j if j >= 0 else -1, ne[i]]
            assert g.desc[row].tolist() == want
            assert (j >= 0) == (r >= seg_len - 1)
            if j >= 0:
                for t in range(nt):
                    pos = want[2] + t * ne[i]
                    assert pos not in slot_r_of_pos
                    slot_r_of_pos[pos] = (slot, r, i, j)
            row += 1
    # ... which is a bijection onto the group's batch, tick-major: position nt * offsets[i] + t * ne_i + j
    assert sorted(slot_r_of_pos) == list(range(nt * g.n_windows))
    for i, p in enumerate(g.plans):
        for t in range(nt):
            for j in range(ne[i]):
                assert slot_r_of_pos[nt * int(g.offsets[i]) + t * ne[i] + j] == (int(p.win[j, 0]), int(p.win[j, 1]), i, j)
    # the window list: sorted by slot, rows ascending inside a slot; w = index in (tick, j) order
    assert sorted(g.win[:, 4].tolist()) == list(range(g.n_windows))
    key = g.win[:, 0].astype(np.int64) * 2 ** 32 + g.win[:, 1]
    assert (np.diff(key) > 0).all()
    for slot, r_last, pos0, n_emit, w in g.win.tolist():
        i = int(np.searchsorted(g.offsets, w, side="right")) - 1
        j = w - int(g.offsets[i])
        assert g.plans[i].win[j].tolist() == [slot, r_last] and pos0 == nt * int(g.offsets[i]) + j and n_emit == ne[i]


def _model_sequential(table, plans, scores_of, nt):
    """NumPy model of one mcd_stream_push_group + mcd_stream_frame_scores_group pair per tick (each tick a group of one), on the
    frame-score ring."""
    L, T = table.ring_len, table.seg_len
    fs = np.full((table.max_tracks, nt, L), 7.0, np.float32)       # (stale cells: pushes must zero what they use)
    finals = []
    for p in plans:
        for slot, r, _ in p.desc.tolist():
            fs[slot, :, r % L] = 0
        for slot, r_last in p.win.tolist():
            sc = np.maximum(scores_of[len(finals)], 0)
            for k in range(T):
                c = (r_last - T + 1 + k) % L
                fs[slot, :, c] = np.maximum(fs[slot, :, c], sc)
            finals.append(fs[slot, :, (r_last - T + 1) % L].copy())
    return fs, finals


def _model_groups(table, groups, scores_of, nt):
    """... and of mcd_stream_push_group + mcd_stream_frame_scores_group: all rows of a group first, then its windows in the order
    of GroupPlan.win, finals to row w."""
    L, T = table.ring_len, table.seg_len
    fs = np.full((table.max_tracks, nt, L), 7.0, np.float32)
    finals = []
    for g in groups:
        for slot, r, _, _ in g.desc.tolist():
            fs[slot, :, r % L] = 0
        out = [None] * g.n_windows
        for slot, r_last, _, _, w in g.win.tolist():
            sc = np.maximum(scores_of[len(finals) + w], 0)
            for k in range(T):
                c = (r_last - T + 1 + k) % L
                fs[slot, :, c] = np.maximum(fs[slot, :, c], sc)
            out[w] = fs[slot, :, (r_last - T + 1) % L].copy()
        finals += out
    return fs, finals


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("ring_len, max_idle, cap", [(SEG_LEN, None, None), (SEG_LEN + 1, 2, None), (SEG_LEN + 3, 1, None),
                                                     (SEG_LEN + 6, 3, 16), (2 * SEG_LEN + 4, None, None)])
def test_groups_concatenate_to_the_sequential_plans_and_respect_the_cutting_rules(seed, ring_len, max_idle, cap):
    ticks = _interleaving(seed)
    table = TrackTable(max_tracks=7, seg_len=SEG_LEN, ring_len=ring_len, max_idle=max_idle)
    for keys, fids in _interleaving(100 + seed)[:9]:           # a table with a history: rows, wrapped rings, free slots
        table.push(keys, fids)
    before, seq = table.copy(), table.copy()
    want = [seq.push(keys, fids) for keys, fids in ticks]
    groups, planned = pack_ticks(table, ticks, NT, cap)
    assert table.same_state(before) and planned.same_state(seq) and not planned.same_state(before)
    got = [p for g in groups for p in g.plans]
    assert len(got) == len(want) and [g.first_tick for g in groups] == np.cumsum([0] + [len(g.plans) for g in groups])[:-1].tolist()
    for a, b in zip(got, want):
        _same_plan(a, b)
    _check_rules(table, groups, 7 * (ring_len - SEG_LEN + 1) if cap is None else cap)
    for g in groups:
        _check_descriptors(g, NT, SEG_LEN)
        assert g.closed.keys == [k for p in g.plans for k in p.closed.keys]
        assert np.array_equal(g.closed.win, np.concatenate([p.closed.win for p in g.plans]))
        assert np.array_equal(g.closed.frames, np.concatenate([p.closed.frames for p in g.plans]))
    if ring_len == SEG_LEN:
        assert all(len(g.plans) == 1 for g in groups) and len(groups) == len(ticks)
    else:
        assert len(groups) < len(ticks) and max(len(g.plans) for g in groups) > 1
        # what the interleavings are meant to hold
        assert any(r == 0 for g in groups for p in g.plans[1:] for r in p.desc[:, 1])                  # a track starting mid-group
        assert any(r == SEG_LEN - 1 for g in groups for p in g.plans[1:] for r in p.desc[:, 1])        # ... reaching seg_len in one
    assert max(int(p.desc[:, 1].max()) for p in got if len(p.desc)) >= ring_len                        # rings that wrap
    if max_idle:
        assert any(len(p.closed) for p in got) and any(len(p.closed.slots) > len(p.closed) for p in got)
    # the launches of the groups leave the frame-score ring and the finals the tick-by-tick launches leave
    rng = np.random.default_rng(seed)
    scores_of = rng.normal(0.5, 1.0, (sum(p.n_emit for p in want), NT)).astype(np.float32)      # per window in (tick, j) order
    fs_a, fin_a = _model_sequential(table, want, scores_of, NT)
    fs_b, fin_b = _model_groups(table, groups, scores_of, NT)
    assert len(fin_a) == len(fin_b) == len(scores_of) > 50
    assert np.array_equal(fs_a, fs_b) and all(np.array_equal(a, b) for a, b in zip(fin_a, fin_b))


@pytest.mark.parametrize("k, ring_len, n_groups", [(1, SEG_LEN, None), (2, SEG_LEN + 1, None), (6, 2 * SEG_LEN - 1, None),
                                                   (7, 2 * SEG_LEN, None), (45, SEG_LEN + 3, 12)])
def test_fixture_replay_in_calls_of_k_ticks(k, ring_len, n_groups):
    """The committed fixture (22 track files, 283 windows) in frame order, K ticks per call with ring_len = seg_len + K - 1 --
    every call is ONE group -- and the whole replay in one call with ring_len = seg_len + 3, which forces cuts."""
    files = T.list_trajectory_files(T.trajectories_root(DATASET, "test"))
    tracks = [(key,) + T.read_trajectory_csv(path) for key, path in files]
    ticks = [(keys, fids) for _, keys, fids, _ in ticks_by_frame(tracks)]
    assert len(ticks) == 45
    table = TrackTable(max_tracks=len(tracks), seg_len=SEG_LEN, ring_len=ring_len)
    seq = table.copy()
    left = {key: len(f) for key, f, _ in tracks}
    n_win = 0
    for lo in range(0, len(ticks), k):
        call = ticks[lo:lo + k]
        groups, planned = pack_ticks(table, call, NT)
        assert len(groups) == (1 if n_groups is None else n_groups)
        for p, (keys, fids) in zip([p for g in groups for p in g.plans], call):
            _same_plan(p, seq.push(keys, fids))
        for g in groups:
            _check_descriptors(g, NT, SEG_LEN)
            n_win += g.n_windows
        _check_rules(table, groups, len(tracks) * (ring_len - SEG_LEN + 1))
        table.adopt(planned)
        done = []
        for keys, _ in call:
            for key in keys:
                left[key] -= 1
                if left[key] == 0:
                    done.append(key)
        a, b = table.close(done), seq.close(done)            # closes at the call boundaries
        assert a.keys == b.keys and np.array_equal(a.win, b.win) and table.same_state(seq)
    assert n_win == 283 and len(table) == 0


def test_a_one_plan_group_is_the_group_pack_ticks_returns_for_the_tick():
    """PoseStream.push plans its tick on the table itself and wraps the plan with _group(0, [plan], ...), without pack_ticks' copy
    of the table: for a tick that emits, one that does not and an empty one, on a table with a history, that is the single group
    pack_ticks returns -- desc, win, offsets, closed."""
    table = TrackTable(max_tracks=7, seg_len=SEG_LEN, ring_len=SEG_LEN + 3, max_idle=2)
    for keys, fids in _interleaving(100)[:9]:
        table.push(keys, fids)
    open_keys = list(table.slot_of)
    emitting = [k for k in open_keys if table.rows[table.slot_of[k]] >= SEG_LEN - 1]
    assert emitting and len(table) < 7
    cases = {"emits": (open_keys, [40] * len(open_keys)), "no window": ([(3, 1, 50), (3, 1, 51)], [40, 40]), "empty": ([], [])}
    n_win = {}
    for name, (keys, fids) in cases.items():
        before = table.copy()
        plan = table.copy().push(keys, fids)
        g = _group(0, [plan], NT, SEG_LEN)
        groups, planned = pack_ticks(table, [(keys, fids)], NT)
        assert table.same_state(before) and len(groups) == 1 and groups[0].first_tick == g.first_tick == 0
        p = groups[0]
        _same_plan(p.plans[0], plan)
        for x, y in ((g.desc, p.desc), (g.win, p.win), (g.offsets, p.offsets), (g.closed.win, p.closed.win), (g.closed.frames, p.closed.frames)):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), name
        assert g.closed.keys == p.closed.keys and g.closed.slots == p.closed.slots and g.clip is None and p.clip is None
        assert g.desc.shape == (len(keys), 4) and g.win.shape == (plan.n_emit, 5) and g.offsets.tolist() == [0, plan.n_emit]
        _check_descriptors(g, NT, SEG_LEN)
        # the single tick as the entries see it: pos0 = j, ne = n_emit, w = j
        assert g.desc[:, 2].tolist() == plan.desc[:, 2].tolist() and (g.desc[:, 3] == plan.n_emit).all()
        assert sorted(g.win[:, 2].tolist()) == list(range(plan.n_emit)) and np.array_equal(g.win[:, 2], g.win[:, 4])
        n_win[name] = plan.n_emit
    assert n_win["emits"] == len(emitting) and n_win["no window"] == 0 and n_win["empty"] == 0


def test_a_rejected_call_names_the_tick_and_leaves_the_table_as_it_was():
    a, b, c = (1, 1, 1), (1, 1, 2), (1, 2, 3)
    table = TrackTable(max_tracks=2, seg_len=SEG_LEN, ring_len=SEG_LEN + 4)
    table.push([a, b], [1, 1])
    table.close([b])
    table.push([a], [2])
    before = table.copy()
    ok = ([a], [3])
    with pytest.raises(ValueError, match=r"tick 2: track \(1, 1, 1\) has two rows in one tick"):
        pack_ticks(table, [ok, ([a], [4]), ([a, c, a], [5, 5, 5])], NT)
    assert table.same_state(before)
    with pytest.raises(ValueError, match=r"tick 1: track \(1, 1, 2\) was closed"):
        pack_ticks(table, [ok, ([a, b], [4, 4])], NT)
    assert table.same_state(before)
    with pytest.raises(RuntimeError, match=r"tick 3: max_tracks = 2 exhausted.*\(1, 2, 4\)"):
        pack_ticks(table, [ok, ([a, c], [4, 4]), ([c], [5]), ([a, c, (1, 2, 4)], [6, 6, 6])], NT)
    assert table.same_state(before)
    with pytest.raises(ValueError, match="tick 1: 1 keys but 2 frame ids"):
        pack_ticks(table, [ok, ([a], [4, 5])], NT)
    with pytest.raises(ValueError, match="max_rows = 1 is less than max_tracks = 2"):
        pack_ticks(table, [ok], NT, max_rows=1)
    assert table.same_state(before)
    # the same ticks without the offending one go through, and only adopting the plan changes the table
    groups, planned = pack_ticks(table, [ok, ([a, c], [4, 4]), ([c], [5])], NT)
    assert len(groups) == 1 and table.same_state(before)
    table.adopt(planned)
    assert table.rows[:2].tolist() == [4, 2] and table.tick == before.tick + 3
    # two rows for a track in ONE tick stay an error of TrackTable.push itself
    with pytest.raises(ValueError, match="two rows in one tick"):
        table.push([a, a], [9, 10])

"""Host half of the online clip scores (mocodad_amd/stream.py: ClipTable, merge_clip_ticks, batch_clip_ticks) without a GPU.

Seeded random feeds -- tracks that start and end mid-clip, frame-id gaps inside tracks, tracks that never reach seg_len, max_idle
closures, explicit closes, several clips per tick, late rows, frame-id jumps beyond the clip ring -- are held against a brute-force
model that keeps the whole history (every row pushed, every final and tail that arrived, in arrival order) and recomputes
completeness, watermark and ring occupancy from it at every tick:
  * every frame of every segment is emitted exactly once, in order, at the first tick the rule allows and not before;
  * a rejected tick (late row, ring overflow, no clip slot) leaves same_state true against a copy taken before;
  * no live cell is overwritten: a NumPy model of the two launches on a ring gives, for every segment, the filter over the whole
    segment computed from the history alone;
  * the plans of pack_ticks groups are the sequential plans, contribution order per cell included, and the NumPy launches fed
    the merged group plans leave the rings and the outputs of the tick-by-tick launches, bit for bit."""
import numpy as np
import pytest

from mocodad_amd.stream import (ClipTable, TrackTable, batch_clip_ticks, merge_clip_ticks, pack_ticks)
from mocodad_amd.utils.eval_utils import gaussian_kernel1d

T = 4                     # seg_len
NT = 2
SIGMA, SHIFT = 1.0, 2
R = int(4 * SIGMA + 0.5)
MAX_IDLE = 3


def _value(key, fid, t, tail):
    """The 'final frame score' of a row: any fixed fp32 function of (track, frame, transform); tails differ from finals."""
    h = (key[0] * 7919 + key[1] * 104729 + key[2] * 1299709 + fid * 15485863 + t * 32452843 + (17 if tail else 0)) % 1000003
    return np.float32(h / 1000003.0 * 3.0)


# ---------------------------------------------------------------------------------------------------------------- the two launches
class NpRings:
    def __init__(self, n_clips, L):
        self.sum, self.lmax, self.lmin = (np.zeros((n_clips, NT, L)) for _ in range(3))
        self.n = np.zeros((n_clips, NT, L), np.int32)
        self.L = L

    def state(self):
        return [a.copy() for a in (self.sum, self.lmax, self.lmin, self.n)]

    def update(self, la, finals, tails):
        seen = set()
        for slot, pos, first, count, zero in la.runs.tolist():
            assert (slot, pos) not in seen                      # one owner per cell
            seen.add((slot, pos))
            for t in range(NT):
                s, hi, lo, n = (0.0, 0.0, 0.0, 0) if zero else (self.sum[slot, t, pos], self.lmax[slot, t, pos],
                                                                self.lmin[slot, t, pos], int(self.n[slot, t, pos]))
                for src, row in la.contrib[first:first + count].tolist():
                    dv = float((finals if src == 0 else tails)[row, t])
                    lg = float(np.log1p(dv))
                    s += dv
                    hi, lo = (lg, lg) if n == 0 else (max(hi, lg), min(lo, lg))
                    n += 1
                self.sum[slot, t, pos], self.lmax[slot, t, pos], self.lmin[slot, t, pos], self.n[slot, t, pos] = s, hi, lo, n

    def emit(self, outs, g):
        res = np.zeros(len(outs))
        for o, (slot, j, m, pbase) in enumerate(outs.tolist()):
            me = m if m >= 0 else 1 << 29

            def at(k, t):
                k %= 2 * me
                if k >= me:
                    k = 2 * me - 1 - k
                if k < SHIFT:
                    return 0.0
                p = (pbase + k - SHIFT) % self.L
                n = self.n[slot, t, p]
                return self.sum[slot, t, p] / n + (self.lmax[slot, t, p] - self.lmin[slot, t, p]) if n else 0.0

            acc = 0.0
            for t in range(NT):
                v = at(j, t) * g[R]
                for i in range(R, 0, -1):
                    v += (at(j - i, t) + at(j + i, t)) * g[R - i]
                acc += v
            res[o] = acc / NT
        return res


# ---------------------------------------------------------------------------------------------------------------- brute force
class History:
    """Everything that happened, nothing derived: the model recomputes what it needs from these lists at every tick."""

    def __init__(self, L, max_clips):
        self.L, self.max_clips = L, max_clips
        self.pushed = {}          # open track key -> frame ids pushed, in order
        self.n_final = {}         # open track key -> rows of it that are final
        self.segs = {}            # clip -> list of segments {origin, head, next, ended, contrib: {frame: [(order, person, key, fid, tail)]}}
        self.order = 0
        self.stale = set()        # clips a close touched since their last emission
        self._slot_of = {}        # open track key -> its slot in the TrackTable (ClosePlan.slots names closed tracks by slot)
        self.slot_of_clip = {}    # the ClipTable's clip -> slot map (outputs of a tick are ordered by clip slot)

    def pending(self, clip):
        return [f for k, fl in self.pushed.items() if k[:2] == clip for f in fl[self.n_final[k]:]]

    def watermark(self, clip):
        s = self.segs[clip][-1]
        return min([f for f in self.pending(clip) if f >= s["origin"]] + [s["head"] + 1])

    def next_now(self, clip):
        """The next frame to emit; a clip touched by a close first catches up at the start of the next tick."""
        s = self.segs[clip][-1]
        return max(s["next"], min(self.watermark(clip) - 1 + SHIFT, s["head"]) - R + 1) if clip in self.stale else s["next"]

    def lo(self, clip):
        return max(self.segs[clip][-1]["origin"], self.next_now(clip) - R - SHIFT)

    def expect(self, keys, fids):
        """The exception type the rules demand for this tick, or None."""
        by = {}
        for k, f in zip(keys, fids):
            by.setdefault(k[:2], []).append(f)
        new = 0
        for clip, fl in by.items():
            if clip not in self.segs or self.segs[clip][-1]["ended"]:
                new += 1
                if new > self.max_clips - sum(not s[-1]["ended"] for s in self.segs.values()):
                    return RuntimeError
                continue
            if min(fl) < self.watermark(clip):
                return ValueError
            if self.decide(clip, fl) == "overflow":
                return RuntimeError
        return None

    def decide(self, clip, fl):
        s = self.segs[clip][-1]
        if max(fl) <= s["head"]:
            return None
        live = s["head"] - self.lo(clip) + 1
        if live + max(fl) - s["head"] <= self.L:
            return "advance"
        o2 = min(f for f in fl if f > s["head"])
        return "jump" if live + max(fl) - o2 + 1 <= self.L else "overflow"

    def add(self, clip, key, fid, tail):
        """A final / tail that arrived -> its segment, or dropped."""
        for s in self.segs[clip]:
            if s["origin"] <= fid <= s["head"] and not s["dead"]:
                s["contrib"].setdefault(fid, []).append((self.order, key[2], key, fid, tail))
                return 0
        return 1

    def tick(self, keys, fids, plan):
        """Apply an accepted tick -> (expected [(clip, frame)] emitted by it, in order; dropped)."""
        self.order += 1
        dropped, touched = 0, set()
        arrivals, out = [], []
        for clip in sorted(self.stale, key=lambda c: self.slot_of_clip[c]):
            s, nn = self.segs[clip][-1], self.next_now(clip)
            out += [(clip, j) for j in range(s["next"], nn)]
            s["next"] = nn
        self.stale.clear()
        n_pre = len(out)
        ci = 0
        for k in list(plan.closed.keys):
            arrivals += [(k, int(f), True) for f in plan.closed.frames[ci]]
            ci += 1
        gone = [k for k in self.pushed if self._slot_of[k] in set(plan.closed.slots)]
        for k in gone:
            touched.add(k[:2])
            del self.pushed[k], self.n_final[k], self._slot_of[k]
        by = {}
        for k, f in zip(keys, fids):
            by.setdefault(k[:2], []).append(f)
        jumped = {}
        for clip, fl in by.items():
            touched.add(clip)
            if clip not in self.segs or self.segs[clip][-1]["ended"]:
                self.segs.setdefault(clip, []).append(dict(origin=min(fl), head=max(fl), next=min(fl), ended=False, dead=False, contrib={}))
                continue
            d, s = self.decide(clip, fl), self.segs[clip][-1]
            if d == "advance":
                s["head"] = max(fl)
            elif d == "jump":
                jumped[clip] = s
                o2 = min(f for f in fl if f > s["head"])
                self.segs[clip].append(dict(origin=o2, head=max(fl), next=o2, ended=False, dead=False, contrib={}))
        for i, (k, f) in enumerate(zip(keys, fids)):
            if k not in self.pushed:
                self.pushed[k], self.n_final[k] = [], 0
                self._slot_of[k] = int(plan.desc[i, 0])
            self.pushed[k].append(f)
        for j, k in enumerate(plan.keys):
            arrivals.append((k, int(plan.frames[j, 0]), False))
            assert self.pushed[k][self.n_final[k]] == int(plan.frames[j, 0])
            self.n_final[k] += 1
        for k, f, tail in sorted(arrivals, key=lambda a: a[0][2]):       # ascending person id within the tick
            dropped += self.add(k[:2], k, f, tail)
        for clip in sorted(touched, key=lambda c: self.slot_of_clip[c]):
            if clip in jumped:
                s = jumped[clip]
                out += [(clip, j) for j in range(s["next"], s["head"] + 1)]
                s["next"], s["ended"], s["dead"] = s["head"] + 1, True, True
            s = self.segs[clip][-1]
            jmax = min(self.watermark(clip) - 1 + SHIFT, s["head"]) - R
            out += [(clip, j) for j in range(s["next"], jmax + 1)]
            s["next"] = max(s["next"], jmax + 1)
        return out, dropped, n_pre

    def close(self, plan):
        ci, dropped = 0, 0
        arrivals = []
        for k in plan.keys:
            arrivals += [(k, int(f), True) for f in plan.frames[ci]]
            ci += 1
        for k in [k for k in self.pushed if self._slot_of[k] in set(plan.slots)]:
            self.stale.add(k[:2])
            del self.pushed[k], self.n_final[k], self._slot_of[k]
        self.order += 1
        for k, f, tail in sorted(arrivals, key=lambda a: a[0][2]):
            dropped += self.add(k[:2], k, f, tail)
        return dropped

    def end(self, clip):
        s = self.segs[clip][-1]
        out = [(clip, j) for j in range(s["next"], s["head"] + 1)]
        s["next"], s["ended"], s["dead"] = s["head"] + 1, True, True
        self.stale.discard(clip)
        return out

    def segment_scores(self, s, g):
        """gaussian_filter1d(shifted raw) over the whole segment, from the contributions alone."""
        m = s["head"] - s["origin"] + 1
        res = np.zeros(m)
        for t in range(NT):
            raw = np.zeros(m)
            for f, lst in s["contrib"].items():
                v = np.asarray([float(_value(k, fid, t, tail)) for _, _, k, fid, tail in lst])      # arrival order, persons ascending
                raw[f - s["origin"]] = v.sum() / len(v) + (np.log1p(v).max() - np.log1p(v).min())
            sh = np.concatenate([np.zeros(min(SHIFT, m)), raw[:max(m - SHIFT, 0)]])
            ext = np.pad(sh, R, mode="symmetric")                 # scipy's 'reflect'
            res += np.asarray([np.dot(ext[j:j + 2 * R + 1], g) for j in range(m)])
        return res / NT


def _tails(cp):
    """The tails tensor of a ClosePlan: (n * (seg_len - 1), NT)."""
    return np.asarray([[_value(k, int(f), t, True) for t in range(NT)] for i, k in enumerate(cp.keys) for f in cp.frames[i]],
                      np.float32).reshape(-1, NT)


def _launch(rings, la, fin, tl, g):
    """One launch pair on the NumPy rings -> the outputs (catch-up outputs are read before the update)."""
    pre = rings.emit(la.outs[:la.n_pre], g)
    rings.update(la, fin, tl)
    return np.concatenate([pre, rings.emit(la.outs[la.n_pre:], g)])


# ---------------------------------------------------------------------------------------------------------------- the feed
def _feed(seed, n_ticks=140, n_clips=3, late=True):
    """-> a generator protocol: yields candidate ticks [(key, fid)], told back whether the tick was accepted."""
    rng = np.random.default_rng(seed)
    frame = {c: int(rng.integers(1, 50)) for c in range(n_clips)}
    active = {c: {} for c in range(n_clips)}          # clip -> person -> rows pushed
    next_person = [100]
    for _ in range(n_ticks):
        rows, closes = [], []
        for c in range(n_clips):
            if rng.random() < 0.2:
                continue                              # nobody of this clip in this tick
            u = rng.random()
            frame[c] += 1 if u < 0.85 else int(rng.integers(2, 4)) if u < 0.97 else int(rng.integers(60, 400))
            if rng.random() < 0.3 and len(active[c]) < 3:
                next_person[0] += int(rng.integers(1, 5))
                active[c][next_person[0] if rng.random() < 0.5 else 100000 - next_person[0]] = 0
            for p in list(active[c]):
                if rng.random() < 0.12:               # the track ends: explicitly closed, or left to max_idle
                    if rng.random() < 0.5:
                        closes.append((1, c, p))
                    del active[c][p]
                elif rng.random() < 0.85:             # (else: a frame-id gap inside the track)
                    rows.append(((1, c, p), frame[c]))
                    active[c][p] += 1
        order = rng.permutation(len(rows))
        yield [rows[i] for i in order], closes, (rng.random() < 0.08 if late else False), rng


def _run_feed(seed, ring_len, group=1, max_clips=3):
    """Drive TrackTable + ClipTable tick by tick (group = 1) against the History model; returns what the comparisons need."""
    per_track = ring_len - T + 1
    L = 2 * R + SHIFT + T + MAX_IDLE + per_track + 1
    table, clips = TrackTable(32, T, ring_len, MAX_IDLE), ClipTable(max_clips, L, R, SHIFT, T)
    hist = History(L, max_clips)
    hist.slot_of_clip = clips.slot_of
    g = gaussian_kernel1d(SIGMA)
    rings = NpRings(max_clips, L)
    log = []          # per accepted step: ("tick", keys, fids, plan, ctick) | ("close", keys, plan, ctick)
    rejected = 0
    emitted = {}      # (clip, segment index) -> [(frame, value)]

    def take(ct, expected):
        assert list(zip(ct.clips, ct.frames.tolist())) == expected
        return ct

    def record(ct, vals):
        for (clip, f), v in zip(zip(ct.clips, ct.frames.tolist()), vals):
            si = max(i for i, s in enumerate(hist.segs[clip]) if s["origin"] <= f <= s["head"])
            emitted.setdefault((clip, si), []).append((f, v))

    def tensors(plan):
        fin = np.asarray([[_value(k, int(plan.frames[j, 0]), t, False) for t in range(NT)] for j, k in enumerate(plan.keys)],
                         np.float32).reshape(-1, NT)
        return fin, _tails(plan.closed)

    for rows, closes, try_late, rng in _feed(seed):
        closes = [k for k in closes if k in table.slot_of]
        if closes:
            plan = table.close(closes)
            ct = clips.close(plan)
            assert ct.n_out == 0 and ct.dropped == hist.close(plan)
            rings.update(merge_clip_ticks([ct], L), None, _tails(plan))
            log.append(("close", closes, plan, ct))
        keys, fids = [r[0] for r in rows], [r[1] for r in rows]
        if try_late and clips.slot_of:
            # a row of a new person below some open clip's watermark: the model says what has to happen
            clip = list(clips.slot_of)[int(rng.integers(len(clips.slot_of)))]
            bad_keys, bad_fids = keys + [clip + (5000 + len(log),)], fids + [hist.watermark(clip) - int(rng.integers(1, 3))]
            want = hist.expect(bad_keys, bad_fids)
            assert want is ValueError or want is RuntimeError
            before_c = clips.copy()
            with pytest.raises(want):
                clips.check(bad_keys, bad_fids)
            assert clips.same_state(before_c)
            rejected += 1
        want = hist.expect(keys, fids)
        before = clips.copy()
        if want is not None:
            with pytest.raises(want):
                clips.check(keys, fids)
            assert clips.same_state(before)
            rejected += 1
            continue
        clips.check(keys, fids)
        assert clips.same_state(before)               # check itself changes nothing
        plan = table.push(keys, fids)
        ct = clips.push(plan, keys, fids)
        exp_out, exp_drop, exp_pre = hist.tick(keys, fids, plan)
        take(ct, exp_out)
        assert ct.dropped == exp_drop and ct.n_pre == exp_pre
        fin, tl = tensors(plan)
        record(ct, _launch(rings, merge_clip_ticks([ct], L), fin, tl, g))
        log.append(("tick", keys, fids, plan, ct))
    # the end: every clip is closed
    for clip in list(clips.slot_of):
        keys = clips.tracks_of(clip)
        assert sorted(keys) == sorted(k for k in table.slot_of if k[:2] == clip)
        plan = table.close(keys)
        ct = clips.close(plan)
        assert ct.dropped == hist.close(plan)
        rings.update(merge_clip_ticks([ct], L), None, _tails(plan))
        end = clips.end_clip(clip)
        assert list(zip(end.clips, end.frames.tolist())) == hist.end(clip)
        record(end, rings.emit(end.outs, g))
    assert len(clips) == 0 and len(table) == 0
    return dict(hist=hist, emitted=emitted, g=g, log=log, rejected=rejected, L=L, rings=rings)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_feeds_follow_the_brute_force_model(seed):
    r = _run_feed(seed, ring_len=T)
    hist, n_seg = r["hist"], 0
    for clip, segs in hist.segs.items():
        for si, s in enumerate(segs):
            got = r["emitted"].get((clip, si), [])
            # every frame origin .. head exactly once, ascending
            assert [f for f, _ in got] == list(range(s["origin"], s["head"] + 1))
            # and its value is the filter over the whole segment: live emissions, reflected tails, no overwritten cell
            want = hist.segment_scores(s, r["g"])
            np.testing.assert_allclose([v for _, v in got], want, rtol=1e-12, atol=1e-300)
            n_seg += 1
    assert n_seg >= 3
    if seed == 1:
        # the feed does what the docstring says (otherwise the comparisons above show less than they claim)
        assert sum(_run_feed(s, ring_len=T)["rejected"] for s in (1, 2)) > 0


def test_the_seeds_cover_jumps_idle_closures_short_tracks_and_drops():
    jumps = idle = short = drops = several = 0
    for seed in (1, 2, 3, 4):
        r = _run_feed(seed, ring_len=T)
        jumps += sum(len(s) - 1 for s in r["hist"].segs.values())
        for step in r["log"]:
            if step[0] == "tick":
                plan, ct = step[3], step[4]
                idle += len(plan.closed.keys)
                short += len(plan.closed.slots) - len(plan.closed.keys)
                drops += ct.dropped
                several += len({k[:2] for k in step[1]}) > 1
    assert jumps > 0 and idle > 0 and short > 0 and drops > 0 and several > 10


@pytest.mark.parametrize("seed, ring_len", [(1, T + 3), (2, T + 3), (3, T + 1)])
def test_group_plans_are_the_sequential_plans_and_give_the_same_rings(seed, ring_len):
    """pack_ticks(..., clips=) over calls of 1 .. 6 ticks: per tick the ClipTick of sequential planning (row numbers shifted by the
    group's offsets), and the NumPy launches fed the merged group plans reproduce the tick-by-tick rings and outputs bit for bit."""
    r = _run_feed(seed, ring_len=ring_len)
    L, g = r["L"], r["g"]
    table, clips = TrackTable(32, T, ring_len, MAX_IDLE), ClipTable(3, L, R, SHIFT, T)
    seq_rings, grp_rings = NpRings(3, L), NpRings(3, L)
    rng = np.random.default_rng(seed)
    log, i, n_multi, n_cut = r["log"], 0, 0, 0
    pend = T - 1

    tails_of = _tails

    while i < len(log):
        if log[i][0] == "close":
            plan = table.close(log[i][1])
            ct = clips.close(plan)
            for rr in (seq_rings, grp_rings):
                rr.update(merge_clip_ticks([ct], L), None, tails_of(plan))
            i += 1
            continue
        k = i
        while k < len(log) and log[k][0] == "tick" and k - i < int(rng.integers(1, 7)):
            k += 1
        call = log[i:k]
        groups, twork, cwork = pack_ticks(table, [(s[1], s[2]) for s in call], NT, None, clips)
        seq_out, grp_out, q = [], [], 0
        for gp in groups:
            n_multi += len(gp.plans) > 1
            assert len(gp.clip) == len(gp.plans)
            fin = np.concatenate([np.asarray([[_value(kk, int(p.frames[j, 0]), t, False) for t in range(NT)]
                                              for j, kk in enumerate(p.keys)], np.float32).reshape(-1, NT) for p in gp.plans])
            tl = tails_of(gp.closed)
            c0 = 0
            for ti, (p, ct) in enumerate(zip(gp.plans, gp.clip)):
                ref = call[q][4]                       # the ClipTick sequential planning gave for this tick
                f0, t0 = int(gp.offsets[ti]), pend * c0
                assert ct.opened == ref.opened and ct.dropped == ref.dropped and ct.span == ref.span and ct.n_pre == ref.n_pre
                assert np.array_equal(ct.outs, ref.outs) and ct.clips == ref.clips and np.array_equal(ct.frames, ref.frames)
                assert [(s, c, src, row - (f0 if src == 0 else t0)) for s, c, src, row in ct.contribs] == ref.contribs
                # tick by tick: this tick's own tensors
                rfin = fin[f0:f0 + p.n_emit]
                rtl = tl[t0:t0 + pend * len(p.closed)]
                seq_out.append(_launch(seq_rings, merge_clip_ticks([ref], L), rfin, rtl, g))
                c0 += len(p.closed)
                q += 1
            batches = batch_clip_ticks(gp.clip, L)
            n_cut += len(batches) > 1
            for b in batches:
                la = merge_clip_ticks([gp.clip[x] for x in b], L)
                vals, o = _launch(grp_rings, la, fin, tl, g), 0
                for c in la.n_out:
                    grp_out.append(vals[o:o + c])
                    o += c
        assert len(seq_out) == len(grp_out) == len(call)
        for a, b in zip(seq_out, grp_out):
            assert np.array_equal(a, b)
        for a, b in zip(seq_rings.state(), grp_rings.state()):
            assert np.array_equal(a, b)
        table.adopt(twork)
        clips.adopt(cwork)
        i = k
    assert n_multi > 5
    print("launch pairs cut inside a group:", n_cut)


def _push(table, clips, keys, fids):
    clips.check(keys, fids)
    return clips.push(table.push(keys, fids), keys, fids)


def test_a_stalled_track_fills_the_ring_and_the_overflow_changes_nothing():
    L = 2 * R + SHIFT + 1 + 6
    table, clips = TrackTable(4, T), ClipTable(2, L, R, SHIFT, T)
    _push(table, clips, [(1, 1, 7), (1, 1, 3)], [10, 10])
    outs, f = [], 10
    with pytest.raises(RuntimeError, match="close idle tracks, set max_idle, or size clip_ring_len"):
        while True:                                  # person 7 stalls with a pending row at frame 10: nothing is ever complete
            f += 1
            before_t, before_c = table.copy(), clips.copy()
            ct = _push(table, clips, [(1, 1, 3)], [f])
            outs.append(ct.n_out)
            assert f < 10 + L + 1
    assert f == 10 + L and sum(outs) == 0            # frames 10 .. 10 + L - 1 fill the ring exactly
    assert table.same_state(before_t) and clips.same_state(before_c)
    ct = clips.close(table.close([(1, 1, 7)]))       # a track of one row: no tail, but its pending row is gone
    assert ct.n_out == 0 and not ct.contribs
    ct = _push(table, clips, [(1, 1, 3)], [f])       # ... and the same row is accepted; the held frames arrive at once
    # frames <= f - (T - 1) are complete now, so frames <= f - (T - 1) + SHIFT - R come out; all but the last were computable
    # before this tick's row (catch-up outputs, read before the update launch: that is what freed the ring)
    assert ct.frames.tolist() == list(range(10, f - (T - 1) + SHIFT - R + 1)) and ct.n_pre == ct.n_out - 1 > L // 2


def test_clip_slots_late_rows_and_settings():
    table, clips = TrackTable(8, T), ClipTable(2, 20, R, SHIFT, T)
    _push(table, clips, [(1, 1, 1), (1, 2, 1)], [5, 9])
    before = clips.copy()
    with pytest.raises(RuntimeError, match="max_clips = 2 exhausted"):
        clips.check([(1, 3, 1)], [1])
    for f in range(6, 6 + T + 2):
        _push(table, clips, [(1, 1, 1)], [f])
    assert clips.wm[clips.slot_of[(1, 1)]] == 9              # rows 5 .. 11: 7 - (T - 1) = 4 of them are final, 9 is the first pending
    before = clips.copy()
    with pytest.raises(ValueError, match="late row"):
        clips.check([(1, 1, 2)], [8])
    assert clips.same_state(before)
    _push(table, clips, [(1, 1, 2)], [9])                   # between the watermark and the head: accepted
    with pytest.raises(ValueError):
        clips.end_clip((1, 1))                              # open tracks
    with pytest.raises(KeyError):
        clips.end_clip((4, 4))
    with pytest.raises(ValueError, match="2 R \\+ shift \\+ 1"):
        ClipTable(2, 2 * R + SHIFT, R, SHIFT, T)
    clips.close(table.close([(1, 2, 1)]))
    end = clips.end_clip((1, 2))                            # a clip of one frame, nobody ever final: one zero-person output
    assert end.frames.tolist() == [9] and end.outs.tolist() == [[1, 0, 1, 0]]
    _push(table, clips, [(1, 3, 1)], [1])                   # its slot is free again


def test_frame_gaps_inside_a_group_cut_the_clip_launches():
    """One track whose frame id advances by 3 per row: every single tick fits the ring, but over a group of 4 ticks the head
    runs 12 frames ahead of the cells that the group's first outputs still read, so the group needs a second launch pair --
    and gives the outputs and rings of the tick-by-tick launches."""
    ring_len, L = T + 3, 24
    g = gaussian_kernel1d(SIGMA)
    table, clips = TrackTable(2, T, ring_len), ClipTable(1, L, R, SHIFT, T)
    seq_table, seq_clips = table.copy(), clips.copy()
    seq_rings, grp_rings = NpRings(1, L), NpRings(1, L)
    key, n_cut, n_out = (1, 1, 1), 0, 0
    fin_of = lambda p: np.asarray([[_value(k, int(p.frames[j, 0]), t, False) for t in range(NT)] for j, k in enumerate(p.keys)],
                                  np.float32).reshape(-1, NT)
    for lo in range(0, 40, 4):
        call = [([key], [1 + 3 * i]) for i in range(lo, lo + 4)]
        want = []
        for keys, fids in call:
            seq_clips.check(keys, fids)
            p = seq_table.push(keys, fids)
            want.append(_launch(seq_rings, merge_clip_ticks([seq_clips.push(p, keys, fids)], L), fin_of(p), _tails(p.closed), g))
        groups, twork, cwork = pack_ticks(table, call, NT, None, clips)
        assert len(groups) == 1 and len(groups[0].plans) == 4
        gp = groups[0]
        fin = np.concatenate([fin_of(p) for p in gp.plans])
        batches, got = batch_clip_ticks(gp.clip, L), []
        n_cut += len(batches) > 1
        for b in batches:
            la = merge_clip_ticks([gp.clip[x] for x in b], L)
            vals, o = _launch(grp_rings, la, fin, _tails(gp.closed), g), 0
            for c in la.n_out:
                got.append(vals[o:o + c])
                o += c
        for a, b in zip(want, got):
            assert np.array_equal(a, b)
            n_out += len(a)
        for a, b in zip(seq_rings.state(), grp_rings.state()):
            assert np.array_equal(a, b)
        table.adopt(twork)
        clips.adopt(cwork)
        assert clips.same_state(seq_clips)
    assert n_cut >= 5 and n_out > 60

"""Live pose streams: many tracked people, one new pose row per track per video frame, an anomaly score a few milliseconds later.

The dataset path takes a whole split at once (data/trajectories.py parses a directory, mcd_normalize_poses normalises every row,
TrajectoryWindows enumerates every window, post_processing assembles the frame scores after the last batch).  Here the state
between two ticks lives on the device (include/mocodad_hip.h: mcd_stream_state_t):

  pose ring   (max_tracks, 2 L, 2, 17): row r of a track is stored at positions r % L and r % L + L, so the seg_len rows from row
              s on are contiguous from position s % L and a window is still ONE base offset of a window view: the scoring
              kernels read the ring exactly as they read a trajectory buffer.
  score ring  (max_tracks, num_transform, L): the running maximum, per row and transform, over the windows covering that row.

and a tick is: one host-to-device copy of the new rows and their descriptors, mcd_stream_push_group (normalise + store + window
descriptors), ONE scoring call on the windows that end at the new rows, mcd_stream_frame_scores_group (max into the score ring;
the oldest row of each window is final and comes back).  These launches take a GROUP of consecutive ticks; a tick is a group of
one, and `PoseStream.push` and `push_many` share the one launch sequence (`PoseStream._run_group`).

`TrackTable` is the host half: (scene, clip, person) -> ring slot, row counts, the frame ids of the last seg_len rows.  It is plain
NumPy and touches no GPU module.  Windows follow the reference's rule (utils/preprocessing.py:14-86, the rule
TrajectoryWindows.from_buffer implements): they run over CONSECUTIVE ROWS of a track, frame-number gaps included, so
meta = [scene, clip, person, frame id of the window's first row] and frames = the frame ids of its seg_len rows.
`PoseStream` owns the rings (engine.StreamRings) and the staging buffers and drives the launches of a tick.

Several ticks at once (a pose estimator that delivers frames in batches, a stream catching up, recorded video on the online path):
`PoseStream.push_many` returns what the same ticks pushed one by one return, bit for bit, but runs them in launch groups --
`pack_ticks` cuts the call into groups of consecutive ticks that the rings can hold at once (ring_len - seg_len + 1 rows per
track), and a group is one copy, mcd_stream_push_group, ONE scoring call on all of its windows, mcd_stream_frame_scores_group.

Online clip scores (opt-in, `PoseStream(clip_scores=ClipScoreCfg(...))`): the number the model is evaluated on -- per video frame
of a clip the person aggregation of the final row scores, shifted, Gaussian-filtered and averaged over the transforms -- leaves
the device with the tick that makes it computable (`Tick.clip`), and `close_clip` ends a clip with the reflected tail.  `ClipTable`
is the host half (clip slots, per clip the frame axis, watermark and emit cursor; plain NumPy), engine.ClipRings the device half
(mcd_clip_state_t); a tick or a group adds one mcd_stream_clip_update and one mcd_stream_clip_emit launch, their descriptors ride
in the tick's one copy.  The definitions stand above `ClipScoreCfg`.

Per-joint frame scores (opt-in, `PoseStream(joint_scores=True)`): the tick's scoring call also yields the error maps
of its windows (mcd_error_maps: per forecast frame and joint, the loss behind the window's score), a second ring (max_tracks,
num_transform, L, 17) takes their per-row maximum with the same window table (mcd_stream_joint_scores_group), and
`Tick.joint_final` / `FrameScores.joints` carry them row for row with the frame scores.

Expected poses (opt-in, `PoseStream(forecasts=ForecastCfg(...))`): what the model expected to see at a row -- the
selected forecasts of the windows covering it collapsed into one pose, in image pixels next to the observed row, with how many
windows forecast it and how much they disagree; the dataset path's --forecast-tracks, bit for bit.  The tick's scoring call also
yields the per-sample losses and poses, a forecast ring (max_tracks, L, n_corrupt, 34) and a ring of the raw rows (max_tracks, L,
34) keep what the rows in flight need (mcd_stream_forecast_group, mcd_stream_forecast_flush), and `Tick.forecast` /
`FrameScores.forecast` carry the rows with the frame scores.  `forecast_cover` is the definition as code."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch      # (module level: the one name every device allocation of this file goes through, tests/guarded.py)

ROW = 34                 # floats of one pose row: (2, 17)
Key = Tuple[int, int, int]


def _key(k) -> Key:
    if type(k) is tuple and len(k) == 3 and type(k[0]) is int and type(k[1]) is int and type(k[2]) is int:
        return k                 # (already normalised: the case of every row of every tick once a feed hands out its own keys)
    k = tuple(int(v) for v in k)
    if len(k) != 3:
        raise ValueError(f"a track key is (scene, clip, person), got {k}")
    return k


def _pose_rows(keys, poses) -> np.ndarray:
    """The raw pose rows of one tick as a contiguous (len(keys), 34) fp32 host array; ValueError for another shape or a row that
    is not finite."""
    raw = np.ascontiguousarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float32)
    if raw.ndim != 2 or raw.shape[1] != ROW or raw.shape[0] != len(keys):
        raise ValueError(f"poses must be ({len(keys)}, {ROW}) = one row x1,y1,...,x17,y17 per key, got {raw.shape}")
    if not np.isfinite(raw).all():
        raise ValueError("raw pose rows hold NaN / inf values (the trajectory CSVs hold finite coordinates only)")
    return raw


@dataclass
class ClosePlan:
    """Tracks leaving the table with at least seg_len rows: their seg_len - 1 rows that no emitted window has finalised yet."""
    keys: List[Key] = field(default_factory=list)
    win: np.ndarray = None            # (n, 2) int32 [slot, index of the track's last row]
    frames: np.ndarray = None         # (n, seg_len - 1) int32 frame ids of the pending rows
    slots: List[int] = field(default_factory=list)   # every slot freed, those of shorter tracks (absent above) included

    def __len__(self):
        return len(self.keys)


@dataclass
class TickPlan:
    """What one tick does to the rings (TrackTable.push)."""
    desc: np.ndarray                  # (n, 3) int32 per pushed row: [slot, row index r, emit index j | -1]
    win: np.ndarray                   # (n_emit, 2) int32 per emitted window: [slot, r_last]
    base: np.ndarray                  # (n_emit,) int64 element offset of the window in the pose ring (the kernel writes the same)
    keys: List[Key]                   # (n_emit) the emitting tracks
    meta: np.ndarray                  # (n_emit, 4) int64 [scene, clip, person, frame id of the window's first row]
    frames: np.ndarray                # (n_emit, seg_len) int32 frame ids of the window's rows
    closed: ClosePlan                 # tracks max_idle closed at the start of this tick

    @property
    def n_emit(self) -> int:
        return int(self.win.shape[0])


class TrackTable:
    """(scene, clip, person) -> slot of the device rings, with a free list; per slot the row count and the frame ids of the
    last seg_len rows.

    max_idle: a track that received no row for `max_idle` ticks is closed at the start of the next push (it comes back in
    TickPlan.closed; a later row for its key starts a new track at row 0).  A track closed by `close` stays closed: a row for
    its key is an error until `reopen` -- offline, one key is one trajectory file."""

    def __init__(self, max_tracks: int, seg_len: int, ring_len: Optional[int] = None, max_idle: Optional[int] = None):
        self.max_tracks, self.seg_len = int(max_tracks), int(seg_len)
        self.ring_len = self.seg_len if ring_len is None else int(ring_len)
        if self.max_tracks < 1 or self.seg_len < 1:
            raise ValueError("max_tracks and seg_len must be at least 1")
        if self.ring_len < self.seg_len:
            raise ValueError(f"ring_len = {self.ring_len} is shorter than seg_len = {self.seg_len}")
        if self.max_tracks * 2 * self.ring_len * ROW >= 2 ** 31:
            raise ValueError("max_tracks * ring_len: the pose ring would exceed 2^31 elements")
        if max_idle is not None and int(max_idle) < 1:
            raise ValueError("max_idle must be at least 1 tick")
        self.max_idle = None if max_idle is None else int(max_idle)
        self.slot_of: Dict[Key, int] = {}
        self._free = list(range(self.max_tracks - 1, -1, -1))      # pop() hands out slot 0 first
        self._closed = set()
        self.rows = np.zeros(self.max_tracks, np.int64)            # rows pushed so far
        self._fids = np.zeros((self.max_tracks, self.seg_len), np.int32)   # frame ids of the last seg_len rows, oldest first
        self._last_tick = np.zeros(self.max_tracks, np.int64)
        self.tick = 0

    def __len__(self):
        return len(self.slot_of)

    def __contains__(self, key):
        return _key(key) in self.slot_of

    @property
    def free_slots(self) -> int:
        return len(self._free)

    def copy(self) -> "TrackTable":
        """An independent table in the same state (pack_ticks plans a call on one)."""
        t = TrackTable.__new__(TrackTable)
        t.__dict__.update(self.__dict__)
        t.slot_of, t._free, t._closed = dict(self.slot_of), list(self._free), set(self._closed)
        t.rows, t._fids, t._last_tick = self.rows.copy(), self._fids.copy(), self._last_tick.copy()
        return t

    def same_state(self, other: "TrackTable") -> bool:
        """Every field equal: the next pushes and closes of both tables give the same plans."""
        return ((self.max_tracks, self.seg_len, self.ring_len, self.max_idle, self.tick) ==
                (other.max_tracks, other.seg_len, other.ring_len, other.max_idle, other.tick)
                and list(self.slot_of.items()) == list(other.slot_of.items()) and self._free == other._free
                and self._closed == other._closed and np.array_equal(self.rows, other.rows)
                and np.array_equal(self._fids, other._fids) and np.array_equal(self._last_tick, other._last_tick))

    def adopt(self, other: "TrackTable") -> None:
        """Take over the state of `other` (a planned copy of this table; `other` is not to be used afterwards)."""
        self.__dict__.update(other.__dict__)

    def base_offset(self, slot: int, first_row: int) -> int:
        """Element offset in the pose ring of the seg_len rows of `slot` from row `first_row` on."""
        return (slot * 2 * self.ring_len + first_row % self.ring_len) * ROW

    def _release(self, keys: Sequence[Key]) -> ClosePlan:
        T = self.seg_len
        plan = ClosePlan()
        win, frames = [], []
        for k in keys:
            s = self.slot_of.pop(k)
            plan.slots.append(int(s))
            if self.rows[s] >= T:          # (shorter tracks have no window and no frame score: offline they are dropped)
                plan.keys.append(k)
                win.append((s, self.rows[s] - 1))
                frames.append(self._fids[s, 1:].copy())
            self.rows[s] = 0
            self._free.append(s)
        plan.win = np.asarray(win, np.int32).reshape(-1, 2)
        plan.frames = np.asarray(frames, np.int32).reshape(-1, T - 1)
        return plan

    def close(self, keys) -> ClosePlan:
        """Free the slots of `keys`.  Tracks of fewer than seg_len rows yield nothing."""
        keys = [_key(k) for k in keys]
        for k in keys:
            if k not in self.slot_of:
                raise KeyError(f"track {k} is not open")
        if len(set(keys)) != len(keys):
            raise ValueError(f"close: a track is named twice in {keys}")
        self._closed.update(keys)
        return self._release(keys)

    def reopen(self, keys) -> None:
        """Let closed keys start new tracks (at row 0) again."""
        self._closed.difference_update(_key(k) for k in keys)

    def push(self, keys, frame_ids) -> TickPlan:
        """One tick: one row for each of `keys` with the frame number `frame_ids[i]`."""
        keys = [_key(k) for k in keys]
        fids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if len(fids) != len(keys):
            raise ValueError(f"{len(keys)} keys but {len(fids)} frame ids")
        if len(fids) and (fids.min() < -2 ** 31 or fids.max() > 2 ** 31 - 1):
            raise ValueError("frame ids must fit int32")
        # every check before any change: a rejected tick leaves the table as it was
        seen = set()
        for k in keys:
            if k in seen:
                raise ValueError(f"track {k} has two rows in one tick (a tick is one video frame: one row per track)")
            if k in self._closed:
                raise ValueError(f"track {k} was closed: reopen({k}) before pushing rows for it again (they start a new track)")
            seen.add(k)
        idle = []
        if self.max_idle is not None:
            idle = [k for k, s in self.slot_of.items() if self.tick - self._last_tick[s] >= self.max_idle and k not in seen]
        new = [k for k in keys if k not in self.slot_of]
        if len(new) > len(self._free) + len(idle):
            k = new[len(self._free) + len(idle)]
            raise RuntimeError(f"max_tracks = {self.max_tracks} exhausted: no free slot for track {k} (close finished tracks, set "
                               "max_idle, or size the stream for more tracks)")
        self.tick += 1
        closed = self._release(idle)
        T = self.seg_len
        slots = np.empty(len(keys), np.int64)
        for i, k in enumerate(keys):
            s = self.slot_of.get(k)
            if s is None:
                s = self.slot_of[k] = self._free.pop()
                self.rows[s] = 0
            slots[i] = s
        r = self.rows[slots]                                          # the new rows' indices (slots are distinct within a tick)
        self._fids[slots] = np.concatenate([self._fids[slots, 1:], fids[:, None].astype(np.int32)], axis=1)
        self.rows[slots] = r + 1
        self._last_tick[slots] = self.tick
        emit = r + 1 >= T
        desc = np.stack([slots, r, np.where(emit, np.cumsum(emit) - 1, -1)], axis=1).astype(np.int32)
        win = np.stack([slots[emit], r[emit]], axis=1).astype(np.int32)
        ekeys = [keys[i] for i in np.flatnonzero(emit).tolist()]
        frames = self._fids[win[:, 0]].copy()
        base = (win[:, 0].astype(np.int64) * 2 * self.ring_len + (win[:, 1].astype(np.int64) - T + 1) % self.ring_len) * ROW
        meta = np.concatenate([np.asarray(ekeys, np.int64).reshape(-1, 3), frames[:, :1].astype(np.int64)], axis=1)
        return TickPlan(desc, win, base, ekeys, meta, frames, closed)


@dataclass
class GroupPlan:
    """Consecutive ticks of one call that share their launches (pack_ticks; PoseStream.push: the one tick of the call): one
    upload, one mcd_stream_push_group, one scoring call, one mcd_stream_frame_scores_group.  The group's windows are tick-major,
    inside a tick transform-major: the window of the j-th emitting row of tick i under transform t is at batch position
    offsets[i] * num_transform + t * n_emit_i + j (a group of one tick: t * n_emit + j, the dataset order)."""
    first_tick: int                   # index of the group's first tick in the call
    plans: List[TickPlan]             # the plans of its ticks, exactly those of sequential TrackTable.push calls
    desc: np.ndarray                  # (n, 4) int32 per pushed row, tick after tick: [slot, row index r, pos0 | -1, n_emit of its tick]
    win: np.ndarray                   # (n_windows, 5) int32 [slot, r_last, pos0, n_emit of its tick, index in (tick, j) order],
    #                                   sorted by slot, then row: the windows of a track are adjacent and ascending
    offsets: np.ndarray               # (len(plans) + 1,) int64 windows (one transform) emitted before each tick of the group
    closed: ClosePlan                 # the idle closures of all its ticks, tick after tick (none of them got a row in the group)
    clip: Optional[list] = None       # with online clip scores: the ClipTick of each of its ticks (pack_ticks(..., clips=))

    @property
    def n_rows(self) -> int:
        return int(self.desc.shape[0])

    @property
    def n_windows(self) -> int:
        return int(self.offsets[-1])


def _group(first_tick: int, plans: List[TickPlan], num_transform: int, seg_len: int) -> GroupPlan:
    # (per-tick host work of PoseStream.push too: the tables are filled in place, a group of one tick takes no concatenation)
    offs = [0]
    for p in plans:
        offs.append(offs[-1] + p.n_emit)
    desc = np.empty((sum(len(p.desc) for p in plans), 4), np.int32)
    win = np.empty((offs[-1], 5), np.int32)
    r0 = 0
    for i, p in enumerate(plans):
        w0, ne, r1 = offs[i], offs[i + 1] - offs[i], r0 + len(p.desc)
        d, w = desc[r0:r1], win[w0:w0 + ne]
        d[:, :3] = p.desc                                      # [slot, r, j | -1] -> pos0 = off_i + j; -1 stays -1
        if w0:
            d[:, 2] += np.where(p.desc[:, 2] >= 0, w0 * num_transform, 0).astype(np.int32)
        d[:, 3] = ne
        w[:, :2] = p.win
        w[:, 2] = np.arange(w0 * num_transform, w0 * num_transform + ne, dtype=np.int32)
        w[:, 3] = ne
        w[:, 4] = np.arange(w0, w0 + ne, dtype=np.int32)
        r0 = r1
    offsets = np.asarray(offs, np.int64)
    win = win[np.argsort(win[:, 0], kind="stable")]            # (stable: within a slot the ticks, hence the rows, stay ascending)
    if len(plans) == 1:
        closed = plans[0].closed         # (nothing to merge: the ClosePlan of the tick itself)
    else:
        closed = ClosePlan()
        for p in plans:
            closed.keys += p.closed.keys
            closed.slots += p.closed.slots
        closed.win = np.concatenate([p.closed.win for p in plans]).reshape(-1, 2)
        closed.frames = np.concatenate([p.closed.frames for p in plans]).reshape(-1, seg_len - 1)
    return GroupPlan(first_tick, plans, desc, win, offsets, closed)


def pack_ticks(table: TrackTable, ticks, num_transform: int = 1, max_rows: Optional[int] = None, clips: Optional["ClipTable"] = None):
    """Plan a call of several ticks: ticks = [(keys, frame_ids), ...], each what one TrackTable.push takes.  Pure host logic on a
    COPY of `table` -> (groups, the copy after the last tick); `table` itself is not changed, so a call that is rejected at tick
    i (ValueError / RuntimeError of TrackTable.push, with "tick i: " in front) leaves no trace.  The caller adopts the copy.

    Consecutive ticks share a group as long as
      1. no track receives more than ring_len - seg_len + 1 rows in it (a track that gets R rows needs its rows
         r0 - seg_len + 1 .. r0 + R - 1 alive at once: ring_len >= seg_len + R - 1; the same bound keeps a frame-score cell that
         is zeroed from aliasing a pending one),
      2. no slot that received a row in it is freed inside it (max_idle closes its track, whether or not the slot is handed out
         again at once) -- idle closures of tracks WITHOUT a row in the group stay inside: their cells are final before the
         group's first launch,
      3. its rows number at most `max_rows` (default max_tracks * (ring_len - seg_len + 1), at least max_tracks).
    With ring_len = seg_len every group is one tick.
    clips: the stream's ClipTable (online clip scores): every tick is checked and planned on a COPY of it as well, in the order
    sequential pushes would (ClipTable.check, TrackTable.push, ClipTable.push), each GroupPlan carries the ClipTicks of its ticks
    (their row numbers count within the group) and the result is (groups, table copy, clip table copy)."""
    work = table.copy()
    cwork = None if clips is None else clips.copy()
    pend = table.seg_len - 1
    per_track = table.ring_len - table.seg_len + 1
    cap = table.max_tracks * per_track if max_rows is None else int(max_rows)
    if cap < table.max_tracks:
        raise ValueError(f"max_rows = {cap} is less than max_tracks = {table.max_tracks}: one tick would not fit a group")
    groups: List[GroupPlan] = []
    first, plans, count, n_rows, cticks = 0, [], {}, 0, []

    def cut():
        groups.append(_group(first, plans, num_transform, table.seg_len))
        if cwork is not None:
            groups[-1].clip = cticks

    for i, (keys, fids) in enumerate(ticks):
        try:
            if cwork is not None:
                keys = [_key(k) for k in keys]
                cwork.check(keys, fids, True)
            plan = work.push(keys, fids)
        except (ValueError, RuntimeError) as e:
            raise type(e)(f"tick {i}: {e}") from None
        slots = plan.desc[:, 0].tolist()
        # (ring_len = seg_len: one tick per group, today's launches, also where two ticks happen to share no track)
        if plans and (per_track == 1 or n_rows + len(slots) > cap or any(count.get(s, 0) >= per_track for s in slots)
                      or any(s in count for s in plan.closed.slots)):
            cut()
            first, plans, count, n_rows, cticks = i, [], {}, 0, []
        if cwork is not None:
            cticks.append(cwork.push(plan, keys, fids, final0=sum(p.n_emit for p in plans),
                                     tail0=pend * sum(len(p.closed) for p in plans), normalised=True))
        plans.append(plan)
        n_rows += len(slots)
        for s in slots:
            count[s] = count.get(s, 0) + 1
    if plans:
        cut()
    return (groups, work) if clips is None else (groups, work, cwork)


# ----------------------------------------------------------------------------------------------------------------------
# Online clip scores (include/mocodad_hip.h: mcd_clip_state_t): one value per video frame of a clip, the number the
# model is evaluated on, incrementally.  Definitions (f = frame id, t = transform):
#   contribution  s_p(f, t) = the FINAL frame score of person p's row at frame f (Tick.final / Tick.closed / close()); rows of
#                 tracks that end with fewer than seg_len rows have none, as offline.
#   raw(f, t)     = sum_p s_p / n + (max_p log1p s_p - min_p log1p s_p) over the n contributing persons, float64; 0 for n = 0.
#                 (The dataset path's dense matrix counts every person of the WHOLE clip, absent ones as zeros, so there a frame's
#                 value depends on who appears later; a live clip has no final roster.  Where every person contributes to every
#                 frame the two coincide.)
#   shifted(k)    = raw(k - shift) for k - origin >= shift, else 0;  out(., t) = scipy gaussian_filter1d(shifted, sigma)
#                 (truncate 4, 'reflect', radius R = int(4 sigma + 0.5)) over the SEGMENT origin .. head;
#                 score(j) = sum_t out(j, t) / num_transform.
#   complete      raw(f) is complete when no open track of the clip has a pending (pushed, not yet final) row at a frame <= f and
#                 the clip's head (largest pushed frame id) is >= f.  The WATERMARK is the smallest frame that is not complete.
#   emission      frame j is emitted once every frame <= j + R - shift is complete and the head is >= j + R (every tap right of j
#                 then lies inside the segment whatever comes later, so the value is the one the filter over the whole segment
#                 gives); each frame once, ascending.  Ending a segment (close_clip, a frame-id jump) emits the rest, up to the
#                 head, with the reflection at the end.
# pad_size and the HR masks of the dataset path are not applied: they need the clip's final length.
# ----------------------------------------------------------------------------------------------------------------------
Clip = Tuple[int, int]


@dataclass
class ClipScoreCfg:
    """PoseStream(clip_scores=ClipScoreCfg(...)).  sigma / shift: None = the model's filter_kernel_size / frames_shift;
    max_clips: clip slots of the device rings; clip_ring_len: frames a clip's ring holds, default
    2 R + shift + seg_len + (max_idle or 64) + (ring_len - seg_len + 1) + 1."""
    sigma: Optional[float] = None
    shift: Optional[int] = None
    max_clips: int = 64
    clip_ring_len: Optional[int] = None


@dataclass
class ClipFrames:
    """Clip scores emitted by one tick (Tick.clip) or by close_clip: values[i] (fp64, device) is the score of frame frames[i] of
    clip clips[i] = (scene, clip); per clip the frames ascend, and over a clip's life every frame origin .. head comes once.
    dropped_rows: final row scores that arrived for frames of an already ended segment (or closed clip) and were not used."""
    clips: List[Clip]
    frames: np.ndarray
    values: "object"
    dropped_rows: int = 0

    def __len__(self):
        return len(self.clips)


@dataclass
class ClipTick:
    """What one tick (ClipTable.push), one close (ClipTable.close) or the end of a clip (ClipTable.end_clip) does to the clip
    rings.  Cells are numbered per clip slot by a counter that never wraps; the ring position of cell c is c % clip_ring_len."""
    opened: List[Tuple[int, int]]                 # (clip slot, cell) newly opened: zeroed before anything is added
    contribs: List[Tuple[int, int, int, int]]     # (clip slot, cell, source: 0 = finals | 1 = tails, row), in order of addition
    outs: np.ndarray                              # (n_out, 4) int32 [clip slot, frame offset, segment length | -1, ring position of the origin]
    clips: List[Clip]                             # (n_out) the clip of each output
    frames: np.ndarray                            # (n_out,) int32 its frame id
    dropped: int                                  # contributions for frames of ended segments
    span: Dict[int, Tuple[int, int]]              # clip slot -> (lowest cell alive at the start, highest cell after it)
    n_pre: int = 0                                # the first n_pre outputs are emitted BEFORE the update (catch-up after a close)

    @property
    def n_out(self) -> int:
        return int(self.outs.shape[0])


@dataclass
class ClipLaunch:
    """One mcd_stream_clip_update + one mcd_stream_clip_emit: the ClipTicks of consecutive ticks merged (merge_clip_ticks)."""
    runs: np.ndarray                  # (n_runs, 5) int32 [clip slot, ring position, first contribution, count, zero-first]
    contrib: np.ndarray               # (n_contrib, 2) int32 [source, row]
    outs: np.ndarray                  # (n_out, 4) int32, tick after tick
    n_out: List[int]                  # outputs of each tick
    n_pre: int = 0                    # outputs (the first ones) to emit before the update launch: ClipTick.n_pre of the first tick


def merge_clip_ticks(ticks: Sequence[ClipTick], ring_len: int) -> ClipLaunch:
    """One launch pair for consecutive ticks: one run per cell touched, its contributions tick after tick in their order within
    the tick.  (batch_clip_ticks says which ticks may share a launch.)"""
    cells: Dict[Tuple[int, int], list] = {}
    for t in ticks:
        for sc in t.opened:
            cells[sc] = [1, []]
        for s, c, src, row in t.contribs:
            cells.setdefault((s, c), [0, []])[1].append((src, row))
    runs, contrib = [], []
    for (s, c), (zero, lst) in cells.items():
        runs.append((s, c % ring_len, len(contrib), len(lst), zero))
        contrib += lst
    if len({(r[0], r[1]) for r in runs}) != len(runs):
        raise AssertionError("two cells of one launch share a ring position")      # (batch_clip_ticks / ClipTable.check prevent it)
    outs = np.concatenate([t.outs for t in ticks]).reshape(-1, 4) if ticks else np.zeros((0, 4), np.int32)
    if any(t.n_pre for t in ticks[1:]):
        raise AssertionError("only the first tick after a close catches up")
    return ClipLaunch(np.asarray(runs, np.int32).reshape(-1, 5), np.asarray(contrib, np.int32).reshape(-1, 2),
                      outs.astype(np.int32), [t.n_out for t in ticks], ticks[0].n_pre if ticks else 0)


def batch_clip_ticks(ticks: Sequence[ClipTick], ring_len: int) -> List[List[int]]:
    """Consecutive ticks (indices) that may share one launch pair.  The emit launch of a batch runs after its update launch, so
    the cells a tick's outputs read must survive the cells later ticks of the batch open: per clip, the lowest cell alive at the
    batch's first tick and the highest cell after its last lie within one ring.  ClipTable.check guarantees that for every single
    tick; a group whose clip advances further (frame-id gaps inside a group) is cut into more than one launch pair."""
    batches, cur, lo = [], [], {}
    for i, t in enumerate(ticks):
        if cur and any(hi - lo.get(s, l) + 1 > ring_len for s, (l, hi) in t.span.items()):
            batches.append(cur)
            cur, lo = [], {}
        cur.append(i)
        for s, (l, _) in t.span.items():
            lo.setdefault(s, l)
    if cur:
        batches.append(cur)
    return batches


class ClipTable:
    """Host half of the online clip scores: (scene, clip) -> slot of the clip rings (free list; opened by the clip's first row,
    freed by end_clip), per clip the current SEGMENT's origin and head, the completeness watermark and the emit cursor, per
    open track its pending frame ids; from a TickPlan plus the keys and frame ids pushed it plans the cell runs, the contribution
    list and the outputs of the two launches.  Plain NumPy, no GPU module (like TrackTable).

    Rules, all decided in `check` before any change (a rejected tick leaves this table as it was):
      late rows     a row whose frame id is below the clip's watermark is a ValueError; rows from the watermark on are accepted.
      ring          the cells alive run from frame (next to emit) - R - shift to the head; a push that would overwrite one raises
                    RuntimeError (a stalled track holds the watermark back).
      jumps         a head that advances by more than the free part of the ring ends the clip's segment (its tail is emitted
                    with the reflection at the end, tracks stay open) and starts a new one whose origin is the smallest new frame
                    id beyond the old head; if even that does not fit beside the live cells: the RuntimeError above.  Finals that
                    arrive later for frames of an ended segment are dropped and counted.
      clip slots    no free slot for a new clip: RuntimeError.
    Contributions to one cell are added tick by tick, within a tick in ascending person id (finals and idle tails alike).
    Emission is planned by push and end_clip only.  An explicit close moves watermarks but emits nothing; the frames it made
    computable are the FIRST outputs of the next push (ClipTick.n_pre), emitted before that tick's update launch -- so the cells
    they read count as free for that tick's rows, and closing a stalled track does unblock a full ring."""

    def __init__(self, max_clips: int, clip_ring_len: int, radius: int, shift: int, seg_len: int):
        self.max_clips, self.ring_len = int(max_clips), int(clip_ring_len)
        self.radius, self.shift, self.seg_len = int(radius), int(shift), int(seg_len)
        if self.max_clips < 1 or self.radius < 0 or self.shift < 0 or self.seg_len < 1:
            raise ValueError("max_clips and seg_len must be at least 1, the radius and the shift not negative")
        if self.ring_len < 2 * self.radius + self.shift + 1:
            raise ValueError(f"clip_ring_len = {self.ring_len} is shorter than 2 R + shift + 1 = {2 * self.radius + self.shift + 1}: "
                             "the cells one output reads would not fit")
        self.slot_of: Dict[Clip, int] = {}
        self._free = list(range(self.max_clips - 1, -1, -1))
        self._clip_of: List[Optional[Clip]] = [None] * self.max_clips
        z = lambda: [0] * self.max_clips             # (per clip slot; plain ints: this is per-tick host work)
        self.origin, self.head, self.cursor, self.cbase, self.wm = z(), z(), z(), z(), z()
        self._tracks: Dict[int, list] = {}           # track slot -> [key, pending frame ids (oldest first), rows pushed]
        self._of_clip: Dict[int, List[int]] = {}     # clip slot -> its open track slots
        self._stale = set()                          # clip slots whose watermark a close moved since their last emission
        self.tick = 0
        self.dropped_total = 0

    def __len__(self):
        return len(self.slot_of)

    def copy(self) -> "ClipTable":
        t = ClipTable.__new__(ClipTable)
        t.__dict__.update(self.__dict__)
        t.slot_of, t._free, t._clip_of = dict(self.slot_of), list(self._free), list(self._clip_of)
        t.origin, t.head, t.cursor, t.cbase, t.wm = (list(a) for a in (self.origin, self.head, self.cursor, self.cbase, self.wm))
        t._tracks = {s: [r[0], list(r[1]), r[2]] for s, r in self._tracks.items()}
        t._of_clip = {s: list(v) for s, v in self._of_clip.items()}
        t._stale = set(self._stale)
        return t

    def same_state(self, other: "ClipTable") -> bool:
        cfg = lambda c: (c.max_clips, c.ring_len, c.radius, c.shift, c.seg_len, c.tick, c.dropped_total)
        return (cfg(self) == cfg(other) and list(self.slot_of.items()) == list(other.slot_of.items()) and self._free == other._free
                and self._clip_of == other._clip_of and self._tracks == other._tracks and self._of_clip == other._of_clip
                and self._stale == other._stale
                and (self.origin, self.head, self.cursor, self.cbase, self.wm)
                == (other.origin, other.head, other.cursor, other.cbase, other.wm))

    def adopt(self, other: "ClipTable") -> None:
        self.__dict__.update(other.__dict__)

    # ---- geometry of a clip slot
    def _cell(self, cs: int, f: int) -> int:
        return int(self.cbase[cs] + f - self.origin[cs])

    def _cursor_now(self, cs: int) -> int:
        """The next frame to emit -- after the catch-up the next push starts with, if a close moved the clip's watermark."""
        c = int(self.cursor[cs])
        if cs in self._stale:
            c = max(c, min(int(self.wm[cs]) - 1 + self.shift, int(self.head[cs])) - self.radius + 1)
        return c

    def _lo_cell(self, cs: int) -> int:
        """The lowest cell still alive: an output at the cursor reads down to frame cursor - R - shift."""
        return self._cell(cs, max(int(self.origin[cs]), self._cursor_now(cs) - self.radius - self.shift))

    def _watermark(self, cs: int) -> int:
        w, o = int(self.head[cs]) + 1, int(self.origin[cs])
        for ts in self._of_clip[cs]:
            for f in self._tracks[ts][1]:
                if o <= f < w:
                    w = f
        return w

    def _decide(self, cs: int, fl: List[int]):
        """New frame ids of a clip -> None (no advance) | ("advance", head) | ("jump", origin, head); RuntimeError if neither fits."""
        hmax, head = max(fl), int(self.head[cs])
        if hmax <= head:
            return None
        lo, hc = self._lo_cell(cs), self._cell(cs, head)
        if hc + (hmax - head) - lo + 1 <= self.ring_len:
            return ("advance", hmax)
        o2 = min(f for f in fl if f > head)
        if hc + 1 + (hmax - o2) - lo + 1 <= self.ring_len:
            return ("jump", o2, hmax)
        raise RuntimeError(f"clip {self._clip_of[cs]}: frame {hmax} would overwrite a live cell of the clip ring (clip_ring_len = "
                           f"{self.ring_len}, frames {int(self.origin[cs]) + lo - int(self.cbase[cs])} .. {head} alive: a track with "
                           "pending rows holds the watermark back): close idle tracks, set max_idle, or size clip_ring_len")

    @staticmethod
    def _by_clip(keys, fids) -> Dict[Clip, List[int]]:
        out: Dict[Clip, List[int]] = {}
        for k, f in zip(keys, fids):
            out.setdefault(k[:2], []).append(f)
        return out

    def check(self, keys, frame_ids, normalised: bool = False) -> None:
        """The rules above for one tick, on the state BEFORE it; changes nothing.  normalised: keys are tuples of ints already."""
        if not normalised:
            keys = [_key(k) for k in keys]
        fids = np.asarray(frame_ids, dtype=np.int64).reshape(-1).tolist()
        if len(fids) != len(keys):
            raise ValueError(f"{len(keys)} keys but {len(fids)} frame ids")
        new = 0
        for clip, fl in self._by_clip(keys, fids).items():
            cs = self.slot_of.get(clip)
            if cs is None:
                new += 1
                if new > len(self._free):
                    raise RuntimeError(f"max_clips = {self.max_clips} exhausted: no clip slot for clip {clip} (close_clip finished "
                                       "clips, or size the stream for more clips)")
                if max(fl) - min(fl) + 1 > self.ring_len:
                    raise RuntimeError(f"clip {clip}: frames {min(fl)} .. {max(fl)} of one tick exceed clip_ring_len = {self.ring_len}")
            else:
                if min(fl) < self.wm[cs]:
                    raise ValueError(f"late row (tick {self.tick + 1} of the stream): frame {min(fl)} of clip {clip} is below the "
                                     f"clip's completeness watermark {int(self.wm[cs])}: its score is final")
                self._decide(cs, fl)

    # ---- planning
    def _finish(self, touched, ended, raw, opened, span, emit: bool = True, pre=None) -> ClipTick:
        """Resolve the tick's contributions (ascending person id) to cells, move the watermarks, then (emit) plan the outputs that
        became computable."""
        raw.sort(key=lambda c: c[2])                  # (stable: a person's tail rows stay in frame order)
        contribs, dropped = [], 0
        for cs, f, _, src, row in raw:
            e = ended.get(cs)
            if self.origin[cs] <= f <= self.head[cs]:
                contribs.append((cs, self._cell(cs, f), src, row))
            elif e is not None and e[0] <= f <= e[1]:
                contribs.append((cs, int(e[3] + f - e[0]), src, row))
            else:
                dropped += 1
        self.dropped_total += dropped
        outs, oc, of = pre if pre is not None else ([], [], [])
        n_pre = len(outs)
        L, R, sh = self.ring_len, self.radius, self.shift
        for cs in sorted(touched):
            clip = self._clip_of[cs]
            if cs in ended:
                o, h, c, b = ended[cs]
                for j in range(c, h + 1):
                    outs.append((cs, j - o, h - o + 1, b % L)); oc.append(clip); of.append(j)
            w = self._watermark(cs)
            self.wm[cs] = w
            if not emit:
                continue
            o, b = int(self.origin[cs]), int(self.cbase[cs])
            jmax = min(w - 1 + sh, int(self.head[cs])) - R
            for j in range(int(self.cursor[cs]), jmax + 1):
                outs.append((cs, j - o, -1, b % L)); oc.append(clip); of.append(j)
            self.cursor[cs] = max(int(self.cursor[cs]), jmax + 1)
        return ClipTick(opened, contribs, np.asarray(outs, np.int32).reshape(-1, 4), oc, np.asarray(of, np.int32), dropped,
                        {s: (a, b) for s, (a, b) in span.items()}, n_pre)

    def _drop_tracks(self, plan: ClosePlan, tail0: int, raw, touch) -> None:
        pend, ci = self.seg_len - 1, 0
        for ts in plan.slots:
            key, _, rows = self._tracks.pop(int(ts))
            cs = self.slot_of[key[:2]]
            self._of_clip[cs].remove(int(ts))
            touch(cs)
            if rows >= self.seg_len:
                if plan.keys[ci] != key:
                    raise AssertionError(f"close plan names {plan.keys[ci]}, the clip table holds {key}")
                raw += [(cs, int(plan.frames[ci, k]), key[2], 1, tail0 + ci * pend + k) for k in range(pend)]
                ci += 1

    def push(self, plan: TickPlan, keys, frame_ids, final0: int = 0, tail0: int = 0, normalised: bool = False) -> ClipTick:
        """One tick, after `check` passed and TrackTable.push returned `plan` for the same keys and frame ids.  final0 / tail0:
        rows of the finals / tails tensors at which this tick's finals / idle tails start (a group of ticks shares them)."""
        if not normalised:
            keys = [_key(k) for k in keys]
        fids = np.asarray(frame_ids, dtype=np.int64).reshape(-1).tolist()
        self.tick += 1
        opened, raw, span, ended = [], [], {}, {}
        pre = ([], [], [])
        for cs in sorted(self._stale):               # catch up on what closes since the last push made computable
            c, o = self._cursor_now(cs), int(self.origin[cs])
            for j in range(int(self.cursor[cs]), c):
                pre[0].append((cs, j - o, -1, int(self.cbase[cs]) % self.ring_len)); pre[1].append(self._clip_of[cs]); pre[2].append(j)
            self.cursor[cs] = c
        self._stale.clear()

        def touch(cs):
            if cs not in span:
                span[cs] = [self._lo_cell(cs), self._cell(cs, int(self.head[cs]))]

        self._drop_tracks(plan.closed, tail0, raw, touch)
        for clip, fl in self._by_clip(keys, fids).items():
            cs = self.slot_of.get(clip)
            if cs is None:
                cs = self.slot_of[clip] = self._free.pop()
                self._clip_of[cs], self._of_clip[cs] = clip, []
                o, h = min(fl), max(fl)
                self.origin[cs], self.head[cs], self.cursor[cs], self.cbase[cs], self.wm[cs] = o, h, o, 0, o
                opened += [(cs, c) for c in range(h - o + 1)]
                span[cs] = [0, h - o]
                continue
            touch(cs)
            d = self._decide(cs, fl)
            if d is None:
                continue
            hc = self._cell(cs, int(self.head[cs]))
            if d[0] == "advance":
                opened += [(cs, c) for c in range(hc + 1, hc + 1 + d[1] - int(self.head[cs]))]
                self.head[cs] = d[1]
            else:
                ended[cs] = (int(self.origin[cs]), int(self.head[cs]), int(self.cursor[cs]), int(self.cbase[cs]))
                self.origin[cs], self.head[cs], self.cursor[cs], self.cbase[cs] = d[1], d[2], d[1], hc + 1
                opened += [(cs, c) for c in range(hc + 1, hc + 2 + d[2] - d[1])]
            span[cs][1] = self._cell(cs, int(self.head[cs]))
        for (ts, r, j), k, f in zip(plan.desc.tolist(), keys, fids):
            cs = self.slot_of[k[:2]]
            if r == 0:
                self._tracks[ts] = [k, [], 0]
                self._of_clip[cs].append(ts)
            rec = self._tracks[ts]
            rec[1].append(f)
            rec[2] += 1
            if j >= 0:
                raw.append((cs, rec[1].pop(0), k[2], 0, final0 + j))
        return self._finish(set(span), ended, raw, opened, span, pre=pre)

    def close(self, plan: ClosePlan, tail0: int = 0) -> ClipTick:
        """Tracks closed by TrackTable.close: their tails are contributions; nothing is emitted (the next push or end_clip does)."""
        raw, span = [], {}

        def touch(cs):
            if cs not in span:
                span[cs] = [self._lo_cell(cs), self._cell(cs, int(self.head[cs]))]

        self._drop_tracks(plan, tail0, raw, touch)
        self._stale |= set(span)
        return self._finish(set(span), {}, raw, [], span, emit=False)

    def tracks_of(self, clip) -> List[Key]:
        """The open tracks of a clip, in the order they were opened."""
        cs = self.slot_of[(int(clip[0]), int(clip[1]))]
        return [self._tracks[ts][0] for ts in self._of_clip[cs]]

    def end_clip(self, clip) -> ClipTick:
        """Free the clip's slot (all of its tracks are closed) -> the outputs of its remaining frames, cursor .. head, with the
        reflection at the end of the segment."""
        clip = (int(clip[0]), int(clip[1]))
        cs = self.slot_of.get(clip)
        if cs is None:
            raise KeyError(f"clip {clip} is not open")
        if self._of_clip[cs]:
            raise ValueError(f"clip {clip} still has open tracks: {self.tracks_of(clip)}")
        o, h, c, b = int(self.origin[cs]), int(self.head[cs]), int(self.cursor[cs]), int(self.cbase[cs])
        fr = np.arange(c, h + 1, dtype=np.int64)
        outs = np.stack([np.full_like(fr, cs), fr - o, np.full_like(fr, h - o + 1), np.full_like(fr, b % self.ring_len)], axis=1)
        span = {cs: (self._lo_cell(cs), self._cell(cs, h))}
        del self.slot_of[clip], self._of_clip[cs]
        self._stale.discard(cs)
        self._clip_of[cs] = None
        self._free.append(cs)
        return ClipTick([], [], outs.astype(np.int32).reshape(-1, 4), [clip] * len(fr), fr.astype(np.int32), 0, span)


# ----------------------------------------------------------------------------------------------------------------------
# Expected poses (include/mocodad_hip.h: mcd_stream_forecast_state_t).  Definition, the dataset path's
# (eval_MoCoDAD.py --forecast-tracks = mcd_forecast_assemble + mcd_denormalize_poses): for row r of a track take the windows of
# transform 0 that FORECAST it -- row r is the window's corrupt frame j when the window ends at row r + seg_len - 1 - corrupt_idx[j]
# -- each with its selected forecast (the pose of the model's best / worst sample; zeros when no sample passes); combine them in
# ascending window order in float64 (unique / mean / median per feature, the population standard deviation per feature and its mean
# or median over the 34 features), and take the result to pixels in the bounding box of the observed row.  A row is final with the
# window whose oldest row it is: every window covering it is in by then.  At a close the pending rows see the windows that exist.
# ----------------------------------------------------------------------------------------------------------------------
FORECAST_METHODS = ("unique", "mean", "median")
FORECAST_SPREADS = ("mean", "median")
FORECAST_TRANSFORMS = ("identity", "all")


@dataclass
class ForecastCfg:
    """PoseStream(forecasts=ForecastCfg(...)): method / spread as eval_MoCoDAD.py's --forecast-method / --forecast-spread;
    transforms as its --forecast-transforms: 'identity' -- the windows of transform 0 forecast a row -- or 'all' -- the windows of
    every transform do, each forecast mapped back through the inverse of its transform and combined transform-major, then in window
    order (up to num_transform * n_corrupt <= 64 forecasts per row; forecast_track_rows(transforms='all') bit for bit)."""
    method: str = "median"
    spread: str = "mean"
    transforms: str = "identity"


def forecast_cover(corrupt_idx: Sequence[int], seg_len: int, r: int, r_last: int) -> List[Tuple[int, int]]:
    """The windows of a track that forecast its row r, the track's last row so far being r_last: [(window end row, j)] in window
    order (ascending end row), j = the index among the corrupt frames at which the window holds the row.  A window ending at row e
    covers rows e - seg_len + 1 .. e and exists when seg_len - 1 <= e <= r_last.  (At finality r_last = r + seg_len - 1.)"""
    seg_len, r, r_last = int(seg_len), int(r), int(r_last)
    out = []
    for j, c in enumerate(corrupt_idx):
        e = r + seg_len - 1 - int(c)
        if int(c) <= r and e <= r_last:
            out.append((e, j))
    return sorted(out)


@dataclass
class ForecastRows:
    """Expected poses, row for row with the FrameScores that carries them (device tensors): expected (n, 34) fp32 image pixels in
    the CSV's order x1,y1,...,x17,y17; expected_norm (n, 34) fp32 the same pose in normalised coordinates; observed (n, 34) fp32
    the raw row the track pushed for that frame; count (n,) int32 windows that forecast the row (0: expected, expected_norm and
    spread are zero -- the first rows of a track); spread (n,) fp32 their disagreement."""
    expected: "object"
    expected_norm: "object"
    observed: "object"
    count: "object"
    spread: "object"

    def __len__(self):
        return int(self.count.shape[0])

    def rows(self, a: int, b: int) -> "ForecastRows":
        return ForecastRows(self.expected[a:b], self.expected_norm[a:b], self.observed[a:b], self.count[a:b], self.spread[a:b])


@dataclass
class FrameScores:
    """Final per-row frame scores: row i belongs to track keys[i] at frame id frames[i]; values (n, num_transform) fp32 on the
    device = the maximum over the windows of that track covering the row, per transform."""
    keys: List[Key]
    frames: np.ndarray
    values: "object"
    joints: "object" = None           # PoseStream(joint_scores=True): (n, num_transform, 17) fp32 device, the same rows per joint
    forecast: Optional[ForecastRows] = None   # PoseStream(forecasts=...): the expected poses of the same rows

    def __len__(self):
        return len(self.keys)

    def rows(self, a: int, b: int) -> "FrameScores":
        return FrameScores(self.keys[a:b], self.frames[a:b].copy(), self.values[a:b], None if self.joints is None else self.joints[a:b],
                           None if self.forecast is None else self.forecast.rows(a, b))


@dataclass
class Tick:
    """Result of PoseStream.push (push_many: one per tick).  The tick's windows are transform-major like the dataset order: entry t * n_emit + j is the
    window of the j-th emitting track under transform t."""
    meta: np.ndarray                  # (num_transform * n_emit, 4) int64
    frames: np.ndarray                # (num_transform * n_emit, seg_len) int32
    trans: np.ndarray                 # (num_transform * n_emit,) int64
    scores: "object"                  # (num_transform * n_emit,) fp32 device tensor (empty when no window was emitted)
    windows: "object"                 # the tick's WindowBatch over the pose ring (None without a window); its rows stay in
    #                                   place for the next ring_len - seg_len pushes of their track
    final: FrameScores                # the row each emitted window finalised
    closed: FrameScores               # tails of the tracks max_idle closed at the start of this tick
    first_window_id: int              # windows this stream had emitted before the tick (keys the in-kernel noise)
    clip: Optional[ClipFrames] = None  # PoseStream(clip_scores=...): the clip scores that became computable with this tick
    joint_final: "object" = None      # PoseStream(joint_scores=True): (n_emit, num_transform, 17) fp32 device, row for row with
    #                                   `final` (= final.joints): per joint the maximum over the windows FORECASTING the row; 0 for
    #                                   a row no window forecasts (the first n_cond rows of a track).  closed.joints: the tails
    forecast: Optional[ForecastRows] = None   # PoseStream(forecasts=...): the expected poses, row for row with `final`
    #                                   (= final.forecast).  closed.forecast: the tails


class PoseStream:
    """Online scoring of live pose tracks with `model` (a MoCoDAD or MoCoDADlatent module on a cuda device).

    vid_res, center, scale: as for engine.normalize_poses (center / scale (34,) = the fitted RobustScaler, or both None).
    max_tracks: slots of the device rings; ring_len: rows kept per track (>= seg_len, default seg_len);
    num_transform: default the model's; max_idle: see TrackTable; max_group_rows: cap on the rows of one launch group of
    push_many (default and upper limit max_tracks * (ring_len - seg_len + 1), at least max_tracks): it sizes the staging buffers.
    clip_scores: None, or a ClipScoreCfg: online per-clip frame scores (the definitions above ClipScoreCfg) -- every Tick then
    carries `clip`, the ClipFrames that became computable with it, and close_clip ends a clip.  The model's pad_size and the HR
    masks are NOT applied online (they need the clip's final length: evaluation devices of the dataset path); whatever
    anomaly_score_pad_size the model has is ignored here.  With clip_scores = None nothing of this runs.
    joint_scores: per-joint frame scores beside the frame scores (pose model only): every scoring call also yields the error maps
    of its windows (mcd_error_maps), a second ring (max_tracks, num_transform, ring_len, 17) takes their per-row, per-joint
    maximum (mcd_stream_joint_scores_group), and `Tick.joint_final`, `Tick.closed.joints` and the `joints` of what `close`
    returns carry them row for row with the frame scores -- bit for bit the dataset path's mcd_joint_scatter_max.  Off (the
    default): no extra launch, no poses requested, nothing allocated.
    forecasts: None, or a ForecastCfg: the expected pose of every row (pose model with fixed conditioning indices and a
    best / worst aggregation only; the definition stands above ForecastCfg).  Every scoring call then also writes the per-sample
    losses and poses, mcd_stream_forecast_group keeps each transform-0 window's selected forecast and the raw rows in two more
    rings and reduces the rows that became final, and `Tick.forecast`, `Tick.closed.forecast` and the `forecast` of what `close`
    returns carry them row for row with the frame scores -- bit for bit eval_MoCoDAD.py's --forecast-tracks.  Off (the default):
    no extra launch, no poses requested, nothing allocated.
    space (MoCoDADlatent only): None = the module's `latent_score_space`, or 'latent' / 'pose'.  In pose space (needs
    load_decoder; RuntimeError with forward's message otherwise) the tick's scoring call is engine.LatentPoseScorer.score
    (mcd_latent_score_pose): `Tick.scores` are the losses of the decoded forecasts against the corrupt frames, the numbers
    eval_MoCoDAD.py gives for the same module, and joint_scores / forecasts work as for the pose model (the decoder handle's frame
    lists).  In latent space both stay refused, and no decoder is packed.

    One PoseStream is driven from ONE stream (the current stream of the first push): its rings, staging buffers and the track
    table are per-tick state, and the launches of a tick are ordered only by that stream."""

    def __init__(self, model, *, vid_res, center=None, scale=None, max_tracks: int = 1024, ring_len: Optional[int] = None,
                 num_transform: Optional[int] = None, max_idle: Optional[int] = None, max_group_rows: Optional[int] = None,
                 clip_scores: Optional[ClipScoreCfg] = None, joint_scores: bool = False, forecasts: Optional[ForecastCfg] = None,
                 space: Optional[str] = None):
        from .engine import ClipRings, StreamRings, forecast_codes
        from .utils.transforms import affine_table
        if getattr(model, "is_pretrain", False):
            raise NotImplementedError(f"PoseStream does not take {type(model).__name__}: the pretrain stage of the latent model "
                                      "reconstructs poses and yields no anomaly score per window (score live streams with "
                                      "MoCoDAD or the diffusion-stage MoCoDADlatent)")
        self.latent = bool(getattr(model, "is_latent", False))
        if space is not None and space not in ("latent", "pose"):
            raise ValueError(f"space must be None, 'latent' or 'pose', got {space!r}")
        if space is not None and not self.latent:
            raise ValueError("space= is for the latent model (MoCoDADlatent): the pose model has one score space")
        # the space a latent module is scored in: the module's own (what forward and eval_MoCoDAD.py use) unless `space` says otherwise
        self.space = (getattr(model, "latent_score_space", "latent") if space is None else space) if self.latent else None
        self.pose_space = self.space == "pose"
        self.joint_scores = bool(joint_scores)
        if self.joint_scores and self.latent and not self.pose_space:
            raise NotImplementedError("PoseStream(joint_scores=True) needs the pose model: MoCoDADlatent takes its loss on a latent "
                                      "code, and a latent has no joints (latent_score_space 'pose' / space='pose' with a loaded "
                                      "decoder scores decoded forecasts, which have)")
        self.forecasts = forecasts
        if forecasts is not None:
            if self.latent and not self.pose_space:
                raise NotImplementedError("PoseStream(forecasts=...) needs the pose model: MoCoDADlatent forecasts a latent code "
                                          "(latent_score_space 'pose' / space='pose' with a loaded decoder decodes it to poses)")
            forecast_codes(forecasts.method, forecasts.spread, ("forecasts: method", "forecasts: spread"), f"one of {FORECAST_SPREADS}")
            if model.aggregation_strategy not in ("best", "worst"):
                raise ValueError(f"PoseStream(forecasts=...) needs an aggregation that selects a pose, best or worst: aggregation_strategy "
                                 f"{model.aggregation_strategy!r} aggregates losses and selects none")
            if forecasts.transforms not in FORECAST_TRANSFORMS:
                raise ValueError(f"forecasts: transforms must be one of {FORECAST_TRANSFORMS}, got {forecasts.transforms!r}")
        if self.latent and model.device.type != "cuda":
            raise ValueError("PoseStream scores the latent model (MoCoDADlatent) on a cuda device only: move the module to one "
                             "first (there is no CPU fallback)")
        if model.conditioning_strategy == "random_imp":
            raise ValueError("PoseStream does not support the 'random_imp' strategy (its per-window condition-frame sets are drawn "
                             "on the host per batch); use a model with fixed conditioning indices")
        aggr = model.aggregation_strategy
        if not (aggr in ("best", "worst", "mean", "median") or "quantile" in aggr) or model.model_return_value != "loss":
            raise ValueError(f"PoseStream needs one loss per window: model_return_value 'loss' and a loss-based aggregation "
                             f"(best, worst, mean, median, quantile:q), not {aggr!r} / {model.model_return_value!r}")
        if self.pose_space and getattr(model, "_decoder_sd", None) is None:       # (forward's message; before any device call)
            raise RuntimeError("latent_score_space 'pose' needs the stage-1 decoder: call load_decoder first")
        self.model = model
        # pose space: engine.LatentPoseScorer, whose results have HipScorer.score_fused's layout and whose frame lists are the
        # decoder handle's -- from here on the stream treats it as it treats the pose model's scorer
        self.scorer = model.pose_scorer() if self.pose_space else model.scorer()
        self.device = dev = self.scorer.device
        self.seg_len = int(model.n_frames)
        self.num_transform = nt = max(1, int(model.num_transforms if num_transform is None else num_transform))
        self.table = TrackTable(max_tracks, self.seg_len, ring_len, max_idle)
        n = self.table.max_tracks
        extra = {"joint_scores": True} if self.joint_scores else {}
        if forecasts is not None:
            extra["forecasts"] = (forecasts.method, forecasts.spread, len(self.scorer.corrupt_idx))
            if forecasts.transforms == "all":      # the ring of every transform in place of transform 0's (refused here beyond 64 per row)
                if nt * len(self.scorer.corrupt_idx) > 64:
                    raise ValueError(f"forecasts: transforms='all' puts num_transform * n_corrupt = {nt} * {len(self.scorer.corrupt_idx)} "
                                     "forecasts on a row; the reduction holds 64")
                extra["forecasts"] += ("all",)
        self.rings = StreamRings(n, self.seg_len, self.table.ring_len, nt, vid_res, center, scale, device=dev, **extra)
        self.ring = self.rings.ring
        self.clips, self.clip_rings, clip_words = None, None, 0
        if clip_scores is not None:
            cc = clip_scores
            sigma = float(model.anomaly_score_filter_kernel_size if cc.sigma is None else cc.sigma)
            shift = int(model.anomaly_score_frames_shift if cc.shift is None else cc.shift)
            if not sigma > 0 or shift < 0:
                raise ValueError(f"clip_scores: need sigma > 0 and shift >= 0, got {sigma}, {shift}")
            radius = int(4.0 * sigma + 0.5)
            per_track = self.table.ring_len - self.seg_len + 1
            clen = (2 * radius + shift + self.seg_len + (self.table.max_idle or 64) + per_track + 1
                    if cc.clip_ring_len is None else int(cc.clip_ring_len))
            self.clips = ClipTable(cc.max_clips, clen, radius, shift, self.seg_len)
            self.clip_rings = ClipRings(self.clips.max_clips, clen, nt, sigma, shift, device=dev)
            # one launch pair of a group: a run (5) and an output (4) per cell of the clip rings at most, a contribution (2) per
            # final of the group and per tail row of an idle closure
            clip_words = self.clips.max_clips * clen * 9 + 2 * n * (self.seg_len - 1)
        with torch.cuda.device(dev):
            self.affine = affine_table(nt).to(dev)
            # one group's host-to-device traffic: raw rows (n, 34) f32 | descriptors (n, 4) i32 | windows (n, 5) i32, in ONE copy;
            # a tick of push is a group of one (at most max_tracks rows), a group of push_many holds at most max_group_rows rows
            per_track = self.table.ring_len - self.seg_len + 1
            self.max_group_rows = n * per_track if max_group_rows is None else min(int(max_group_rows), n * per_track)
            if self.max_group_rows < n:
                raise ValueError(f"max_group_rows = {max_group_rows} is less than max_tracks = {n}: one tick would not fit a group")
            words = self.max_group_rows * (ROW + 4 + 5 + (2 if self.clips is not None else 0)) + clip_words
            self._pinned = torch.empty(words, dtype=torch.int32).pin_memory()
            self._staged = torch.empty(words, device=dev, dtype=torch.int32)
            self._copied = torch.cuda.Event()
        self._host = self._pinned.numpy()
        self.n_emitted = 0          # windows (x transforms) emitted so far = first_window_id of the next tick
        self._busy = False

    # ------------------------------------------------------------------ helpers
    def _upload(self, parts):
        """int32 / float32 host arrays -> views of the device staging buffer, through the pinned buffer, in one copy."""
        if self._busy:
            self._copied.synchronize()       # the previous copy out of the pinned buffer (long done in steady state)
        off, views = 0, []
        for a in parts:
            w = a.size
            self._host[off:off + w] = np.ascontiguousarray(a).reshape(-1).view(np.int32)
            views.append((off, w))
            off += w
        self._staged[:off].copy_(self._pinned[:off], non_blocking=True)
        self._copied.record()
        self._busy = True
        return [self._staged[o:o + w] for o, w in views]

    def _flush(self, plan: ClosePlan) -> FrameScores:
        n, pend = len(plan), self.seg_len - 1
        keys = [k for k in plan.keys for _ in range(pend)]
        with torch.cuda.device(self.device):
            win = self._upload([plan.win])[0] if n and pend else None
            out = self.rings.flush(win, n)
            joints = self.rings.joint_flush(win, n) if self.joint_scores else None
            fc = ForecastRows(*self.rings.forecast_flush(win, n, self._forecast_cfg(0))) if self.forecasts is not None else None
        return FrameScores(keys, plan.frames.reshape(-1).copy(), out, joints, fc)

    def _forecast_cfg(self, n_windows: int):
        """The frame lists and the sample count the forecast entries read."""
        return self.scorer._score_cfg(n_windows, int(self.model.n_generated_samples), 2)

    def _clip_launches(self, cticks: List[ClipTick], parts: list):
        """The launch pairs of a tick's / a group's ClipTicks (one, unless batch_clip_ticks has to cut) -> (launches, index in
        `parts` of the first one's three arrays, appended there so that they ride in the caller's one copy)."""
        launches = [merge_clip_ticks([cticks[i] for i in b], self.clips.ring_len) for b in batch_clip_ticks(cticks, self.clips.ring_len)]
        at = len(parts)
        first = launches[0]
        if len(first.runs) or len(first.outs):
            parts += [first.runs, first.contrib, first.outs]
        return launches, at

    def _clip_run(self, cticks: List[ClipTick], launches, views, finals, tails) -> List[ClipFrames]:
        """Run the launch pairs -> one ClipFrames per ClipTick.  views: the device views of the first launch's arrays (None if it
        is empty); a further launch pair of the same group (rare: batch_clip_ticks) takes a copy of its own."""
        vals = []
        for k, la in enumerate(launches):
            n_runs, n_out = len(la.runs), len(la.outs)
            if k == 0:
                v = views
            else:
                v = self._upload([la.runs, la.contrib, la.outs]) if n_runs or n_out else None
            pre = self.clip_rings.emit(v[2][:4 * la.n_pre], la.n_pre) if la.n_pre else None      # (before the update: see ClipTable)
            if n_runs:
                self.clip_rings.update(v[0], n_runs, v[1], len(la.contrib), finals, tails)
            out = self.clip_rings.emit(v[2][4 * la.n_pre:] if n_out > la.n_pre else None, n_out - la.n_pre)
            if pre is not None:
                out = torch.cat([pre, out])
            o = 0
            for c in la.n_out:
                vals.append(out[o:o + c])
                o += c
        return [ClipFrames(list(t.clips), t.frames.copy(), vals[i], t.dropped) for i, t in enumerate(cticks)]

    # ------------------------------------------------------------------ the tick
    def push(self, keys, frame_ids, poses, *, noise=None) -> Tick:
        """One tick = one video frame: poses (n, 34) raw rows x1,y1,...,x17,y17 (as in the trajectory CSVs) of the tracks
        keys[i] = (scene, clip, person) at frame number frame_ids[i].  Asynchronous on the current stream.
        noise: (S, max(ns-1,1), num_transform * n_emit, C, Tx, V) -- for a latent model (S, max(ns-1,1), num_transform * n_emit, D)
        -- replacing the in-kernel Philox draws for the tick's windows (parity tests); by default the draws are keyed by
        (model.seed, Tick.first_window_id + position in the tick)."""
        raw = _pose_rows(keys, poses)
        if self.clips is not None:
            keys = [_key(k) for k in keys]
            self.clips.check(keys, frame_ids, True)   # (before any change: a tick the clip rules reject leaves both tables alone)
        plan = self.table.push(keys, frame_ids)
        g = _group(0, [plan], self.num_transform, self.seg_len)
        if self.clips is not None:
            g.clip = [self.clips.push(plan, keys, frame_ids, normalised=True)]
        return self._run_group(g, [raw], noise)[0]

    def push_many(self, ticks, *, noise=None) -> List[Tick]:
        """Several ticks in one call: ticks = [(keys, frame_ids, poses), ...], each triple what one `push` takes.  Returns, bit
        for bit, what [push(*t) for t in ticks] returns on a stream in the same state, and leaves the stream in the same state;
        the work runs in as few launch groups as the rings allow (pack_ticks: with ring_len = seg_len one group per tick, with
        ring_len = seg_len + K - 1 up to K ticks per group), each group ONE upload, mcd_stream_push_group, ONE scoring call and
        mcd_stream_frame_scores_group.  The windows of a group are tick-major, so each keeps the global window id -- hence the
        Philox draws -- sequential pushes give it, and every Tick holds contiguous views of its group's device tensors.
        noise: (S, max(ns-1,1), windows of the whole call, ...) in that order: tick after tick, inside a tick as for `push`.
        A rejected call (a bad shape, a non-finite row, a duplicate or closed key, no free slot: the error names the tick) changes
        nothing."""
        ticks = list(ticks)
        raws = []
        for i, t in enumerate(ticks):
            if len(t) != 3:
                raise ValueError(f"tick {i}: a tick is a (keys, frame_ids, poses) triple")
            try:
                raws.append(_pose_rows(t[0], t[2]))
            except ValueError as e:
                raise ValueError(f"tick {i}: {e}") from None
        packed = pack_ticks(self.table, [(t[0], t[1]) for t in ticks], self.num_transform, self.max_group_rows, self.clips)
        groups, planned = packed[0], packed[1]
        total = self.num_transform * sum(g.n_windows for g in groups)
        if noise is not None and (noise.dim() < 3 or noise.shape[2] != total):
            raise ValueError(f"noise must hold the {total} windows of the call on its third axis, got {tuple(noise.shape)}")
        self.table.adopt(planned)
        if self.clips is not None:
            self.clips.adopt(packed[2])
        out, lo = [], 0
        for g in groups:
            nw = self.num_transform * g.n_windows
            part = None if noise is None or not nw else noise if nw == total else noise[:, :, lo:lo + nw].contiguous()
            out += self._run_group(g, raws[g.first_tick:g.first_tick + len(g.plans)], part)
            lo += nw
        return out

    def _run_group(self, g: GroupPlan, raws, noise) -> List[Tick]:
        from .data.windows import WindowBatch
        n, nw, nt, dev, pend = g.n_rows, g.n_windows, self.num_transform, self.device, self.seg_len - 1
        first = self.n_emitted
        with torch.cuda.device(dev):
            closed = self._flush(g.closed)            # before the new rows: a freed slot may be handed out again in this group
            scores = torch.empty(nt * nw, device=dev, dtype=torch.float32)
            parts = [raws[0] if len(raws) == 1 else np.concatenate(raws), g.desc, g.win] if n else []
            if g.clip is not None:
                launches, at = self._clip_launches(g.clip, parts)
            views = self._upload(parts) if parts else []
            if n:
                raw_d, desc_d, win_d = views[:3]
                base, trans = self.rings.push_group(raw_d, desc_d, n, nw)
            if nw:
                m = self.model
                wb = WindowBatch(self.ring, base, trans, self.affine, self.seg_len)
                # (a MoCoDADlatent module: engine.LatentScorer.score, the encode + chain launches -- in pose space
                # engine.LatentPoseScorer.score, + the decode, aggregate and maps launches; else HipScorer.score_fused)
                score = self.scorer.score if self.latent else self.scorer.score_fused
                res = score(wb, n_samples=m.n_generated_samples, noise_steps=m.noise_steps, aggregation=m.aggregation_strategy,
                            noise=noise, seed=m.seed, first_window_id=first, loss_fn=m.loss_name, out=scores,
                            **({"want_maps": True} if self.joint_scores else {}),
                            # forecasts: the per-sample losses and the poses come back (the maps launch then reads these: written once)
                            **({"want_all": True, "want_poses": True} if self.forecasts is not None else {}))
                final = self.rings.frame_scores_group(scores, win_d, nw)
                if self.joint_scores:       # the windows' error maps into the joint ring, by the same sorted window table
                    jfinal = self.rings.joint_scores_group(res[3], win_d, nw, self.scorer._score_cfg(nw, 1, 2))
            else:
                res = (None, None, None)
                final = torch.empty(0, nt, device=dev, dtype=torch.float32)
                if self.joint_scores:
                    jfinal = torch.empty(0, nt, 17, device=dev, dtype=torch.float32)
            if self.forecasts is not None:  # the raw rows and the windows' selected forecasts into their rings; the final rows out
                fc = ForecastRows(*self.rings.forecast_group(raw_d if n else None, desc_d if n else None, n, res[1], res[2],
                                                             win_d if nw else None, nw, self._forecast_cfg(nt * nw),
                                                             self.model.aggregation_strategy))
            clips = [None] * len(g.plans)
            if g.clip is not None:
                clips = self._clip_run(g.clip, launches, views[at:at + 3] or None, final, closed.values)
        self.n_emitted += nt * nw
        out, c0 = [], 0
        for i, plan in enumerate(g.plans):
            ne, w0, c1 = plan.n_emit, int(g.offsets[i]), c0 + len(plan.closed)
            a, b = nt * w0, nt * (w0 + ne)
            wb = WindowBatch(self.ring, base[a:b], trans[a:b], self.affine, self.seg_len) if ne else None
            jf = jfinal[w0:w0 + ne] if self.joint_scores else None
            ff = fc.rows(w0, w0 + ne) if self.forecasts is not None else None
            tail = closed.rows(c0 * pend, c1 * pend)
            out.append(Tick(meta=np.tile(plan.meta, (nt, 1)), frames=np.tile(plan.frames, (nt, 1)),
                            trans=np.repeat(np.arange(nt, dtype=np.int64), ne), scores=scores[a:b], windows=wb,
                            final=FrameScores(list(plan.keys), plan.frames[:, 0].copy(), final[w0:w0 + ne], jf, ff), closed=tail,
                            first_window_id=first + a, clip=clips[i], joint_final=jf, forecast=ff))
            c0 = c1
        return out

    def close(self, keys) -> FrameScores:
        """End the tracks `keys` and free their slots -> the frame scores of their last seg_len - 1 rows (tracks that never had
        seg_len rows return nothing).  Asynchronous on the current stream."""
        return self._close(keys)[0]

    def _close(self, keys):
        plan = self.table.close(keys)
        tails = self._flush(plan)
        if self.clips is None:
            return tails, None
        ct = self.clips.close(plan)          # the tails into their cells at once, in a launch of their own; nothing is emitted
        if ct.contribs:
            with torch.cuda.device(self.device):
                la = merge_clip_ticks([ct], self.clips.ring_len)
                runs_d, contrib_d = self._upload([la.runs, la.contrib])
                self.clip_rings.update(runs_d, len(la.runs), contrib_d, len(la.contrib), None, tails.values)
        return tails, ct

    def close_clip(self, key):
        """End the clip key = (scene, clip): close its open tracks (their tails come back as `close` returns them), emit the
        clip's remaining frames up to its head with the reflection at the end of the sequence, and free its slot
        -> (FrameScores, ClipFrames).  Across the ticks and this tail, the clip's output is the filter over its whole current
        segment.  A later row for the clip opens a new clip (its tracks need `reopen` first)."""
        if self.clips is None:
            raise RuntimeError("close_clip needs PoseStream(clip_scores=ClipScoreCfg(...))")
        clip = (int(key[0]), int(key[1]))
        if clip not in self.clips.slot_of:
            raise KeyError(f"clip {clip} is not open")
        tails, ct = self._close(self.clips.tracks_of(clip))
        end = self.clips.end_clip(clip)
        with torch.cuda.device(self.device):
            outs = self._upload([end.outs])[0] if end.n_out else None
            values = self.clip_rings.emit(outs, end.n_out)
        return tails, ClipFrames(end.clips, end.frames, values, ct.dropped)

    def close_all(self) -> FrameScores:
        return self.close(list(self.table.slot_of))

    def reopen(self, keys) -> None:
        self.table.reopen(keys)

def ticks_by_frame(tracks, per_clip: bool = False):
    """Replay recorded tracks as a live feed: tracks = [((scene, clip, person), frame ids (F,), poses (F, 34)), ...] -> one
    (frame id, keys, frame ids, poses) tuple per distinct frame id, ascending: one tick is one frame id across all clips (all
    cameras run together).  per_clip: one tick per (scene, clip, frame id) instead, clip after clip (one camera at a time).
    The rows of a track keep their file order."""
    tracks = [t for t in tracks if len(t[1])]
    if not tracks:
        return
    keys = [_key(k) for k, _, _ in tracks]
    fr = np.concatenate([np.asarray(f, np.int64).reshape(-1) for _, f, _ in tracks])
    po = np.concatenate([np.asarray(p, np.float32).reshape(-1, ROW) for _, _, p in tracks])
    ti = np.repeat(np.arange(len(tracks)), [len(f) for _, f, _ in tracks])
    group = fr
    if per_clip:
        clips = sorted({k[:2] for k in keys})
        group = np.asarray([clips.index(k[:2]) for k in keys], np.int64)[ti] * (int(fr.max()) - int(fr.min()) + 1) + (fr - fr.min())
    order = np.argsort(group, kind="stable")
    for idx in np.split(order, np.flatnonzero(np.diff(group[order])) + 1):
        yield int(fr[idx[0]]), [keys[t] for t in ti[idx]], fr[idx], po[idx]

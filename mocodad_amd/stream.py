"""Live pose streams: many tracked people, one new pose row per track per video frame, an anomaly score a few milliseconds later.

The dataset path takes a whole split at once (data/trajectories.py parses a directory, mcd_normalize_poses normalises every row,
TrajectoryWindows enumerates every window, post_processing assembles the frame scores after the last batch).  Here the state
between two ticks lives on the device (include/mocodad_hip.h: mcd_stream_state_t):

  pose ring   (max_tracks, 2 L, 2, 17): row r of a track is stored at positions r % L and r % L + L, so the seg_len rows from row
              s on are contiguous from position s % L and a window is still ONE base offset of a window view: the scoring
              kernels read the ring exactly as they read a trajectory buffer.
  score ring  (max_tracks, num_transform, L): the running maximum, per row and transform, over the windows covering that row.

and a tick is: one host-to-device copy of the new rows and their descriptors, mcd_stream_push (normalise + store + window
descriptors), ONE scoring call on the windows that end at the new rows, mcd_stream_frame_scores (max into the score ring; the
oldest row of each window is final and comes back).

`TrackTable` is the host half: (scene, clip, person) -> ring slot, row counts, the frame ids of the last seg_len rows.  It is plain
NumPy and imports no GPU module.  Windows follow the reference's rule (utils/preprocessing.py:14-86, the rule
TrajectoryWindows.from_buffer implements): they run over CONSECUTIVE ROWS of a track, frame-number gaps included, so
meta = [scene, clip, person, frame id of the window's first row] and frames = the frame ids of its seg_len rows.
`PoseStream` owns the rings (engine.StreamRings) and the staging buffers and drives the launches of a tick.

Several ticks at once (a pose estimator that delivers frames in batches, a stream catching up, recorded video on the online path):
`PoseStream.push_many` returns what the same ticks pushed one by one return, bit for bit, but runs them in launch groups --
`pack_ticks` cuts the call into groups of consecutive ticks that the rings can hold at once (ring_len - seg_len + 1 rows per
track), and a group is one copy, mcd_stream_push_group, ONE scoring call on all of its windows, mcd_stream_frame_scores_group."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ROW = 34                 # floats of one pose row: (2, 17)
Key = Tuple[int, int, int]


def _key(k) -> Key:
    k = tuple(int(v) for v in k)
    if len(k) != 3:
        raise ValueError(f"a track key is (scene, clip, person), got {k}")
    return k


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
        if len(fids) and (fids.min() < np.iinfo(np.int32).min or fids.max() > np.iinfo(np.int32).max):
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
        ekeys = [keys[i] for i in np.flatnonzero(emit)]
        frames = self._fids[win[:, 0]].copy()
        base = (win[:, 0].astype(np.int64) * 2 * self.ring_len + (win[:, 1].astype(np.int64) - T + 1) % self.ring_len) * ROW
        meta = np.concatenate([np.asarray(ekeys, np.int64).reshape(-1, 3), frames[:, :1].astype(np.int64)], axis=1)
        return TickPlan(desc, win, base, ekeys, meta, frames, closed)


@dataclass
class GroupPlan:
    """Consecutive ticks of one call that share their launches (pack_ticks): one upload, one mcd_stream_push_group, one scoring
    call, one mcd_stream_frame_scores_group.  The group's windows are tick-major, inside a tick transform-major: the window of
    the j-th emitting row of tick i under transform t is at batch position offsets[i] * num_transform + t * n_emit_i + j."""
    first_tick: int                   # index of the group's first tick in the call
    plans: List[TickPlan]             # the plans of its ticks, exactly those of sequential TrackTable.push calls
    desc: np.ndarray                  # (n, 4) int32 per pushed row, tick after tick: [slot, row index r, pos0 | -1, n_emit of its tick]
    win: np.ndarray                   # (n_windows, 5) int32 [slot, r_last, pos0, n_emit of its tick, index in (tick, j) order],
    #                                   sorted by slot, then row: the windows of a track are adjacent and ascending
    offsets: np.ndarray               # (len(plans) + 1,) int64 windows (one transform) emitted before each tick of the group
    closed: ClosePlan                 # the idle closures of all its ticks, tick after tick (none of them got a row in the group)

    @property
    def n_rows(self) -> int:
        return int(self.desc.shape[0])

    @property
    def n_windows(self) -> int:
        return int(self.offsets[-1])


def _group(first_tick: int, plans: List[TickPlan], num_transform: int, seg_len: int) -> GroupPlan:
    ne = np.asarray([p.n_emit for p in plans], np.int64)
    offsets = np.zeros(len(plans) + 1, np.int64)
    offsets[1:] = np.cumsum(ne)
    desc, win = [], []
    for i, p in enumerate(plans):
        j = p.desc[:, 2].astype(np.int64)
        pos0 = np.where(j >= 0, offsets[i] * num_transform + j, -1)
        desc.append(np.stack([p.desc[:, 0], p.desc[:, 1], pos0, np.full(len(j), ne[i])], axis=1))
        jj = np.arange(ne[i])
        win.append(np.stack([p.win[:, 0], p.win[:, 1], offsets[i] * num_transform + jj, np.full(ne[i], ne[i]), offsets[i] + jj],
                            axis=1))
    desc = np.concatenate(desc).astype(np.int32).reshape(-1, 4)
    win = np.concatenate(win).astype(np.int32).reshape(-1, 5)
    win = win[np.argsort(win[:, 0], kind="stable")]            # (stable: within a slot the ticks, hence the rows, stay ascending)
    closed = ClosePlan()
    for p in plans:
        closed.keys += p.closed.keys
        closed.slots += p.closed.slots
    closed.win = np.concatenate([p.closed.win for p in plans]).reshape(-1, 2)
    closed.frames = np.concatenate([p.closed.frames for p in plans]).reshape(-1, seg_len - 1)
    return GroupPlan(first_tick, plans, desc, win, offsets, closed)


def pack_ticks(table: TrackTable, ticks, num_transform: int = 1, max_rows: Optional[int] = None):
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
    With ring_len = seg_len every group is one tick."""
    work = table.copy()
    per_track = table.ring_len - table.seg_len + 1
    cap = table.max_tracks * per_track if max_rows is None else int(max_rows)
    if cap < table.max_tracks:
        raise ValueError(f"max_rows = {cap} is less than max_tracks = {table.max_tracks}: one tick would not fit a group")
    groups: List[GroupPlan] = []
    first, plans, count, n_rows = 0, [], {}, 0
    for i, (keys, fids) in enumerate(ticks):
        try:
            plan = work.push(keys, fids)
        except (ValueError, RuntimeError) as e:
            raise type(e)(f"tick {i}: {e}") from None
        slots = plan.desc[:, 0].tolist()
        # (ring_len = seg_len: one tick per group, today's launches, also where two ticks happen to share no track)
        if plans and (per_track == 1 or n_rows + len(slots) > cap or any(count.get(s, 0) >= per_track for s in slots)
                      or any(s in count for s in plan.closed.slots)):
            groups.append(_group(first, plans, num_transform, table.seg_len))
            first, plans, count, n_rows = i, [], {}, 0
        plans.append(plan)
        n_rows += len(slots)
        for s in slots:
            count[s] = count.get(s, 0) + 1
    if plans:
        groups.append(_group(first, plans, num_transform, table.seg_len))
    return groups, work


@dataclass
class FrameScores:
    """Final per-row frame scores: row i belongs to track keys[i] at frame id frames[i]; values (n, num_transform) fp32 on the
    device = the maximum over the windows of that track covering the row, per transform."""
    keys: List[Key]
    frames: np.ndarray
    values: "object"

    def __len__(self):
        return len(self.keys)


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


class PoseStream:
    """Online scoring of live pose tracks with `model` (a MoCoDAD or MoCoDADlatent module on a cuda device).

    vid_res, center, scale: as for engine.normalize_poses (center / scale (34,) = the fitted RobustScaler, or both None).
    max_tracks: slots of the device rings; ring_len: rows kept per track (>= seg_len, default seg_len);
    num_transform: default the model's; max_idle: see TrackTable; max_group_rows: cap on the rows of one launch group of
    push_many (default and upper limit max_tracks * (ring_len - seg_len + 1), at least max_tracks): it sizes the staging buffers.

    One PoseStream is driven from ONE stream (the current stream of the first push): its rings, staging buffers and the track
    table are per-tick state, and the launches of a tick are ordered only by that stream."""

    def __init__(self, model, *, vid_res, center=None, scale=None, max_tracks: int = 1024, ring_len: Optional[int] = None,
                 num_transform: Optional[int] = None, max_idle: Optional[int] = None, max_group_rows: Optional[int] = None):
        import torch
        from .engine import StreamRings
        from .utils.transforms import affine_table
        self.latent = bool(getattr(model, "is_latent", False))
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
        self.model = model
        self.scorer = model.scorer()
        self.device = dev = self.scorer.device
        self.seg_len = int(model.n_frames)
        self.num_transform = nt = max(1, int(model.num_transforms if num_transform is None else num_transform))
        self.table = TrackTable(max_tracks, self.seg_len, ring_len, max_idle)
        n = self.table.max_tracks
        self.rings = StreamRings(n, self.seg_len, self.table.ring_len, nt, vid_res, center, scale, device=dev)
        self.ring = self.rings.ring
        with torch.cuda.device(dev):
            self.affine = affine_table(nt).to(dev)
            # one group's host-to-device traffic: raw rows (n, 34) f32 | descriptors (n, 4) i32 | windows (n, 5) i32, in ONE copy
            # (a tick of push: (n, 3) and (n, 2)); a group of push_many holds at most max_group_rows rows
            per_track = self.table.ring_len - self.seg_len + 1
            self.max_group_rows = n * per_track if max_group_rows is None else min(int(max_group_rows), n * per_track)
            if self.max_group_rows < n:
                raise ValueError(f"max_group_rows = {max_group_rows} is less than max_tracks = {n}: one tick would not fit a group")
            self._pinned = torch.empty(self.max_group_rows * (ROW + 4 + 5), dtype=torch.int32).pin_memory()
            self._staged = torch.empty(self.max_group_rows * (ROW + 4 + 5), device=dev, dtype=torch.int32)
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
        import torch
        n, pend = len(plan), self.seg_len - 1
        keys = [k for k in plan.keys for _ in range(pend)]
        with torch.cuda.device(self.device):
            win = self._upload([plan.win])[0] if n and pend else None
            out = self.rings.flush(win, n)
        return FrameScores(keys, plan.frames.reshape(-1).copy(), out)

    # ------------------------------------------------------------------ the tick
    def push(self, keys, frame_ids, poses, *, noise=None) -> Tick:
        """One tick = one video frame: poses (n, 34) raw rows x1,y1,...,x17,y17 (as in the trajectory CSVs) of the tracks
        keys[i] = (scene, clip, person) at frame number frame_ids[i].  Asynchronous on the current stream.
        noise: (S, max(ns-1,1), num_transform * n_emit, C, Tx, V) -- for a latent model (S, max(ns-1,1), num_transform * n_emit, D)
        -- replacing the in-kernel Philox draws for the tick's windows (parity tests); by default the draws are keyed by
        (model.seed, Tick.first_window_id + position in the tick)."""
        import torch
        from .data.windows import WindowBatch
        raw = np.ascontiguousarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float32)
        if raw.ndim != 2 or raw.shape[1] != ROW or raw.shape[0] != len(keys):
            raise ValueError(f"poses must be ({len(keys)}, {ROW}) = one row x1,y1,...,x17,y17 per key, got {raw.shape}")
        if not np.isfinite(raw).all():
            raise ValueError("raw pose rows hold NaN / inf values (the trajectory CSVs hold finite coordinates only)")
        plan = self.table.push(keys, frame_ids)
        n, ne, nt, dev = len(plan.desc), plan.n_emit, self.num_transform, self.device
        first = self.n_emitted
        with torch.cuda.device(dev):
            closed = self._flush(plan.closed)         # before the new rows: a freed slot may be handed out again in this tick
            wb = None
            scores = torch.empty(nt * ne, device=dev, dtype=torch.float32)
            if n:
                raw_d, desc_d, win_d = self._upload([raw, plan.desc, plan.win])
                base, trans = self.rings.push(raw_d, desc_d, n, ne)
            if ne:
                m = self.model
                wb = WindowBatch(self.ring, base, trans, self.affine, self.seg_len)
                # (a MoCoDADlatent module: engine.LatentScorer.score, the encode + chain launches; else HipScorer.score_fused)
                score = self.scorer.score if self.latent else self.scorer.score_fused
                score(wb, n_samples=m.n_generated_samples, noise_steps=m.noise_steps, aggregation=m.aggregation_strategy,
                      noise=noise, seed=m.seed, first_window_id=first, loss_fn=m.loss_name, out=scores)
                final = self.rings.frame_scores(scores, win_d, ne)
            else:
                final = torch.empty(0, nt, device=dev, dtype=torch.float32)
        self.n_emitted += nt * ne
        return Tick(meta=np.tile(plan.meta, (nt, 1)), frames=np.tile(plan.frames, (nt, 1)),
                    trans=np.repeat(np.arange(nt, dtype=np.int64), ne), scores=scores, windows=wb,
                    final=FrameScores(list(plan.keys), plan.frames[:, 0].copy(), final), closed=closed, first_window_id=first)

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
        import torch
        ticks = list(ticks)
        raws = []
        for i, t in enumerate(ticks):
            if len(t) != 3:
                raise ValueError(f"tick {i}: a tick is a (keys, frame_ids, poses) triple")
            keys, _, poses = t
            raw = np.ascontiguousarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float32)
            if raw.ndim != 2 or raw.shape[1] != ROW or raw.shape[0] != len(keys):
                raise ValueError(f"tick {i}: poses must be ({len(keys)}, {ROW}) = one row x1,y1,...,x17,y17 per key, got {raw.shape}")
            if not np.isfinite(raw).all():
                raise ValueError(f"tick {i}: raw pose rows hold NaN / inf values (the trajectory CSVs hold finite coordinates only)")
            raws.append(raw)
        groups, planned = pack_ticks(self.table, [(t[0], t[1]) for t in ticks], self.num_transform, self.max_group_rows)
        total = self.num_transform * sum(g.n_windows for g in groups)
        if noise is not None and (noise.dim() < 3 or noise.shape[2] != total):
            raise ValueError(f"noise must hold the {total} windows of the call on its third axis, got {tuple(noise.shape)}")
        self.table.adopt(planned)
        out, lo = [], 0
        for g in groups:
            nw = self.num_transform * g.n_windows
            part = None if noise is None or not nw else noise if nw == total else noise[:, :, lo:lo + nw].contiguous()
            out += self._run_group(g, raws[g.first_tick:g.first_tick + len(g.plans)], part)
            lo += nw
        return out

    def _run_group(self, g: GroupPlan, raws, noise) -> List[Tick]:
        import torch
        from .data.windows import WindowBatch
        n, nw, nt, dev, pend = g.n_rows, g.n_windows, self.num_transform, self.device, self.seg_len - 1
        first = self.n_emitted
        with torch.cuda.device(dev):
            closed = self._flush(g.closed)            # before the new rows: a freed slot may be handed out again in this group
            scores = torch.empty(nt * nw, device=dev, dtype=torch.float32)
            if n:
                raw_d, desc_d, win_d = self._upload([np.concatenate(raws), g.desc, g.win])
                base, trans = self.rings.push_group(raw_d, desc_d, n, nw)
            if nw:
                m = self.model
                wb = WindowBatch(self.ring, base, trans, self.affine, self.seg_len)
                score = self.scorer.score if self.latent else self.scorer.score_fused
                score(wb, n_samples=m.n_generated_samples, noise_steps=m.noise_steps, aggregation=m.aggregation_strategy,
                      noise=noise, seed=m.seed, first_window_id=first, loss_fn=m.loss_name, out=scores)
                final = self.rings.frame_scores_group(scores, win_d, nw)
            else:
                final = torch.empty(0, nt, device=dev, dtype=torch.float32)
        self.n_emitted += nt * nw
        out, c0 = [], 0
        for i, plan in enumerate(g.plans):
            ne, w0, c1 = plan.n_emit, int(g.offsets[i]), c0 + len(plan.closed)
            a, b = nt * w0, nt * (w0 + ne)
            wb = WindowBatch(self.ring, base[a:b], trans[a:b], self.affine, self.seg_len) if ne else None
            tail = FrameScores(closed.keys[c0 * pend:c1 * pend], closed.frames[c0 * pend:c1 * pend].copy(),
                               closed.values[c0 * pend:c1 * pend])
            out.append(Tick(meta=np.tile(plan.meta, (nt, 1)), frames=np.tile(plan.frames, (nt, 1)),
                            trans=np.repeat(np.arange(nt, dtype=np.int64), ne), scores=scores[a:b], windows=wb,
                            final=FrameScores(list(plan.keys), plan.frames[:, 0].copy(), final[w0:w0 + ne]), closed=tail,
                            first_window_id=first + a))
            c0 = c1
        return out

    def close(self, keys) -> FrameScores:
        """End the tracks `keys` and free their slots -> the frame scores of their last seg_len - 1 rows (tracks that never had
        seg_len rows return nothing).  Asynchronous on the current stream."""
        return self._flush(self.table.close(keys))

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

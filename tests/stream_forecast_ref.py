"""NumPy model of the forecast ring of a live stream (include/mocodad_hip.h: mcd_stream_forecast_state_t), cell for cell:

    forecast ring (n_slots, L, Tx, 34): cell (r % L, j) = row r as corrupt frame j of its one window (the window ending at row
                  r + seg_len - 1 - corrupt_idx[j]); observed ring (n_slots, L, 34): the raw row r.
    validity      by arithmetic, nothing stored: cell (r, j) is valid, the track's last row so far being r_hi, iff
                  corrupt_idx[j] <= r and r + seg_len - 1 - corrupt_idx[j] <= r_hi.
    order         the valid cells in ascending window order = descending j.

The rings start as NaN bit patterns no forecast holds (an initial value nobody may depend on).  The per-row reduction is
forecast_ref.assemble on the staged values as k one-frame "windows" of one cell, then forecast_ref.denormalize: what this module
adds, and what tests/test_stream_forecast_host.py holds to forecast_ref.assemble over the whole track, is the layout, the validity
rule and the order.  Plain NumPy, no GPU module."""
import numpy as np

import forecast_ref

GARBAGE = np.float32(np.nan)


def interleave(pose):
    """A window's forecast (2, Tx, 17) -> (Tx, 34) rows x1,y1,...,x17,y17."""
    return np.ascontiguousarray(np.asarray(pose, np.float32).transpose(1, 2, 0).reshape(pose.shape[1], 34))


class RingModel:
    def __init__(self, n_slots, ring_len, seg_len, corrupt_idx, method="median", spread="mean", vid_res=(640, 360), center=None,
                 scale=None):
        self.L, self.T, self.cidx = int(ring_len), int(seg_len), [int(c) for c in corrupt_idx]
        assert self.L >= self.T and self.cidx == sorted(set(self.cidx)) and 0 <= self.cidx[0] and self.cidx[-1] < self.T
        self.method, self.spread_method, self.vid_res, self.center, self.scale = method, spread, vid_res, center, scale
        self.fc = np.full((n_slots, self.L, len(self.cidx), 34), GARBAGE, np.float32)
        self.obs = np.full((n_slots, self.L, 34), GARBAGE, np.float32)

    # ---- the two writers of a group (mcd_stream_forecast_group, first launch)
    def store_row(self, slot, r, raw_row):
        self.obs[slot, r % self.L] = raw_row

    def store_window(self, slot, r_last, pose):
        """pose (2, Tx, 17): the selected forecast of the window ending at row r_last (zeros where no sample passed)."""
        rows = interleave(pose)
        for j, c in enumerate(self.cidx):
            self.fc[slot, (r_last - self.T + 1 + c) % self.L, j] = rows[j]

    # ---- the reader (second launch, and mcd_stream_forecast_flush)
    def valid(self, r, r_hi):
        """The valid j of row r in ascending window order (descending j)."""
        return [j for j in range(len(self.cidx) - 1, -1, -1) if self.cidx[j] <= r and r + self.T - 1 - self.cidx[j] <= r_hi]

    def row(self, slot, r, r_hi):
        """-> (expected (34,), expected_norm (34,), observed (34,), count, spread) of row r."""
        js = self.valid(r, r_hi)
        k = len(js)
        staged = np.stack([self.fc[slot, r % self.L, j] for j in js]) if k else np.zeros((0, 34), np.float32)
        poses = staged.reshape(k, 1, 17, 2).transpose(0, 3, 1, 2)                   # k windows of one forecast frame each
        norm, count, spread = forecast_ref.assemble(poses, np.zeros((k, 1), np.int64), 1, self.method, self.spread_method)
        observed = self.obs[slot, r % self.L].copy()
        expected = forecast_ref.denormalize(norm, observed[None], self.vid_res, self.center, self.scale, count=count)
        return expected[0], norm[0], observed, int(count[0]), spread[0]

    def final(self, slot, r_last):
        """The row the window ending at r_last finalises."""
        return self.row(slot, r_last - self.T + 1, r_last)

    def flush(self, slot, r_last):
        """The seg_len - 1 pending rows of a track being closed, oldest first."""
        return [self.row(slot, r, r_last) for r in range(r_last - self.T + 2, r_last + 1)]

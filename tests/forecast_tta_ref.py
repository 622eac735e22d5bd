"""NumPy float64 restatement of what mcd_forecast_assemble_view and the stream's forecast ring of every transform add to
mcd_forecast_assemble (include/mocodad_hip.h): the inverse table of the test-time transforms and the per-joint map of a forecast back
through it, each operation a float64 operation in the stated order, rounded to fp32 once.  The mapped poses then go through
forecast_ref.assemble unchanged.  What the kernels are held to bit for bit (tests/test_forecast_tta_gpu.py,
tests/test_stream_forecast_tta_gpu.py); tests/test_forecast_tta_host.py holds the ring model of the stream to it."""
import numpy as np

import forecast_ref as FR


def inverse_table(affine):
    """(n, 6) rows [a00 a01 a02 a10 a11 a12] (any float type, taken as they are) -> (n, 6) float64 rows [i00 i01 i02 i10 i11 i12]."""
    a = np.asarray(affine).astype(np.float64).reshape(-1, 6)
    out = np.zeros_like(a)
    for k, (a00, a01, a02, a10, a11, a12) in enumerate(a):
        det = a00 * a11 - a01 * a10
        if det == 0:
            raise ValueError("singular transform")
        i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
        i02 = -(i00 * a02 + i01 * a12)
        i12 = -(i10 * a02 + i11 * a12)
        out[k] = [i00, i01, i02, i10, i11, i12]
    return out + 0.0          # (a -0.0 becomes +0.0; no value changes)


def is_identity_row(m):
    return bool(m[0] == 1.0 and m[1] == 0.0 and m[2] == 0.0 and m[3] == 0.0 and m[4] == 1.0 and m[5] == 0.0)


def map_back(poses, trans, inv):
    """poses (N, 2, Tx, 17) f32 forecasts, trans (N,) their transforms (all inside the table), inv (n_transform, 6) float64 ->
    (N, 2, Tx, 17) f32: x = fp32((i00 x' + i01 y') + i02), y = fp32((i10 x' + i11 y') + i12); an identity row copies the bits."""
    poses = np.ascontiguousarray(poses, np.float32)
    inv = np.asarray(inv, np.float64)
    out = poses.copy()
    with np.errstate(all="ignore"):
        for i, t in enumerate(np.asarray(trans).reshape(-1)):
            m = inv[int(t)]
            if is_identity_row(m):
                continue
            xp, yp = poses[i, 0].astype(np.float64), poses[i, 1].astype(np.float64)
            out[i, 0] = ((m[0] * xp + m[1] * yp) + m[2]).astype(np.float32)
            out[i, 1] = ((m[3] * xp + m[4] * yp) + m[5]).astype(np.float32)
    return out


def assemble(poses, cell, trans, inv, n_cells, method="median", spread_method="mean", max_cover=64):
    """mcd_forecast_assemble_view: windows whose transform is outside the table are ignored, the others mapped back, then
    forecast_ref.assemble in ascending pair index.  (forecast_ref.assemble asserts max_cover <= 32, the existing entry's limit; a
    larger list holds the same pairs, so the reduction runs with the cover that fits and the NaN rule is applied here.)"""
    poses, cell, trans = np.asarray(poses, np.float32), np.asarray(cell).astype(np.int64).copy(), np.asarray(trans).astype(np.int64).reshape(-1)
    n_t = len(np.asarray(inv).reshape(-1, 6))
    ok = (trans >= 0) & (trans < n_t)
    cell[~ok] = -1
    mapped = map_back(poses, np.where(ok, trans, 0), np.asarray(inv, np.float64).reshape(-1, 6))      # (ignored windows: any row)
    if max_cover <= 32:
        return FR.assemble(mapped, cell, n_cells, method, spread_method, max_cover)
    return _assemble_wide(mapped, cell, n_cells, method, spread_method, max_cover)


def _assemble_wide(poses, cell, n_cells, method, spread_method, max_cover):
    """forecast_ref.assemble's loops, restated for lists of 33 .. 64 pairs (that function asserts max_cover <= 32, the existing entry's
    limit): the pairs of a cell in ascending pair index, the sums in that order, forecast_ref's own middle value.  Where both apply
    they agree in every bit (tests/test_forecast_tta_host.py)."""
    assert 32 < max_cover <= 64
    N, _, Tx, _ = poses.shape
    rows = poses.transpose(0, 2, 3, 1).reshape(N * Tx, 34)
    flat = cell.reshape(-1)
    pose = np.zeros((n_cells, 34), np.float32)
    count = np.zeros(n_cells, np.int32)
    spread = np.zeros(n_cells, np.float32)
    with np.errstate(all="ignore"):
        for c in range(n_cells):
            pairs = np.flatnonzero(flat == c)
            k = count[c] = len(pairs)
            if k == 0:
                continue
            if k > max_cover:
                pose[c], spread[c] = np.nan, np.nan
                continue
            x = rows[pairs].astype(np.float64)
            sd = np.zeros(34)
            for f in range(34):
                s = np.float64(0.0)
                for j in range(k):
                    s = s + x[j, f]
                mean = s / np.float64(k)
                ss = np.float64(0.0)
                for j in range(k):
                    d = x[j, f] - mean
                    ss = ss + d * d
                sd[f] = np.sqrt(ss / np.float64(k))
                pose[c, f] = np.float32(x[0, f] if method == "unique" else mean if method == "mean" else FR._middle(x[:, f]))
            if spread_method == "mean":
                s = np.float64(0.0)
                for f in range(34):
                    s = s + sd[f]
                spread[c] = np.float32(s / np.float64(34.0))
            else:
                spread[c] = np.float32(FR._middle(sd))
    return pose, count, spread


class TtaRingModel:
    """The forecast ring of every transform (mcd_stream_forecast_tta_state_t), cell for cell, beside stream_forecast_ref.RingModel:
    ring (n_slots, L, n_transform, Tx, 34), cell (r % L, t, j) = row r as corrupt frame j of its one window under transform t,
    ALREADY mapped back; validity by the same arithmetic, whatever t; a row's valid cells in the order transform ascending, then
    window ascending (= j descending).  The rings start as NaN (an initial value nobody may depend on) and are never cleared."""

    def __init__(self, n_slots, ring_len, seg_len, corrupt_idx, inv, method="median", spread="mean", vid_res=(640, 360), center=None,
                 scale=None):
        self.L, self.T, self.cidx = int(ring_len), int(seg_len), [int(c) for c in corrupt_idx]
        self.inv = np.asarray(inv, np.float64).reshape(-1, 6)
        self.nt = len(self.inv)
        assert self.L >= self.T and self.cidx == sorted(set(self.cidx)) and self.nt * len(self.cidx) <= 64
        self.method, self.spread_method, self.vid_res, self.center, self.scale = method, spread, vid_res, center, scale
        self.fc = np.full((n_slots, self.L, self.nt, len(self.cidx), 34), np.float32(np.nan), np.float32)
        self.obs = np.full((n_slots, self.L, 34), np.float32(np.nan), np.float32)

    def store_row(self, slot, r, raw_row):
        self.obs[slot, r % self.L] = raw_row

    def store_window(self, slot, r_last, t, pose):
        """pose (2, Tx, 17): the selected forecast of the window ending at row r_last under transform t, as the model made it."""
        back = map_back(np.asarray(pose, np.float32)[None], [t], self.inv)[0]
        rows = np.ascontiguousarray(back.transpose(1, 2, 0).reshape(back.shape[1], 34))
        for j, c in enumerate(self.cidx):
            self.fc[slot, (r_last - self.T + 1 + c) % self.L, t, j] = rows[j]

    def valid(self, r, r_hi):
        js = [j for j in range(len(self.cidx) - 1, -1, -1) if self.cidx[j] <= r and r + self.T - 1 - self.cidx[j] <= r_hi]
        return [(t, j) for t in range(self.nt) for j in js]

    def row(self, slot, r, r_hi):
        """-> (expected (34,), expected_norm (34,), observed (34,), count, spread) of row r."""
        tj = self.valid(r, r_hi)
        k = len(tj)
        staged = np.stack([self.fc[slot, r % self.L, t, j] for t, j in tj]) if k else np.zeros((0, 34), np.float32)
        poses = staged.reshape(k, 1, 17, 2).transpose(0, 3, 1, 2)
        asm = FR.assemble if k <= 32 else (lambda p, c, n, m, s: _assemble_wide(p, c, n, m, s, 64))
        norm, count, spread = asm(poses, np.zeros((k, 1), np.int64), 1, self.method, self.spread_method)
        observed = self.obs[slot, r % self.L].copy()
        expected = FR.denormalize(norm, observed[None], self.vid_res, self.center, self.scale, count=count)
        return expected[0], norm[0], observed, int(count[0]), spread[0]

    def final(self, slot, r_last):
        return self.row(slot, r_last - self.T + 1, r_last)

    def flush(self, slot, r_last):
        return [self.row(slot, r, r_last) for r in range(r_last - self.T + 2, r_last + 1)]

// mcd_stream_kernel.hpp — the device code of a live stream (launched by mcd_stream_api.hpp): the loader step, sliding windows and
// scatter-max of the dataset path (utils/preprocessing.py:14-86, models/mocodad.py:392-393) one group of ticks at a time on device
// rings -- stream_push_group / stream_frame_scores_group / stream_joint_scores_group / stream_flush<W>, the forecast ring's
// stream_forecast_store / _emit / _flush and, over every transform, stream_forecast_store_tta / _emit_tta / _flush_tta -- and the online
// clip scores stream_clip_update / stream_clip_emit, with their parameter
// blocks and the three table rows the host hands them, each decoded and validated ONCE: WindowRow, ClosedRow, PushedRow.
// Included once, by mcd_api.hip, behind mcd_post_kernel.hpp, whose pieces it shares: normalize_pose_row / denormalize_pose_row,
// wave_select and stage_samples, forecast_reduce_staged, inverse_affine_coord, and person_aggr_* / reflect_index / gauss_taps of
// frame_scores_kernel.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Live pose streams (mcd_stream_state_t): the state between two ticks lives in two caller-owned rings.
//   pose ring  (n_slots, 2 L, 2, 17): row r of a track sits at positions r % L and r % L + L, so the seg_len rows from row s on
//              are contiguous from position s % L and a window stays ONE base offset of mcd_window_view_t.
//   score ring (n_slots, num_transform, L): running max, per row and transform, over the windows covering the row.
// The launches on them take a GROUP of consecutive ticks; a single tick is a group of one.  No two threads of a launch touch the
// same cell (the bound on a group, below, and one thread per track where windows overlap): plain loads and stores.
// ------------------------------------------------------------------------------------------------
struct StreamParams {
    float* ring; float* fs;
    int n_slots, L, seg_len, nt;
};

// The rows of the three tables a launch reads.  A row the host table cannot produce touches nothing: the kernels skip it.
// win (n, 5) = [slot, r_last, pos0, ne, w] per window, sorted by slot and, within a slot, by row; w = the window's index in
// (tick, j) order = its row of the launch's outputs.  valid: under transform t (t = 0: what the forecast kernels read)
struct WindowRow {
    int slot, r_last, pos0, ne, w;
    __device__ __forceinline__ long long pos(int t) const { return (long long)pos0 + (long long)t * ne; }
    __device__ __forceinline__ bool valid(const StreamParams& S, int t, int n_win, int n_windows) const {
        return slot >= 0 && slot < S.n_slots && r_last >= S.seg_len - 1 && pos0 >= 0 && ne >= 1 && pos(t) < n_win && w >= 0 && w < n_windows;
    }
};
__device__ __forceinline__ WindowRow load_window_row(const int* __restrict__ win, int q) {
    return WindowRow{win[5 * q], win[5 * q + 1], win[5 * q + 2], win[5 * q + 3], win[5 * q + 4]};
}
// win (n, 2) = [slot, r_last] per closed track: its pending rows are r_last - seg_len + 2 .. r_last
struct ClosedRow {
    int slot, r_last;
    __device__ __forceinline__ bool valid(const StreamParams& S) const { return slot >= 0 && slot < S.n_slots && r_last >= S.seg_len - 1; }
};
__device__ __forceinline__ ClosedRow load_closed_row(const int* __restrict__ win, int i) { return ClosedRow{win[2 * i], win[2 * i + 1]}; }
// desc (n, 4) = [slot, row index r, pos0 | -1, ne] per pushed row: the row itself, and the window ending at it if there is one
struct PushedRow {
    int slot, r, pos0, ne;
    __device__ __forceinline__ bool valid(const StreamParams& S) const { return slot >= 0 && slot < S.n_slots && r >= 0; }
    __device__ __forceinline__ bool has_window(const StreamParams& S, int n_win) const {
        return pos0 >= 0 && ne >= 1 && r >= S.seg_len - 1 && (long long)pos0 + (long long)(S.nt - 1) * ne < n_win;
    }
};
__device__ __forceinline__ PushedRow load_pushed_row(const int* __restrict__ desc, int i) {
    return PushedRow{desc[4 * i], desc[4 * i + 1], desc[4 * i + 2], desc[4 * i + 3]};
}

// one thread per (closed track i, pending row k, transform t, lane v of the row): the seg_len - 1 cells of rows r_last - seg_len + 2
// .. r_last of a ring (n_slots, nt, L, W) -- W = 1: the score ring (mcd_stream_flush), W = 17: the joint ring (mcd_stream_joint_flush)
template <int W>
__global__ __launch_bounds__(256) void stream_flush_kernel(StreamParams S, const float* __restrict__ cells, const int* __restrict__ win,
                                                           int n, float* __restrict__ out) {
    const int pend = S.seg_len - 1;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n * pend * S.nt * W) return;
    const int v = u % W, t = (u / W) % S.nt, k = (u / (W * S.nt)) % pend, i = u / (W * S.nt * pend);
    const ClosedRow c = load_closed_row(win, i);
    if (!c.valid(S)) return;
    out[u] = cells[(((size_t)c.slot * S.nt + t) * S.L + (c.r_last - S.seg_len + 2 + k) % S.L) * W + v];
}

// A GROUP of ticks in one launch (PoseStream.push / push_many): a track may receive R <= L - seg_len + 1 rows, so the rows
// r0 - seg_len + 1 .. r0 + R - 1 of a track -- the pending ones and the new ones -- sit at distinct ring positions, and no two
// rows of the launch share a pose position or a frame-score cell.  The group's windows are tick-major, inside a tick
// transform-major: the window of transform t of a row is at batch position pos0 + t * ne, with ne = its tick's window count
// (a single tick with n_emit windows: pos0 = the row's emit index j, ne = n_emit, the dataset's transform-major order).
// one thread per pushed row of desc; n_win = windows x transforms of the group.
// Per row: the normalised pose to both ring positions, the row's frame-score cell zeroed for every transform, and for pos0 >= 0
// the descriptors of the window ENDING at row r for every transform.
__global__ __launch_bounds__(256) void stream_push_group_kernel(StreamParams S, const float* __restrict__ raw,
                                                                const int* __restrict__ desc, int n, int n_win, float vid_w,
                                                                float vid_h, const double* __restrict__ center,
                                                                const double* __restrict__ scale, long long* __restrict__ base_out,
                                                                int* __restrict__ trans_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PushedRow d = load_pushed_row(desc, i);
    if (!d.valid(S)) return;
    const int p = d.r % S.L;
    float* o = S.ring + ((size_t)d.slot * 2 * S.L + p) * 34;
    normalize_pose_row(raw + (size_t)i * 34, vid_w, vid_h, center, scale, o, o + (size_t)S.L * 34);
    for (int t = 0; t < S.nt; ++t) S.fs[((size_t)d.slot * S.nt + t) * S.L + p] = 0.f;
    if (!d.has_window(S, n_win)) return;
    const long long base = ((long long)d.slot * 2 * S.L + (d.r - S.seg_len + 1) % S.L) * 34;
    for (int t = 0; t < S.nt; ++t) {
        base_out[(size_t)d.pos0 + (size_t)t * d.ne] = base;
        trans_out[(size_t)d.pos0 + (size_t)t * d.ne] = t;
    }
}

// The windows of one track overlap, so one thread per (track, transform) -- the thread of the track's FIRST window of the table --
// applies them in row order with plain loads and stores: per window max(score, 0), the clamp and zero start of scatter_max_kernel,
// goes into the cells of its rows r_last - seg_len + 1 .. r_last, so the cells end as after one launch per tick, and each window's
// oldest row, which no later window covers, is final once that window is in; final_out (n, num_transform) takes it at row w.
// (An emitting slot holds ONE track within a group: a slot is only handed out again inside a group when its track got no row in it.)
// walk_track_windows: that walk for transform t, begun at window q0 -- nothing unless q0 is its track's first window; then
// body(slot, r_last, pos, w) for every valid window of the track in row order, pos = its batch position under transform t.
template <class Body>
__device__ __forceinline__ void walk_track_windows(const StreamParams& S, const int* __restrict__ win, int n, int n_win, int q0, int t,
                                                   Body body) {
    const int slot = win[5 * q0];
    if (slot < 0 || slot >= S.n_slots) return;
    if (q0 > 0 && win[5 * (q0 - 1)] == slot) return;           // not the track's first window: the thread of that one walks on
    for (int q = q0; q < n && win[5 * q] == slot; ++q) {
        const WindowRow w = load_window_row(win, q);
        if (!w.valid(S, t, n_win, n)) continue;
        body(slot, w.r_last, w.pos(t), w.w);
    }
}

__global__ __launch_bounds__(256) void stream_frame_scores_group_kernel(StreamParams S, const float* __restrict__ scores,
                                                                        const int* __restrict__ win, int n, int n_win,
                                                                        float* __restrict__ final_out) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n * S.nt) return;
    const int q0 = u / S.nt, t = u - q0 * S.nt;
    walk_track_windows(S, win, n, n_win, q0, t, [&](int slot, int r_last, long long pos, int w) {
        float* row = S.fs + ((size_t)slot * S.nt + t) * S.L;
        const float sc = fmaxf(scores[pos], 0.f);
        const int first = r_last - S.seg_len + 1;
        for (int k = S.seg_len - 1; k >= 0; --k) {
            float* c = row + (first + k) % S.L;
            const float m = fmaxf(*c, sc);
            *c = m;
            if (k == 0) final_out[(size_t)w * S.nt + t] = m;
        }
    });
}

// Per-joint frame scores of a stream (mcd_stream_joint_state_t): ring (n_slots, nt, L, 17).  tx_of[k] = the index among the corrupt
// frames of window row k, or -1 (a condition frame: the window forecasts nothing there).
struct StreamJointParams {
    float* js;
    int tx_of[MCD_MAX_FRAMES];
    int Tx;
};
// The walk of stream_frame_scores_group_kernel, per joint: one thread per (track's FIRST window, transform, joint).  The window
// ending at row r_last INITIALISES that row's cell (its value there if it forecasts the row, else 0) -- the track's first window
// (r_last = seg_len - 1) all seg_len cells, which is what lets a reused slot or a wrapped ring start clean without the push kernel
// -- and takes the maximum into the older rows it forecasts; its oldest row is then final.  max(value, 0) as scatter_max_kernel.
__global__ __launch_bounds__(256) void stream_joint_scores_group_kernel(StreamParams S, StreamJointParams J, const float* __restrict__ maps,
                                                                        const int* __restrict__ win, int n, int n_win,
                                                                        float* __restrict__ final_out) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n * S.nt * 17) return;
    const int v = u % 17, qt = u / 17, q0 = qt / S.nt, t = qt - q0 * S.nt;
    walk_track_windows(S, win, n, n_win, q0, t, [&](int slot, int r_last, long long pos, int w) {
        float* cells = J.js + ((size_t)slot * S.nt + t) * S.L * 17 + v;
        const float* m = maps + (size_t)pos * J.Tx * 17 + v;
        const int first = r_last - S.seg_len + 1;
        const bool init_all = first == 0;
        for (int k = S.seg_len - 1; k >= 0; --k) {
            float* c = cells + (size_t)((first + k) % S.L) * 17;
            const int tx = J.tx_of[k];
            const float val = tx >= 0 ? fmaxf(m[tx * 17], 0.f) : 0.f;
            const float cur = (init_all || k == S.seg_len - 1) ? val : fmaxf(*c, val);
            *c = cur;
            if (k == 0) final_out[((size_t)w * S.nt + t) * 17 + v] = cur;
        }
    });
}

// ------------------------------------------------------------------------------------------------
// Forecast ring of a stream (mcd_stream_forecast_state_t): the expected pose of a row, leaving with the tick that makes it final.
//   forecast ring (n_slots, L, Tx, 34): cell (r % L, j) = row r as corrupt frame j of its ONE window, the window that ends at row
//                 r + seg_len - 1 - corrupt_idx[j]: that window's selected forecast of the row (pose_agg of aggregate_kernel: the
//                 best / worst sample by wave_select, zeros when no sample passes), interleaved x1,y1,...,x17,y17.
//   observed ring (n_slots, L, 34): the raw row r as it was pushed.
// Cell rule: a cell has exactly one writer, and nothing is stored about validity -- cell (r, j) is valid, seen from a track whose
// last row so far is r_hi, iff its window exists: corrupt_idx[j] <= r (the window does not begin before row 0) and
// r + seg_len - 1 - corrupt_idx[j] <= r_hi (it has been scored).  corrupt_idx ascends, so the valid j are ONE run [jb, ja) and
// ascending window order is descending j.  A reused slot and a wrapped ring need no initialisation: an invalid cell is never read,
// and a valid one was written by this track after any older content (a group holds at most L - seg_len + 1 rows per track, the
// bound that keeps rows r0 - seg_len + 1 .. r0 + R - 1 at distinct positions).
//   stream_forecast_store_kernel: workgroups 0 .. n_windows - 1, one 64-lane wave per transform-0 window of the group: select, then
//                 the Tx x 34 values into their cells; the workgroups behind them copy the group's raw rows, one thread per element.
//   stream_forecast_emit_kernel / stream_forecast_flush_kernel: one wave per final / pending row (forecast_emit_row): the k valid
//                 cells staged in LDS in window order, forecast_reduce_staged, denormalize_pose_row in the box of the observed row.
// Plain loads and stores; what a lane indexes at run time is LDS or global memory.
// ------------------------------------------------------------------------------------------------
struct StreamForecastParams {
    float* fc; float* obs;
    const float* loss_all; const float* poses_all;      // (n_win, S), (n_win, S, 2, Tx, 17) of the group's scoring call
    float* expected; float* norm; float* observed; int* count; float* spread;
    const double* center; const double* scale;
    float vid_w, vid_h;
    int Tx, S, strategy, in_lds, method, spread_method;
    int cidx[MCD_MAX_FRAMES];
};

__global__ __launch_bounds__(64) void stream_forecast_store_kernel(StreamParams S, StreamForecastParams F, const float* __restrict__ raw,
                                                                   const int* __restrict__ desc, int n, const int* __restrict__ win,
                                                                   int n_windows, int n_win) {
    extern __shared__ float sfc_lds[];      // [SEL_LDS_WORDS] wave_select's, [S] staged losses (in_lds)
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_windows) {     // the raw rows of desc, as stream_push_group_kernel reads it
        const long long u = (long long)((int)blockIdx.x - n_windows) * 64 + lane;
        if (u >= (long long)n * 34) return;
        const int i = (int)(u / 34), f = (int)(u - (long long)i * 34);
        const PushedRow d = load_pushed_row(desc, i);
        if (!d.valid(S)) return;
        F.obs[((size_t)d.slot * S.L + d.r % S.L) * 34 + f] = raw[u];
        return;
    }
    const WindowRow w = load_window_row(win, blockIdx.x);      // win (n_windows, 5): the window's transform-0 position is pos0
    if (!w.valid(S, 0, n_win, n_windows)) return;
    const SampleVals X = stage_samples(F.loss_all + (size_t)w.pos0 * F.S, 1, F.S, sfc_lds + SEL_LDS_WORDS, F.in_lds != 0, lane);
    const Selection sel = wave_select(X, F.S, lane, F.strategy, 0.f, sfc_lds);
    const float* p = F.poses_all + ((size_t)w.pos0 * F.S + (sel.i0 >= 0 ? sel.i0 : 0)) * 34 * F.Tx;
    const int first = w.r_last - S.seg_len + 1;
    for (int j = 0; j < F.Tx; ++j) {        // (j is wave-uniform: corrupt_idx is read from the kernel arguments)
        const int r = first + F.cidx[j];
        if (lane < 34)
            F.fc[(((size_t)w.slot * S.L + r % S.L) * F.Tx + j) * 34 + lane] = sel.i0 >= 0 ? p[((lane & 1) * F.Tx + j) * 17 + (lane >> 1)] : 0.f;
    }
}

// Row r of `slot`, seen with r_hi the track's last row so far, into row o of the five outputs.  vals [MCD_MAX_FRAMES * 34], pn [34],
// sd [34], mid [2]: LDS.  One wave; every lane takes the same branches.
// TTA (the ring of every transform, below): the row's cells are (S.nt, Tx, 34), its pairs the k1 windows of transform 0, then those
// of transform 1, ...: k = S.nt * k1 <= FORECAST_VIEW_COVER rows of vals.
template <bool TTA = false>
__device__ __forceinline__ void forecast_emit_row(const StreamParams& S, const StreamForecastParams& F, int slot, int r, int r_hi, size_t o,
                                                  int lane, float* vals, float* pn, double* sd, double* mid) {
    int ja = 0, jb = 0;
    for (int j = 0; j < F.Tx; ++j) {
        const int c = F.cidx[j];
        ja += c <= r ? 1 : 0;
        jb += r + S.seg_len - 1 - c > r_hi ? 1 : 0;
    }
    const int k1 = ja > jb ? ja - jb : 0, k = TTA ? k1 * S.nt : k1;
    const size_t row = (size_t)slot * S.L + r % S.L;
    const float* cell = F.fc + row * (TTA ? S.nt : 1) * F.Tx * 34;
    for (int e = lane; e < k * 34; e += 64) {      // window order: the m-th window of the row holds it as corrupt frame ja - 1 - m
        const int p = e / 34, f = e - p * 34, t = TTA ? p / k1 : 0, m = p - t * k1;
        vals[e] = cell[(t * F.Tx + ja - 1 - m) * 34 + f];
    }
    if (lane < 34) F.observed[o * 34 + lane] = F.obs[row * 34 + lane];
    if (lane == 0) F.count[o] = k;
    if (k == 0) {                                   // no window forecasts the row: all zero
        if (lane < 34) { F.norm[o * 34 + lane] = 0.f; F.expected[o * 34 + lane] = 0.f; }
        if (lane == 0) F.spread[o] = 0.f;
        return;
    }
    __syncthreads();
    forecast_reduce_staged(vals, k, F.method, F.spread_method, lane, sd, mid, pn, F.spread + o);
    __syncthreads();
    if (lane < 34) F.norm[o * 34 + lane] = pn[lane];
    if (lane == 0) denormalize_pose_row(pn, F.obs + row * 34, F.vid_w, F.vid_h, F.center, F.scale, F.expected + o * 34);
}

// one wave per window of the group's table: its oldest row r_last - seg_len + 1 is final, every window covering it is in
__global__ __launch_bounds__(64) void stream_forecast_emit_kernel(StreamParams S, StreamForecastParams F, const int* __restrict__ win,
                                                                  int n_windows, int n_win) {
    __shared__ float vals[MCD_MAX_FRAMES * 34], pn[34];
    __shared__ double sd[34], mid[2];
    const int q = blockIdx.x;
    if (q >= n_windows) return;
    const WindowRow w = load_window_row(win, q);
    if (!w.valid(S, 0, n_win, n_windows)) return;
    forecast_emit_row(S, F, w.slot, w.r_last - S.seg_len + 1, w.r_last, (size_t)w.w, threadIdx.x, vals, pn, sd, mid);
}

// one wave per (closed track i, pending row k): rows r_last - seg_len + 2 .. r_last see only the windows that exist
__global__ __launch_bounds__(64) void stream_forecast_flush_kernel(StreamParams S, StreamForecastParams F, const int* __restrict__ win, int n) {
    __shared__ float vals[MCD_MAX_FRAMES * 34], pn[34];
    __shared__ double sd[34], mid[2];
    const int pend = S.seg_len - 1, u = blockIdx.x;
    if (u >= n * pend) return;
    const int i = u / pend, k = u - i * pend;
    const ClosedRow c = load_closed_row(win, i);
    if (!c.valid(S)) return;
    forecast_emit_row(S, F, c.slot, c.r_last - S.seg_len + 2 + k, c.r_last, (size_t)u, threadIdx.x, vals, pn, sd, mid);
}

// ------------------------------------------------------------------------------------------------
// The forecast ring over EVERY transform (mcd_stream_forecast_tta_state_t): ring (n_slots, L, nt, Tx, 34), cell (r % L, t, j) = row r
// as corrupt frame j of its one window under transform t, already mapped back by inverse_affine_coord (mcd_post_kernel.hpp) with row t
// of the inverse table -- what forecast_reduce_view_kernel stages on the dataset path.  The cell rule above does not depend on t.
//   stream_forecast_store_tta_kernel: workgroups 0 .. n_windows * nt - 1, one wave per (window of the table, transform); behind them
//                 the raw rows, as stream_forecast_store_kernel copies them.
//   stream_forecast_emit_tta_kernel / _flush_tta_kernel: forecast_emit_row<true>: transform ascending, then window order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void stream_forecast_store_tta_kernel(StreamParams S, StreamForecastParams F, const double* __restrict__ inv,
                                                                       const float* __restrict__ raw, const int* __restrict__ desc, int n,
                                                                       const int* __restrict__ win, int n_windows, int n_win) {
    extern __shared__ float sft_lds[];      // [SEL_LDS_WORDS] wave_select's, [S] staged losses (in_lds)
    const int lane = threadIdx.x, n_wt = n_windows * S.nt;
    if ((int)blockIdx.x >= n_wt) {
        const long long u = (long long)((int)blockIdx.x - n_wt) * 64 + lane;
        if (u >= (long long)n * 34) return;
        const int i = (int)(u / 34), f = (int)(u - (long long)i * 34);
        const PushedRow d = load_pushed_row(desc, i);
        if (!d.valid(S)) return;
        F.obs[((size_t)d.slot * S.L + d.r % S.L) * 34 + f] = raw[u];
        return;
    }
    const int q = blockIdx.x / S.nt, t = blockIdx.x - q * S.nt;
    const WindowRow w = load_window_row(win, q);
    if (!w.valid(S, t, n_win, n_windows)) return;
    const size_t pos = (size_t)w.pos(t);    // the window's batch position under transform t (trans_out[pos] = t)
    const SampleVals X = stage_samples(F.loss_all + pos * F.S, 1, F.S, sft_lds + SEL_LDS_WORDS, F.in_lds != 0, lane);
    const Selection sel = wave_select(X, F.S, lane, F.strategy, 0.f, sft_lds);
    const float* p = F.poses_all + (pos * F.S + (sel.i0 >= 0 ? sel.i0 : 0)) * 34 * F.Tx;
    const int first = w.r_last - S.seg_len + 1;
    for (int j = 0; j < F.Tx; ++j) {
        const int r = first + F.cidx[j];
        if (lane < 34) {                    // no sample passes: the zeros of pose_agg, mapped like any forecast
            const float xp = sel.i0 >= 0 ? p[j * 17 + (lane >> 1)] : 0.f, yp = sel.i0 >= 0 ? p[(F.Tx + j) * 17 + (lane >> 1)] : 0.f;
            F.fc[((((size_t)w.slot * S.L + r % S.L) * S.nt + t) * F.Tx + j) * 34 + lane] = inverse_affine_coord(inv + 6 * t, xp, yp, lane & 1);
        }
    }
}

__global__ __launch_bounds__(64) void stream_forecast_emit_tta_kernel(StreamParams S, StreamForecastParams F, const int* __restrict__ win,
                                                                      int n_windows, int n_win) {
    __shared__ float vals[FORECAST_VIEW_COVER * 34], pn[34];
    __shared__ double sd[34], mid[2];
    const int q = blockIdx.x;
    if (q >= n_windows) return;
    const WindowRow w = load_window_row(win, q);
    if (!w.valid(S, 0, n_win, n_windows)) return;
    forecast_emit_row<true>(S, F, w.slot, w.r_last - S.seg_len + 1, w.r_last, (size_t)w.w, threadIdx.x, vals, pn, sd, mid);
}

__global__ __launch_bounds__(64) void stream_forecast_flush_tta_kernel(StreamParams S, StreamForecastParams F, const int* __restrict__ win, int n) {
    __shared__ float vals[FORECAST_VIEW_COVER * 34], pn[34];
    __shared__ double sd[34], mid[2];
    const int pend = S.seg_len - 1, u = blockIdx.x;
    if (u >= n * pend) return;
    const int i = u / pend, k = u - i * pend;
    const ClosedRow c = load_closed_row(win, i);
    if (!c.valid(S)) return;
    forecast_emit_row<true>(S, F, c.slot, c.r_last - S.seg_len + 2 + k, c.r_last, (size_t)u, threadIdx.x, vals, pn, sd, mid);
}

// ------------------------------------------------------------------------------------------------
// Online clip scores of a live stream (mcd_clip_state_t): per (clip slot, transform, ring position) one CELL = the person
// aggregate of one video frame so far, sum / lmax / lmin in f64 and the person count n.  The host (mocodad_amd/stream.py:
// ClipTable) owns the frame axis: which frame sits at which position, which cells are open, complete, emitted.
//   stream_clip_update_kernel: the final per-row frame scores of a tick (or a group of ticks) into their cells.
//   stream_clip_emit_kernel  : shift + gaussian_filter1d ('reflect') + mean over the transforms for the frames that became
//                              computable, with the functions and the summation order of frame_scores_kernel.
// ------------------------------------------------------------------------------------------------
struct ClipParams {
    double* sum; double* lmax; double* lmin; int* n;
    int n_clips, L, nt;
};

// One thread per (cell run, transform): runs (n_runs, 5) = [clip slot, ring position, first contribution, count, zero-first];
// contrib (n_contrib, 2) = [source: 0 = finals, 1 = tails; row of that (rows, num_transform) f32 tensor].  A launch names a cell
// at most once, so its thread owns it: plain loads and stores, contributions added in list order.
__global__ __launch_bounds__(256) void stream_clip_update_kernel(ClipParams C, const int* __restrict__ runs, int n_runs,
                                                                 const int* __restrict__ contrib, int n_contrib,
                                                                 const float* __restrict__ finals, int n_finals,
                                                                 const float* __restrict__ tails, int n_tails) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_runs * C.nt) return;
    const int q = u / C.nt, t = u - q * C.nt;
    const int slot = runs[5 * q], pos = runs[5 * q + 1], first = runs[5 * q + 2], count = runs[5 * q + 3], zero = runs[5 * q + 4];
    if (slot < 0 || slot >= C.n_clips || pos < 0 || pos >= C.L) return;      // (a run the host table cannot produce: touch nothing)
    const size_t c = ((size_t)slot * C.nt + t) * C.L + pos;
    double sum = 0.0, lmax = 0.0, lmin = 0.0;
    int cnt = 0;
    if (!zero) { sum = C.sum[c]; lmax = C.lmax[c]; lmin = C.lmin[c]; cnt = C.n[c]; }
    if (first >= 0 && count > 0 && (long long)first + count <= n_contrib)
        for (int i = first; i < first + count; ++i) {
            const int src = contrib[2 * i], row = contrib[2 * i + 1];
            const float* p = src == 0 ? finals : src == 1 ? tails : nullptr;
            if (!p || row < 0 || row >= (src == 0 ? n_finals : n_tails)) continue;
            person_aggr_add(sum, lmax, lmin, cnt, p[(size_t)row * C.nt + t]);
        }
    C.sum[c] = sum; C.lmax[c] = lmax; C.lmin[c] = lmin; C.n[c] = cnt;
}

struct ClipEmitParams {
    const int* outs;          // (n_out, 4) = [clip slot, frame offset j from the segment's origin, segment length m | -1 = open, ring position of the origin]
    const double* gauss;      // (2 radius + 1,)
    double* out;              // (n_out,)
    int n_out, radius, shift, opb, staged;
};
constexpr int CLIP_OPEN_LEN = 1 << 29;      // "no end yet": offsets stay below it, so 'reflect' only acts at the origin

// shifted(k) of transform t: the raw score of frame offset k - shift (0 before the origin + shift, 0 for a frame nobody contributed to)
__device__ __forceinline__ double clip_shifted(const ClipParams& C, int slot, int t, int pbase, int k, int m, int shift) {
    k = reflect_index(k, m);
    if (k < shift) return 0.0;
    const size_t c = ((size_t)slot * C.nt + t) * C.L + (size_t)(((long long)pbase + (k - shift)) % C.L);
    const int cnt = C.n[c];
    return cnt > 0 ? person_aggr_value(C.sum[c], C.lmax[c], C.lmin[c], cnt) : 0.0;
}

// One workgroup per `opb` outputs.  Staged mapping: all threads fill the 2 radius + 1 shifted values of every (output, transform)
// into LDS (the divisions and the cell loads run in parallel), then one thread per (output, transform) runs the tap chain in the
// stated order, then one thread per output adds the transforms in ascending order.  A kernel too wide for LDS (staged = 0) lets the
// tap thread compute its values itself.  Outputs with a slot, offset or origin position out of range come back as 0.
__global__ __launch_bounds__(256) void stream_clip_emit_kernel(ClipParams C, ClipEmitParams E) {
    extern __shared__ __attribute__((aligned(16))) double csm[];
    const int W = 2 * E.radius + 1, o0 = blockIdx.x * E.opb, tid = threadIdx.x;
    double* part = csm;                          // [opb * nt] filtered value per (output, transform)
    double* sh = csm + E.opb * C.nt;             // staged: [opb * nt][W]
    auto valid = [&](int o, int& slot, int& j, int& m, int& pbase) -> bool {
        if (o >= E.n_out) return false;
        slot = E.outs[4 * o]; j = E.outs[4 * o + 1]; m = E.outs[4 * o + 2]; pbase = E.outs[4 * o + 3];
        if (m < 0) m = CLIP_OPEN_LEN;
        return slot >= 0 && slot < C.n_clips && j >= 0 && j < m && m <= CLIP_OPEN_LEN && pbase >= 0 && pbase < C.L;
    };
    int slot, j, m, pbase;
    if (E.staged)
        for (int e = tid; e < E.opb * C.nt * W; e += blockDim.x) {
            const int ot = e / W, i = e - ot * W, ol = ot / C.nt, t = ot - ol * C.nt;
            if (valid(o0 + ol, slot, j, m, pbase)) sh[e] = clip_shifted(C, slot, t, pbase, j - E.radius + i, m, E.shift);
        }
    __syncthreads();
    if (tid < E.opb * C.nt) {
        const int ol = tid / C.nt, t = tid - ol * C.nt;
        if (valid(o0 + ol, slot, j, m, pbase)) {
            if (E.staged) {
                const double* row = sh + (size_t)tid * W + (E.radius - j);
                part[tid] = gauss_taps([&](int k) -> double { return row[k]; }, j, E.gauss, E.radius);
            } else {
                part[tid] = gauss_taps([&](int k) -> double { return clip_shifted(C, slot, t, pbase, k, m, E.shift); }, j, E.gauss, E.radius);
            }
        }
    }
    __syncthreads();
    if (tid < E.opb && o0 + tid < E.n_out) {
        double acc = 0.0;
        const bool ok = valid(o0 + tid, slot, j, m, pbase);
        for (int t = 0; ok && t < C.nt; ++t) acc += part[tid * C.nt + t];
        E.out[o0 + tid] = acc / (double)C.nt;
    }
}

}  // namespace

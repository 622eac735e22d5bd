// mcd_post_kernel.hpp — the device code of mcd_api.hip's own launches, everything around the trajectory kernels:
//   aggregate_kernel            MoCoDAD._aggregation_strategy                                  models/mocodad.py:454-520
//   error_maps_kernel           the per-element loss of :484 before its mean, under the same sample selection (mcd_error_maps)
//                               -- both on ONE statement of that selection: SelectParams, corrupt_frame, wave_select, wave_pose_stat
//   scatter_max<W> / frame_scatter / frame_scores kernels   post_processing                    models/mocodad.py:362-425
//                               (W = 1: window scores, W = 17: per-joint maps; atomic_max_nonneg is the one scatter-max idiom)
//   normalize_poses_kernel      dataset loader: bbox-centre coordinates + RobustScaler      utils/data.py:11-43,165-186,350-359
//   denormalize_poses_kernel    its inverse, back to image pixels in the observed row's bounding box (mcd_denormalize_poses)
//   forecast_claim / forecast_reduce kernels   overlapping window forecasts -> one pose per (person, frame) cell + their spread
//                               (mcd_forecast_assemble)                                         utils/eval_utils.py:13-24,37-72
//   stream_push_group / stream_frame_scores_group / stream_flush<W> kernels   the same loader step + sliding windows + scatter-max,
//                               one group of ticks at a time (a single tick is a group of one) on device rings
//                                                               utils/preprocessing.py:14-86, models/mocodad.py:392-393
//   stream_clip_update / stream_clip_emit kernels   online per-clip frame scores: the person aggregate, shift and Gaussian of
//                               post_processing, incrementally on a per-clip ring     models/mocodad.py:399-424, utils/eval_utils.py:100-106
//   stream_joint_scores_group kernel   the per-joint sibling of the stream's score ring, fed by the error maps: the same walk over a
//                               track's windows (walk_track_windows) with its own cell rule; flushed by stream_flush<17>
//   stream_forecast_store / stream_forecast_emit / stream_forecast_flush kernels   the stream's forecast ring: per window the selected
//                               forecast (wave_select) into the cells of the rows it forecasts, per final / pending row the
//                               reduction of forecast_reduce_kernel (forecast_reduce_staged) and denormalize_pose_row
//   philox_noise / random_imp_masks kernels   the perf mode's draws, exported (mcd_philox_noise, mcd_random_imp_masks)
//   gather_frames_kernel        the dense copy of the condition frames cond_encode_kernel reads
//   poison_lds_kernel           test aid (mcd_debug_poison_lds)
// with the parameter blocks the host fills (SelectParams inside AggrParams and MapParams, StreamParams, StreamJointParams,
// StreamForecastParams, FrameParams, ClipParams, ClipEmitParams).  Included once, by mcd_api.hip (which defines API_THREADS and says `using namespace mcd`), in front
// of its host code.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Which samples a window's score comes from (mocodad.py:454-520), stated once for aggregate_kernel and error_maps_kernel: one
// 64-lane wave per window, ANY S (the reference's shipped n_generated_samples is 50, config/*/mocodad_test.yaml; its
// _aggregation_strategy has no cap)
// ------------------------------------------------------------------------------------------------
struct SelectParams {         // filled by fill_select, in_lds by launch_select (mcd_api.hip)
    const float* loss_all; const float* pose_all;
    const int* win_mask;      // random_imp: (B,) condition-frame bitmasks; the window's corrupt frames are its clear bits in ascending
                              // order and corrupt_idx is not read.  null = corrupt_idx
    int B, S, Tx, seg_len, strategy, loss_fn, in_lds;
    float q;
    int corrupt_idx[MCD_MAX_FRAMES];
};
constexpr int AGG_LDS_MAX = 8192;       // sample values staged in LDS (32 KB); a longer sample axis is read in place
constexpr int SEL_LDS_WORDS = 4;        // in front of them: the two selected order statistics and their sample indices

// data frame of the window's tx-th corrupt frame (max: a mask with more than seg_len - Tx bits set, which the caller must not
// pass, still reads inside the window)
__device__ __forceinline__ int corrupt_frame(const SelectParams& P, int b, int tx) {
    return P.win_mask ? max(nth_set_bit(~(unsigned)P.win_mask[b] & low_bits(P.seg_len), tx), 0) : P.corrupt_idx[tx];
}

// The S values of one window (its per-sample losses, or one pose element across the samples): staged in LDS, or -- beyond
// AGG_LDS_MAX samples -- read where they lie (stride = floats between consecutive samples).
struct SampleVals {
    const float* p; long long stride;
    __device__ __forceinline__ float operator()(int k) const { return p[(long long)k * stride]; }
};
__device__ __forceinline__ SampleVals stage_samples(const float* src, long long stride, int S, float* lds, bool in_lds, int lane) {
    if (!in_lds) return SampleVals{src, stride};
    __syncthreads();                                     // the previous round's readers are done with `lds`
    for (int k = lane; k < S; k += 64) lds[k] = src[(long long)k * stride];
    __syncthreads();
    return SampleVals{lds, 1};
}
// Sums and best / worst run in sample order on wave-uniform values: bit-identical to the sequential loops of
// aggregate_losses in the fused kernel.
__device__ __forceinline__ float wave_mean(const SampleVals& X, int S) {
    float sum = 0.f;
    for (int k = 0; k < S; ++k) sum += X(k);
    return sum / (float)S;
}
// torch.lerp's two-sided form (torch.quantile): the interpolation of two order statistics a <= c (also applied per map cell by
// error_maps_kernel, where a, c are any two values)
__device__ __forceinline__ float lerp_two_sided(float a, float c, float wgt) {
    return wgt < 0.5f ? a + wgt * (c - a) : c - (c - a) * (1.f - wgt);
}
// The selection of the loss-based strategies best / worst / median / quantile (mean needs none) on the staged losses X of one
// window: the aggregated loss `value` (aggregate_kernel) and the one or two samples i0, i1 it comes from, with the interpolation
// weight between them (error_maps_kernel; best / worst / median: the same sample twice, weight 0).  All lanes return the same.
//   best / worst (mocodad.py:504-512): strict comparisons from 1e10 / -1, so the FIRST of equal samples stays; no sample
//     passes (all NaN, or none below 1e10) -> i0 = i1 = -1.
//   median / quantile: order statistics by rank counting: sample i's rank = #{k : x_k < x_i or (x_k == x_i and k < i)} is a
//     permutation of 0 .. S-1 whatever the ties; lane l ranks the samples l, l + 64, ...; the samples of rank r0 / r1 land in
//     slot[0] / slot[1], their indices in slot[2] / slot[3].  (No sort, no per-thread array: O(S^2 / 64) broadcast reads per lane.)
//     torch.median: the lower middle value; torch.quantile: linear interpolation.
//     A NaN among the samples (a diverged chain) breaks the permutation -- every NaN ranks 0 and the rank asked for may have no
//     writer -- and torch.median / torch.quantile return NaN then (mocodad.py:489-492,513-516): so does this, with i0 = i1 = -1.
struct Selection { int i0, i1; float wgt, value; };
__device__ __forceinline__ Selection wave_select(const SampleVals& X, int S, int lane, int strategy, float q, float* slot) {
    if (strategy == MCD_AGGR_BEST || strategy == MCD_AGGR_WORST) {
        const bool best = strategy == MCD_AGGR_BEST;
        float cur = best ? 1e10f : -1.f;
        int sel = -1;
        for (int k = 0; k < S; ++k) {
            const float y = X(k);
            if (best ? (y < cur) : (y > cur)) { cur = y; sel = k; }
        }
        return Selection{sel, sel, 0.f, cur};
    }
    int r0 = (S - 1) / 2, r1 = r0;
    float wgt = 0.f;
    if (strategy != MCD_AGGR_MEDIAN) {      // (as aggregate_losses, mcd_chain.hpp: sharing the text moved the trajectory objects)
        const float pos = fminf(fmaxf(q, 0.f), 1.f) * (float)(S - 1);      // (q is validated on the host; the clamp is a backstop)
        r0 = (int)floorf(pos);
        r1 = r0 + 1 < S ? r0 + 1 : S - 1;
        wgt = pos - (float)r0;
    }
    int* islot = reinterpret_cast<int*>(slot + 2);
    bool nan = false;
    for (int i = lane; i < S; i += 64) {
        const float x = X(i);
        nan |= x != x;
        int r = 0;
        for (int k = 0; k < S; ++k) {
            const float y = X(k);
            r += (y < x || (y == x && k < i)) ? 1 : 0;
        }
        if (r == r0) { slot[0] = x; islot[0] = i; }
        if (r == r1) { slot[1] = x; islot[1] = i; }
    }
    __syncthreads();
    const bool any_nan = __ballot(nan) != 0ull;        // (one 64-lane wave per workgroup: the kernels' launch bound)
    const float a = any_nan ? __builtin_nanf("") : slot[0], c = any_nan ? __builtin_nanf("") : slot[1];
    const Selection sel{any_nan ? -1 : islot[0], any_nan ? -1 : islot[1], wgt, strategy == MCD_AGGR_MEDIAN ? a : lerp_two_sided(a, c, wgt)};
    __syncthreads();
    return sel;
}
// mean_pose / median_pose (mocodad.py:493-503): the mean or the lower median of ONE pose element across the S samples, wave-uniform
__device__ __forceinline__ float wave_pose_stat(const SampleVals& X, int S, int lane, int strategy, float* slot) {
    return strategy == MCD_AGGR_MEAN_POSE ? wave_mean(X, S) : wave_select(X, S, lane, MCD_AGGR_MEDIAN, 0.f, slot).value;
}

// aggregation over the S samples: loss_agg (B,), and pose_agg under best / worst and the *_pose strategies.  data: dense
// (B,C,T,V) windows at any C, V (read by the *_pose strategies only)
struct AggrParams {
    SelectParams s;
    const float* data; float* loss_agg; float* pose_agg;
    int C, V;
};
__global__ __launch_bounds__(64) void aggregate_kernel(const AggrParams A) {
    extern __shared__ float agg_lds[];
    float* slot = agg_lds;                      // [SEL_LDS_WORDS] wave_select's
    float* vals = agg_lds + SEL_LDS_WORDS;      // [S] staged sample values (in_lds)
    const SelectParams& P = A.s;
    const int lane = threadIdx.x, S = P.S, per = A.C * P.Tx * A.V;
    const bool in_lds = P.in_lds != 0;
    for (int b = blockIdx.x; b < P.B; b += gridDim.x) {
        if (P.strategy != MCD_AGGR_MEAN_POSE && P.strategy != MCD_AGGR_MEDIAN_POSE) {
            const SampleVals X = stage_samples(P.loss_all + (size_t)b * S, 1, S, vals, in_lds, lane);
            if (P.strategy == MCD_AGGR_MEAN) {
                const float mean = wave_mean(X, S);
                if (lane == 0) A.loss_agg[b] = mean;
                continue;
            }
            const Selection sel = wave_select(X, S, lane, P.strategy, P.q, slot);
            if (lane == 0) A.loss_agg[b] = sel.value;
            if (A.pose_agg && (P.strategy == MCD_AGGR_BEST || P.strategy == MCD_AGGR_WORST))
                for (int e = lane; e < per; e += 64)
                    A.pose_agg[(size_t)b * per + e] = sel.i0 >= 0 ? P.pose_all[((size_t)b * S + sel.i0) * per + e] : 0.f;
        } else {  // per element over the S generated poses, then the loss of that pose
            float acc = 0.f;      // (every lane carries the same running sum: the per-element values are wave-uniform)
            for (int e = 0; e < per; ++e) {
                const SampleVals X = stage_samples(P.pose_all + (size_t)b * S * per + e, per, S, vals, in_lds, lane);
                const float val = wave_pose_stat(X, S, lane, P.strategy, slot);
                if (A.pose_agg && lane == 0) A.pose_agg[(size_t)b * per + e] = val;
                const int c = e / (P.Tx * A.V), tx = (e / A.V) % P.Tx, v = e % A.V;
                const float gt = A.data[(((size_t)b * A.C + c) * P.seg_len + corrupt_frame(P, b, tx)) * A.V + v];
                acc += loss_elem(val, gt, P.loss_fn);
            }
            if (lane == 0) A.loss_agg[b] = acc / (float)per;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Error maps (mcd_error_maps): which joints and forecast frames a window's score comes from.  One 64-lane wave per window like
// aggregate_kernel, with the same selection on the same loss_all bits -- wave_select, wave_pose_stat, corrupt_frame above:
// E[b,s,t,v] = (1/C) sum_c loss_elem(pose, gt), the ground truth loaded by load_coord -- the trajectory kernels' loader, so the
// bits the loss saw.  The window's sample(s) are chosen by the wave, then the lanes take the Tx * V cells.
// ------------------------------------------------------------------------------------------------
struct MapParams {
    SelectParams s;
    DataView dv;
    float* maps;
};
// E of one cell for the pose at `p` (element (c, cell) at p[c * cells + cell]) against the ground truth (g0, g1)
__device__ __forceinline__ float map_cell(const float* __restrict__ p, int cells, int cell, float g0, float g1, int loss_fn) {
    return (loss_elem(p[cell], g0, loss_fn) + loss_elem(p[cells + cell], g1, loss_fn)) / (float)C0;
}

__global__ __launch_bounds__(64) void error_maps_kernel(const MapParams M) {
    extern __shared__ float map_lds[];
    float* slot = map_lds;                      // [SEL_LDS_WORDS] wave_select's
    float* vals = map_lds + SEL_LDS_WORDS;      // [S] staged sample values (in_lds)
    const SelectParams& P = M.s;
    const int lane = threadIdx.x, S = P.S, cells = P.Tx * 17, per = C0 * cells;
    const bool in_lds = P.in_lds != 0;
    const float nanv = __builtin_nanf("");
    for (int b = blockIdx.x; b < P.B; b += gridDim.x) {
        const float* pose_b = P.pose_all + (size_t)b * S * per;
        if (P.strategy == MCD_AGGR_MEAN_POSE || P.strategy == MCD_AGGR_MEDIAN_POSE) {
            // per element over the S poses as aggregate_kernel forms pose_agg (wave-uniform values), cell by cell
            float* out = M.maps + (size_t)b * cells;
            for (int cell = 0; cell < cells; ++cell) {
                const int tx = cell / 17, v = cell - tx * 17, frame = corrupt_frame(P, b, tx);
                float acc = 0.f;
                for (int c = 0; c < C0; ++c) {
                    const SampleVals X = stage_samples(pose_b + c * cells + cell, per, S, vals, in_lds, lane);
                    acc += loss_elem(wave_pose_stat(X, S, lane, P.strategy, slot), load_coord(M.dv, b, c, frame, v, P.seg_len), P.loss_fn);
                }
                if (lane == 0) out[cell] = acc / (float)C0;
            }
            continue;
        }
        if (P.strategy == MCD_AGGR_ALL) {
            float* out = M.maps + (size_t)b * S * cells;
            for (int u = lane; u < S * cells; u += 64) {
                const int s = u / cells, cell = u - s * cells, tx = cell / 17, v = cell - tx * 17, frame = corrupt_frame(P, b, tx);
                out[u] = map_cell(pose_b + (size_t)s * per, cells, cell, load_coord(M.dv, b, 0, frame, v, P.seg_len),
                                  load_coord(M.dv, b, 1, frame, v, P.seg_len), P.loss_fn);
            }
            continue;
        }
        // loss-based strategies: the sample(s), decided on the loss_all bits alone
        Selection sel{-1, -1, 0.f, 0.f};
        if (P.strategy != MCD_AGGR_MEAN) sel = wave_select(stage_samples(P.loss_all + (size_t)b * S, 1, S, vals, in_lds, lane), S, lane, P.strategy, P.q, slot);
        float* out = M.maps + (size_t)b * cells;
        for (int cell = lane; cell < cells; cell += 64) {
            const int tx = cell / 17, v = cell - tx * 17, frame = corrupt_frame(P, b, tx);
            const float g0 = load_coord(M.dv, b, 0, frame, v, P.seg_len), g1 = load_coord(M.dv, b, 1, frame, v, P.seg_len);
            float m;
            if (P.strategy == MCD_AGGR_MEAN) {
                float sum = 0.f;
                for (int k = 0; k < S; ++k) sum += map_cell(pose_b + (size_t)k * per, cells, cell, g0, g1, P.loss_fn);
                m = sum / (float)S;
            } else if (sel.i0 < 0 || sel.i1 < 0) {
                m = nanv;
            } else {
                m = map_cell(pose_b + (size_t)sel.i0 * per, cells, cell, g0, g1, P.loss_fn);
                if (P.strategy == MCD_AGGR_QUANTILE && sel.i1 != sel.i0)
                    m = lerp_two_sided(m, map_cell(pose_b + (size_t)sel.i1 * per, cells, cell, g0, g1, P.loss_fn), sel.wgt);
            }
            out[cell] = m;
        }
    }
}

// Scatter-max (mocodad.py:392-393 + eval_utils.py:27-34).  Non-negative floats order like their bit patterns, so the maximum of
// max(v, 0) (a NaN adds 0) over many writers is one atomicMax on the int view of a cell that starts at 0 (= absent).
__device__ __forceinline__ void atomic_max_nonneg(float* cell, float v) {
    atomicMax(reinterpret_cast<int*>(cell), __float_as_int(fmaxf(v, 0.f)));
}
// One thread per (window i, frame slot k, lane v of the W-wide row): out (n_rows, n_frames, W).  W = 1 (mcd_scatter_max): the
// window's score for each of its n_slot = seg_len frames; W = 17 (mcd_joint_scatter_max): vals = maps (n, n_slot = Tx, 17), per
// joint.  Frames outside [1, n_frames] and rows outside [0, n_rows) are ignored.
template <int W>
__global__ void scatter_max_kernel(const float* __restrict__ vals, const int* __restrict__ frames, const int* __restrict__ row,
                                   long long n, int n_slot, int n_rows, int n_frames, float* __restrict__ out) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n * n_slot * W) return;
    const long long ik = u / W, i = ik / n_slot;
    const int v = (int)(u - ik * W), f = frames[ik] - 1, r = row[i];
    if (f < 0 || f >= n_frames || r < 0 || r >= n_rows) return;
    atomic_max_nonneg(out + ((size_t)r * n_frames + f) * W + v, vals[W == 1 ? i : u]);
}

// Per-frame pose normalisation of the dataset loader (utils/data.py:11-43,165-186 + 350-359), one thread per frame, in the
// reference's own precision (NumPy >= 2 scalar rules, DESIGN.md "Dataset loading"): the box, its margin and the clip in fp32,
// round-half-even to int, (x - centre) / size correctly rounded in fp32 (computed in double and rounded once: exact, 53 >= 2*24+2),
// then sklearn's RobustScaler.transform, which runs x - center_ and / scale_ in float64 and rounds to fp32 after each.
// raw (n, 34) = x1,y1,...,x17,y17; out (n, 2, 17).
// normalize_pose_row: one row, written to `o` and, when o2 != nullptr, to `o2` as well (the mirrored copy of a track ring).
__device__ __forceinline__ void normalize_pose_row(const float* __restrict__ r, float vid_w, float vid_h,
                                                   const double* __restrict__ center, const double* __restrict__ scale,
                                                   float* __restrict__ o, float* __restrict__ o2) {
#pragma clang fp contract(off)      // the margin is 0.1 * (r - l + 1), then l - margin: two roundings, never an FMA
    float v[34];
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int k = 0; k < 34; k += 2) {
        v[k] = r[k]; v[k + 1] = r[k + 1];
        if (v[k] != 0.f) { xmin = fminf(xmin, v[k]); xmax = fmaxf(xmax, v[k]); }
        if (v[k + 1] != 0.f) { ymin = fminf(ymin, v[k + 1]); ymax = fmaxf(ymax, v[k + 1]); }
    }
    if (xmin > xmax || ymin > ymax) {
        // all joints missing, or no non-zero x (y): box (0, 0, 0, 0), zero width and height -> the frame is all zeros
        for (int k = 0; k < 34; ++k) v[k] = 0.f;
    } else {
        const float ew = 0.1f * ((xmax - xmin) + 1.f), eh = 0.1f * ((ymax - ymin) + 1.f);
        const float wm1 = vid_w - 1.f, hm1 = vid_h - 1.f;
        const int L = (int)rintf(fminf(fmaxf(xmin - ew, 0.f), wm1)), R = (int)rintf(fminf(fmaxf(xmax + ew, 0.f), wm1));
        const int T = (int)rintf(fminf(fmaxf(ymin - eh, 0.f), hm1)), B = (int)rintf(fminf(fmaxf(ymax + eh, 0.f), hm1));
        const double cx = 0.5 * (double)(L + R), cy = 0.5 * (double)(T + B);
        const double w = (double)(R - L), h = (double)(B - T);
        for (int k = 0; k < 34; k += 2) {
            // missing joints (0) take the centre, which the subtraction then removes
            const float dx = (float)((double)(v[k] == 0.f ? (float)cx : v[k]) - cx);
            const float dy = (float)((double)(v[k + 1] == 0.f ? (float)cy : v[k + 1]) - cy);
            v[k] = w != 0.0 ? (float)((double)dx / w) : 0.f;
            v[k + 1] = h != 0.0 ? (float)((double)dy / h) : 0.f;
        }
    }
    for (int k = 0; k < 34; ++k) {
        float t = v[k];
        if (center) {
            // exact zeros are NaN (missing) for the scaler and come back as 0, as does any other NaN of the transform
            if (t == 0.f) t = 0.f;
            else {
                t = (float)((double)t - center[k]);
                t = (float)((double)t / scale[k]);
                if (t != t) t = 0.f;
            }
        }
        o[(k & 1) * 17 + (k >> 1)] = t;
        if (o2) o2[(k & 1) * 17 + (k >> 1)] = t;
    }
}

__global__ __launch_bounds__(256) void normalize_poses_kernel(const float* __restrict__ raw, long long n, float vid_w, float vid_h,
                                                              const double* __restrict__ center, const double* __restrict__ scale,
                                                              float* __restrict__ out) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    normalize_pose_row(raw + f * 34, vid_w, vid_h, center, scale, out + f * 34, nullptr);
}

// The inverse of normalize_pose_row (mcd_denormalize_poses): a normalised row p (34, interleaved) back to image pixels in the
// bounding box of the observed row r.  The box L, R, T, B is normalize_pose_row's, restated operation for operation (fp32 margin,
// clip, round-half-even) rather than shared, so that the forward kernels' code stays what it was; per element, in float64 and
// unfused, rounded to fp32 once: ((p * scale_k + center_k) * s + c), s = w | h, c = cx | cy.  A side of the box that is
// degenerate (s = 0, where the forward kernel writes zeros; also the box of a row without joints) gives c.
__device__ __forceinline__ void denormalize_pose_row(const float* __restrict__ p, const float* __restrict__ r, float vid_w, float vid_h,
                                                     const double* __restrict__ center, const double* __restrict__ scale,
                                                     float* __restrict__ o) {
#pragma clang fp contract(off)
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int k = 0; k < 34; k += 2) {
        const float x = r[k], y = r[k + 1];
        if (x != 0.f) { xmin = fminf(xmin, x); xmax = fmaxf(xmax, x); }
        if (y != 0.f) { ymin = fminf(ymin, y); ymax = fmaxf(ymax, y); }
    }
    double cx = 0.0, cy = 0.0, w = 0.0, h = 0.0;
    if (!(xmin > xmax || ymin > ymax)) {
        const float ew = 0.1f * ((xmax - xmin) + 1.f), eh = 0.1f * ((ymax - ymin) + 1.f);
        const float wm1 = vid_w - 1.f, hm1 = vid_h - 1.f;
        const int L = (int)rintf(fminf(fmaxf(xmin - ew, 0.f), wm1)), R = (int)rintf(fminf(fmaxf(xmax + ew, 0.f), wm1));
        const int T = (int)rintf(fminf(fmaxf(ymin - eh, 0.f), hm1)), B = (int)rintf(fminf(fmaxf(ymax + eh, 0.f), hm1));
        cx = 0.5 * (double)(L + R); cy = 0.5 * (double)(T + B);
        w = (double)(R - L); h = (double)(B - T);
    }
    for (int k = 0; k < 34; ++k) {
        const double s = (k & 1) ? h : w, c = (k & 1) ? cy : cx;
        double t = (double)p[k];
        if (center) {
            t = t * scale[k];
            t = t + center[k];
        }
        t = t * s;
        o[k] = s != 0.0 ? (float)(t + c) : (float)c;
    }
}

// one thread per row, like normalize_poses_kernel; count != nullptr: a row with count 0 is all zeros (the CSV's "missing")
__global__ __launch_bounds__(256) void denormalize_poses_kernel(const float* __restrict__ norm, const float* __restrict__ raw,
                                                                const int* __restrict__ count, long long n, float vid_w, float vid_h,
                                                                const double* __restrict__ center, const double* __restrict__ scale,
                                                                float* __restrict__ out) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    if (count && count[f] == 0) {
        for (int k = 0; k < 34; ++k) out[f * 34 + k] = 0.f;
        return;
    }
    denormalize_pose_row(norm + f * 34, raw + f * 34, vid_w, vid_h, center, scale, out + f * 34);
}

// ------------------------------------------------------------------------------------------------
// Forecast tracks (mcd_forecast_assemble): the overlapping window forecasts of a (person, frame) cell collapsed into one pose
// (utils/eval_utils.py:13-24 compute_fig_matrix + :37-72 extract_single_pose), in two launches on a caller-owned list workspace.
//   forecast_claim_kernel : one thread per (window, forecast frame) PAIR; a pair whose cell is in range claims a slot of the
//                           cell's list with an atomic on the cell's count and stores its pair index there.  Which slot a pair
//                           gets depends on arrival order; nothing else does:
//   forecast_reduce_kernel: one 64-lane wave per cell orders the claimed pair indices (ascending pair index = ascending window
//                           index, and within a window ascending forecast frame) by rank counting, stages the k x 34 values in
//                           LDS in that order, and lanes 0 .. 33 take one feature each -- float64, unfused, in list order.
// Everything a lane indexes at run time lives in LDS: no per-thread array.
// ------------------------------------------------------------------------------------------------
struct ForecastParams {
    const float* poses; const int* cell;      // (N, 2, Tx, 17), (N, Tx)
    int* list;                                // workspace (n_cells, max_cover) pair indices
    float* pose_out; int* count_out; float* spread_out;
    int n_pairs, Tx, n_cells, method, spread_method, max_cover;
};

__global__ __launch_bounds__(256) void forecast_claim_kernel(const ForecastParams F) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= F.n_pairs) return;
    const int c = F.cell[u];
    if (c < 0 || c >= F.n_cells) return;
    const int slot = atomicAdd(F.count_out + c, 1);
    if (slot < F.max_cover) F.list[(size_t)c * F.max_cover + slot] = (int)u;
}

// the middle of the k values x[0], x[stride], ... (np.median: for even k the half-sum of the two middle values), by rank
// counting as wave_select does: rank of j = #{m : x_m < x_j or (x_m == x_j and m < j)}; a NaN among them gives NaN
__device__ __forceinline__ double forecast_median(const float* x, int stride, int k) {
    const int r0 = (k - 1) / 2, r1 = k / 2;
    double lo = 0.0, hi = 0.0;
    bool nan = false;
    for (int j = 0; j < k; ++j) {
        const float xj = x[j * stride];
        nan |= xj != xj;
        int r = 0;
        for (int m = 0; m < k; ++m) {
            const float xm = x[m * stride];
            r += (xm < xj || (xm == xj && m < j)) ? 1 : 0;
        }
        if (r == r0) lo = (double)xj;
        if (r == r1) hi = (double)xj;
    }
    return nan ? (double)NAN : (lo + hi) / 2.0;
}

// The reduction of ONE cell, shared by forecast_reduce_kernel and the stream's forecast rows (forecast_emit_row): the k x 34 values
// staged in LDS in list order (vals[j * 34 + f]) -> lanes 0 .. 33 store their feature's pose to po[lane], the spread goes to *so.
// sd (34 doubles) and mid (2 doubles) are LDS.  Called by all 64 lanes of the one-wave workgroup, behind the barrier that makes
// `vals` visible; 1 <= k <= MCD_MAX_FRAMES.
__device__ __forceinline__ void forecast_reduce_staged(const float* vals, int k, int method, int spread_method, int lane, double* sd,
                                                       double* mid, float* po, float* so) {
#pragma clang fp contract(off)      // sum((x - mean)^2) is a product, then a sum: never an FMA
    if (lane < 34) {
        const float* x = vals + lane;
        double sum = 0.0;
        for (int j = 0; j < k; ++j) sum += (double)x[j * 34];
        const double mean = sum / (double)k;
        double ss = 0.0;
        for (int j = 0; j < k; ++j) {
            const double d = (double)x[j * 34] - mean;
            ss += d * d;
        }
        sd[lane] = sqrt(ss / (double)k);
        po[lane] = (float)(method == MCD_FORECAST_UNIQUE ? (double)x[0] : method == MCD_FORECAST_MEAN ? mean : forecast_median(x, 34, k));
    }
    __syncthreads();
    if (spread_method == MCD_FORECAST_MEAN) {
        if (lane == 0) {
            double s = 0.0;
            for (int f = 0; f < 34; ++f) s += sd[f];
            *so = (float)(s / 34.0);
        }
    } else {
        // the half-sum of ranks 16 and 17 of the 34 values, by rank counting again; a NaN among them gives NaN
        bool nan = false;
        if (lane < 34) {
            const double mine = sd[lane];
            nan = mine != mine;
            int r = 0;
            for (int m = 0; m < 34; ++m) r += (sd[m] < mine || (sd[m] == mine && m < lane)) ? 1 : 0;
            if (r == 16) mid[0] = mine;
            if (r == 17) mid[1] = mine;
        }
        const bool any_nan = __ballot(nan) != 0ull;
        __syncthreads();
        if (lane == 0) *so = any_nan ? __builtin_nanf("") : (float)((mid[0] + mid[1]) / 2.0);
    }
}

__global__ __launch_bounds__(64) void forecast_reduce_kernel(const ForecastParams F) {
    __shared__ int claimed[MCD_MAX_FRAMES], ordered[MCD_MAX_FRAMES];
    __shared__ float vals[MCD_MAX_FRAMES * 34];
    __shared__ double sd[34], mid[2];         // per-feature standard deviations; their two middle values
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < F.n_cells; c += gridDim.x) {
        const int k = F.count_out[c];
        float* po = F.pose_out + (size_t)c * 34;
        if (k <= 0 || k > F.max_cover) {      // no forecast: zeros; more pairs than the list holds: NaN (count_out says how many)
            const float v = k <= 0 ? 0.f : __builtin_nanf("");
            if (lane < 34) po[lane] = v;
            if (lane == 0) F.spread_out[c] = v;
            continue;
        }
        __syncthreads();                       // the previous cell's readers are done with the LDS
        if (lane < k) claimed[lane] = F.list[(size_t)c * F.max_cover + lane];
        __syncthreads();
        if (lane < k) {                        // pair indices are distinct: the ranks are a permutation of 0 .. k-1
            const int mine = claimed[lane];
            int r = 0;
            for (int m = 0; m < k; ++m) r += claimed[m] < mine ? 1 : 0;
            ordered[r] = mine;
        }
        __syncthreads();
        for (int e = lane; e < k * 34; e += 64) {
            const int j = e / 34, f = e - j * 34, pair = ordered[j], i = pair / F.Tx, tx = pair - i * F.Tx;
            vals[e] = F.poses[(((size_t)i * 2 + (f & 1)) * F.Tx + tx) * 17 + (f >> 1)];
        }
        __syncthreads();
        forecast_reduce_staged(vals, k, F.method, F.spread_method, lane, sd, mid, po, F.spread_out + c);
    }
}

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

// one thread per (closed track i, pending row k, transform t, lane v of the row): the seg_len - 1 cells of rows r_last - seg_len + 2
// .. r_last of a ring (n_slots, nt, L, W) -- W = 1: the score ring (mcd_stream_flush), W = 17: the joint ring (mcd_stream_joint_flush)
template <int W>
__global__ __launch_bounds__(256) void stream_flush_kernel(StreamParams S, const float* __restrict__ cells, const int* __restrict__ win,
                                                           int n, float* __restrict__ out) {
    const int pend = S.seg_len - 1;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n * pend * S.nt * W) return;
    const int v = u % W, t = (u / W) % S.nt, k = (u / (W * S.nt)) % pend, i = u / (W * S.nt * pend);
    const int slot = win[2 * i], r_last = win[2 * i + 1];
    if (slot < 0 || slot >= S.n_slots || r_last < S.seg_len - 1) return;
    out[u] = cells[(((size_t)slot * S.nt + t) * S.L + (r_last - S.seg_len + 2 + k) % S.L) * W + v];
}

// A GROUP of ticks in one launch (PoseStream.push / push_many): a track may receive R <= L - seg_len + 1 rows, so the rows
// r0 - seg_len + 1 .. r0 + R - 1 of a track -- the pending ones and the new ones -- sit at distinct ring positions, and no two
// rows of the launch share a pose position or a frame-score cell.  The group's windows are tick-major, inside a tick
// transform-major: the window of transform t of a row is at batch position pos0 + t * ne, with ne = its tick's window count
// (a single tick with n_emit windows: pos0 = the row's emit index j, ne = n_emit, the dataset's transform-major order).
// one thread per pushed row: desc (n, 4) = [slot, row index r, pos0 | -1, ne]; n_win = windows x transforms of the group.
// Per row: the normalised pose to both ring positions, the row's frame-score cell zeroed for every transform, and for pos0 >= 0
// the descriptors of the window ENDING at row r for every transform.
__global__ __launch_bounds__(256) void stream_push_group_kernel(StreamParams S, const float* __restrict__ raw,
                                                                const int* __restrict__ desc, int n, int n_win, float vid_w,
                                                                float vid_h, const double* __restrict__ center,
                                                                const double* __restrict__ scale, long long* __restrict__ base_out,
                                                                int* __restrict__ trans_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = desc[4 * i], r = desc[4 * i + 1], pos0 = desc[4 * i + 2], ne = desc[4 * i + 3];
    if (slot < 0 || slot >= S.n_slots || r < 0) return;        // (a descriptor the host table cannot produce: touch nothing)
    const int p = r % S.L;
    float* o = S.ring + ((size_t)slot * 2 * S.L + p) * 34;
    normalize_pose_row(raw + (size_t)i * 34, vid_w, vid_h, center, scale, o, o + (size_t)S.L * 34);
    for (int t = 0; t < S.nt; ++t) S.fs[((size_t)slot * S.nt + t) * S.L + p] = 0.f;
    if (pos0 < 0 || ne < 1 || r < S.seg_len - 1 || (long long)pos0 + (long long)(S.nt - 1) * ne >= n_win) return;
    const long long base = ((long long)slot * 2 * S.L + (r - S.seg_len + 1) % S.L) * 34;
    for (int t = 0; t < S.nt; ++t) {
        base_out[(size_t)pos0 + (size_t)t * ne] = base;
        trans_out[(size_t)pos0 + (size_t)t * ne] = t;
    }
}

// win (n, 5) = [slot, r_last, pos0, ne, w] per window, sorted by slot and, within a slot, by row; w = the window's index in
// (tick, j) order = its row of final_out (n, num_transform).  The windows of one track overlap, so one thread per (track,
// transform) -- the thread of the track's FIRST window -- applies them in row order with plain loads and stores: per window
// max(score, 0), the clamp and zero start of scatter_max_kernel, goes into the cells of its rows r_last - seg_len + 1 .. r_last,
// so the cells end as after one launch per tick, and each window's oldest row, which no later window covers, is final once
// that window is in.
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
        const int r_last = win[5 * q + 1], pos0 = win[5 * q + 2], ne = win[5 * q + 3], w = win[5 * q + 4];
        const long long pos = (long long)pos0 + (long long)t * ne;
        if (r_last < S.seg_len - 1 || pos0 < 0 || ne < 1 || pos >= n_win || w < 0 || w >= n) continue;
        body(slot, r_last, pos, w);
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
    if ((int)blockIdx.x >= n_windows) {     // the raw rows: desc (n, 4) = [slot, row index r, ...] as stream_push_group_kernel reads it
        const long long u = (long long)((int)blockIdx.x - n_windows) * 64 + lane;
        if (u >= (long long)n * 34) return;
        const int i = (int)(u / 34), f = (int)(u - (long long)i * 34);
        const int slot = desc[4 * i], r = desc[4 * i + 1];
        if (slot < 0 || slot >= S.n_slots || r < 0) return;
        F.obs[((size_t)slot * S.L + r % S.L) * 34 + f] = raw[u];
        return;
    }
    const int q = blockIdx.x;               // win (n_windows, 5) = [slot, r_last, pos0, ne, w]: the window's transform-0 position is pos0
    const int slot = win[5 * q], r_last = win[5 * q + 1], pos0 = win[5 * q + 2], ne = win[5 * q + 3], w = win[5 * q + 4];
    if (slot < 0 || slot >= S.n_slots || r_last < S.seg_len - 1 || pos0 < 0 || ne < 1 || pos0 >= n_win || w < 0 || w >= n_windows) return;
    const SampleVals X = stage_samples(F.loss_all + (size_t)pos0 * F.S, 1, F.S, sfc_lds + SEL_LDS_WORDS, F.in_lds != 0, lane);
    const Selection sel = wave_select(X, F.S, lane, F.strategy, 0.f, sfc_lds);
    const float* p = F.poses_all + ((size_t)pos0 * F.S + (sel.i0 >= 0 ? sel.i0 : 0)) * 34 * F.Tx;
    const int first = r_last - S.seg_len + 1;
    for (int j = 0; j < F.Tx; ++j) {        // (j is wave-uniform: corrupt_idx is read from the kernel arguments)
        const int r = first + F.cidx[j];
        if (lane < 34)
            F.fc[(((size_t)slot * S.L + r % S.L) * F.Tx + j) * 34 + lane] = sel.i0 >= 0 ? p[((lane & 1) * F.Tx + j) * 17 + (lane >> 1)] : 0.f;
    }
}

// Row r of `slot`, seen with r_hi the track's last row so far, into row o of the five outputs.  vals [MCD_MAX_FRAMES * 34], pn [34],
// sd [34], mid [2]: LDS.  One wave; every lane takes the same branches.
__device__ __forceinline__ void forecast_emit_row(const StreamParams& S, const StreamForecastParams& F, int slot, int r, int r_hi, size_t o,
                                                  int lane, float* vals, float* pn, double* sd, double* mid) {
    int ja = 0, jb = 0;
    for (int j = 0; j < F.Tx; ++j) {
        const int c = F.cidx[j];
        ja += c <= r ? 1 : 0;
        jb += r + S.seg_len - 1 - c > r_hi ? 1 : 0;
    }
    const int k = ja > jb ? ja - jb : 0;
    const size_t row = (size_t)slot * S.L + r % S.L;
    const float* cell = F.fc + row * F.Tx * 34;
    for (int e = lane; e < k * 34; e += 64) {      // window order: the m-th window of the row holds it as corrupt frame ja - 1 - m
        const int m = e / 34, f = e - m * 34;
        vals[e] = cell[(ja - 1 - m) * 34 + f];
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
    const int slot = win[5 * q], r_last = win[5 * q + 1], pos0 = win[5 * q + 2], ne = win[5 * q + 3], w = win[5 * q + 4];
    if (slot < 0 || slot >= S.n_slots || r_last < S.seg_len - 1 || pos0 < 0 || ne < 1 || pos0 >= n_win || w < 0 || w >= n_windows) return;
    forecast_emit_row(S, F, slot, r_last - S.seg_len + 1, r_last, (size_t)w, threadIdx.x, vals, pn, sd, mid);
}

// one wave per (closed track i, pending row k): win (n, 2) = [slot, r_last]; rows r_last - seg_len + 2 .. r_last see only the
// windows that exist
__global__ __launch_bounds__(64) void stream_forecast_flush_kernel(StreamParams S, StreamForecastParams F, const int* __restrict__ win, int n) {
    __shared__ float vals[MCD_MAX_FRAMES * 34], pn[34];
    __shared__ double sd[34], mid[2];
    const int pend = S.seg_len - 1, u = blockIdx.x;
    if (u >= n * pend) return;
    const int i = u / pend, k = u - i * pend;
    const int slot = win[2 * i], r_last = win[2 * i + 1];
    if (slot < 0 || slot >= S.n_slots || r_last < S.seg_len - 1) return;
    forecast_emit_row(S, F, slot, r_last - S.seg_len + 2 + k, r_last, (size_t)u, threadIdx.x, vals, pn, sd, mid);
}

// ------------------------------------------------------------------------------------------------
// Frame-score assembly after the path (mocodad.py:362-425; eval_utils.py:27-34,100-106,133-149), on device, in float64
// like the reference's NumPy code.
//   frame_scatter_kernel: window score -> max over the windows covering each frame of its (transform, clip, person) row.
//   frame_scores_kernel : one workgroup per clip; for every transform: per person pad_scores, then
//                         mean_p + (max_p - min_p) of log1p over the persons present, HR-mask compaction, shift,
//                         gaussian_filter1d (scipy defaults: truncate 4 sigma, 'reflect'), accumulated over the transforms
//                         and divided by their number.
// Rows are dense: row = (transform * n_clips + clip) * P + person id; `used[row]` marks persons that have windows.
// ------------------------------------------------------------------------------------------------
struct FrameParams {
    const float* scores; const long long* trans; const long long* meta; const int* frames;
    const long long* clip_keys;     // (n_clips,) sorted (scene << 32 | clip)
    const int* clip_n;              // (n_clips,) frames of the clip = len(gt)
    const int* dst;                 // per clip F entries: position of the frame after the HR masks, -1 = dropped
    const int* out_len;             // (n_clips,) frames kept
    const long long* out_off;       // (n_clips,) offset of the clip in the concatenated output
    const double* gauss;            // (2 radius + 1,) normalised weights
    float* mat; int* used; double* out;
    long long n;
    int seg_len, n_clips, num_transform, P, F, pad, shift, radius;
};

// The pieces frame_scores_kernel shares with the online clip kernels (stream_clip_update / stream_clip_emit below): one
// definition each, so the operations, their order and the FMA contraction are the same in both and the online scores of a clip
// whose persons are all present on every frame carry the bits of the dataset path.
//   person_aggr_add / person_aggr_value: mean_p s + (max_p log1p s - min_p log1p s) over the persons added (mocodad.py:399-401)
//   reflect_index: position k of scipy's 'reflect' extension (d c b a | a b c d | d c b a) of a sequence of m entries, any k
//   gauss_taps: correlation with the symmetric weights g[0 .. 2 radius]: the centre tap, then the pairs from the outermost inwards
__device__ __forceinline__ void person_aggr_add(double& sum, double& lmax, double& lmin, int& cnt, float v) {
    const double dv = (double)v, lg = log1p(dv);
    sum += dv;
    if (cnt == 0) { lmax = lg; lmin = lg; } else { lmax = fmax(lmax, lg); lmin = fmin(lmin, lg); }
    ++cnt;
}
__device__ __forceinline__ double person_aggr_value(double sum, double lmax, double lmin, int cnt) {
    return sum / (double)cnt + (lmax - lmin);
}
__device__ __forceinline__ int reflect_index(int k, int m) {
    const int per = 2 * m;
    k %= per; if (k < 0) k += per;
    if (k >= m) k = per - 1 - k;
    return k;
}
template <class At>
__device__ __forceinline__ double gauss_taps(const At& at, int j, const double* __restrict__ g, int radius) {
    double t = at(j) * g[radius];
    for (int i = radius; i >= 1; --i) t += (at(j - i) + at(j + i)) * g[radius - i];
    return t;
}

__global__ void frame_scatter_kernel(const FrameParams Q) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= Q.n * Q.seg_len) return;
    const long long i = u / Q.seg_len;
    const long long tr = Q.trans[i];
    if (tr < 0 || tr >= Q.num_transform) return;
    const long long key = (Q.meta[i * 4 + 0] << 32) | (Q.meta[i * 4 + 1] & 0xffffffffll);
    int lo = 0, hi = Q.n_clips;                     // lower bound in the sorted clip keys
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (Q.clip_keys[mid] < key) lo = mid + 1; else hi = mid; }
    if (lo >= Q.n_clips || Q.clip_keys[lo] != key) return;        // a clip without a ground-truth file is not evaluated
    const long long person = Q.meta[i * 4 + 2];
    if (person < 0 || person >= Q.P) return;
    const int f = Q.frames[u] - 1;
    if (f < 0 || f >= Q.clip_n[lo]) return;
    const long long row = ((long long)tr * Q.n_clips + lo) * Q.P + person;
    Q.used[row] = 1;
    atomic_max_nonneg(Q.mat + row * Q.F + f, Q.scores[i]);      // np.nanmax over the windows covering the frame; 0 = absent
}

__global__ __launch_bounds__(256) void frame_scores_kernel(const FrameParams Q) {
    extern __shared__ __attribute__((aligned(16))) double fsm[];
    const int ci = blockIdx.x, n = Q.clip_n[ci], m = Q.out_len[ci];
    double* cs = fsm;                 // [m] compacted clip score of the current transform
    double* acc = fsm + Q.F;          // [m] sum over the transforms
    const int* dst = Q.dst + (size_t)ci * Q.F;
    for (int j = threadIdx.x; j < m; j += blockDim.x) acc[j] = 0.0;
    for (int tr = 0; tr < Q.num_transform; ++tr) {
        const size_t row0 = ((size_t)tr * Q.n_clips + ci) * Q.P;
        __syncthreads();
        for (int f = threadIdx.x; f < n; f += blockDim.x) {
            double sum = 0.0, lmax = 0.0, lmin = 0.0;
            int cnt = 0;
            for (int p = 0; p < Q.P; ++p) {
                if (!Q.used[row0 + p]) continue;
                const float* r = Q.mat + (row0 + p) * Q.F;
                float v = r[f];
                if (Q.pad >= 0 && v != 0.f) {
                    // pad_scores (eval_utils.py:133-149): zero `pad` frames before and pad-1 frames after every interval of
                    // absence inside frames [0, n-2]; an interval touching frame 0 / frame n-2 is not extended on that side
                    bool z = false;
                    for (int d = 1; d <= Q.pad && !z; ++d) z = (f + d <= n - 2) && r[f + d] == 0.f;
                    if (!z) {
                        // backwards: for the last frame, the run of absence that ends at frame n-2 does not count
                        bool in_tail = (f == n - 1);
                        for (int d = 1; d <= Q.pad - 1 && f - d >= 0 && !z; ++d) {
                            const bool zero = r[f - d] == 0.f;
                            if (in_tail) { if (!zero) in_tail = false; }
                            else z = zero;
                        }
                    }
                    if (z) v = 0.f;
                }
                person_aggr_add(sum, lmax, lmin, cnt, v);
            }
            const int j = dst[f];
            // a (transform, clip) block without any person: NaN (the reference fails on np.stack of an empty list; the host
            // wrapper turns the NaN into that error)
            if (j >= 0) cs[j] = cnt > 0 ? person_aggr_value(sum, lmax, lmin, cnt) : (double)NAN;
        }
        __syncthreads();
        // score_process (eval_utils.py:100-106): shift by `shift` frames (zeros enter), then correlate with the Gaussian
        // in scipy's symmetric form: in[c] w[c] + sum_{i=1..radius} (in[c-i] + in[c+i]) w[c-i], outermost pair first
        for (int j = threadIdx.x; j < m; j += blockDim.x) {
            auto at = [&](int k) -> double {          // shifted, 'reflect'-extended
                k = reflect_index(k, m);
                return k >= Q.shift ? cs[k - Q.shift] : 0.0;
            };
            acc[j] += gauss_taps(at, j, Q.gauss, Q.radius);
        }
    }
    __syncthreads();
    double* o = Q.out + Q.out_off[ci];
    for (int j = threadIdx.x; j < m; j += blockDim.x) o[j] = acc[j] / (double)Q.num_transform;
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

// test aid (mcd_debug_poison_lds): every CU's LDS filled with signalling garbage (NaN bit patterns), so that a kernel reading
// shared memory it never wrote produces NaNs instead of depending on what the previous kernel happened to leave there
__global__ __launch_bounds__(API_THREADS) void poison_lds_kernel(unsigned* sink, int words) {
    extern __shared__ unsigned psm[];
    for (int u = threadIdx.x; u < words; u += API_THREADS) psm[u] = 0x7fc00000u | (unsigned)u;
    __syncthreads();
    if (threadIdx.x == 0 && sink) atomicOr(sink, psm[(blockIdx.x * 7919) % words] & 1u);      // (keeps the stores alive)
    __builtin_amdgcn_s_sleep(64);
}

// the kernels the exported entry points launch by name: C linkage, default visibility
#pragma GCC visibility push(default)
extern "C" {

__global__ void philox_noise_kernel(unsigned long long seed, long long first_window, int B, int S, int K, int Tx, float* __restrict__ out) {
    // one thread per (s, k, b, tx, joint pair): the Philox half of chain_xT / chain_step_noise4 (mcd_chain.hpp), so the export
    // is the kernels' draw by construction
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)S * K * B * Tx * 9;
    if (u >= total) return;
    const int jp = (int)(u % 9), tx = (int)((u / 9) % Tx);
    const int b = (int)((u / (9 * Tx)) % B), k = (int)((u / ((long long)9 * Tx * B)) % K), s = (int)(u / ((long long)9 * Tx * B * K));
    const int v0 = 2 * jp, CTV = C0 * Tx * 17;
    float* o = out + ((size_t)(s * K + k) * B + b) * CTV;
    float z[4];
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i & 1, v = v0 + (i >> 1);
            z[i] = v < 17 ? chain_xT_philox(seed, first_window, b, s, Tx, c, tx, v) : 0.f;
        }
    } else {
        chain_step_philox4(seed, first_window, b, s, k, tx, v0, z);
    }
    o[tx * 17 + v0] = z[0];
    o[Tx * 17 + tx * 17 + v0] = z[1];
    if (v0 + 1 < 17) { o[tx * 17 + v0 + 1] = z[2]; o[Tx * 17 + tx * 17 + v0 + 1] = z[3]; }
}

// One thread per window: n_cond steps, each picking uniformly among the frames not chosen yet (word i % 4 of Philox call i / 4,
// multiply-high onto 0 .. seg_len-i-1, then the r-th clear bit), so the set is a uniform n_cond-subset of the seg_len frames.
// Counter (call, ~0, ~0, window id): the noise streams use c1 = slot < ns and c2 = sample < S, so no call coincides with theirs.
__global__ __launch_bounds__(256) void random_imp_masks_kernel(unsigned long long seed, long long first_window, int B, int T, int n_cond,
                                                               int* __restrict__ mask_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned all = low_bits(T), win = (unsigned)(first_window + b);
    unsigned chosen = 0u, w[4];
    for (int i = 0; i < n_cond; ++i) {
        if ((i & 3) == 0) philox_words4(seed, (unsigned)(i >> 2), 0xFFFFFFFFu, 0xFFFFFFFFu, win, w);
        const unsigned word = (i & 3) == 0 ? w[0] : (i & 3) == 1 ? w[1] : (i & 3) == 2 ? w[2] : w[3];      // (selects: w stays in registers)
        const int r = (int)(((unsigned long long)word * (unsigned)(T - i)) >> 32);
        chosen |= 1u << nth_set_bit(~chosen & all, r);
    }
    mask_out[b] = (int)chosen;
}

__global__ void gather_frames_kernel(const DataView dv, float* __restrict__ out, int B, int C, int T, int V, int n,
                                     const FrameIdx fi) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= B * C * n * V) return;
    const int v = u % V, k = (u / V) % n, c = (u / (V * n)) % C, b = u / (V * n * C);
    out[u] = load_coord(dv, b, c, fi.idx[k], v, T);
}

}  // extern "C"
#pragma GCC visibility pop

// mcd_post_kernel.hpp — the device code of mcd_api.hip's own launches, everything around the trajectory kernels:
//   aggregate_kernel            MoCoDAD._aggregation_strategy                                  models/mocodad.py:454-520
//   error_maps_kernel           the per-element loss of :484 before its mean, under the same sample selection (mcd_error_maps)
//                               -- both on ONE statement of that selection: SelectParams, corrupt_frame, wave_select, wave_pose_stat
//   scatter_max<W> / frame_scatter / frame_scores kernels   post_processing                    models/mocodad.py:362-425
//                               (W = 1: window scores, W = 17: per-joint maps; atomic_max_nonneg is the one scatter-max idiom)
//   normalize_poses_kernel      dataset loader: bbox-centre coordinates + RobustScaler      utils/data.py:11-43,165-186,350-359
//   denormalize_poses_kernel    its inverse, back to image pixels in the observed row's bounding box (mcd_denormalize_poses)
//                               -- both in ONE statement of that box: pose_box
//   forecast_claim / forecast_reduce kernels   overlapping window forecasts -> one pose per (person, frame) cell + their spread
//                               (mcd_forecast_assemble)                                         utils/eval_utils.py:13-24,37-72
//   forecast_claim_view / forecast_reduce_view kernels   the same over the windows of EVERY test-time transform, each forecast
//                               mapped back by inverse_affine_coord (mcd_forecast_assemble_view)
//   forecast_fan_kernel         behind the same claim kernels: quantile bands, mean, deviation and observed mid-rank over ALL
//                               samples of the pairs covering a cell (mcd_forecast_fan)
//   philox_noise / random_imp_masks kernels   the perf mode's draws, exported (mcd_philox_noise, mcd_random_imp_masks)
//   gather_frames_kernel        the dense copy of the condition frames cond_encode_kernel reads
//   poison_lds_kernel           test aid (mcd_debug_poison_lds)
// with the parameter blocks the host fills (SelectParams inside AggrParams and MapParams, ForecastParams, FrameParams).  Included
// once, by mcd_api.hip (which defines API_THREADS and says `using namespace mcd`), in front of its host code.  The kernels of a live
// stream are mcd_stream_kernel.hpp, included behind this file: they share normalize_pose_row / denormalize_pose_row, wave_select,
// forecast_reduce_staged, inverse_affine_coord and the pieces of frame_scores_kernel (person_aggr_*, reflect_index, gauss_taps) defined here.
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
// pose_box: the bounding box of one row v (34 values, a zero = a missing coordinate), for the forward and the inverse kernel alike:
// centre and size in double, from the integer box L, R, T, B.  empty: all joints missing, or no non-zero x (y) -- box (0, 0, 0, 0).
struct PoseBox { double cx, cy, w, h; bool empty; };
__device__ __forceinline__ PoseBox pose_box(const float* v, float vid_w, float vid_h) {
#pragma clang fp contract(off)      // the margin is 0.1 * (r - l + 1), then l - margin: two roundings, never an FMA
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int k = 0; k < 34; k += 2) {
        if (v[k] != 0.f) { xmin = fminf(xmin, v[k]); xmax = fmaxf(xmax, v[k]); }
        if (v[k + 1] != 0.f) { ymin = fminf(ymin, v[k + 1]); ymax = fmaxf(ymax, v[k + 1]); }
    }
    if (xmin > xmax || ymin > ymax) return PoseBox{0.0, 0.0, 0.0, 0.0, true};
    const float ew = 0.1f * ((xmax - xmin) + 1.f), eh = 0.1f * ((ymax - ymin) + 1.f);
    const float wm1 = vid_w - 1.f, hm1 = vid_h - 1.f;
    const int L = (int)rintf(fminf(fmaxf(xmin - ew, 0.f), wm1)), R = (int)rintf(fminf(fmaxf(xmax + ew, 0.f), wm1));
    const int T = (int)rintf(fminf(fmaxf(ymin - eh, 0.f), hm1)), B = (int)rintf(fminf(fmaxf(ymax + eh, 0.f), hm1));
    return PoseBox{0.5 * (double)(L + R), 0.5 * (double)(T + B), (double)(R - L), (double)(B - T), false};
}
// normalize_pose_row: one row, written to `o` and, when o2 != nullptr, to `o2` as well (the mirrored copy of a track ring).
__device__ __forceinline__ void normalize_pose_row(const float* __restrict__ r, float vid_w, float vid_h,
                                                   const double* __restrict__ center, const double* __restrict__ scale,
                                                   float* __restrict__ o, float* __restrict__ o2) {
#pragma clang fp contract(off)
    float v[34];
    for (int k = 0; k < 34; ++k) v[k] = r[k];
    const PoseBox box = pose_box(v, vid_w, vid_h);
    if (box.empty) {
        // zero width and height -> the frame is all zeros
        for (int k = 0; k < 34; ++k) v[k] = 0.f;
    } else {
        const double cx = box.cx, cy = box.cy, w = box.w, h = box.h;
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
// bounding box of the observed row r (pose_box, the forward kernel's); per element, in float64 and
// unfused, rounded to fp32 once: ((p * scale_k + center_k) * s + c), s = w | h, c = cx | cy.  A side of the box that is
// degenerate (s = 0, where the forward kernel writes zeros; also the box of a row without joints) gives c.
__device__ __forceinline__ void denormalize_pose_row(const float* __restrict__ p, const float* __restrict__ r, float vid_w, float vid_h,
                                                     const double* __restrict__ center, const double* __restrict__ scale,
                                                     float* __restrict__ o) {
#pragma clang fp contract(off)
    const PoseBox box = pose_box(r, vid_w, vid_h);
    for (int k = 0; k < 34; ++k) {
        const double s = (k & 1) ? box.h : box.w, c = (k & 1) ? box.cy : box.cx;
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

// Forecasts from every test-time transform (mcd_forecast_assemble_view; the stream's store kernel): coordinate c (0 = x, 1 = y) of
// the joint (xp, yp) forecast under a transform, mapped back by the row m = [i00 i01 i02 i10 i11 i12] of the inverse table:
// (i_c0 xp + i_c1 yp) + i_c2 in float64, unfused, rounded to fp32 once.  A row equal to (1,0,0,0,1,0) copies the value: a -0.0
// keeps its sign and a NaN in the other coordinate stays where it is, so the identity's pairs carry the bits they carry without a map.
constexpr int FORECAST_VIEW_COVER = MCD_FORECAST_VIEW_COVER;      // pairs on a cell with all transforms
__device__ __forceinline__ float inverse_affine_coord(const double* __restrict__ m, float xp, float yp, int c) {
#pragma clang fp contract(off)
    if (m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[3] == 0.0 && m[4] == 1.0 && m[5] == 0.0) return c ? yp : xp;
    const double px = m[3 * c] * (double)xp, py = m[3 * c + 1] * (double)yp;
    return (float)((px + py) + m[3 * c + 2]);
}
struct ForecastViewParams {
    ForecastParams f;
    const int* trans; const double* inv;      // (N,), (n_transform, 6)
    int n_transform;
};
// forecast_claim_kernel with one more reason to ignore a pair: its window's transform is not in the table
__global__ __launch_bounds__(256) void forecast_claim_view_kernel(const ForecastViewParams V) {
    const ForecastParams& F = V.f;
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= F.n_pairs) return;
    const int c = F.cell[u], t = V.trans[u / F.Tx];
    if (c < 0 || c >= F.n_cells || t < 0 || t >= V.n_transform) return;
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
// `vals` visible; 1 <= k <= the rows `vals` holds (MCD_MAX_FRAMES, or FORECAST_VIEW_COVER with all transforms).
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

// The cells of a launch, for forecast_reduce_kernel (COVER = MCD_MAX_FRAMES, value = the pose element as it lies) and
// forecast_reduce_view_kernel (COVER = FORECAST_VIEW_COVER, value = it mapped back): value(window i, forecast frame tx, feature f).
template <int COVER, class Value>
__device__ __forceinline__ void forecast_reduce_cells(const ForecastParams& F, Value value) {
    __shared__ int claimed[COVER], ordered[COVER];
    __shared__ float vals[COVER * 34];
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
            vals[e] = value(i, tx, f);
        }
        __syncthreads();
        forecast_reduce_staged(vals, k, F.method, F.spread_method, lane, sd, mid, po, F.spread_out + c);
    }
}

__global__ __launch_bounds__(64) void forecast_reduce_kernel(const ForecastParams F) {
    forecast_reduce_cells<MCD_MAX_FRAMES>(F, [&](int i, int tx, int f) -> float {
        return F.poses[(((size_t)i * 2 + (f & 1)) * F.Tx + tx) * 17 + (f >> 1)];
    });
}

__global__ __launch_bounds__(64) void forecast_reduce_view_kernel(const ForecastViewParams V) {
    const ForecastParams& F = V.f;
    forecast_reduce_cells<FORECAST_VIEW_COVER>(F, [&](int i, int tx, int f) -> float {
        const float* p = F.poses + ((size_t)i * 2 * F.Tx + tx) * 17 + (f >> 1);      // a claimed pair's transform is in the table
        return inverse_affine_coord(V.inv + 6 * V.trans[i], p[0], p[(size_t)F.Tx * 17], f & 1);
    });
}

// ------------------------------------------------------------------------------------------------
// Forecast fan (mcd_forecast_fan): per cell and feature the distribution of ALL S samples of every covering pair -- quantile bands,
// mean, standard deviation and the mid-rank of the observed coordinate.  The pairs are claimed by forecast_claim_kernel /
// forecast_claim_view_kernel as they are; then one 256-lane workgroup per cell:
//   - the claimed pair indices are ordered by rank counting (k <= 64), as forecast_reduce_cells orders them;
//   - the 17 joints are walked in groups of `jg` (the launcher's choice: what 60 KB of LDS hold at the launch's largest list).  Per
//     group the K = k * S values of each feature are staged in list order (vals, row stride kp + 1 words: in the summing pass below
//     lane f walks row f, and the odd stride puts the lanes on banks of their own) beside one 64-bit key per value, (order-preserving
//     image of the value) << 32 | list position, padded to the cell's power of two with all-ones keys (keys, row stride kp: the
//     lanes of a sort stage take consecutive positions of a row, never one position of many rows, so this stride needs no pad);
//   - one lane per feature sums in list order (mean, two-pass deviation, NaN flag) -- float64, unfused.  At most 34 of the 256
//     lanes work in this pass, 2 K dependent additions each, while the others wait at the next barrier: the definition fixes the
//     order of the sum, not who computes it, and overlapping this pass with the sort is open;
//   - a bitonic network sorts each feature's keys: the keys are distinct, so ANY network gives the stable order (ties by position;
//     -0.0 and +0.0 share an image and a NaN feature's order is never read);
//   - one lane per (feature, level) interpolates between two sorted values, read from `vals` through the key's position (a -0.0
//     keeps its sign); one lane per feature finds the observed coordinate's rank by two lower bounds in the sorted keys.
// Everything a lane indexes at run time lives in LDS or global memory: no per-thread array, no scratch.
// ------------------------------------------------------------------------------------------------
constexpr int FORECAST_FAN_VALUES = MCD_FORECAST_FAN_VALUES;
constexpr int FORECAST_FAN_LEVELS = MCD_FORECAST_FAN_LEVELS;
constexpr int FORECAST_FAN_THREADS = 256;
constexpr int FORECAST_FAN_LDS = 60 * 1024;      // dynamic LDS of a launch, at most (with the static lists: inside 64 KB)
struct ForecastFanParams {
    ForecastViewParams v;                     // f.poses: (N, S, 2, Tx, 17); f.count_out: the claimed counts; v.trans == nullptr: no map
    const float* observed;                    // (n_cells, 2, 17) frame-major, or nullptr with rank_out
    float* quant_out; float* mean_out; float* std_out; float* rank_out;
    double levels[FORECAST_FAN_LEVELS];
    int n_samples, n_levels;
    int kp, jg;                               // row stride of the keys (a power of two >= every list the launch reduces); joints per group
};
// bytes of dynamic LDS for groups of jg joints at key stride kp: per feature kp keys and kp + 1 staged values
__host__ __device__ constexpr size_t forecast_fan_lds_bytes(int kp, int jg) {
    return (size_t)2 * jg * ((size_t)kp * sizeof(unsigned long long) + (size_t)(kp + 1) * sizeof(float));
}
// fp32 -> u32 whose unsigned order is the order of the values, -0.0 == +0.0; every non-NaN image is below 0xffffffff
__device__ __forceinline__ unsigned forecast_fan_image(float x) {
    const unsigned u = x == 0.f ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the first position of the ascending keys[0 .. n) that is not below `key`
__device__ __forceinline__ int forecast_fan_lower_bound(const unsigned long long* keys, int n, unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(FORECAST_FAN_THREADS) void forecast_fan_kernel(const ForecastFanParams Q) {
#pragma clang fp contract(off)      // (1 - g) x[i] + g x[i + 1] and sum((x - mean)^2): products, then sums -- never an FMA
    extern __shared__ unsigned long long fan_lds[];
    __shared__ int claimed[FORECAST_VIEW_COVER], ordered[FORECAST_VIEW_COVER];
    __shared__ int fnan[34];                  // per feature of the group: a NaN among its values
    const ForecastParams& F = Q.v.f;
    const int tid = threadIdx.x, S = Q.n_samples, kp = Q.kp, vstride = kp + 1, nl = Q.n_levels;
    unsigned long long* keys = fan_lds;                                            // [2 jg][kp]
    float* vals = reinterpret_cast<float*>(fan_lds + (size_t)2 * Q.jg * kp);      // [2 jg][kp + 1]
    for (int c = blockIdx.x; c < F.n_cells; c += gridDim.x) {
        const int k = F.count_out[c];
        const int K = k > 0 && k <= F.max_cover && (long long)k * S <= FORECAST_FAN_VALUES ? k * S : 0;
        if (K == 0) {                              // no forecast: zeros; more pairs or values than a list holds: NaN (count_out says how many)
            const float v = k <= 0 ? 0.f : __builtin_nanf("");
            if (tid < 34) {
                const size_t o = (size_t)c * 34 + tid;
                Q.mean_out[o] = v;
                Q.std_out[o] = v;
                if (Q.rank_out) Q.rank_out[o] = v;
                for (int l = 0; l < nl; ++l) Q.quant_out[(size_t)l * F.n_cells * 34 + o] = v;
            }
            continue;
        }
        int Kp = 1;
        while (Kp < K) Kp <<= 1;                   // <= kp
        const int half = Kp >> 1, lg_half = half ? __builtin_ctz(half) : 0;
        __syncthreads();                           // the previous cell's readers are done with the lists
        if (tid < k) claimed[tid] = F.list[(size_t)c * F.max_cover + tid];
        __syncthreads();
        if (tid < k) {                             // pair indices are distinct: the ranks are a permutation of 0 .. k-1
            const int mine = claimed[tid];
            int r = 0;
            for (int m = 0; m < k; ++m) r += claimed[m] < mine ? 1 : 0;
            ordered[r] = mine;
        }
        for (int j0 = 0; j0 < 17; j0 += Q.jg) {
            const int nj = 17 - j0 < Q.jg ? 17 - j0 : Q.jg, nf = 2 * nj;
            __syncthreads();                       // `ordered` is complete; the previous group's readers are done with keys / vals
            for (int e = tid; e < nj * K; e += FORECAST_FAN_THREADS) {      // stage: list position p of joint j0 + jj, x and y
                const int jj = e / K, p = e - jj * K, j = p / S, s = p - j * S, pair = ordered[j], i = pair / F.Tx, tx = pair - i * F.Tx;
                const float* ptr = F.poses + ((((size_t)i * S + s) * 2) * F.Tx + tx) * 17 + (j0 + jj);
                float x = ptr[0], y = ptr[(size_t)F.Tx * 17];
                if (Q.v.trans) {                   // a claimed pair's transform is in the table
                    const double* m = Q.v.inv + 6 * Q.v.trans[i];
                    const float xp = x, yp = y;
                    x = inverse_affine_coord(m, xp, yp, 0);
                    y = inverse_affine_coord(m, xp, yp, 1);
                }
                vals[(2 * jj) * vstride + p] = x;
                vals[(2 * jj + 1) * vstride + p] = y;
                keys[(size_t)(2 * jj) * kp + p] = ((unsigned long long)forecast_fan_image(x) << 32) | (unsigned)p;
                keys[(size_t)(2 * jj + 1) * kp + p] = ((unsigned long long)forecast_fan_image(y) << 32) | (unsigned)p;
            }
            for (int e = tid; e < nf * (Kp - K); e += FORECAST_FAN_THREADS) {      // the padding sorts behind every value
                const int f = e / (Kp - K), p = K + (e - f * (Kp - K));
                keys[(size_t)f * kp + p] = ~0ull;
            }
            __syncthreads();
            if (tid < nf) {                        // mean and deviation in list order (forecast_reduce_staged's definitions)
                const float* x = vals + tid * vstride;
                double sum = 0.0;
                bool nan = false;
                for (int p = 0; p < K; ++p) {
                    const float xv = x[p];
                    nan |= xv != xv;
                    sum += (double)xv;
                }
                const double mean = sum / (double)K;
                double ss = 0.0;
                for (int p = 0; p < K; ++p) {
                    const double d = (double)x[p] - mean;
                    ss += d * d;
                }
                const size_t o = (size_t)c * 34 + 2 * j0 + tid;
                Q.mean_out[o] = (float)mean;
                Q.std_out[o] = (float)sqrt(ss / (double)K);
                fnan[tid] = nan ? 1 : 0;
            }
            for (int size = 2; size <= Kp; size <<= 1)                             // bitonic network on every feature's Kp keys
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int e = tid; e < nf * half; e += FORECAST_FAN_THREADS) {
                        const int f = e >> lg_half, t = e & (half - 1), lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                        unsigned long long* row = keys + (size_t)f * kp;
                        const unsigned long long a = row[lo], b = row[hi];
                        if ((a > b) == ((lo & size) == 0)) { row[lo] = b; row[hi] = a; }
                    }
                    __syncthreads();
                }
            __syncthreads();                       // (K == 1: no stage ran; fnan is visible either way)
            for (int e = tid; e < nf * (nl + 1); e += FORECAST_FAN_THREADS) {
                const int f = e / (nl + 1), l = e - f * (nl + 1);
                const unsigned long long* row = keys + (size_t)f * kp;
                const float* x = vals + f * vstride;
                const size_t o = (size_t)c * 34 + 2 * j0 + f;
                if (l < nl) {                      // level l: h = q (K - 1), between the sorted values floor(h) and floor(h) + 1
                    double q = Q.levels[0];
#pragma unroll
                    for (int m = 1; m < FORECAST_FAN_LEVELS; ++m) q = l == m ? Q.levels[m] : q;      // (no lane-indexed kernel argument)
                    const double h = q * (double)(K - 1), fl = floor(h), g = h - fl;
                    const int i = (int)fl;
                    double v = (double)x[(unsigned)row[i]];
                    if (g != 0.0) {
                        const double a = (1.0 - g) * v, b = g * (double)x[(unsigned)row[i + 1]];
                        v = a + b;
                    }
                    Q.quant_out[(size_t)l * F.n_cells * 34 + o] = fnan[f] ? __builtin_nanf("") : (float)v;
                } else if (Q.rank_out) {           // (below + equal / 2) / K of the observed coordinate
                    const float obs = Q.observed[(size_t)c * 34 + (size_t)(f & 1) * 17 + j0 + (f >> 1)];
                    const unsigned long long img = (unsigned long long)forecast_fan_image(obs) << 32;
                    const int below = forecast_fan_lower_bound(row, K, img);
                    const int upto = forecast_fan_lower_bound(row, K, img + (1ull << 32));
                    const double r = ((double)below + (double)(upto - below) / 2.0) / (double)K;
                    Q.rank_out[o] = (fnan[f] || obs != obs) ? __builtin_nanf("") : (float)r;
                }
            }
        }
    }
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

// The pieces frame_scores_kernel shares with the online clip kernels (stream_clip_update / stream_clip_emit, mcd_stream_kernel.hpp): one
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

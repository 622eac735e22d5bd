// mcd_stream_api.hpp — host side of the live-stream entry points mcd_stream_* (include/mocodad_hip.h): the checks of a state and of
// a group, and the launches of mcd_stream_kernel.hpp.  Included by mcd_api.hip behind its own entry points, whose checks of
// mcd_call.hpp it shares.  Every check comes before the first device call, and the ORDER of an entry's checks is part of its
// behaviour (tests/golden/call_errors.json).  It holds no device code.
#pragma once

static int stream_params(const mcd_stream_state_t* s, StreamParams* P) {
    if (!s || !s->ring || !s->frame_scores) return fail(MCD_EINVAL, "null stream state");
    if (s->n_slots <= 0 || s->num_transform <= 0 || s->seg_len <= 0 || s->seg_len > MCD_MAX_FRAMES || s->ring_len < s->seg_len)
        return fail(MCD_EINVAL, "stream state: need n_slots, num_transform >= 1 and 1 <= seg_len <= ring_len (seg_len <= 32)");
    if ((int64_t)s->n_slots * 2 * s->ring_len > 0x7fffffffll / 34 || (int64_t)s->n_slots * s->num_transform * s->ring_len > 0x7fffffffll)
        return fail(MCD_EUNSUPPORTED, "stream rings of more than 2^31 elements");
    P->ring = s->ring; P->fs = s->frame_scores;
    P->n_slots = s->n_slots; P->L = s->ring_len; P->seg_len = s->seg_len; P->nt = s->num_transform;
    return MCD_OK;
}

// the pending cells of n closed tracks out of a ring (n_slots, nt, L, W): the score ring (W = 1) or the joint ring (W = 17)
template <int W>
static int stream_flush(const StreamParams& P, const float* cells, const int32_t* win, int32_t n, float* out, void* stream) {
    if (n < 0 || n > P.n_slots) return fail(MCD_EINVAL, "need 0 <= n <= n_slots");
    const long long total = (long long)n * (P.seg_len - 1) * P.nt * W;
    if (total == 0) return MCD_OK;
    if (!win || !out) return fail(MCD_EINVAL, "null argument");
    if (total > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many tracks for one launch");
    hipLaunchKernelGGL(stream_flush_kernel<W>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, cells, win, n, out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

// rows (windows) one group may hold: n_slots * (ring_len - seg_len + 1), the per-track bound times the tracks
static int64_t stream_group_rows(const mcd_stream_state_t* s) { return (int64_t)s->n_slots * (s->ring_len - s->seg_len + 1); }
// the rows a group pushes and the windows among them: 0 <= n_windows <= n <= stream_group_rows
static int check_group_rows(const mcd_stream_state_t* s, int32_t n, int32_t n_windows) {
    if (n < 0 || n_windows < 0 || n_windows > n) return fail(MCD_EINVAL, "need 0 <= n_windows <= n");
    if (n > stream_group_rows(s))
        return fail(MCD_EINVAL, "more rows than n_slots * (ring_len - seg_len + 1): a group holds at most ring_len - seg_len + 1 rows per track");
    return MCD_OK;
}
// the window count of a group's score launch, one thread per (window, transform, lane of a W-wide cell): *total = the threads
static int check_group_windows(const mcd_stream_state_t* s, int32_t n_windows, int W, long long* total) {
    if (n_windows < 0 || n_windows > stream_group_rows(s)) return fail(MCD_EINVAL, "need 0 <= n_windows <= n_slots * (ring_len - seg_len + 1)");
    *total = (long long)n_windows * s->num_transform * W;
    if (*total > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many windows for one launch");
    return MCD_OK;
}

// The corrupt frames of a stream's cfg as the ring kernels read them (seg_len <= 32: check_frame_partition has passed).
//   tx_of != NULL (joint ring): tx_of[window row] = its index among the corrupt frames, -1 = a condition frame; the frames are distinct
//   tx_of == NULL (forecast ring): cidx[k] = the k-th corrupt frame; the frames ascend
static int corrupt_frames(const mcd_score_cfg_t* cfg, int* tx_of, int* cidx) {
    for (int k = 0; tx_of && k < MCD_MAX_FRAMES; ++k) tx_of[k] = -1;
    for (int k = 0; k < cfg->n_corrupt; ++k) {
        const int t = cfg->corrupt_idx[k];
        const bool inside = t >= 0 && t < cfg->seg_len;
        if (tx_of) {
            if (!inside || tx_of[t] >= 0) return fail(MCD_EINVAL, "bad corrupt_idx");
            tx_of[t] = k;
        } else {
            if (!inside || (k > 0 && t <= cfg->corrupt_idx[k - 1])) return fail(MCD_EINVAL, "corrupt_idx must ascend inside [0, seg_len)");
            cidx[k] = t;
        }
    }
    return MCD_OK;
}

// the joint ring beside a stream state: (n_slots, num_transform, ring_len, 17) floats
static int stream_joint_params(const mcd_stream_state_t* s, const mcd_stream_joint_state_t* js, StreamParams* P) {
    if (int rc = stream_params(s, P)) return rc;
    if (!js || !js->joint_scores) return fail(MCD_EINVAL, "null stream joint state");
    if ((int64_t)s->n_slots * s->num_transform * s->ring_len > 0x7fffffffll / 17)
        return fail(MCD_EUNSUPPORTED, "stream joint ring of more than 2^31 elements");
    return MCD_OK;
}

// the forecast rings beside a stream state: (n_slots, ring_len, n_corrupt, 34) and (n_slots, ring_len, 34) floats; everything the two
// forecast entries share is checked here, before any device call
static int stream_forecast_params(const mcd_stream_state_t* s, const mcd_stream_forecast_state_t* fs, const mcd_score_cfg_t* cfg,
                                  int32_t method, int32_t spread_method, float vid_w, float vid_h, const double* center,
                                  const double* scale, StreamParams* P, StreamForecastParams* F) {
    memset(F, 0, sizeof(*F));
    if (int rc = stream_params(s, P)) return rc;
    if (!fs || !fs->forecast || !fs->observed) return fail(MCD_EINVAL, "null stream forecast state");
    if (fs->n_corrupt < 1 || fs->n_corrupt > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "stream forecast state: need 1 <= n_corrupt <= 32");
    if (!cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->seg_len != P->seg_len) return fail(MCD_EINVAL, "cfg->seg_len is not the stream state's seg_len");
    if (cfg->n_corrupt != fs->n_corrupt) return fail(MCD_EINVAL, "cfg->n_corrupt is not the stream forecast state's n_corrupt");
    if (int rc = check_frame_partition(cfg)) return rc;
    if (int rc = corrupt_frames(cfg, nullptr, F->cidx)) return rc;
    if (int rc = check_forecast_methods(method, spread_method)) return rc;
    if (int rc = check_pose_geometry(vid_w, vid_h, center, scale)) return rc;
    if ((int64_t)s->n_slots * s->ring_len > 0x7fffffffll / (34 * fs->n_corrupt))
        return fail(MCD_EUNSUPPORTED, "stream forecast ring of more than 2^31 elements");
    F->fc = fs->forecast; F->obs = fs->observed; F->center = center; F->scale = scale; F->vid_w = vid_w; F->vid_h = vid_h;
    F->Tx = fs->n_corrupt; F->method = method; F->spread_method = spread_method;
    return MCD_OK;
}

// the forecast rings of every transform: (n_slots, ring_len, num_transform, n_corrupt, 34) and (n_slots, ring_len, 34) floats.  What is
// new is checked here, the rest by stream_forecast_params on the same three fields
static int stream_forecast_tta_params(const mcd_stream_state_t* s, const mcd_stream_forecast_tta_state_t* fs, const mcd_score_cfg_t* cfg,
                                      int32_t method, int32_t spread_method, float vid_w, float vid_h, const double* center,
                                      const double* scale, const double* inv_affine, StreamParams* P, StreamForecastParams* F) {
    memset(F, 0, sizeof(*F));
    if (int rc = stream_params(s, P)) return rc;
    if (!fs || !fs->forecast || !fs->observed) return fail(MCD_EINVAL, "null stream forecast state");
    if (fs->num_transform != P->nt) return fail(MCD_EINVAL, "stream forecast state: num_transform is not the stream state's");
    if (fs->n_corrupt < 1 || fs->n_corrupt > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "stream forecast state: need 1 <= n_corrupt <= 32");
    if ((int64_t)fs->num_transform * fs->n_corrupt > MCD_FORECAST_VIEW_COVER)
        return fail(MCD_EINVAL, "stream forecast state: num_transform * n_corrupt exceeds 64, the pairs one row's reduction holds");
    if ((int64_t)s->n_slots * s->ring_len > 0x7fffffffll / (34ll * fs->n_corrupt * fs->num_transform))
        return fail(MCD_EUNSUPPORTED, "stream forecast ring of more than 2^31 elements");
    const mcd_stream_forecast_state_t one{fs->forecast, fs->observed, fs->n_corrupt};
    if (int rc = stream_forecast_params(s, &one, cfg, method, spread_method, vid_w, vid_h, center, scale, P, F)) return rc;
    if (!inv_affine) return fail(MCD_EINVAL, "null inv_affine");
    return MCD_OK;
}

// What the forecast entries of one transform and of every transform share behind their state's checks: the checks of a group (a
// flush), then the launches.  inv == nullptr: the ring of transform 0 (mcd_stream_forecast_state_t); else the ring of every transform
// and its inverse table.
static int stream_forecast_group_run(const mcd_stream_state_t* s, const StreamParams& P, StreamForecastParams& F, const double* inv,
                                     const float* raw, const int32_t* desc, int32_t n, const float* loss_all, const float* poses_all,
                                     const int32_t* win, int32_t n_windows, const mcd_score_cfg_t* cfg, int32_t aggregation,
                                     float* expected_out, float* norm_out, float* observed_out, int32_t* count_out, float* spread_out,
                                     void* stream) {
    if (aggregation != MCD_AGGR_BEST && aggregation != MCD_AGGR_WORST)
        return fail(MCD_EINVAL, "a forecast is the pose of ONE sample: aggregation must be MCD_AGGR_BEST or MCD_AGGR_WORST");
    if (int rc = check_group_rows(s, n, n_windows)) return rc;
    long long total;
    if (int rc = check_group_windows(s, n_windows, 1, &total)) return rc;
    if (cfg->n_samples < 1) return fail(MCD_EINVAL, "need n_samples >= 1");
    if (n == 0) return MCD_OK;
    if (!raw || !desc) return fail(MCD_EINVAL, "null argument");
    if (n_windows > 0 && (!loss_all || !poses_all || !win || !expected_out || !norm_out || !observed_out || !count_out || !spread_out))
        return fail(MCD_EINVAL, "null argument");
    F.loss_all = loss_all; F.poses_all = poses_all; F.S = cfg->n_samples; F.strategy = aggregation; F.in_lds = F.S <= AGG_LDS_MAX;
    F.expected = expected_out; F.norm = norm_out; F.observed = observed_out; F.count = count_out; F.spread = spread_out;
    hipStream_t st = (hipStream_t)stream;
    // the windows' forecasts and the raw rows in one launch; the final rows in a second one behind it (stream order)
    const long long blocks = (inv ? total : (long long)n_windows) + ((long long)n * 34 + 63) / 64;
    const size_t lds = (size_t)(SEL_LDS_WORDS + (F.in_lds ? F.S : 0)) * sizeof(float);
    if (inv) hipLaunchKernelGGL(stream_forecast_store_tta_kernel, dim3((unsigned)blocks), dim3(64), lds, st, P, F, inv, raw, desc, n, win, n_windows, (int)total);
    else hipLaunchKernelGGL(stream_forecast_store_kernel, dim3((unsigned)blocks), dim3(64), lds, st, P, F, raw, desc, n, win, n_windows, (int)total);
    HIP_TRY(hipGetLastError());
    if (n_windows == 0) return MCD_OK;
    if (inv) hipLaunchKernelGGL(stream_forecast_emit_tta_kernel, dim3((unsigned)n_windows), dim3(64), 0, st, P, F, win, n_windows, (int)total);
    else hipLaunchKernelGGL(stream_forecast_emit_kernel, dim3((unsigned)n_windows), dim3(64), 0, st, P, F, win, n_windows, (int)total);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

static int stream_forecast_flush_run(const StreamParams& P, StreamForecastParams& F, bool tta, const int32_t* win, int32_t n,
                                     float* expected_out, float* norm_out, float* observed_out, int32_t* count_out, float* spread_out,
                                     void* stream) {
    if (n < 0 || n > P.n_slots) return fail(MCD_EINVAL, "need 0 <= n <= n_slots");
    const long long rows = (long long)n * (P.seg_len - 1);
    if (rows == 0) return MCD_OK;
    if (!win || !expected_out || !norm_out || !observed_out || !count_out || !spread_out) return fail(MCD_EINVAL, "null argument");
    if (rows > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many tracks for one launch");
    F.expected = expected_out; F.norm = norm_out; F.observed = observed_out; F.count = count_out; F.spread = spread_out;
    if (tta) hipLaunchKernelGGL(stream_forecast_flush_tta_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, P, F, win, n);
    else hipLaunchKernelGGL(stream_forecast_flush_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, P, F, win, n);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

static int clip_params(const mcd_clip_state_t* c, ClipParams* P) {
    if (!c || !c->sum || !c->lmax || !c->lmin || !c->n) return fail(MCD_EINVAL, "null clip state");
    if (c->n_clips <= 0 || c->num_transform <= 0 || c->clip_ring_len <= 0)
        return fail(MCD_EINVAL, "clip state: need n_clips, num_transform, clip_ring_len >= 1");
    if (c->num_transform > 256) return fail(MCD_EUNSUPPORTED, "clip state: more than 256 transforms");
    if ((int64_t)c->n_clips * c->clip_ring_len > 0x7fffffffll / c->num_transform)
        return fail(MCD_EUNSUPPORTED, "clip rings of more than 2^31 cells");
    P->sum = c->sum; P->lmax = c->lmax; P->lmin = c->lmin; P->n = c->n;
    P->n_clips = c->n_clips; P->L = c->clip_ring_len; P->nt = c->num_transform;
    return MCD_OK;
}

extern "C" {

int mcd_stream_flush(const mcd_stream_state_t* s, const int32_t* win, int32_t n, float* out, void* stream) {
    StreamParams P;
    if (int rc = stream_params(s, &P)) return rc;
    return stream_flush<1>(P, P.fs, win, n, out, stream);
}

int mcd_stream_push_group(const mcd_stream_state_t* s, const float* raw, const int32_t* desc, int32_t n, int32_t n_windows,
                          float vid_w, float vid_h, const double* center, const double* scale, int64_t* base_out,
                          int32_t* trans_out, void* stream) {
    StreamParams P;
    if (int rc = stream_params(s, &P)) return rc;
    if (int rc = check_group_rows(s, n, n_windows)) return rc;
    if ((int64_t)n_windows * P.nt > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many windows for one launch");
    if (int rc = check_pose_geometry(vid_w, vid_h, center, scale)) return rc;
    if (n == 0) return MCD_OK;
    if (!raw || !desc || (n_windows > 0 && (!base_out || !trans_out))) return fail(MCD_EINVAL, "null argument");
    hipLaunchKernelGGL(stream_push_group_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, raw, desc,
                       n, n_windows * P.nt, vid_w, vid_h, center, scale, reinterpret_cast<long long*>(base_out), trans_out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_stream_frame_scores_group(const mcd_stream_state_t* s, const float* scores, const int32_t* win, int32_t n_windows,
                                  float* final_out, void* stream) {
    StreamParams P;
    if (int rc = stream_params(s, &P)) return rc;
    long long total;
    if (int rc = check_group_windows(s, n_windows, 1, &total)) return rc;
    if (n_windows == 0) return MCD_OK;
    if (!scores || !win || !final_out) return fail(MCD_EINVAL, "null argument");
    hipLaunchKernelGGL(stream_frame_scores_group_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P,
                       scores, win, n_windows, (int)total, final_out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_stream_joint_scores_group(const mcd_stream_state_t* s, const mcd_stream_joint_state_t* js, const float* maps,
                                  const int32_t* win, int32_t n_windows, const mcd_score_cfg_t* cfg, float* final_out, void* stream) {
    StreamParams P;
    if (int rc = stream_joint_params(s, js, &P)) return rc;
    if (!cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->seg_len != P.seg_len) return fail(MCD_EINVAL, "cfg->seg_len is not the stream state's seg_len");
    if (int rc = check_frame_partition(cfg)) return rc;
    StreamJointParams J;
    memset(&J, 0, sizeof(J));
    J.js = js->joint_scores; J.Tx = cfg->n_corrupt;
    if (int rc = corrupt_frames(cfg, J.tx_of, nullptr)) return rc;
    long long total;
    if (int rc = check_group_windows(s, n_windows, 17, &total)) return rc;
    if (n_windows == 0) return MCD_OK;
    if (!maps || !win || !final_out) return fail(MCD_EINVAL, "null argument");
    hipLaunchKernelGGL(stream_joint_scores_group_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, J,
                       maps, win, n_windows, n_windows * P.nt, final_out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_stream_joint_flush(const mcd_stream_state_t* s, const mcd_stream_joint_state_t* js, const int32_t* win, int32_t n,
                           float* out, void* stream) {
    StreamParams P;
    if (int rc = stream_joint_params(s, js, &P)) return rc;
    return stream_flush<17>(P, js->joint_scores, win, n, out, stream);
}

int mcd_stream_forecast_group(const mcd_stream_state_t* s, const mcd_stream_forecast_state_t* fs, const float* raw, const int32_t* desc,
                              int32_t n, const float* loss_all, const float* poses_all, const int32_t* win, int32_t n_windows,
                              const mcd_score_cfg_t* cfg, int32_t aggregation, int32_t method, int32_t spread_method, float vid_w,
                              float vid_h, const double* center, const double* scale, float* expected_out, float* norm_out,
                              float* observed_out, int32_t* count_out, float* spread_out, void* stream) {
    StreamParams P;
    StreamForecastParams F;
    if (int rc = stream_forecast_params(s, fs, cfg, method, spread_method, vid_w, vid_h, center, scale, &P, &F)) return rc;
    return stream_forecast_group_run(s, P, F, nullptr, raw, desc, n, loss_all, poses_all, win, n_windows, cfg, aggregation, expected_out,
                                     norm_out, observed_out, count_out, spread_out, stream);
}

int mcd_stream_forecast_flush(const mcd_stream_state_t* s, const mcd_stream_forecast_state_t* fs, const int32_t* win, int32_t n,
                              const mcd_score_cfg_t* cfg, int32_t method, int32_t spread_method, float vid_w, float vid_h,
                              const double* center, const double* scale, float* expected_out, float* norm_out, float* observed_out,
                              int32_t* count_out, float* spread_out, void* stream) {
    StreamParams P;
    StreamForecastParams F;
    if (int rc = stream_forecast_params(s, fs, cfg, method, spread_method, vid_w, vid_h, center, scale, &P, &F)) return rc;
    return stream_forecast_flush_run(P, F, false, win, n, expected_out, norm_out, observed_out, count_out, spread_out, stream);
}

int mcd_stream_forecast_group_tta(const mcd_stream_state_t* s, const mcd_stream_forecast_tta_state_t* fs, const float* raw,
                                  const int32_t* desc, int32_t n, const float* loss_all, const float* poses_all, const int32_t* win,
                                  int32_t n_windows, const mcd_score_cfg_t* cfg, int32_t aggregation, int32_t method,
                                  int32_t spread_method, float vid_w, float vid_h, const double* center, const double* scale,
                                  const double* inv_affine, float* expected_out, float* norm_out, float* observed_out,
                                  int32_t* count_out, float* spread_out, void* stream) {
    StreamParams P;
    StreamForecastParams F;
    if (int rc = stream_forecast_tta_params(s, fs, cfg, method, spread_method, vid_w, vid_h, center, scale, inv_affine, &P, &F)) return rc;
    return stream_forecast_group_run(s, P, F, inv_affine, raw, desc, n, loss_all, poses_all, win, n_windows, cfg, aggregation,
                                     expected_out, norm_out, observed_out, count_out, spread_out, stream);
}

int mcd_stream_forecast_flush_tta(const mcd_stream_state_t* s, const mcd_stream_forecast_tta_state_t* fs, const int32_t* win, int32_t n,
                                  const mcd_score_cfg_t* cfg, int32_t method, int32_t spread_method, float vid_w, float vid_h,
                                  const double* center, const double* scale, const double* inv_affine, float* expected_out,
                                  float* norm_out, float* observed_out, int32_t* count_out, float* spread_out, void* stream) {
    StreamParams P;
    StreamForecastParams F;
    if (int rc = stream_forecast_tta_params(s, fs, cfg, method, spread_method, vid_w, vid_h, center, scale, inv_affine, &P, &F)) return rc;
    return stream_forecast_flush_run(P, F, true, win, n, expected_out, norm_out, observed_out, count_out, spread_out, stream);
}

int mcd_stream_clip_update(const mcd_clip_state_t* c, const int32_t* runs, int32_t n_runs, const int32_t* contrib,
                           int32_t n_contrib, const float* finals, int32_t n_finals, const float* tails, int32_t n_tails,
                           void* stream) {
    ClipParams P;
    if (int rc = clip_params(c, &P)) return rc;
    if (n_runs < 0 || n_runs > (int64_t)c->n_clips * c->clip_ring_len)
        return fail(MCD_EINVAL, "need 0 <= n_runs <= n_clips * clip_ring_len: a call names a cell at most once");
    if (n_contrib < 0 || n_finals < 0 || n_tails < 0) return fail(MCD_EINVAL, "need n_contrib, n_finals, n_tails >= 0");
    if (n_runs == 0) return MCD_OK;
    if (!runs || (n_contrib > 0 && !contrib) || (n_finals > 0 && !finals) || (n_tails > 0 && !tails))
        return fail(MCD_EINVAL, "null argument");
    const long long total = (long long)n_runs * P.nt;
    hipLaunchKernelGGL(stream_clip_update_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, runs,
                       n_runs, contrib, n_contrib, finals, n_finals, tails, n_tails);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_stream_clip_emit(const mcd_clip_state_t* c, const int32_t* outs, int32_t n_out, const double* gauss, int32_t radius,
                         int32_t shift, double* out, void* stream) {
    ClipParams P;
    if (int rc = clip_params(c, &P)) return rc;
    if (n_out < 0 || n_out > (int64_t)c->n_clips * c->clip_ring_len) return fail(MCD_EINVAL, "need 0 <= n_out <= n_clips * clip_ring_len");
    if (radius < 0 || radius > (1 << 24) || shift < 0) return fail(MCD_EINVAL, "need 0 <= radius <= 2^24 and shift >= 0");
    if (n_out == 0) return MCD_OK;
    if (!outs || !gauss || !out) return fail(MCD_EINVAL, "null argument");
    // outputs per workgroup: as many (output, transform) tap threads as a workgroup has, fewer when their staged values
    // (2 radius + 1 doubles each) would not fit 48 KB of LDS; a kernel wider than that reads its values in place
    const size_t per_out = (size_t)P.nt * (2 * (size_t)radius + 1) * sizeof(double);
    ClipEmitParams E;
    E.outs = outs; E.gauss = gauss; E.out = out; E.n_out = n_out; E.radius = radius; E.shift = shift;
    E.staged = per_out <= (size_t)48 * 1024 ? 1 : 0;
    E.opb = 256 / P.nt;
    if (E.staged) E.opb = std::min<int>(E.opb, (int)((size_t)48 * 1024 / per_out));
    E.opb = std::max(1, std::min(E.opb, 16));         // (few outputs per tick: more workgroups, shorter staging loops)
    const size_t lds = ((size_t)E.opb * P.nt + (E.staged ? (size_t)E.opb * P.nt * (2 * (size_t)radius + 1) : 0)) * sizeof(double);
    hipLaunchKernelGGL(stream_clip_emit_kernel, dim3((unsigned)((n_out + E.opb - 1) / E.opb)), dim3(256), lds, (hipStream_t)stream, P, E);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

}  // extern "C"

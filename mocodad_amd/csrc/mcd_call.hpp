// mcd_call.hpp — the front end of a scoring call, shared by the pose entry points (mcd_api.hip) and the latent ones
// (mcd_latent_api.hpp): the window view, the checks of the frame lists, the aggregation, the pose geometry and the forecast methods, the workspace layouts, the launch of
// a condition encoder for a route, and the condition-encoder fields of a handle.  Host code only, like mcd_pack.hpp.  Included by
// mcd_api.hip behind its routes and launchers (cond_route, launch_cond_view, launch_cond_plain, the *_ws_bytes functions), which it
// calls.  The ORDER in which an entry point applies the checks is part of its behaviour (the first failing check names the
// error): the functions here are the checks, the entry points keep their order.
#pragma once

namespace {

using namespace mcd;

int64_t round256(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// mcd_window_view_t (NULL = dense (B,C,seg_len,V) windows at `data`) -> the view the kernels load through
int window_view(const float* data, const mcd_window_view_t* view, int seg_len, DataView& dv) {
    memset(&dv, 0, sizeof(dv));
    dv.data = data;
    if (!view) return MCD_OK;
    if (view->trans && !view->affine) return fail(MCD_EINVAL, "window view: trans given without an affine table");
    dv.base = reinterpret_cast<const long long*>(view->base); dv.sc = view->stride_c; dv.st = view->stride_t;
    dv.trans = view->trans; dv.aff = view->affine;
    if (!view->base) { dv.sc = (long long)seg_len * 17; dv.st = 17; }
    return MCD_OK;
}

// the two frame lists of a call: together they are the window's frames ...
int check_frame_partition(const mcd_score_cfg_t* cfg) {
    if (cfg->n_corrupt < 1 || cfg->n_cond + cfg->n_corrupt != cfg->seg_len || cfg->seg_len > MCD_MAX_FRAMES)
        return fail(MCD_EINVAL, "cond/corrupt index lists do not partition seg_len");
    return MCD_OK;
}
// ... and every frame the kernels read (load_coord) lies inside the window
int check_frame_lists(const mcd_score_cfg_t* cfg) {
    for (int k = 0; k < cfg->n_cond; ++k)
        if (cfg->cond_idx[k] < 0 || cfg->cond_idx[k] >= cfg->seg_len) return fail(MCD_EINVAL, "cond_idx outside [0, seg_len)");
    for (int k = 0; k < cfg->n_corrupt; ++k)
        if (cfg->corrupt_idx[k] < 0 || cfg->corrupt_idx[k] >= cfg->seg_len) return fail(MCD_EINVAL, "corrupt_idx outside [0, seg_len)");
    return MCD_OK;
}

// aggregation over the samples: `allowed` = bit MCD_AGGR_* per strategy the entry point takes, `unknown` = its text for another
constexpr unsigned AGGR_LOSSES = 1u << MCD_AGGR_BEST | 1u << MCD_AGGR_WORST | 1u << MCD_AGGR_MEAN | 1u << MCD_AGGR_MEDIAN | 1u << MCD_AGGR_QUANTILE;
constexpr unsigned AGGR_ANY = AGGR_LOSSES | 1u << MCD_AGGR_MEAN_POSE | 1u << MCD_AGGR_MEDIAN_POSE;
int check_aggregation(int strategy, float quantile, unsigned allowed, const char* unknown) {
    if (strategy < 0 || strategy > 31 || !((allowed >> strategy) & 1u)) return fail(MCD_EINVAL, unknown);
    if (strategy == MCD_AGGR_QUANTILE && !(quantile >= 0.f && quantile <= 1.f))       // (also rejects NaN; torch.quantile raises)
        return fail(MCD_EINVAL, "quantile must be in [0, 1]");
    return MCD_OK;
}

// the geometry of a pose row's (de)normalisation: the image size and the RobustScaler's statistics
int check_pose_geometry(float vid_w, float vid_h, const double* center, const double* scale) {
    if (!std::isfinite(vid_w) || !std::isfinite(vid_h)) return fail(MCD_EINVAL, "vid_res must be finite");
    if (!center != !scale) return fail(MCD_EINVAL, "center and scale are both given or both NULL");
    return MCD_OK;
}
// how the overlapping forecasts of a (person, frame) cell become one pose, and their spread one number
int check_forecast_methods(int method, int spread_method) {
    if (method != MCD_FORECAST_UNIQUE && method != MCD_FORECAST_MEAN && method != MCD_FORECAST_MEDIAN)
        return fail(MCD_EINVAL, "method must be MCD_FORECAST_UNIQUE, MEAN or MEDIAN");
    if (spread_method != MCD_FORECAST_MEAN && spread_method != MCD_FORECAST_MEDIAN)
        return fail(MCD_EINVAL, "spread_method must be MCD_FORECAST_MEAN or MEDIAN");
    return MCD_OK;
}

// ------------------------------------------------------------------------------------------------
// Workspace layouts: byte offsets of the regions of a call's workspace and its size.  The *_workspace_bytes entry returns
// `bytes`, the call carves at the offsets: both read the one function.
// ------------------------------------------------------------------------------------------------
// pose: [condition embeddings (B,16) | gathered condition frames (B,C,Tc,V)][per-sample losses (B,S)][scratch slabs of the
// slab-tiled / runtime-shape kernels -- one region: the condition encoder has finished with it when the trajectories start]
struct PoseWorkspace { int64_t gather, loss, scratch, bytes; };      // (the embeddings are at offset 0)
PoseWorkspace pose_workspace(const mcd_weights* w, int64_t B, int64_t S) {
    PoseWorkspace L;
    L.gather = (B * EDIM + 16) * 4;
    L.loss = round256(B * (EDIM + C0 * (w->cfg.t_cond > 0 ? w->cfg.t_cond : 0) * 17) * 4 + 256);
    L.scratch = L.loss + round256(B * S * 4);
    L.bytes = L.scratch + std::max(unet_ws_bytes(w, B * S), cond_ws_bytes(w, B));
    return L;
}
// latent: [condition embeddings (B,16)][z0 (B,D)][gathered condition frames][third buffer of the plain encoder under gmode][H]; the
// gather and the third buffer only where the plain encoder serves the handle, H (B, h_floats: the last encoder layer's output,
// 640 floats per corrupt frame) only where to_time_dim is a launch of its own (h_floats = 0 otherwise).  cw: the handle's condition
// encoder (mcd_latent_weights::cw)
struct LatentWorkspace { int64_t z0, gather, plain, h, bytes; };
LatentWorkspace latent_workspace(const mcd_weights* cw, int64_t B, int D, int64_t h_floats) {
    const CondRoute r = cond_route(cw);
    const bool plain = r == COND_PLAIN || r == COND_PLAIN_SCRATCH;
    LatentWorkspace L;
    L.z0 = round256(B * EDIM * 4);
    L.gather = L.z0 + round256(B * D * 4);
    L.plain = L.gather + (plain ? round256(B * C0 * cw->cfg.t_cond * 17 * 4) : 0);
    L.h = L.plain + (plain ? round256(cond_scratch_bytes(cw, COND_PLAIN_SCRATCH, B)) : 0);
    L.bytes = L.h + (h_floats ? round256(B * h_floats * 4) : 0);
    return L;
}

// latent, mcd_latent_decode_samples: [condition embeddings (B,16)][gathered condition frames][third buffer of the plain encoder][G];
// the middle two as above, G = g_bytes: the rows of one window chunk (mcd_latent_api.hpp bounds it)
struct LatentDecodeWorkspace { int64_t gather, plain, g, bytes; };
LatentDecodeWorkspace latent_decode_workspace(const mcd_weights* cw, int64_t B, int64_t g_bytes) {
    const CondRoute r = cond_route(cw);
    const bool plain = r == COND_PLAIN || r == COND_PLAIN_SCRATCH;
    LatentDecodeWorkspace L;
    L.gather = round256(B * EDIM * 4);
    L.plain = L.gather + (plain ? round256(B * C0 * cw->cfg.t_cond * 17 * 4) : 0);
    L.g = L.plain + (plain ? round256(cond_scratch_bytes(cw, COND_PLAIN_SCRATCH, B)) : 0);
    L.bytes = L.g + round256(g_bytes);
    return L;
}

// latent, mcd_latent_score_pose: [the chain call's workspace: latent_workspace of the diffusion-stage handle, cond_emb (B,16) at its
// head][per-sample losses (B,S)][generated latents (B,S,D)][decoded poses (B,S,2,Tx,17)][the decode call's workspace:
// latent_decode_workspace of the autoencoder handle, of which only G is used -- cond_emb is the chain call's].  The three middle
// regions are reserved whatever the caller asks for (the size does not depend on the outputs); one the caller passes a buffer for
// stays unused.  score_bytes / decode_bytes: the `bytes` of the two layouts above
struct LatentPoseWorkspace { int64_t loss, latent, pose, decode, bytes; };      // (the chain call's workspace is at offset 0)
LatentPoseWorkspace latent_pose_workspace(int64_t score_bytes, int64_t decode_bytes, int64_t B, int64_t S, int D, int Tx) {
    LatentPoseWorkspace L;
    L.loss = round256(score_bytes);
    L.latent = L.loss + round256(B * S * 4);
    L.pose = L.latent + round256(B * S * D * 4);
    L.decode = L.pose + round256(B * S * C0 * Tx * 17 * 4);
    L.bytes = L.decode + round256(decode_bytes);
    return L;
}

// One condition encoder launch (with its gather, for the plain routes) -> emb (B,16).  r: a route with a launch of its own (not
// COND_NONE / COND_INKERNEL).  gather: where the plain encoder's dense (B,C,Tc,V) copy of the condition frames goes; NULL = dv.data
// IS that copy (mcd_cond_encode).  scratch: cond_scratch_bytes(w, r, B) of device memory, NULL if that is 0.
int launch_cond(const mcd_weights* w, CondRoute r, const DataView& dv, const FrameIdx& fi, int seg_len, float* emb, int B, float* gather,
                float* scratch, hipStream_t st) {
    if (r != COND_PLAIN && r != COND_PLAIN_SCRATCH) return launch_cond_view(w, r, dv, fi, seg_len, emb, B, scratch, st);
    if (!gather) return launch_cond_plain(w, dv.data, B, emb, scratch, st);
    const int Tc = w->cond.Tc;
    const long long total = (long long)B * C0 * Tc * 17;
    if (total > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x condition frames exceeds 2^31 - 1 elements: score in smaller batches");
    hipLaunchKernelGGL(gather_frames_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dv, gather, B, C0, seg_len, 17, Tc, fi);
    HIP_TRY(hipGetLastError());
    return launch_cond_plain(w, gather, B, emb, scratch, st);
}

// the condition-encoder fields of a handle (the pose handle itself, or mcd_latent_weights::cw) from the packed model at dbuf
void set_cond_weights(mcd_weights* w, const PackedModel& m, float* dbuf) {
    w->has_cond = m.cond.has; w->cond_fast = m.cond.fast; w->cond_unet = m.cond.unet;
    w->cond = m.cond.Cw;
    w->cond.base = dbuf;
}

}  // namespace

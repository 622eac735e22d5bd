// mcd_latent_api.hpp — host side of the MoCoDADlatent entry points (include/mocodad_hip.h): the handle and the calls around the
// launchers of mcd_latent.hip.  Included at the end of mcd_api.hip, whose upload helper and condition-encoder launches it shares; the
// packer is pack_latent_model of mcd_pack.hpp.  It holds no device code.
#pragma once
#include "mcd_latent.hpp"

struct mcd_latent_weights {
    mcd_model_cfg_t cfg;
    int device;
    float* dbuf;
    size_t n_floats;
    mcd::LatentNet net;
    bool fused_ok;        // cond_fast_body's table is packed and t_cond = t_unet: the encode launch can run the condition encoder itself
    mcd_weights cw;       // the condition encoder as the pose model's launchers take it: dbuf, cond and the cond_* flags; nothing else is set
    int opt[MCD_LATENT_OPT_COUNT];
};

namespace {

using namespace mcd;

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
int64_t lat_ws_cond_bytes(int64_t B) { return (B * EDIM * 4 + 255) / 256 * 256; }
int64_t lat_ws_z0_bytes(int64_t B, int D) { return (B * D * 4 + 255) / 256 * 256; }

int latent_view(const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view, DataView& dv) {
    memset(&dv, 0, sizeof(dv));
    dv.data = data;
    if (view) {
        if (view->trans && !view->affine) return fail(MCD_EINVAL, "window view: trans given without an affine table");
        dv.base = reinterpret_cast<const long long*>(view->base); dv.sc = view->stride_c; dv.st = view->stride_t;
        dv.trans = view->trans; dv.aff = view->affine;
        if (!view->base) { dv.sc = (long long)cfg->seg_len * 17; dv.st = 17; }
    }
    return MCD_OK;
}

int latent_frames(const mcd_latent_weights* w, const mcd_score_cfg_t* cfg, FrameIdx& cond_fi, FrameIdx& fi) {
    if (cfg->n_corrupt != w->cfg.t_unet || cfg->n_cond != w->cfg.t_cond) return fail(MCD_EINVAL, "frame split does not match the packed model (t_unet / t_cond)");
    if (cfg->n_cond + cfg->n_corrupt != cfg->seg_len || cfg->seg_len > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "cond/corrupt index lists do not partition seg_len");
    memset(&cond_fi, 0, sizeof(cond_fi));
    memset(&fi, 0, sizeof(fi));
    for (int k = 0; k < cfg->n_cond; ++k) {
        if (cfg->cond_idx[k] < 0 || cfg->cond_idx[k] >= cfg->seg_len) return fail(MCD_EINVAL, "cond_idx outside [0, seg_len)");
        cond_fi.idx[k] = cfg->cond_idx[k];
    }
    for (int k = 0; k < cfg->n_corrupt; ++k) {
        if (cfg->corrupt_idx[k] < 0 || cfg->corrupt_idx[k] >= cfg->seg_len) return fail(MCD_EINVAL, "corrupt_idx outside [0, seg_len)");
        fi.idx[k] = cfg->corrupt_idx[k];
    }
    return MCD_OK;
}

// Which condition-encoder kernel serves a latent handle (decided here and nowhere else)
enum LatentCondRoute {
    LAT_COND_FUSED,       // shipped encoder at t_cond = t_unet: inside the encode launch
    LAT_COND_FAST,        // shipped channel list, another t_cond (or MCD_LATENT_OPT_SPLIT_ENCODE): cond_fast_kernel
    LAT_COND_UNET,        // 'E_unet': cond_unet_kernel
    LAT_COND_PLAIN        // any other channel list: gather_frames_kernel + cond_encode_kernel
};
LatentCondRoute latent_cond_route(const mcd_latent_weights* w) {
    if (w->cw.cond_unet) return LAT_COND_UNET;
    if (w->fused_ok && !w->opt[MCD_LATENT_OPT_SPLIT_ENCODE]) return LAT_COND_FUSED;
    return w->cw.cond_fast ? LAT_COND_FAST : LAT_COND_PLAIN;      // (no cond_fast_kernel for t_cond: a developer build)
}
// scratch of the plain encoder (independent of the options): the gathered condition frames, and its third buffer under gmode
int64_t lat_ws_gather_bytes(const mcd_latent_weights* w, int64_t B) {
    if (w->cw.cond_unet || w->cw.cond_fast) return 0;
    return (B * C0 * w->cfg.t_cond * 17 * 4 + 255) / 256 * 256;
}
int64_t lat_ws_plain_bytes(const mcd_latent_weights* w, int64_t B) {
    if (w->cw.cond_unet || w->cw.cond_fast) return 0;
    return (cond_scratch_bytes(&w->cw, COND_PLAIN_SCRATCH, B) + 255) / 256 * 256;
}

// scratch: lat_ws_gather_bytes + lat_ws_plain_bytes of device memory (null when both are 0)
int latent_encode_impl(const mcd_latent_weights* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                       const float* step_table, float* cond_out, float* z0_out, char* scratch, hipStream_t st) {
    DataView dv;
    int rc = latent_view(cfg, data, view, dv);
    if (rc != MCD_OK) return rc;
    FrameIdx cond_fi, fi;
    rc = latent_frames(w, cfg, cond_fi, fi);
    if (rc != MCD_OK) return rc;
    // row ns of the table: the constant time step -1 the encoder is given (mocodad_latent.py:95)
    const float* pe_row = step_table + (size_t)cfg->noise_steps * (4 + EDIM) + 4;
    const int B = cfg->n_windows;
    const LatentCondRoute route = latent_cond_route(w);
    if (route == LAT_COND_FAST) {
        rc = launch_cond_fast(&w->cw, dv, cond_fi, cfg->seg_len, cond_out, B, st);
    } else if (route == LAT_COND_UNET) {
        rc = launch_cond_unet(&w->cw, dv, cond_fi, cfg->seg_len, cond_out, B, st);
    } else if (route == LAT_COND_PLAIN) {
        if (!scratch) return fail(MCD_EINVAL, "workspace required (mcd_latent_workspace_bytes) for this condition encoder");
        float* cbuf = reinterpret_cast<float*>(scratch);
        const int Tc = cfg->n_cond;
        const long long total = (long long)B * C0 * Tc * 17;
        if (total > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x condition frames exceeds 2^31 - 1 elements: score in smaller batches");
        hipLaunchKernelGGL(gather_frames_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dv, cbuf, B, C0, cfg->seg_len, 17, Tc, cond_fi);
        HIP_TRY(hipGetLastError());
        rc = launch_cond_plain(&w->cw, cbuf, B, cond_out, reinterpret_cast<float*>(scratch + lat_ws_gather_bytes(w, B)), st);
    }
    if (rc != MCD_OK) return rc;
    return launch_latent_encode(w->cfg.t_unet, route == LAT_COND_FUSED, w->dbuf, dv, cond_fi, fi, cfg->seg_len, pe_row, cond_out, z0_out, w->net.D,
                                B, st);
}

}  // namespace

extern "C" {

int mcd_pack_latent_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, const mcd_latent_cfg_t* lcfg,
                            int32_t device, mcd_latent_weights_t** out) {
    if (!tensors || !cfg || !lcfg || !out) return fail(MCD_EINVAL, "null argument");
    PackedModel m;
    int rc = pack_latent_model(tensors, n_tensors, cfg, lcfg, m);
    if (rc != MCD_OK) return rc;
    float* dbuf = nullptr;
    rc = upload_packed(m.buf, device, &dbuf);
    if (rc != MCD_OK) return rc;
    mcd_latent_weights* w = new mcd_latent_weights();
    w->cfg = *cfg; w->device = device; w->n_floats = m.buf.size(); w->net = m.net; w->dbuf = dbuf;
    memset(w->opt, 0, sizeof(w->opt));
    w->fused_ok = m.fused_ok != 0;
    w->cw.cfg = *cfg; w->cw.device = device; w->cw.dbuf = w->dbuf; w->cw.n_floats = w->n_floats;
    w->cw.has_cond = true; w->cw.cond_fast = m.cond.fast; w->cw.cond_unet = m.cond.unet;
    w->cw.cond = m.cond.Cw;
    w->cw.cond.base = w->dbuf;
    *out = w;
    return MCD_OK;
}

int mcd_latent_set_option(mcd_latent_weights_t* w, int32_t option, int32_t value) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (option < 0 || option >= MCD_LATENT_OPT_COUNT) return fail(MCD_EINVAL, "unknown latent option " + std::to_string(option));
    w->opt[option] = value;
    return MCD_OK;
}

void mcd_free_latent_weights(mcd_latent_weights_t* w) {
    if (!w) return;
    if (w->dbuf) (void)hipFree(w->dbuf);
    delete w;
}

int64_t mcd_latent_workspace_bytes(const mcd_latent_weights_t* w, int32_t n_windows) {
    if (!w || n_windows <= 0) return 0;
    return lat_ws_cond_bytes(n_windows) + lat_ws_z0_bytes(n_windows, w->net.D) + lat_ws_gather_bytes(w, n_windows) + lat_ws_plain_bytes(w, n_windows);
}

int mcd_latent_encode(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                      const float* step_table, float* cond_emb_out, float* z0_out, void* stream) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_windows <= 0) return MCD_OK;
    if (!data || !step_table || !cond_emb_out || !z0_out) return fail(MCD_EINVAL, "null argument");
    if (cfg->noise_steps < 2) return fail(MCD_EINVAL, "need noise_steps >= 2 (the table's row noise_steps holds t = -1)");
    hipStream_t st = (hipStream_t)stream;
    // no workspace argument here: the plain encoder's scratch comes from the stream-ordered allocator
    const int64_t need = lat_ws_gather_bytes(w, cfg->n_windows) + lat_ws_plain_bytes(w, cfg->n_windows);
    char* scratch = nullptr;
    if (need > 0) HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), (size_t)need, st));
    const int rc = latent_encode_impl(w, cfg, data, view, step_table, cond_emb_out, z0_out, scratch, st);
    if (scratch) {
        const hipError_t e = hipFreeAsync(scratch, st);
        if (rc == MCD_OK && e != hipSuccess) return fail(MCD_EDEVICE, std::string("hipFreeAsync: ") + hipGetErrorString(e));
    }
    return rc;
}

int mcd_latent_denoise(const mcd_latent_weights_t* w, const float* x, const float* cond, const float* step_table, int32_t t,
                       int32_t n_rows, float* eps_out, void* stream) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (n_rows <= 0) return MCD_OK;
    if (!x || !cond || !step_table || !eps_out) return fail(MCD_EINVAL, "null argument");
    if (t < 0) return fail(MCD_EINVAL, "t must be >= 0 (step_table needs at least t + 1 rows)");
    if (!aligned16(x) || !aligned16(eps_out)) return fail(MCD_EINVAL, "x and eps_out must be 16-byte aligned");
    LatentChainParams P;
    memset(&P, 0, sizeof(P));
    P.wbuf = w->dbuf; P.net = w->net; P.cond = cond; P.step_table = step_table; P.x_in = x; P.eps_out = eps_out;
    P.B = n_rows; P.S = 1; P.ns = t + 1; P.wpg = LAT_NC; P.mode = 1; P.step_single = t;
    return launch_latent_chain(P, (hipStream_t)stream);
}

int mcd_latent_score(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                     const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                     int32_t aggregation, float quantile, float* loss_agg, float* loss_all, float* latent_all, float* latent_code,
                     void* stream) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    const int B = cfg->n_windows, S = cfg->n_samples, D = w->net.D;
    if (B <= 0) return MCD_OK;
    if (!data || !step_table || !workspace) return fail(MCD_EINVAL, "null argument (the workspace of mcd_latent_workspace_bytes is required)");
    if (aggregation == MCD_AGGR_ALL) {
        if (!loss_all) return fail(MCD_EINVAL, "null argument");
    } else {
        if (!loss_agg) return fail(MCD_EINVAL, "null argument");
        if (aggregation != MCD_AGGR_BEST && aggregation != MCD_AGGR_WORST && aggregation != MCD_AGGR_MEAN && aggregation != MCD_AGGR_MEDIAN &&
            aggregation != MCD_AGGR_QUANTILE)
            return fail(MCD_EINVAL, "mcd_latent_score aggregates losses (best, worst, mean, median, quantile)");
        if (aggregation == MCD_AGGR_QUANTILE && !(quantile >= 0.f && quantile <= 1.f)) return fail(MCD_EINVAL, "quantile must be in [0, 1]");
    }
    if (S < 1 || cfg->noise_steps < 2) return fail(MCD_EINVAL, "need n_samples >= 1 and noise_steps >= 2");
    if (S > LAT_MAX_S) return fail(MCD_EUNSUPPORTED, "n_samples " + std::to_string(S) + ": at most " + std::to_string(LAT_MAX_S) + " per call");
    if ((long long)B * S > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x n_samples exceeds 2^31 - 1: score in smaller batches");
    if (cfg->loss_fn < MCD_LOSS_SMOOTH_L1 || cfg->loss_fn > MCD_LOSS_MSE) return fail(MCD_EINVAL, "unknown loss_fn");
    if (noise && !aligned16(noise)) return fail(MCD_EINVAL, "noise must be 16-byte aligned");
    if (!aligned16(workspace)) return fail(MCD_EINVAL, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* cond = reinterpret_cast<float*>(workspace);
    float* z0 = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + lat_ws_cond_bytes(B));
    char* scratch = reinterpret_cast<char*>(workspace) + lat_ws_cond_bytes(B) + lat_ws_z0_bytes(B, D);
    int rc = latent_encode_impl(w, cfg, data, view, step_table, cond, z0, scratch, st);
    if (rc != MCD_OK) return rc;
    LatentChainParams P;
    memset(&P, 0, sizeof(P));
    P.wbuf = w->dbuf; P.net = w->net; P.cond = cond; P.z0 = z0; P.noise = noise; P.step_table = step_table;
    P.loss_agg = aggregation == MCD_AGGR_ALL ? nullptr : loss_agg; P.loss_all = loss_all; P.latent_all = latent_all; P.latent_code = latent_code;
    P.seed = seed; P.first_window = first_window_id;
    P.B = B; P.S = S; P.ns = cfg->noise_steps; P.wpg = S >= LAT_NC ? 1 : LAT_NC / S;
    P.mode = 0; P.loss_fn = cfg->loss_fn; P.aggr = aggregation; P.aggr_q = quantile;
    return launch_latent_chain(P, st);
}

int mcd_latent_philox_noise(uint64_t seed, int64_t first_window_id, int32_t n_windows, int32_t n_samples, int32_t noise_steps,
                            int32_t latent_dim, float* noise_out, void* stream) {
    if (n_windows <= 0) return MCD_OK;
    if (!noise_out) return fail(MCD_EINVAL, "null argument");
    if (n_samples < 1 || noise_steps < 2 || !latent_dim_ok(latent_dim)) return fail(MCD_EINVAL, "bad sizes");
    if (!aligned16(noise_out)) return fail(MCD_EINVAL, "noise_out must be 16-byte aligned");
    const int K = noise_steps > 2 ? noise_steps - 1 : 1;
    return launch_latent_philox(seed, first_window_id, n_windows, n_samples, K, latent_dim, noise_out, (hipStream_t)stream);
}

}  // extern "C"

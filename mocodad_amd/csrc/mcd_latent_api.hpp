// mcd_latent_api.hpp — host side of the MoCoDADlatent entry points (include/mocodad_hip.h): the handle and the calls around the
// launchers of mcd_latent.hip.  Included at the end of mcd_api.hip, whose upload helper and condition-encoder routes it shares; the
// front end of a call (view, checks, workspace layout, launch_cond) is mcd_call.hpp, the packers pack_latent_model / pack_latent_ae_model
// of mcd_pack.hpp.  A handle is of one of two kinds: diffusion stage (mcd_latent_score, mcd_latent_denoise) or autoencoder (stage
// 'pretrain': mcd_latent_reconstruct, mcd_latent_decode_samples); mcd_latent_encode, the workspace size, the options and the release
// take both.
// It holds no device code.
#pragma once
#include "mcd_latent.hpp"

struct mcd_latent_weights {
    mcd_model_cfg_t cfg;
    int device;
    float* dbuf;
    size_t n_floats;
    mcd::LatentNet net;
    bool fused_ok;        // cond_fast_body's table is packed and t_cond = t_unet: the encode launch can run the condition encoder itself
    int h_floats;         // per window: the last encoder layer's output H that the encode launch leaves for latent_project_kernel; 0 = the
                          // encode launch computes z0 itself (3 corrupt frames)
    bool ae;              // the autoencoder of stage 'pretrain' (mcd_pack_latent_ae_weights): decoder tables, no denoiser
    int g_floats;         // ... per window: rev_to_time_dim's output G for latent_decode_kernel (it takes H's place once z0 is formed); else 0
    mcd_weights cw;       // the condition encoder as the pose model's launchers take it: dbuf, cond and the cond_* flags; nothing else is set
    int opt[MCD_LATENT_OPT_COUNT];
};

namespace {

using namespace mcd;

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The regions of a latent call's workspace (latent_workspace) from its base pointer: cond_emb, z0, the plain encoder's gather and
// third buffer, H / G.  origin: the layout offset `base` stands for (mcd_latent_encode allocates the part from `gather` on); a
// region in front of it, or any region of a null base, is null.
struct LatentRegions { float *cond, *z0, *gather, *plain, *h; };
LatentRegions latent_regions(void* base, const LatentWorkspace& lay, int64_t origin = 0) {
    auto at = [&](int64_t off) { return base && off >= origin ? reinterpret_cast<float*>(static_cast<char*>(base) + (off - origin)) : nullptr; };
    return {at(0), at(lay.z0), at(lay.gather), at(lay.plain), at(lay.h)};
}

// cfg, view and step_table of a call against the handle -> what the launches take
int latent_call(const mcd_latent_weights* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                const float* step_table, LatentCall& c) {
    if (int rc = window_view(data, view, cfg->seg_len, c.dv)) return rc;
    if (cfg->n_corrupt != w->cfg.t_unet || cfg->n_cond != w->cfg.t_cond) return fail(MCD_EINVAL, "frame split does not match the packed model (t_unet / t_cond)");
    if (int rc = check_frame_partition(cfg)) return rc;
    if (int rc = check_frame_lists(cfg)) return rc;
    memset(&c.cond_fi, 0, sizeof(c.cond_fi));
    memset(&c.fi, 0, sizeof(c.fi));
    for (int k = 0; k < cfg->n_cond; ++k) c.cond_fi.idx[k] = cfg->cond_idx[k];
    for (int k = 0; k < cfg->n_corrupt; ++k) c.fi.idx[k] = cfg->corrupt_idx[k];
    c.seg_len = cfg->seg_len;
    // row ns of the table: the constant time step -1 the encoder is given (mocodad_latent.py:95)
    c.pe_row = step_table + (size_t)cfg->noise_steps * (4 + EDIM) + 4;
    return MCD_OK;
}

// [condition encoder] -> encode -> [project]: cond_emb (B,16) and z0 (B,D) of B windows.  R: the scratch regions gather / plain / h
// (null where the handle's route has none)
int latent_encode_impl(const mcd_latent_weights* w, const LatentCall& c, int B, float* cond_out, float* z0_out, const LatentRegions& R,
                       hipStream_t st) {
    // the pose model's routes: in the encode launch (shipped encoder at t_cond = t_unet), or a launch of its own in front of it
    const CondRoute route = cond_route(&w->cw, w->fused_ok && !w->opt[MCD_LATENT_OPT_SPLIT_ENCODE]);
    const bool plain_route = route == COND_PLAIN || route == COND_PLAIN_SCRATCH;
    if (route != COND_INKERNEL && route != COND_FAST && route != COND_UNET && !plain_route)      // (a developer build without the frame count)
        return fail(MCD_EUNSUPPORTED, "E_unet condition encoder: frame count not instantiated");
    if (plain_route && !R.gather) return fail(MCD_EINVAL, "workspace required (mcd_latent_workspace_bytes) for this condition encoder");
    if (route != COND_INKERNEL)
        if (int rc = launch_cond(&w->cw, route, c.dv, c.cond_fi, c.seg_len, cond_out, B, R.gather, R.plain, st)) return rc;
    if (!w->h_floats) return launch_latent_encode(w->cfg.t_unet, {w->dbuf, c, route == COND_INKERNEL, cond_out, z0_out, w->net.D, B, st});
    // 5 .. 12 corrupt frames: the encode launch leaves H, one projection launch computes every window's z0
    if (!R.h) return fail(MCD_EINVAL, "workspace required (mcd_latent_workspace_bytes) for this frame count");
    if (int rc = launch_latent_encode(w->cfg.t_unet, {w->dbuf, c, false, cond_out, R.h, w->net.D, B, st})) return rc;
    return launch_latent_project(w->cfg.t_unet, w->dbuf, R.h, z0_out, w->net.D, B, st);
}

// a packer's result (rc, m) -> the uploaded handle; ae: the autoencoder's kind
int make_latent_weights(int rc, const PackedModel& m, const mcd_model_cfg_t* cfg, int32_t device, bool ae, mcd_latent_weights_t** out) {
    if (rc != MCD_OK) return rc;
    float* dbuf = nullptr;
    rc = upload_packed(m.buf, device, &dbuf);
    if (rc != MCD_OK) return rc;
    mcd_latent_weights* w = new mcd_latent_weights();
    w->cfg = *cfg; w->device = device; w->n_floats = m.buf.size(); w->net = m.net; w->dbuf = dbuf;
    memset(w->opt, 0, sizeof(w->opt));
    w->fused_ok = m.fused_ok != 0;
    w->h_floats = latent_project_in_kernel(cfg->t_unet) ? 0 : LAT_ENC_C * cfg->t_unet * 10;
    w->ae = ae; w->g_floats = ae ? LAT_ENC_C * cfg->t_unet * 10 : 0;
    w->cw.cfg = *cfg; w->cw.device = device; w->cw.dbuf = w->dbuf; w->cw.n_floats = w->n_floats;
    memset(w->cw.opt, 0, sizeof(w->cw.opt));
    set_cond_weights(&w->cw, m, dbuf);
    *out = w;
    return MCD_OK;
}

// ---- mcd_latent_decode_samples: G = rev_to_time_dim of every latent row is 640 t_unet floats per row (315 MB at 1024 windows x 10
// samples x 12 frames), so the call walks the batch in chunks of windows -- unproject + decode per chunk, on the one stream -- and G
// never exceeds LAT_DECODE_G_BYTES.  A row of G belongs to one window and one sample: the chunking changes no bit.
constexpr int64_t LAT_DECODE_G_BYTES = 256ll << 20;
// bytes of G per window (S rows)
int64_t decode_window_bytes(const mcd_latent_weights* w, int64_t S) { return S * w->g_floats * 4; }
// the most windows a chunk may hold (>= 1: S <= LAT_MAX_S rows of a window are 31 MB at 12 frames): what the bound holds, or the
// value of MCD_LATENT_OPT_DECODE_CHUNK if that is smaller
int64_t decode_chunk_max(const mcd_latent_weights* w, int64_t S) {
    const int64_t n = std::max<int64_t>(1, LAT_DECODE_G_BYTES / decode_window_bytes(w, S));
    const int forced = w->opt[MCD_LATENT_OPT_DECODE_CHUNK];
    return forced > 0 ? std::min<int64_t>(n, forced) : n;
}
// the G region the size query reserves: every row while that stays under the bound (and under the forced chunk), else the bound --
// monotone in both arguments, and never less than the largest chunk of the call
int64_t decode_g_bytes(const mcd_latent_weights* w, int64_t B, int64_t S) {
    const int forced = w->opt[MCD_LATENT_OPT_DECODE_CHUNK];
    const int64_t rows_of = forced > 0 ? std::min<int64_t>(B, forced) : B;
    return std::min(rows_of * decode_window_bytes(w, S), LAT_DECODE_G_BYTES);
}

// ---- mcd_latent_score_pose: the workspace of a diffusion-stage handle w and its decoder ae (latent_pose_workspace): the size query
// and the call read this one function
LatentPoseWorkspace latent_pose_layout(const mcd_latent_weights* w, const mcd_latent_weights* ae, int64_t B, int64_t S) {
    return latent_pose_workspace(latent_workspace(&w->cw, B, w->net.D, w->h_floats).bytes,
                                 latent_decode_workspace(&ae->cw, B, decode_g_bytes(ae, B, S)).bytes, B, S, w->net.D, w->cfg.t_unet);
}

}  // namespace

extern "C" {

int mcd_pack_latent_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, const mcd_latent_cfg_t* lcfg,
                            int32_t device, mcd_latent_weights_t** out) {
    if (!tensors || !cfg || !lcfg || !out) return fail(MCD_EINVAL, "null argument");
    PackedModel m;
    return make_latent_weights(pack_latent_model(tensors, n_tensors, cfg, lcfg, m), m, cfg, device, false, out);
}

int mcd_pack_latent_ae_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, int32_t latent_dim,
                               int32_t device, mcd_latent_weights_t** out) {
    if (!tensors || !cfg || !out) return fail(MCD_EINVAL, "null argument");
    PackedModel m;
    return make_latent_weights(pack_latent_ae_model(tensors, n_tensors, cfg, latent_dim, m), m, cfg, device, true, out);
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
    return latent_workspace(&w->cw, n_windows, w->net.D, std::max(w->h_floats, w->g_floats)).bytes;
}

int mcd_latent_encode(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                      const float* step_table, float* cond_emb_out, float* z0_out, void* stream) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_windows <= 0) return MCD_OK;
    if (!data || !step_table || !cond_emb_out || !z0_out) return fail(MCD_EINVAL, "null argument");
    if (cfg->noise_steps < 2) return fail(MCD_EINVAL, "need noise_steps >= 2 (the table's row noise_steps holds t = -1)");
    // 5 .. 12 corrupt frames: latent_project_kernel writes z0 with 16-byte stores (the 3-frame encode launch stores single floats;
    // mcd_latent_score's z0 is a region of its 16-byte aligned workspace)
    if (w->h_floats && !aligned16(z0_out)) return fail(MCD_EINVAL, "z0_out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    // no workspace argument here: the plain encoder's scratch and H come from the stream-ordered allocator
    const LatentWorkspace lay = latent_workspace(&w->cw, cfg->n_windows, w->net.D, w->h_floats);      // (no G: nothing decodes here)
    const int64_t need = lay.bytes - lay.gather;
    char* scratch = nullptr;
    if (need > 0) HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), (size_t)need, st));
    LatentCall c;
    int rc = latent_call(w, cfg, data, view, step_table, c);
    if (rc == MCD_OK) rc = latent_encode_impl(w, c, cfg->n_windows, cond_emb_out, z0_out, latent_regions(scratch, lay, lay.gather), st);
    if (scratch) {
        const hipError_t e = hipFreeAsync(scratch, st);
        if (rc == MCD_OK && e != hipSuccess) return fail(MCD_EDEVICE, std::string("hipFreeAsync: ") + hipGetErrorString(e));
    }
    return rc;
}

int mcd_latent_denoise(const mcd_latent_weights_t* w, const float* x, const float* cond, const float* step_table, int32_t t,
                       int32_t n_rows, float* eps_out, void* stream) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (w->ae) return fail(MCD_EUNSUPPORTED, "mcd_latent_denoise needs a diffusion-stage handle (mcd_pack_latent_weights): an autoencoder handle has no denoiser");
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
    if (w->ae) return fail(MCD_EUNSUPPORTED, "mcd_latent_score needs a diffusion-stage handle (mcd_pack_latent_weights): an autoencoder handle has no denoiser");
    const int B = cfg->n_windows, S = cfg->n_samples, D = w->net.D;
    if (B <= 0) return MCD_OK;
    if (!data || !step_table || !workspace) return fail(MCD_EINVAL, "null argument (the workspace of mcd_latent_workspace_bytes is required)");
    if (aggregation == MCD_AGGR_ALL) {
        if (!loss_all) return fail(MCD_EINVAL, "null argument");
    } else {
        if (!loss_agg) return fail(MCD_EINVAL, "null argument");
        if (int rc = check_aggregation(aggregation, quantile, AGGR_LOSSES, "mcd_latent_score aggregates losses (best, worst, mean, median, quantile)")) return rc;
    }
    if (S < 1 || cfg->noise_steps < 2) return fail(MCD_EINVAL, "need n_samples >= 1 and noise_steps >= 2");
    if (S > LAT_MAX_S) return fail(MCD_EUNSUPPORTED, "n_samples " + std::to_string(S) + ": at most " + std::to_string(LAT_MAX_S) + " per call");
    if ((long long)B * S > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x n_samples exceeds 2^31 - 1: score in smaller batches");
    if (cfg->loss_fn < MCD_LOSS_SMOOTH_L1 || cfg->loss_fn > MCD_LOSS_MSE) return fail(MCD_EINVAL, "unknown loss_fn");
    if (noise && !aligned16(noise)) return fail(MCD_EINVAL, "noise must be 16-byte aligned");
    if (!aligned16(workspace)) return fail(MCD_EINVAL, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const LatentWorkspace lay = latent_workspace(&w->cw, B, D, w->h_floats);
    const LatentRegions R = latent_regions(workspace, lay);
    LatentCall c;
    if (int rc = latent_call(w, cfg, data, view, step_table, c)) return rc;
    if (int rc = latent_encode_impl(w, c, B, R.cond, R.z0, R, st)) return rc;
    LatentChainParams P;
    memset(&P, 0, sizeof(P));
    P.wbuf = w->dbuf; P.net = w->net; P.cond = R.cond; P.z0 = R.z0; P.noise = noise; P.step_table = step_table;
    P.loss_agg = aggregation == MCD_AGGR_ALL ? nullptr : loss_agg; P.loss_all = loss_all; P.latent_all = latent_all; P.latent_code = latent_code;
    P.seed = seed; P.first_window = first_window_id;
    P.B = B; P.S = S; P.ns = cfg->noise_steps; P.wpg = S >= LAT_NC ? 1 : LAT_NC / S;
    P.mode = 0; P.loss_fn = cfg->loss_fn; P.aggr = aggregation; P.aggr_q = quantile;
    return launch_latent_chain(P, st);
}

int mcd_latent_reconstruct(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                           const float* step_table, void* workspace, const float* z_in, float* pose_out, float* loss_out,
                           float* cond_emb_out, float* z0_out, void* stream) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    if (!w->ae) return fail(MCD_EUNSUPPORTED, "mcd_latent_reconstruct needs an autoencoder handle (mcd_pack_latent_ae_weights): a diffusion-stage handle has no decoder");
    const int B = cfg->n_windows, D = w->net.D, T = w->cfg.t_unet;
    if (B <= 0) return MCD_OK;
    if (!data || !step_table || !workspace) return fail(MCD_EINVAL, "null argument (the workspace of mcd_latent_workspace_bytes is required)");
    if (cfg->noise_steps < 2) return fail(MCD_EINVAL, "need noise_steps >= 2 (the table's row noise_steps holds t = -1)");
    if (cfg->loss_fn < MCD_LOSS_SMOOTH_L1 || cfg->loss_fn > MCD_LOSS_MSE) return fail(MCD_EINVAL, "unknown loss_fn");
    if (z_in && !aligned16(z_in)) return fail(MCD_EINVAL, "z_in must be 16-byte aligned");
    if (!aligned16(workspace)) return fail(MCD_EINVAL, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const LatentWorkspace lay = latent_workspace(&w->cw, B, D, std::max(w->h_floats, w->g_floats));
    const LatentRegions R = latent_regions(workspace, lay);      // (R.h: H of the encode launch, then G of the unproject launch)
    LatentCall c;
    if (int rc = latent_call(w, cfg, data, view, step_table, c)) return rc;
    if (int rc = latent_encode_impl(w, c, B, R.cond, R.z0, R, st)) return rc;
    if (pose_out || loss_out) {
        if (int rc = launch_latent_unproject(T, w->dbuf, z_in ? z_in : R.z0, R.h, D, B, st)) return rc;
        if (int rc = launch_latent_decode(T, {w->dbuf, c, R.cond, R.h, pose_out, loss_out, cfg->loss_fn, B, st})) return rc;
    }
    if (cond_emb_out) HIP_TRY(hipMemcpyAsync(cond_emb_out, R.cond, (size_t)B * EDIM * 4, hipMemcpyDeviceToDevice, st));
    if (z0_out) HIP_TRY(hipMemcpyAsync(z0_out, R.z0, (size_t)B * D * 4, hipMemcpyDeviceToDevice, st));
    return MCD_OK;
}

int64_t mcd_latent_decode_workspace_bytes(const mcd_latent_weights_t* w, int32_t n_windows, int32_t n_samples) {
    if (!w || !w->ae || n_windows <= 0 || n_samples < 1 || n_samples > LAT_MAX_S) return 0;
    return latent_decode_workspace(&w->cw, n_windows, decode_g_bytes(w, n_windows, n_samples)).bytes;
}

int mcd_latent_decode_samples(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                              const float* step_table, void* workspace, const float* cond_emb_in, const float* latents, float* pose_all,
                              float* loss_all, void* stream) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    if (!w->ae) return fail(MCD_EUNSUPPORTED, "mcd_latent_decode_samples needs an autoencoder handle (mcd_pack_latent_ae_weights): a diffusion-stage handle has no decoder");
    const int B = cfg->n_windows, S = cfg->n_samples, D = w->net.D, T = w->cfg.t_unet;
    if (B <= 0) return MCD_OK;
    if (!data || !step_table || !workspace) return fail(MCD_EINVAL, "null argument (the workspace of mcd_latent_decode_workspace_bytes is required)");
    if (!latents || !loss_all) return fail(MCD_EINVAL, "null argument (latents and loss_all are required)");
    if (S < 1) return fail(MCD_EINVAL, "need n_samples >= 1");
    if (S > LAT_MAX_S) return fail(MCD_EUNSUPPORTED, "n_samples " + std::to_string(S) + ": at most " + std::to_string(LAT_MAX_S) + " per call");
    if ((long long)B * S > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x n_samples exceeds 2^31 - 1: decode in smaller batches");
    if (cfg->noise_steps < 2) return fail(MCD_EINVAL, "need noise_steps >= 2 (the table's row noise_steps holds t = -1)");
    if (cfg->loss_fn < MCD_LOSS_SMOOTH_L1 || cfg->loss_fn > MCD_LOSS_MSE) return fail(MCD_EINVAL, "unknown loss_fn");
    if (!aligned16(latents)) return fail(MCD_EINVAL, "latents must be 16-byte aligned");
    if (!aligned16(workspace)) return fail(MCD_EINVAL, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    LatentCall c;
    if (int rc = latent_call(w, cfg, data, view, step_table, c)) return rc;
    const LatentDecodeWorkspace lay = latent_decode_workspace(&w->cw, B, decode_g_bytes(w, B, S));
    auto at = [&](int64_t off) { return reinterpret_cast<float*>(static_cast<char*>(workspace) + off); };
    const float* cond = cond_emb_in;
    if (!cond) {      // the handle's own condition encoder, as the launch in front of the encode launch (latent_encode_impl)
        const CondRoute route = cond_route(&w->cw);
        const bool plain_route = route == COND_PLAIN || route == COND_PLAIN_SCRATCH;
        if (route != COND_FAST && route != COND_UNET && !plain_route)
            return fail(MCD_EUNSUPPORTED, "E_unet condition encoder: frame count not instantiated");
        if (int rc = launch_cond(&w->cw, route, c.dv, c.cond_fi, c.seg_len, at(0), B, plain_route ? at(lay.gather) : nullptr,
                                 plain_route ? at(lay.plain) : nullptr, st)) return rc;
        cond = at(0);
    }
    // chunks of equal size (the last one may be shorter), none above decode_chunk_max
    const int64_t cmax = decode_chunk_max(w, S), n_chunks = (B + cmax - 1) / cmax;
    const int chunk = (int)((B + n_chunks - 1) / n_chunks);
    float* const G = at(lay.g);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        if (int rc = launch_latent_unproject(T, w->dbuf, latents + (size_t)b0 * S * D, G, D, nb * S, st)) return rc;
        if (int rc = launch_latent_decode_samples(T, {w->dbuf, c, cond, G, pose_all, loss_all, cfg->loss_fn, b0, nb, B, S,
                                                      w->opt[MCD_LATENT_OPT_DECODE_SPW], st})) return rc;
    }
    return MCD_OK;
}

int64_t mcd_latent_pose_workspace_bytes(const mcd_latent_weights_t* w, const mcd_latent_weights_t* ae, int32_t n_windows, int32_t n_samples) {
    if (n_windows <= 0 || n_samples < 1 || n_samples > LAT_MAX_S || !w || !ae || w->ae || !ae->ae) return 0;
    return latent_pose_layout(w, ae, n_windows, n_samples).bytes;
}

int mcd_latent_score_pose(const mcd_latent_weights_t* w, const mcd_latent_weights_t* ae, const mcd_score_cfg_t* cfg, const float* data,
                          const mcd_window_view_t* view, const float* noise, uint64_t seed, int64_t first_window_id,
                          const float* step_table, void* workspace, int32_t aggregation, float quantile, float* loss_agg,
                          float* loss_all, float* pose_all, float* pose_agg, float* maps, float* latent_all, void* stream) {
    // every check of the four calls below comes here, before the first launch
    if (!cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_windows <= 0) return MCD_OK;      // (before anything else is read, the handles included)
    if (!w || !ae) return fail(MCD_EINVAL, "null argument (two handles: the diffusion stage and its autoencoder)");
    if (w->ae) return fail(MCD_EUNSUPPORTED, "mcd_latent_score_pose needs a diffusion-stage handle (mcd_pack_latent_weights) as its first handle: an autoencoder handle has no denoiser");
    if (!ae->ae) return fail(MCD_EUNSUPPORTED, "mcd_latent_score_pose needs an autoencoder handle (mcd_pack_latent_ae_weights) as its second handle: a diffusion-stage handle has no decoder");
    const int B = cfg->n_windows, S = cfg->n_samples, D = w->net.D;
    if (!data || !step_table || !workspace) return fail(MCD_EINVAL, "null argument (the workspace of mcd_latent_pose_workspace_bytes is required)");
    if (!loss_agg) return fail(MCD_EINVAL, "null argument (loss_agg is required)");
    if (int rc = check_aggregation(aggregation, quantile, AGGR_LOSSES, "mcd_latent_score_pose aggregates losses (best, worst, mean, median, quantile)")) return rc;
    if (pose_agg && aggregation != MCD_AGGR_BEST && aggregation != MCD_AGGR_WORST)
        return fail(MCD_EINVAL, "pose_agg: only best and worst select a pose");
    if (S < 1 || cfg->noise_steps < 2) return fail(MCD_EINVAL, "need n_samples >= 1 and noise_steps >= 2");
    if (S > LAT_MAX_S) return fail(MCD_EUNSUPPORTED, "n_samples " + std::to_string(S) + ": at most " + std::to_string(LAT_MAX_S) + " per call");
    if ((long long)B * S > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x n_samples exceeds 2^31 - 1: score in smaller batches");
    if (cfg->loss_fn < MCD_LOSS_SMOOTH_L1 || cfg->loss_fn > MCD_LOSS_MSE) return fail(MCD_EINVAL, "unknown loss_fn");
    // the two handles are the two stages of one model
    if (ae->cfg.t_unet != w->cfg.t_unet || ae->cfg.t_cond != w->cfg.t_cond)
        return fail(MCD_EINVAL, "the two handles differ in their frame split (t_unet / t_cond)");
    if (ae->net.D != D) return fail(MCD_EINVAL, "the two handles differ in latent_dim");
    if (ae->device != w->device) return fail(MCD_EINVAL, "the two handles are on different devices");
    if (noise && !aligned16(noise)) return fail(MCD_EINVAL, "noise must be 16-byte aligned");
    if (!aligned16(workspace)) return fail(MCD_EINVAL, "workspace must be 16-byte aligned");
    if (latent_all && !aligned16(latent_all)) return fail(MCD_EINVAL, "latent_all must be 16-byte aligned (the decode launches read it)");
    if (view && view->cond_mask) return fail(MCD_EINVAL, "cond_mask: the latent model has fixed frame lists");
    {   // the frame lists and the view, against both handles (seg_len and the lists are the call's: one cfg serves both)
        LatentCall c;
        if (int rc = latent_call(w, cfg, data, view, step_table, c)) return rc;
        if (int rc = latent_call(ae, cfg, data, view, step_table, c)) return rc;
    }
    const LatentPoseWorkspace lay = latent_pose_layout(w, ae, B, S);
    auto at = [&](int64_t off) { return reinterpret_cast<float*>(static_cast<char*>(workspace) + off); };
    float* const la = loss_all ? loss_all : at(lay.loss);
    float* const lat = latent_all ? latent_all : at(lay.latent);
    float* const pa = pose_all ? pose_all : (pose_agg || maps) ? at(lay.pose) : nullptr;
    // 1. the chain call: latents into `lat`, cond_emb at the head of the workspace (`la` takes the latent-space losses until step 2)
    if (int rc = mcd_latent_score(w, cfg, data, view, noise, seed, first_window_id, step_table, workspace, MCD_AGGR_ALL, 0.f, nullptr, la,
                                  lat, nullptr, stream)) return rc;
    // 2. the decoder on every sample, with that cond_emb: the pose-space losses, and the poses where something reads them
    if (int rc = mcd_latent_decode_samples(ae, cfg, data, view, step_table, at(lay.decode), at(0), lat, pa, la, stream)) return rc;
    // 3. the pose model's aggregation (losses only: no ground truth is read)
    if (int rc = mcd_aggregate_view(cfg, C0, 17, aggregation, quantile, la, pa, nullptr, nullptr, loss_agg, pose_agg, stream)) return rc;
    // 4. the error maps under that aggregation
    if (maps) return mcd_error_maps(cfg, C0, 17, aggregation, quantile, la, pa, data, view, maps, stream);
    return MCD_OK;
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

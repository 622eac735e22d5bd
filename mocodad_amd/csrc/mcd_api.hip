// mcd_api.hip — host side of libmocodad_hip.so: the C ABI of include/mocodad_hip.h, the upload of a packed model, and dispatch to
// the kernel instantiations of mcd_inst.hip (declared `extern template` in mcd_launch.hpp; every switch over frame counts is an
// expansion of the tables of mcd_instances.hpp, and which kernel family serves a handle is decided by unet_route() / cond_route()
// alone: entry points, launches and workspace sizing ask them).  Host code only -- routes, launches, ABI -- around these headers:
//   mcd_post_kernel.hpp      this file's own kernels (aggregation, frame scores, pose normalisation, forecast tracks, the exported
//                            Philox draws, gather, LDS poison) and their parameter blocks
//   mcd_stream_kernel.hpp    the kernels of a live stream (track, score, joint and forecast rings, online clip scores)
//   mcd_stream_api.hpp       ... and their entry points mcd_stream_*, included behind this file's own (no device code)
//   mcd_generic_kernel.hpp   the runtime-shape kernels (cond_encode_kernel, score_generic_kernel, cond_unet_generic_kernel)
//   mcd_pack.hpp             the weight packer (BatchNorm folding, MFMA fragment order)
//   mcd_call.hpp             the front end of a scoring call, shared with the latent entry points (mcd_latent_api.hpp, included
//                            at the end): window view, frame-list and aggregation checks, workspace layouts, launch_cond
// The device code shared by the trajectory kernels is mcd_chain.hpp (what a chain is) and mcd_device.hpp (stage functions, LDS plan); the kernels themselves are
// mcd_score_kernel.hpp (1 .. 12 U-Net frames) and mcd_tiled_kernel.hpp (13 .. 32).  See DESIGN.md section 2.

#include <algorithm>
#include "mcd_launch.hpp"
#include "mcd_generic_kernel.hpp"
#include "mcd_pack.hpp"

#if MCD_NWAVES != 8 && !defined(MCD_FAST_T)      // (developer builds pass one flag set to every file)
#error "mcd_api.hip is built with the default wave count: per-unit wave counts belong to mcd_inst.hip (MCD_UNIT_FLAGS_<n>)"
#endif
namespace { constexpr int API_THREADS = 512; }      // block size of this file's own kernels
#pragma GCC poison NWAVES NTHREADS                  // (translation-unit constants of the kernel units: see mcd_launch.hpp)

using namespace mcd;

#include "mcd_post_kernel.hpp"      // this file's own kernels ...
#include "mcd_stream_kernel.hpp"    // ... and those of the live-stream entries; everything below is host code

namespace {

// Dispatch to the launchers of mcd_inst.hip is generated from the tables of mcd_instances.hpp (this file only CALLS launchers).
// score_kernel<T, ...>: the production form (or, in a build that holds tuning variants, the workgroup shape MCD_OPT_VARIANT
// names); layer_test: the form behind mcd_layer_forward
int launch_score(const mcd_weights* w, int T, ScoreParams& P, hipStream_t st, bool* fused = nullptr, bool layer_test = false) {
    if (!layer_test) {
        P.force_split = w->opt[MCD_OPT_SPLIT];
        const int variant = w->opt[MCD_OPT_VARIANT];
        if (variant != 0 && !score_has_variants()) return fail(MCD_EUNSUPPORTED, "MCD_OPT_VARIANT needs a -DMCD_TUNING_VARIANTS build");
#define MCD_CASE(unit, V, T_, NB, MINW) if (T == T_ && variant == V) return launch_score_t<T_, NB, MINW>(P, st, fused);
        MCD_SCORE_VARIANT_INSTANCES(MCD_CASE)
#undef MCD_CASE
    }
    switch (layer_test ? -T : T) {
#define MCD_CASE(unit, T_, NB, MINW, LT) case (LT ? -T_ : T_): return launch_score_t<T_, NB, MINW, LT>(P, st, fused);
        MCD_SCORE_INSTANCES(MCD_CASE)
#undef MCD_CASE
        default: break;
    }
    if (layer_test) return fail(MCD_EUNSUPPORTED, "mcd_layer_forward: no layer-test kernel for " + std::to_string(T) + " U-Net frames (the LT rows of mcd_instances.hpp)");
    return fail(MCD_EUNSUPPORTED, "U-Net frame count " + std::to_string(T) + " not instantiated (MCD_SCORE_INSTANCES, mcd_instances.hpp)");
}

// T_c -> NB of the MFMA condition encoders (the chains-per-workgroup of the trajectory kernels' LDS plans)
#define MCD_COND_CASE(fn, unit, T, NB) case T: return fn<T, NB>(w, data, fi, seg_len, emb, B, st);
int launch_cond_fast(const mcd_weights* w, const DataView& data, const FrameIdx& fi, int seg_len, float* emb, int B, hipStream_t st) {
    switch (w->cond.Tc) {
#define MCD_CASE(unit, T, NB) MCD_COND_CASE(launch_cond_fast_t, unit, T, NB)
        MCD_COND_FAST_INSTANCES(MCD_CASE)
#undef MCD_CASE
        default: break;
    }
    return fail(MCD_EUNSUPPORTED, "cond_fast: frame count not instantiated");
}
int launch_cond_unet(const mcd_weights* w, const DataView& data, const FrameIdx& fi, int seg_len, float* emb, int B, hipStream_t st) {
    switch (w->cond.Tc) {
#define MCD_CASE(unit, T, NB) MCD_COND_CASE(launch_cond_unet_t, unit, T, NB)
        MCD_COND_UNET_INSTANCES(MCD_CASE)
#undef MCD_CASE
        default: break;
    }
    return fail(MCD_EUNSUPPORTED, "E_unet condition encoder: frame count not instantiated");
}
constexpr int GEN_MAX_WGS = 2048;       // persistent grid of the runtime-shape kernels (8 workgroups of 4 waves per CU)
int64_t gen_scratch_bytes(int64_t units, int T) {
    const int64_t wgs = units < GEN_MAX_WGS ? units : GEN_MAX_WGS;
    return wgs * (int64_t)GEN_SLAB * T * 4;
}
int launch_score_generic(const mcd_weights* w, const ScoreParams& P, const FrameMaps& M, float* scratch, hipStream_t st) {
    const int T = w->cfg.t_unet;
    const int wgs = P.n_chains < GEN_MAX_WGS ? P.n_chains : GEN_MAX_WGS;
    const size_t lds = (size_t)GenericLds(T).floats() * 4;
    hipLaunchKernelGGL(score_generic_kernel, dim3(wgs), dim3(GEN_THREADS), lds, st, P, M, w->gen, T, scratch);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}
int tiled_wgs(const mcd_weights* w, int64_t chains, int TP) {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, w->device);     // the handle's device, whatever the caller's current one
    if (cus < 1) cus = 256;
    const int64_t units = (chains + tl_nb(TP) - 1) / tl_nb(TP);
    cus *= tl_wgs_per_cu(TP);
    return (int)(units < cus ? units : cus);         // one workgroup per CU (110 - 135 KB of LDS), persistent over the chains
}
int64_t tiled_scratch_bytes(const mcd_weights* w, int64_t chains, int TP) { return (int64_t)tiled_wgs(w, chains, TP) * tl_slab_floats(TP * tl_nb(TP)) * 4; }
int launch_score_tiled(const mcd_weights* w, const ScoreParams& P, const FrameMaps& M, float* scratch, hipStream_t st, bool layer_test = false) {
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != w->device) return fail(MCD_EINVAL, "the current device is not the handle's device (the workspace slabs are sized for it)");
    const int wgs = tiled_wgs(w, P.n_chains, w->tiled_tp);
    switch (layer_test ? -w->tiled_tp : w->tiled_tp) {
#define MCD_CASE(unit, TP, NB, LT) case (LT ? -TP : TP): return launch_score_tiled_t<TP, NB, LT>(w, P, M, scratch, wgs, st);
        MCD_TILED_INSTANCES(MCD_CASE)
#undef MCD_CASE
        default: return fail(MCD_EUNSUPPORTED, "tiled kernel: frame count");
    }
}
// plain condition encoder (any channel list; 21 .. 31 condition frames of the shipped one).  scratch: cond_scratch_bytes() of
// global memory when three LDS buffers do not fit (W.gmode), else unused
constexpr int CE_MAX_WGS = 512;
int launch_cond_plain(const mcd_weights* w, const float* cond_data, int B, float* emb, float* scratch, hipStream_t st) {
    const bool g = w->cond.gmode != 0;
    if (g && !scratch) return fail(MCD_EINVAL, "workspace required (mcd_score_workspace_bytes) for this many condition frames");
    const size_t lds = w->cond.lds_floats() * 4;
    LDS_LIMIT(&cond_encode_kernel, (size_t)160 * 1024);
    const int wgs = g && B > CE_MAX_WGS ? CE_MAX_WGS : B;
    hipLaunchKernelGGL(cond_encode_kernel, dim3(wgs), dim3(CE_THREADS), lds, st, w->cond, cond_data, emb, B, g ? scratch : nullptr);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}
// Which kernel family serves a handle, decided here and nowhere else: the entry points, the launches and the workspace sizing
// below all ask these two functions.
enum UnetRoute { UNET_KERNEL, UNET_TILED, UNET_GENERIC };      // score_kernel<T,...> | score_tiled_kernel | score_generic_kernel
UnetRoute unet_route(const mcd_weights* w, bool honour_option = true) {
    if (honour_option && w->opt[MCD_OPT_GENERIC_UNET]) return UNET_GENERIC;
    return w->fast_unet ? UNET_KERNEL : w->tiled_tp ? UNET_TILED : UNET_GENERIC;
}
enum CondRoute {
    COND_NONE,              // the model has no condition encoder
    COND_INKERNEL,          // shipped architecture, inside the trajectory kernel
    COND_FAST,              // ... as its own launch: cond_fast_kernel
    COND_UNET,              // 'E_unet': cond_unet_kernel
    COND_TILED,             // 'E_unet' at a frame count of the slab-tiled kernel: its COND form
    COND_UNET_GENERIC,      // 'E_unet', runtime-shape kernel (any frame count; MCD_OPT_COND_GENERIC)
    COND_PLAIN,             // cond_encode_kernel: any channel list / frame count, activations in LDS
    COND_PLAIN_SCRATCH      // ... with its third buffer in global scratch (cond.gmode)
};
// whole_windows: the caller runs score_kernel with workgroups that own whole windows (split == 1) and as many condition frames
// as U-Net frames -- the shipped encoder then runs inside that kernel (otherwise every workgroup of a window would repeat it)
CondRoute cond_route(const mcd_weights* w, bool whole_windows = false) {
    if (!w->has_cond) return COND_NONE;
    const bool generic = w->opt[MCD_OPT_COND_GENERIC] != 0;
    if (w->cond_unet) {
        if (generic) return COND_UNET_GENERIC;
        return cond_unet_has_kernel(w->cond.Tc) ? COND_UNET : w->tiled_cond_tp ? COND_TILED : COND_UNET_GENERIC;
    }
    if (w->cond_fast && !generic) return whole_windows ? COND_INKERNEL : COND_FAST;
    return w->cond.gmode ? COND_PLAIN_SCRATCH : COND_PLAIN;
}
// global scratch a route needs for `chains` trajectories / `B` windows: what its launch below is given, and what the sizing
// entry points reserve
int64_t unet_scratch_bytes(const mcd_weights* w, UnetRoute r, int64_t chains) {
    switch (r) {
        case UNET_TILED: return w->tiled_tp ? tiled_scratch_bytes(w, chains, w->tiled_tp) : 0;
        case UNET_GENERIC: return gen_scratch_bytes(chains, w->cfg.t_unet);
        default: return 0;
    }
}
int64_t cond_scratch_bytes(const mcd_weights* w, CondRoute r, int64_t B) {
    switch (r) {
        case COND_TILED: return w->cond_unet && w->tiled_cond_tp ? tiled_scratch_bytes(w, B, w->tiled_cond_tp) : 0;
        case COND_UNET_GENERIC: return w->cond_unet ? gen_scratch_bytes(B, w->cond.Tc) : 0;
        case COND_PLAIN_SCRATCH:
            return w->has_cond && !w->cond_unet && w->cond.gmode ? (B < CE_MAX_WGS ? B : CE_MAX_WGS) * (int64_t)w->cond.buf_floats() * 4 : 0;
        default: return 0;
    }
}
// The sizing entry points return an UPPER BOUND over the options, not the need of the route that would run now (callers size
// once and reuse): a handle without a specialised U-Net kernel reserves for both of its routes, an 'E_unet' handle for the
// slab-tiled and the runtime-shape encoder even while cond_unet_kernel serves it, and the plain encoder's scratch whenever
// cond.gmode is set.
int64_t unet_ws_bytes(const mcd_weights* w, int64_t chains) {
    if (!w->fast_unet) return std::max(unet_scratch_bytes(w, UNET_TILED, chains), unet_scratch_bytes(w, UNET_GENERIC, chains));
    return unet_scratch_bytes(w, unet_route(w), chains);
}
int64_t cond_ws_bytes(const mcd_weights* w, int64_t B) {
    return std::max({cond_scratch_bytes(w, COND_TILED, B), cond_scratch_bytes(w, COND_UNET_GENERIC, B), cond_scratch_bytes(w, COND_PLAIN_SCRATCH, B)});
}

int launch_unet(const mcd_weights* w, UnetRoute r, ScoreParams& P, const FrameMaps& M, float* scratch, hipStream_t st, bool* fused = nullptr) {
    P.phase = w->opt[MCD_OPT_PHASE];      // (the launchers decode it: decode_phase; score_kernel reads it raw)
    switch (r) {
        case UNET_KERNEL: return launch_score(w, w->cfg.t_unet, P, st, fused);
        case UNET_TILED: return launch_score_tiled(w, P, M, scratch, st);
        default: return launch_score_generic(w, P, M, scratch, st);
    }
}
// the condition encoders that read the condition frames straight from the window view (scratch: cond_scratch_bytes(w, r, B))
int launch_cond_view(const mcd_weights* w, CondRoute r, const DataView& data, const FrameIdx& fi, int seg_len, float* emb, int B, float* scratch,
                     hipStream_t st) {
    if (r == COND_FAST) return launch_cond_fast(w, data, fi, seg_len, emb, B, st);
    if (r == COND_UNET) return launch_cond_unet(w, data, fi, seg_len, emb, B, st);
    const int Tc = w->cond.Tc;
    if (!scratch) return fail(MCD_EINVAL, "workspace required (mcd_score_workspace_bytes) for the runtime-shape condition encoder");
    if (r == COND_TILED) {      // the slab-tiled MFMA stages, one window per "chain"
        ScoreParams P;
        memset(&P, 0, sizeof(P));
        P.wbuf = w->dbuf; P.dv = data; P.seg_len = seg_len; P.B = B; P.S = 1; P.n_chains = B; P.ns = 2; P.eps_out = emb;
        FrameMaps M;
        memset(&M, 0, sizeof(M));
        for (int t = 0; t < Tc; ++t) M.src_frame[t] = fi.idx[t];
        const int wgs = tiled_wgs(w, B, w->tiled_cond_tp);
        switch (w->tiled_cond_tp) {
#define MCD_CASE(unit, TP, NB) case TP: return launch_score_tiled_t<TP, NB, false, true>(w, P, M, scratch, wgs, st);
            MCD_TILED_COND_INSTANCES(MCD_CASE)
#undef MCD_CASE
            default: return fail(MCD_EUNSUPPORTED, "tiled condition encoder: frame count");
        }
    }
    const int wgs = B < GEN_MAX_WGS ? B : GEN_MAX_WGS;
    hipLaunchKernelGGL(cond_unet_generic_kernel, dim3(wgs), dim3(GEN_THREADS), 0, st, w->dbuf, w->gcond, data, fi, seg_len, Tc, B, emb, scratch);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}
// The device copy of a packed buffer (and, with `tune`, the trajectory kernel's 4 tuning words, zeroed) on `device`, leaving the
// calling thread's current device as it was.  On an error nothing stays allocated.
int upload_packed(const std::vector<float>& buf, int device, float** dbuf, int** tune = nullptr) {
    int prev_dev = 0;
    HIP_TRY(hipGetDevice(&prev_dev));
    HIP_TRY(hipSetDevice(device));
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{prev_dev};
    *dbuf = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dbuf), buf.size() * sizeof(float));
    if (e != hipSuccess) return fail(MCD_EDEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
    e = hipMemcpy(*dbuf, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(*dbuf); return fail(MCD_EDEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e)); }
    if (tune) {
        *tune = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(tune), 4 * sizeof(int)) != hipSuccess || hipMemset(*tune, 0, 4 * sizeof(int)) != hipSuccess) {
            if (*tune) (void)hipFree(*tune);
            (void)hipFree(*dbuf);
            return fail(MCD_EDEVICE, "hipMalloc (tuning words)");
        }
    }
    return MCD_OK;
}
}  // namespace

#include "mcd_call.hpp"      // the front end of a call: view, checks, workspace layouts, launch_cond

static unsigned long long* g_prof = nullptr;  // MCD_PROFILE builds: device buffer of 32 accumulators

// ---- host helpers shared by several entries below (templates: outside the extern "C" block)
// The sample selection of aggregate_kernel / error_maps_kernel (Params = AggrParams / MapParams, zeroed and with P.s first):
// the block both read, and their launch -- one 64-lane wave per window
static void fill_select(SelectParams& s, const mcd_score_cfg_t* cfg, int strategy, float quantile, const float* loss_all,
                        const float* pose_all, const mcd_window_view_t* view) {
    s.loss_all = loss_all; s.pose_all = pose_all; s.win_mask = view ? view->cond_mask : nullptr;
    s.B = cfg->n_windows; s.S = cfg->n_samples; s.Tx = cfg->n_corrupt; s.seg_len = cfg->seg_len;
    s.strategy = strategy; s.loss_fn = cfg->loss_fn; s.q = quantile;
    for (int t = 0; t < cfg->n_corrupt && t < MCD_MAX_FRAMES; ++t) s.corrupt_idx[t] = cfg->corrupt_idx[t];
}
template <class Params>
static int launch_select(void (*kernel)(Params), Params& P, hipStream_t st) {
    P.s.in_lds = P.s.S <= AGG_LDS_MAX;
    const size_t lds = (size_t)(SEL_LDS_WORDS + (P.s.in_lds ? P.s.S : 0)) * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3(P.s.B < 65536 ? P.s.B : 65536), dim3(64), lds, st, P);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

// mcd_scatter_max (W = 1, n_slot = seg_len, any) / mcd_joint_scatter_max (W = 17, n_slot = n_corrupt <= 32): vals (n,) / (n, n_slot, 17)
// -> out (n_rows, n_frames, W), zeroed here; every check before the first device call
template <int W>
static int scatter_max(const float* vals, const int32_t* frames, const int32_t* row, int64_t n, int32_t n_slot, int32_t n_rows,
                       int32_t n_frames, float* out, void* stream) {
    if (!out) return fail(MCD_EINVAL, "null argument");
    if (n < 0 || n_slot < 1 || (W > 1 && n_slot > MCD_MAX_FRAMES) || n_rows < 0 || n_frames < 0)
        return fail(MCD_EINVAL, W > 1 ? "need n, n_rows, n_frames >= 0 and 1 <= n_corrupt <= 32" : "need n, n_rows, n_frames >= 0 and 1 <= seg_len");
    if (n > 0 && (!vals || !frames || !row)) return fail(MCD_EINVAL, "null argument");
    if (n > 0x7fffffffffffffffll / ((long long)n_slot * W)) return fail(MCD_EUNSUPPORTED, "too many windows for one launch");
    const long long total = (long long)n * n_slot * W;
    if ((total + 255) / 256 > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many windows for one launch");
    hipStream_t st = (hipStream_t)stream;
    if ((size_t)n_rows * n_frames == 0) return MCD_OK;
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_rows * n_frames * W * sizeof(float), st));
    if (n == 0) return MCD_OK;
    hipLaunchKernelGGL(scatter_max_kernel<W>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, vals, frames, row,
                       (long long)n, n_slot, n_rows, n_frames, out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

// the library is built with -fvisibility=hidden: only the C ABI of include/mocodad_hip.h is exported
#pragma GCC visibility push(default)
extern "C" {

void mcd_debug_set_prof(void* p) { g_prof = reinterpret_cast<unsigned long long*>(p); }

int mcd_debug_poison_lds(void* stream) {
    constexpr size_t lds = 160 * 1024;
    LDS_LIMIT(poison_lds_kernel, lds);
    // one 160 KB workgroup per CU at a time; several waves of them so that every CU of every XCD takes at least one
    hipLaunchKernelGGL(poison_lds_kernel, dim3(4096), dim3(API_THREADS), lds, static_cast<hipStream_t>(stream), (unsigned*)nullptr, (int)(lds / 4));
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

const char* mcd_last_error(void) { return g_err.c_str(); }
int32_t mcd_abi_version(void) { return MCD_ABI_VERSION; }

int mcd_pack_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, int32_t device,
                     mcd_weights_t** out) {
    if (!tensors || !cfg || !out) return fail(MCD_EINVAL, "null argument");
    PackedModel m;
    int rc = pack_pose_model(tensors, n_tensors, cfg, m);
    if (rc != MCD_OK) return rc;
    float* dbuf = nullptr;
    int* tune = nullptr;
    rc = upload_packed(m.buf, device, &dbuf, &tune);
    if (rc != MCD_OK) return rc;
    mcd_weights* w = new mcd_weights();
    memset(w->opt, 0, sizeof(w->opt));
    w->cfg = *cfg; w->device = device; w->dbuf = dbuf; w->tune = tune; w->n_floats = m.buf.size();
    w->zero_row = m.zero_row; w->fast_unet = m.fast_unet != 0; w->gen = m.gen; w->tiled = m.tiled; w->tiled_tp = m.tiled_tp;
    w->gcond = m.cond.GC; w->tiled_cond = m.cond.TNc; w->tiled_cond_tp = m.cond.tiled_cond_tp;
    set_cond_weights(w, m, dbuf);
    *out = w;
    return MCD_OK;
}

int mcd_debug_pack_digest(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, const mcd_latent_cfg_t* latent_cfg,
                          int64_t* n_floats_out, uint64_t* digest_out) {
    if (!tensors || !cfg || !n_floats_out || !digest_out) return fail(MCD_EINVAL, "null argument");
    PackedModel m;
    const int rc = latent_cfg ? pack_latent_model(tensors, n_tensors, cfg, latent_cfg, m) : pack_pose_model(tensors, n_tensors, cfg, m);
    if (rc != MCD_OK) return rc;
    *n_floats_out = (int64_t)m.buf.size();
    *digest_out = pack_digest(m);
    return MCD_OK;
}

int mcd_debug_pack_ae_digest(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, int32_t latent_dim,
                             int64_t* n_floats_out, uint64_t* digest_out) {
    if (!tensors || !cfg || !n_floats_out || !digest_out) return fail(MCD_EINVAL, "null argument");
    PackedModel m;
    const int rc = pack_latent_ae_model(tensors, n_tensors, cfg, latent_dim, m);
    if (rc != MCD_OK) return rc;
    *n_floats_out = (int64_t)m.buf.size();
    *digest_out = pack_digest(m);
    return MCD_OK;
}

int mcd_set_option(mcd_weights_t* w, int32_t option, int32_t value) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (option < 0 || option >= MCD_OPT_COUNT) return fail(MCD_EINVAL, "unknown option " + std::to_string(option));
    w->opt[option] = value;
    return MCD_OK;
}

void mcd_free_weights(mcd_weights_t* w) {
    if (!w) return;
    if (w->dbuf) (void)hipFree(w->dbuf);
    if (w->tune) (void)hipFree(w->tune);
    delete w;
}

int mcd_cond_encode(const mcd_weights_t* w, const float* cond_data, int32_t n_windows, float* emb_out, void* stream) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (!w->has_cond) return fail(MCD_EINVAL, "model has no condition encoder");
    if (n_windows <= 0) return MCD_OK;
    if (!cond_data || !emb_out) return fail(MCD_EINVAL, "null argument");
    const CondRoute route = cond_route(w);
    if (w->cond_unet && !cond_unet_has_kernel(w->cond.Tc))
        return fail(MCD_EUNSUPPORTED, "mcd_cond_encode: the 'E_unet' encoder at this frame count needs scratch memory; use mcd_score");
    if (route == COND_PLAIN_SCRATCH) return fail(MCD_EUNSUPPORTED, "mcd_cond_encode: this many condition frames need scratch memory; use mcd_score");
    FrameIdx fi;
    for (int k = 0; k < MCD_MAX_FRAMES; ++k) fi.idx[k] = k;
    DataView dv;
    window_view(cond_data, nullptr, w->cond.Tc, dv);      // cond_data holds the condition frames alone: nothing to gather
    return launch_cond(w, route, dv, fi, w->cond.Tc, emb_out, n_windows, nullptr, nullptr, (hipStream_t)stream);
}

// scratch of the single-pass entries: the slabs of the slab-tiled kernel (13 .. 32 U-Net frames) or of the runtime-shape kernel
int64_t mcd_pass_workspace_bytes(const mcd_weights_t* w, int32_t n_windows) {
    if (!w || n_windows <= 0) return 0;
    return unet_ws_bytes(w, n_windows);
}

int mcd_unet_forward(const mcd_weights_t* w, const float* x, const float* cond, const float* step_table, int32_t t,
                     int32_t n_windows, float* eps_out, void* workspace, void* stream) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (n_windows <= 0) return MCD_OK;
    if (!x || !step_table || !eps_out) return fail(MCD_EINVAL, "null argument");
    if (t < 0) return fail(MCD_EINVAL, "t must be >= 0 (step_table needs at least t + 1 rows)");
    ScoreParams P;
    memset(&P, 0, sizeof(P));
    P.wbuf = w->dbuf; P.x_in = x; P.cond_emb = cond; P.step_table = step_table; P.eps_out = eps_out;
    P.B = n_windows; P.S = 1; P.ns = t + 1; P.seg_len = w->cfg.t_unet; P.n_corrupt = w->cfg.t_unet; P.fixed_mask = 0;
    P.mode = 1; P.step_single = t; P.n_chains = n_windows;
    hipStream_t st = (hipStream_t)stream;
    const UnetRoute route = unet_route(w);      // (the slab-tiled and the runtime-shape kernel in single-pass mode)
    if (route != UNET_KERNEL && !workspace) return fail(MCD_EINVAL, "workspace required (mcd_pass_workspace_bytes)");
    FrameMaps M;
    memset(&M, 0, sizeof(M));
    return launch_unet(w, route, P, M, reinterpret_cast<float*>(workspace), st);
}

int mcd_layer_forward(const mcd_weights_t* w, int32_t stage, const float* x, const float* skip, const float* emb, int32_t n_windows,
                      float* out, void* workspace, void* stream) {
    if (!w) return fail(MCD_EINVAL, "null argument");
    if (stage < 0 || stage > 14) return fail(MCD_EINVAL, "stage must be 0..10 (ST-GCN layers) or 11..14 (down1, down2, up3, up2)");
    if (n_windows <= 0) return MCD_OK;
    if (!x || !out || !emb) return fail(MCD_EINVAL, "null argument");
    ScoreParams P;
    memset(&P, 0, sizeof(P));
    P.wbuf = w->dbuf; P.cond_emb = emb; P.step_table = w->dbuf + w->zero_row;   // pe = 0: the layers see SiLU(emb)
    P.B = n_windows; P.S = 1; P.ns = 1; P.seg_len = w->cfg.t_unet; P.n_corrupt = w->cfg.t_unet;
    P.mode = 1; P.step_single = 0; P.n_chains = n_windows;
    P.lt_stage = stage; P.lt_in = x; P.lt_out = out; P.lt_skip = skip;
    P.x_in = stage == 0 ? x : nullptr;     // layer 0 reads the chain state itself; the other stages start from x = 0
    hipStream_t st = (hipStream_t)stream;
    // the stage code of the MFMA kernels, whatever MCD_OPT_GENERIC_UNET says
    if (unet_route(w, false) == UNET_TILED) {      // 13 .. 32 frames: the joint resamplers are fused into layers 3, 5, 7, 9 (no stages of their own)
        if (stage > 10) return fail(MCD_EUNSUPPORTED, "13 .. 32 U-Net frames: the joint resamplers are part of stages 3, 5, 7, 9");
        if (skip && stage != 7 && stage != 9) return fail(MCD_EINVAL, "skip tensor: stages 7 (d2) and 9 (d1) only");
        if (!workspace) return fail(MCD_EINVAL, "workspace required (mcd_pass_workspace_bytes)");
        FrameMaps M;
        memset(&M, 0, sizeof(M));
        return launch_score_tiled(w, P, M, reinterpret_cast<float*>(workspace), st, true);
    }
    if (skip) return fail(MCD_EINVAL, "skip tensor: only the fused stages of 13 .. 32 U-Net frames take one");
    return launch_score(w, w->cfg.t_unet, P, st, nullptr, true);      // (the layer-test forms: the template arguments and unit flags of the production kernels)
}

int mcd_philox_noise(uint64_t seed, int64_t first_window_id, int32_t n_windows, int32_t n_samples, int32_t noise_steps,
                     int32_t n_corrupt, float* noise_out, void* stream) {
    if (n_windows <= 0) return MCD_OK;
    if (!noise_out) return fail(MCD_EINVAL, "null argument");
    if (n_samples < 1 || noise_steps < 2 || n_corrupt < 1 || n_corrupt > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "bad sizes");
    const int K = noise_steps > 2 ? noise_steps - 1 : 1;
    const long long total = (long long)n_samples * K * n_windows * n_corrupt * 9;
    hipLaunchKernelGGL(philox_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)seed, (long long)first_window_id, n_windows, n_samples, K, n_corrupt, noise_out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_random_imp_masks(uint64_t seed, int64_t first_window_id, int32_t n_windows, int32_t seg_len, int32_t n_cond,
                         int32_t* mask_out, void* stream) {
    // every argument check comes before the first device call
    if (seg_len < 2 || seg_len > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "seg_len must be in 2 .. 32 (one mask bit per frame)");
    if (n_cond < 1 || n_cond >= seg_len) return fail(MCD_EINVAL, "n_cond must be in 1 .. seg_len - 1");
    if (n_windows < 0) return fail(MCD_EINVAL, "n_windows must be >= 0");
    if (n_windows == 0) return MCD_OK;
    if (!mask_out) return fail(MCD_EINVAL, "mask_out is null");
    hipLaunchKernelGGL(random_imp_masks_kernel, dim3((unsigned)((n_windows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)seed, (long long)first_window_id, n_windows, seg_len, n_cond, mask_out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int32_t mcd_plan_split(const mcd_weights_t* w, const mcd_score_cfg_t* cfg) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_windows <= 0) return 1;
    if (unet_route(w) != UNET_KERNEL) return 0;
    ScoreParams P;
    memset(&P, 0, sizeof(P));
    P.B = cfg->n_windows; P.S = cfg->n_samples; P.ns = cfg->noise_steps; P.mode = 0; P.plan_only = 1;
    const int rc = launch_score(w, w->cfg.t_unet, P, nullptr);
    return rc != MCD_OK ? rc : P.split;
}

int64_t mcd_score_workspace_bytes(const mcd_weights_t* w, const mcd_score_cfg_t* cfg) {
    if (!w || !cfg) return 0;
    return pose_workspace(w, cfg->n_windows, cfg->n_samples).bytes;
}

// One scoring call.  aggr = 0: per-sample losses only (loss_all required).  aggr = a loss-based MCD_AGGR_* strategy: loss_agg
// (B,) is produced too -- inside the trajectory kernel when its workgroups see all samples of their windows (one launch per
// call), by aggregate_kernel otherwise.
static int score_impl(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                      const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                      int aggr, float quantile, float* loss_agg, float* loss_all, float* pose_out, void* stream) {
    if (!w || !cfg) return fail(MCD_EINVAL, "null argument");
    const int B = cfg->n_windows, S = cfg->n_samples;
    if (B <= 0) return MCD_OK;
    if (!data || !step_table) return fail(MCD_EINVAL, "null argument");
    if (aggr == 0 && !loss_all) return fail(MCD_EINVAL, "null argument");
    if (aggr != 0) {
        if (!loss_agg) return fail(MCD_EINVAL, "null argument");
        if (int rc = check_aggregation(aggr, quantile, AGGR_LOSSES, "mcd_score_fused aggregates losses (best, worst, mean, median, quantile); "
                                                                    "the *_pose strategies go through mcd_score + mcd_aggregate")) return rc;
    }
    if (S < 1 || cfg->noise_steps < 2) return fail(MCD_EINVAL, "need n_samples >= 1 and noise_steps >= 2");
    if ((long long)B * S > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x n_samples exceeds 2^31 - 1: score in smaller batches");
    if (int rc = check_frame_partition(cfg)) return rc;
    const int strat = w->cfg.strategy;
    const int Tu = w->cfg.t_unet;
    const bool rnd = strat == MCD_STRATEGY_RANDOM_IMP;
    const bool keeps_cond = strat == MCD_STRATEGY_CONCAT || strat == MCD_STRATEGY_INBETWEEN_IMP || rnd;   // condition frames are U-Net input
    if (rnd && !(view && view->cond_mask)) return fail(MCD_EINVAL, "random_imp needs mcd_window_view_t.cond_mask");
    const int tf = keeps_cond ? cfg->n_cond : 0;
    if (tf + cfg->n_corrupt != Tu) return fail(MCD_EINVAL, "frame split does not match the packed U-Net (t_unet)");
    const UnetRoute route = unet_route(w);
    if (strat == MCD_STRATEGY_INJECT && cfg->n_cond != w->cfg.t_cond) return fail(MCD_EINVAL, "n_cond does not match the packed condition encoder");
    hipStream_t st = (hipStream_t)stream;
    ScoreParams P;
    memset(&P, 0, sizeof(P));
    P.wbuf = w->dbuf; P.prof = g_prof;
    P.tune = decode_phase(w->opt[MCD_OPT_PHASE]).self_tune ? w->tune : nullptr;      // (off: the host's estimate only -- A/B of the self-calibration)
    if (int rc = window_view(data, view, cfg->seg_len, P.dv)) return rc;
    if (rnd) P.win_mask = view->cond_mask;
    P.noise = noise; P.step_table = step_table; P.pose_out = pose_out;
    P.seed = seed; P.first_window = first_window_id;
    P.B = B; P.S = S; P.ns = cfg->noise_steps; P.seg_len = cfg->seg_len; P.n_corrupt = cfg->n_corrupt;
    P.loss_fn = cfg->loss_fn; P.mode = 0; P.n_chains = B * S; P.split = 1;
    P.aggr = aggr; P.aggr_q = quantile; P.loss_agg = aggr ? loss_agg : nullptr;
    // U-Net frame layout: concat = condition frames first (mocodad.py:668), imputation = natural frame order
    // (mocodad.py:672-683), inject / no_condition = the corrupt frames only
    FrameMaps M;
    memset(&M, 0, sizeof(M));
    if (int rc = check_frame_lists(cfg)) return rc;
    for (int k = 0; k < tf && !rnd; ++k) {
        const int t = strat == MCD_STRATEGY_INBETWEEN_IMP ? cfg->cond_idx[k] : k;
        if (t < 0 || t >= Tu || ((P.fixed_mask >> t) & 1)) return fail(MCD_EINVAL, "bad cond_idx");
        P.fixed_mask |= 1u << t;
        M.src_frame[t] = cfg->cond_idx[k];
    }
    for (int k = 0; k < cfg->n_corrupt && !rnd; ++k) {
        const int t = strat == MCD_STRATEGY_INBETWEEN_IMP ? cfg->corrupt_idx[k] : tf + k;
        if (t < 0 || t >= Tu || ((P.fixed_mask >> t) & 1)) return fail(MCD_EINVAL, "bad corrupt_idx");
        M.src_frame[t] = cfg->corrupt_idx[k];
        M.tx_of[t] = k;
        M.pos_of[k] = t;
    }
    for (int t = 0; t < MCD_MAX_FRAMES; ++t) M.upd_of[t] = -1;
    for (int k = 0; k < cfg->n_corrupt && !rnd; ++k) {
        const int t = keeps_cond ? cfg->corrupt_idx[k] : k;     // mocodad.py:829-838: mask built from corrupt_idxs
        if (t < 0 || t >= Tu || M.upd_of[t] >= 0) return fail(MCD_EINVAL, "bad corrupt_idx");
        M.upd_of[t] = k;
        if (M.pos_of[k] != t) P.upd_shift = 1;
    }
    for (int t = 0; t < 12; ++t) {      // the specialised kernels (<= 12 frames) carry the maps in their parameter block
        P.src_frame[t] = M.src_frame[t]; P.tx_of[t] = M.tx_of[t]; P.pos_of[t] = M.pos_of[t]; P.upd_of[t] = M.upd_of[t];
    }
    const PoseWorkspace lay = pose_workspace(w, B, S);
    char* wsb = reinterpret_cast<char*>(workspace);
    float* ws_loss = wsb ? reinterpret_cast<float*>(wsb + lay.loss) : nullptr;
    float* gen_scratch = wsb ? reinterpret_cast<float*>(wsb + lay.scratch) : nullptr;
    P.loss_out = loss_all ? loss_all : ws_loss;       // (skipped by a fused launch when the caller did not ask for it)
    if (route == UNET_KERNEL) {           // how the call is cut into workgroups (decides where the condition encoder runs)
        P.plan_only = 1;
        const int rc = launch_score(w, Tu, P, st);
        if (rc != MCD_OK) return rc;
        P.plan_only = 0;
    }
    auto score = [&]() -> int {
        bool fused = false;
        if (route == UNET_KERNEL) P.loss_out_optional = loss_all == nullptr;
        else if (!workspace) return fail(MCD_EINVAL, "workspace required (mcd_score_workspace_bytes) for the runtime-shape kernel");
        // UNET_TILED: the MFMA kernel over an L2-resident slab; UNET_GENERIC: plain FMAs
        const int rc = launch_unet(w, route, P, M, gen_scratch, st, &fused);
        if (rc != MCD_OK || aggr == 0 || fused) return rc;
        AggrParams A;        // the workgroups did not see all samples of their windows: aggregate the (B,S) losses afterwards
        memset(&A, 0, sizeof(A));
        fill_select(A.s, cfg, aggr, quantile, P.loss_out, nullptr, nullptr);
        A.loss_agg = loss_agg; A.C = C0; A.V = 17;
        return launch_select(aggregate_kernel, A, st);
    };
    // (strategy inject <=> the handle has a condition encoder)
    const CondRoute croute = cond_route(w, route == UNET_KERNEL && P.split == 1 && cfg->n_cond == Tu);
    if (croute == COND_INKERNEL) {
        P.cond_inkernel = 1;
        for (int k = 0; k < Tu; ++k) P.cond_idx[k] = cfg->cond_idx[k];
    } else if (croute != COND_NONE) {
        if (!workspace) return fail(MCD_EINVAL, "workspace required for this condition encoder");
        float* emb = reinterpret_cast<float*>(workspace);
        FrameIdx fi;
        for (int k = 0; k < MCD_MAX_FRAMES; ++k) fi.idx[k] = cfg->cond_idx[k];
        if (int rc = launch_cond(w, croute, P.dv, fi, cfg->seg_len, emb, B, reinterpret_cast<float*>(wsb + lay.gather), gen_scratch, st)) return rc;
        P.cond_emb = emb;
    }
    return score();
}

int mcd_score(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const float* noise, uint64_t seed,
              int64_t first_window_id, const float* step_table, void* workspace, float* loss_out, float* pose_out,
              void* stream) {
    return score_impl(w, cfg, data, nullptr, noise, seed, first_window_id, step_table, workspace, 0, 0.f, nullptr, loss_out, pose_out, stream);
}

int mcd_score_view(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                   const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                   float* loss_out, float* pose_out, void* stream) {
    return score_impl(w, cfg, data, view, noise, seed, first_window_id, step_table, workspace, 0, 0.f, nullptr, loss_out, pose_out, stream);
}

int mcd_score_fused(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                    const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                    int32_t aggregation, float quantile, float* loss_agg, float* loss_all, float* pose_out, void* stream) {
    if (aggregation == MCD_AGGR_ALL) return fail(MCD_EINVAL, "MCD_AGGR_ALL is mcd_score");
    return score_impl(w, cfg, data, view, noise, seed, first_window_id, step_table, workspace, aggregation, quantile, loss_agg, loss_all,
                      pose_out, stream);
}

int mcd_aggregate(const mcd_score_cfg_t* cfg, int32_t num_coords, int32_t n_joints, int32_t strategy, float quantile,
                  const float* loss_all, const float* pose_all, const float* data, float* loss_agg, float* pose_agg,
                  void* stream) {
    return mcd_aggregate_view(cfg, num_coords, n_joints, strategy, quantile, loss_all, pose_all, data, nullptr, loss_agg, pose_agg, stream);
}

int mcd_aggregate_view(const mcd_score_cfg_t* cfg, int32_t num_coords, int32_t n_joints, int32_t strategy, float quantile,
                       const float* loss_all, const float* pose_all, const float* data, const mcd_window_view_t* view,
                       float* loss_agg, float* pose_agg, void* stream) {
    if (!cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_windows <= 0) return MCD_OK;
    if (!loss_all || !loss_agg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_samples < 1) return fail(MCD_EINVAL, "need n_samples >= 1");
    if (int rc = check_aggregation(strategy, quantile, AGGR_ANY, "unknown aggregation strategy")) return rc;
    const bool need_pose = strategy == MCD_AGGR_MEAN_POSE || strategy == MCD_AGGR_MEDIAN_POSE;
    if (need_pose && (!pose_all || !data)) return fail(MCD_EINVAL, "pose strategies need pose_all and data");
    if (pose_agg && !pose_all) return fail(MCD_EINVAL, "pose_agg requested without pose_all");
    if (view && view->base) return fail(MCD_EINVAL, "mcd_aggregate_view reads dense (B,C,T,V) windows: materialise the view (base must be NULL)");
    const int32_t* win_mask = view ? view->cond_mask : nullptr;
    if (win_mask && (cfg->seg_len < 1 || cfg->seg_len > MCD_MAX_FRAMES || cfg->n_corrupt < 1 || cfg->n_corrupt > cfg->seg_len))
        return fail(MCD_EINVAL, "cond_mask: need 1 <= n_corrupt <= seg_len <= 32");
    AggrParams P;
    memset(&P, 0, sizeof(P));
    fill_select(P.s, cfg, strategy, quantile, loss_all, pose_all, view);
    P.data = data; P.loss_agg = loss_agg; P.pose_agg = pose_agg; P.C = num_coords; P.V = n_joints;
    return launch_select(aggregate_kernel, P, (hipStream_t)stream);
}

int mcd_error_maps(const mcd_score_cfg_t* cfg, int32_t num_coords, int32_t n_joints, int32_t strategy, float quantile,
                   const float* loss_all, const float* pose_all, const float* data, const mcd_window_view_t* view,
                   float* maps_out, void* stream) {
    // every argument check comes before the first device call
    if (!cfg) return fail(MCD_EINVAL, "null argument");
    if (cfg->n_windows < 0) return fail(MCD_EINVAL, "n_windows must be >= 0");
    if (num_coords != C0 || n_joints != 17) return fail(MCD_EINVAL, "mcd_error_maps: num_coords must be 2 and n_joints 17 (the window layout)");
    if (cfg->n_samples < 1) return fail(MCD_EINVAL, "need n_samples >= 1");
    if (int rc = check_aggregation(strategy, quantile, AGGR_ANY | 1u << MCD_AGGR_ALL, "unknown aggregation strategy")) return rc;
    if (cfg->seg_len < 1 || cfg->seg_len > MCD_MAX_FRAMES || cfg->n_corrupt < 1 || cfg->n_corrupt > cfg->seg_len)
        return fail(MCD_EINVAL, "need 1 <= n_corrupt <= seg_len <= 32");
    const int32_t* win_mask = view ? view->cond_mask : nullptr;
    if (win_mask) {
        if (cfg->n_cond + cfg->n_corrupt != cfg->seg_len)
            return fail(MCD_EINVAL, "cond_mask: the mask carries n_cond = seg_len - n_corrupt set bits (n_cond + n_corrupt != seg_len)");
    } else {
        for (int k = 0; k < cfg->n_corrupt; ++k)
            if (cfg->corrupt_idx[k] < 0 || cfg->corrupt_idx[k] >= cfg->seg_len) return fail(MCD_EINVAL, "corrupt_idx outside [0, seg_len)");
    }
    const bool needs_loss = strategy != MCD_AGGR_ALL && strategy != MCD_AGGR_MEAN_POSE && strategy != MCD_AGGR_MEDIAN_POSE && strategy != MCD_AGGR_MEAN;
    if (!pose_all || !data || !maps_out || (needs_loss && !loss_all)) return fail(MCD_EINVAL, "null argument");
    if ((long long)cfg->n_windows * cfg->n_samples > 0x7fffffffll) return fail(MCD_EINVAL, "n_windows x n_samples exceeds 2^31 - 1");
    MapParams P;
    memset(&P, 0, sizeof(P));
    if (int rc = window_view(data, view, cfg->seg_len, P.dv)) return rc;
    if (cfg->n_windows == 0) return MCD_OK;
    fill_select(P.s, cfg, strategy, quantile, loss_all, pose_all, view);
    P.maps = maps_out;
    return launch_select(error_maps_kernel, P, (hipStream_t)stream);
}

int mcd_joint_scatter_max(const float* maps, const int32_t* frames, const int32_t* row, int64_t n, int32_t n_corrupt,
                          int32_t n_rows, int32_t n_frames, float* out, void* stream) {
    return scatter_max<17>(maps, frames, row, n, n_corrupt, n_rows, n_frames, out, stream);
}

int mcd_scatter_max(const float* scores, const int32_t* frames, const int32_t* row, int64_t n, int32_t seg_len,
                    int32_t n_rows, int32_t n_frames, float* out, void* stream) {
    return scatter_max<1>(scores, frames, row, n, seg_len, n_rows, n_frames, out, stream);
}

int mcd_normalize_poses(const float* raw, int64_t n_frames, float vid_w, float vid_h, const double* center,
                        const double* scale, float* out, void* stream) {
    if (n_frames < 0) return fail(MCD_EINVAL, "n_frames < 0");
    if (int rc = check_pose_geometry(vid_w, vid_h, center, scale)) return rc;
    if (n_frames == 0) return MCD_OK;
    if (!raw || !out) return fail(MCD_EINVAL, "null argument");
    const long long blocks = (n_frames + 255) / 256;
    if (blocks > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many frames for one launch");
    hipLaunchKernelGGL(normalize_poses_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, raw,
                       (long long)n_frames, vid_w, vid_h, center, scale, out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_denormalize_poses(const float* norm, const float* raw, const int32_t* count, int64_t n, float vid_w, float vid_h,
                          const double* center, const double* scale, float* out, void* stream) {
    if (n < 0) return fail(MCD_EINVAL, "n < 0");
    if (int rc = check_pose_geometry(vid_w, vid_h, center, scale)) return rc;
    if (n == 0) return MCD_OK;
    if (!norm || !raw || !out) return fail(MCD_EINVAL, "null argument");
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffll) return fail(MCD_EUNSUPPORTED, "too many rows for one launch");
    hipLaunchKernelGGL(denormalize_poses_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, norm, raw, count,
                       (long long)n, vid_w, vid_h, center, scale, out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_forecast_assemble(const float* poses, const int32_t* cell, int64_t n, int32_t n_corrupt, int32_t n_cells, int32_t method,
                          int32_t spread_method, int32_t max_cover, int32_t* workspace, float* pose_out, int32_t* count_out,
                          float* spread_out, void* stream) {
    if (n < 0 || n_cells < 0) return fail(MCD_EINVAL, "need n, n_cells >= 0");
    if (n_corrupt < 1 || n_corrupt > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "need 1 <= n_corrupt <= 32");
    if (max_cover < 1 || max_cover > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "need 1 <= max_cover <= 32");
    if (int rc = check_forecast_methods(method, spread_method)) return rc;
    if (n > 0x7fffffffll / n_corrupt) return fail(MCD_EINVAL, "n x n_corrupt exceeds 2^31 - 1: assemble in smaller batches");
    if (n_cells == 0) return MCD_OK;
    if (!workspace || !pose_out || !count_out || !spread_out) return fail(MCD_EINVAL, "null argument");
    if (n > 0 && (!poses || !cell)) return fail(MCD_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    ForecastParams F{poses, cell, workspace, pose_out, count_out, spread_out, (int)(n * n_corrupt), n_corrupt, n_cells, method,
                     spread_method, max_cover};
    HIP_TRY(hipMemsetAsync(count_out, 0, (size_t)n_cells * sizeof(int32_t), st));
    if (n == 0) {      // nothing forecasts anything: the empty result, as mcd_scatter_max leaves it, without a launch
        HIP_TRY(hipMemsetAsync(pose_out, 0, (size_t)n_cells * 34 * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(spread_out, 0, (size_t)n_cells * sizeof(float), st));
        return MCD_OK;
    }
    hipLaunchKernelGGL(forecast_claim_kernel, dim3((unsigned)((F.n_pairs + 255ll) / 256)), dim3(256), 0, st, F);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(forecast_reduce_kernel, dim3(n_cells < 65536 ? n_cells : 65536), dim3(64), 0, st, F);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_forecast_assemble_view(const float* poses, const int32_t* cell, const int32_t* trans, const double* inv_affine,
                               int32_t n_transform, int64_t n, int32_t n_corrupt, int32_t n_cells, int32_t method,
                               int32_t spread_method, int32_t max_cover, int32_t* workspace, float* pose_out, int32_t* count_out,
                               float* spread_out, void* stream) {
    if (!trans)      // no transforms: the call is mcd_forecast_assemble, its checks and its kernels
        return mcd_forecast_assemble(poses, cell, n, n_corrupt, n_cells, method, spread_method, max_cover, workspace, pose_out, count_out,
                                     spread_out, stream);
    if (n < 0 || n_cells < 0) return fail(MCD_EINVAL, "need n, n_cells >= 0");
    if (n_corrupt < 1 || n_corrupt > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "need 1 <= n_corrupt <= 32");
    if (max_cover < 1 || max_cover > MCD_FORECAST_VIEW_COVER) return fail(MCD_EINVAL, "need 1 <= max_cover <= 64");
    if (int rc = check_forecast_methods(method, spread_method)) return rc;
    if (n > 0x7fffffffll / n_corrupt) return fail(MCD_EINVAL, "n x n_corrupt exceeds 2^31 - 1: assemble in smaller batches");
    if (!inv_affine) return fail(MCD_EINVAL, "trans needs inv_affine, the inverse table of its transforms");
    if (n_transform < 1) return fail(MCD_EINVAL, "need n_transform >= 1");
    if (n_cells == 0) return MCD_OK;
    if (!workspace || !pose_out || !count_out || !spread_out) return fail(MCD_EINVAL, "null argument");
    if (n > 0 && (!poses || !cell)) return fail(MCD_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    ForecastViewParams V{{poses, cell, workspace, pose_out, count_out, spread_out, (int)(n * n_corrupt), n_corrupt, n_cells, method,
                          spread_method, max_cover}, trans, inv_affine, n_transform};
    HIP_TRY(hipMemsetAsync(count_out, 0, (size_t)n_cells * sizeof(int32_t), st));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(pose_out, 0, (size_t)n_cells * 34 * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(spread_out, 0, (size_t)n_cells * sizeof(float), st));
        return MCD_OK;
    }
    hipLaunchKernelGGL(forecast_claim_view_kernel, dim3((unsigned)((V.f.n_pairs + 255ll) / 256)), dim3(256), 0, st, V);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(forecast_reduce_view_kernel, dim3(n_cells < 65536 ? n_cells : 65536), dim3(64), 0, st, V);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int mcd_forecast_fan(const float* poses_all, const int32_t* cell, const int32_t* trans, const double* inv_affine,
                     int32_t n_transform, int64_t n, int32_t n_samples, int32_t n_corrupt, int32_t n_cells, const double* levels,
                     int32_t n_levels, int32_t max_cover, const float* observed, int32_t* workspace, float* quant_out, float* mean_out,
                     float* std_out, float* rank_out, int32_t* count_out, void* stream) {
    const int cover_max = trans ? MCD_FORECAST_VIEW_COVER : MCD_MAX_FRAMES;
    if (n < 0 || n_cells < 0) return fail(MCD_EINVAL, "need n, n_cells >= 0");
    if (n_corrupt < 1 || n_corrupt > MCD_MAX_FRAMES) return fail(MCD_EINVAL, "need 1 <= n_corrupt <= 32");
    if (max_cover < 1 || max_cover > cover_max) return fail(MCD_EINVAL, trans ? "need 1 <= max_cover <= 64" : "need 1 <= max_cover <= 32");
    if (n_samples < 1) return fail(MCD_EINVAL, "need n_samples >= 1");
    if (n > 0x7fffffffll / n_corrupt) return fail(MCD_EINVAL, "n x n_corrupt exceeds 2^31 - 1: assemble in smaller batches");
    if (trans && !inv_affine) return fail(MCD_EINVAL, "trans needs inv_affine, the inverse table of its transforms");
    if (trans && n_transform < 1) return fail(MCD_EINVAL, "need n_transform >= 1");
    if (n_levels < 1 || n_levels > MCD_FORECAST_FAN_LEVELS) return fail(MCD_EINVAL, "need 1 <= n_levels <= 8");
    if (!levels) return fail(MCD_EINVAL, "null argument");
    for (int l = 0; l < n_levels; ++l) {
        if (!(levels[l] >= 0.0 && levels[l] <= 1.0)) return fail(MCD_EINVAL, "levels outside [0, 1]");
        if (l && !(levels[l] > levels[l - 1])) return fail(MCD_EINVAL, "levels must be strictly ascending");
    }
    if ((observed == nullptr) != (rank_out == nullptr)) return fail(MCD_EINVAL, "observed and rank_out go together (both NULL: no rank)");
    if (n_cells == 0) return MCD_OK;
    if (!workspace || !quant_out || !mean_out || !std_out || !count_out) return fail(MCD_EINVAL, "null argument");
    if (n > 0 && (!poses_all || !cell)) return fail(MCD_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    ForecastFanParams Q;
    memset(&Q, 0, sizeof(Q));
    Q.v = ForecastViewParams{{poses_all, cell, workspace, nullptr, count_out, nullptr, (int)(n * n_corrupt), n_corrupt, n_cells, 0, 0, max_cover},
                             trans, inv_affine, n_transform};
    Q.observed = observed; Q.quant_out = quant_out; Q.mean_out = mean_out; Q.std_out = std_out; Q.rank_out = rank_out;
    for (int l = 0; l < n_levels; ++l) Q.levels[l] = levels[l];
    Q.n_samples = n_samples; Q.n_levels = n_levels;
    HIP_TRY(hipMemsetAsync(count_out, 0, (size_t)n_cells * sizeof(int32_t), st));
    if (n == 0) {      // nothing forecasts anything: the empty result, without a launch
        const size_t plane = (size_t)n_cells * 34 * sizeof(float);
        HIP_TRY(hipMemsetAsync(quant_out, 0, plane * n_levels, st));
        HIP_TRY(hipMemsetAsync(mean_out, 0, plane, st));
        HIP_TRY(hipMemsetAsync(std_out, 0, plane, st));
        if (rank_out) HIP_TRY(hipMemsetAsync(rank_out, 0, plane, st));
        return MCD_OK;
    }
    // the longest list a cell of this launch reduces -> the stride of its keys, and the joints 60 KB of LDS hold at that stride
    const long long most = (long long)max_cover * n_samples;
    Q.kp = 1;
    while (Q.kp < most && Q.kp < MCD_FORECAST_FAN_VALUES) Q.kp <<= 1;
    Q.jg = 17;
    while (Q.jg > 1 && forecast_fan_lds_bytes(Q.kp, Q.jg) > (size_t)FORECAST_FAN_LDS) --Q.jg;
    const dim3 claim_grid((unsigned)((Q.v.f.n_pairs + 255ll) / 256));
    if (trans) hipLaunchKernelGGL(forecast_claim_view_kernel, claim_grid, dim3(256), 0, st, Q.v);
    else hipLaunchKernelGGL(forecast_claim_kernel, claim_grid, dim3(256), 0, st, Q.v.f);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(forecast_fan_kernel, dim3(n_cells < 65536 ? n_cells : 65536), dim3(FORECAST_FAN_THREADS),
                       forecast_fan_lds_bytes(Q.kp, Q.jg), st, Q);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int64_t mcd_frame_scores_workspace_bytes(const mcd_frame_cfg_t* c) {
    if (!c || c->n_clips <= 0 || c->num_transform <= 0 || c->n_persons <= 0 || c->max_frames <= 0) return 0;
    const int64_t rows = (int64_t)c->num_transform * c->n_clips * c->n_persons;
    return rows * c->max_frames * 4 + round256(rows * 4);
}

int mcd_frame_scores(const mcd_frame_cfg_t* c, const float* scores, const int64_t* trans, const int64_t* meta,
                     const int32_t* frames, int64_t n_windows, int32_t seg_len, void* workspace, double* out, void* stream) {
    if (!c || !workspace || !out) return fail(MCD_EINVAL, "null argument");
    if (c->n_clips <= 0 || c->num_transform <= 0 || c->n_persons <= 0 || c->max_frames <= 0) return fail(MCD_EINVAL, "bad sizes");
    if (!c->clip_keys || !c->clip_n_frames || !c->frame_dst || !c->clip_out_len || !c->clip_out_off || !c->gauss_weights)
        return fail(MCD_EINVAL, "null table");
    if (n_windows > 0 && (!scores || !trans || !meta || !frames)) return fail(MCD_EINVAL, "null argument");
    if (c->frames_shift < 1) return fail(MCD_EINVAL, "frames_shift must be >= 1 (the reference's score[:-shift] is empty for 0)");
    if (c->gauss_radius < 0) return fail(MCD_EINVAL, "bad gauss_radius");
    const size_t lds = (size_t)2 * c->max_frames * sizeof(double);
    if (lds > 150 * 1024) return fail(MCD_EUNSUPPORTED, "clips longer than 9600 frames");
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)c->num_transform * c->n_clips * c->n_persons;
    FrameParams Q;
    memset(&Q, 0, sizeof(Q));
    Q.scores = scores; Q.trans = reinterpret_cast<const long long*>(trans); Q.meta = reinterpret_cast<const long long*>(meta);
    Q.frames = frames; Q.clip_keys = reinterpret_cast<const long long*>(c->clip_keys); Q.clip_n = c->clip_n_frames;
    Q.dst = c->frame_dst; Q.out_len = c->clip_out_len; Q.out_off = reinterpret_cast<const long long*>(c->clip_out_off);
    Q.gauss = c->gauss_weights;
    Q.mat = reinterpret_cast<float*>(workspace);
    Q.used = reinterpret_cast<int*>(Q.mat + rows * c->max_frames);
    Q.out = out; Q.n = n_windows; Q.seg_len = seg_len; Q.n_clips = c->n_clips; Q.num_transform = c->num_transform;
    Q.P = c->n_persons; Q.F = c->max_frames; Q.pad = c->pad_size; Q.shift = c->frames_shift; Q.radius = c->gauss_radius;
    HIP_TRY(hipMemsetAsync(workspace, 0, (size_t)(rows * c->max_frames * 4 + rows * 4), st));
    if (n_windows > 0) {
        const long long total = (long long)n_windows * seg_len;
        hipLaunchKernelGGL(frame_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Q);
        HIP_TRY(hipGetLastError());
    }
    LDS_LIMIT(&frame_scores_kernel, (size_t)150 * 1024);
    hipLaunchKernelGGL(frame_scores_kernel, dim3(c->n_clips), dim3(256), lds, st, Q);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

}  // extern "C"

// the live-stream entry points (the kernels of mcd_stream_kernel.hpp)
#include "mcd_stream_api.hpp"
// the MoCoDADlatent entry points (packer + calls; their kernels live in mcd_latent.hip)
#include "mcd_latent_api.hpp"
#pragma GCC visibility pop

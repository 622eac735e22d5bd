// mcd_launch.hpp — host side shared by the translation units of libmocodad_hip.so: the weights handle, error plumbing and the
// launcher templates whose explicit instantiations (mcd_inst.hip, one unit of mcd_instances.hpp per compilation) hold the kernels.
#pragma once
#include "mcd_device.hpp"
#include "mcd_score_kernel.hpp"
#include "mcd_tiled_kernel.hpp"
#include "mcd_instances.hpp"

namespace mcd {

struct GLayer { int cin, cout, V, tq, am, wt, wr, bias, embo; float slope; };    // wr < 0: identity residual; embo < 0: no embedding
constexpr int CE_THREADS = 512;      // block size of cond_encode_kernel (the packer sizes its LDS by it: CondW::gmode)
struct CondW {
    const float* base;
    int n_layers, Tc, latent, cmax;
    int gmode;       // 1: three LDS buffers of cmax x Tc x 17 do not fit (25 .. 31 condition frames of the shipped encoder): the third one lives in global scratch
    GLayer L[MCD_MAX_COND_LAYERS];
    int lw, lb;
    // cond_encode_kernel's memory plan: three rotating activation buffers of buf_floats() -- all in LDS, or under gmode two of
    // them and one per workgroup in global scratch -- and behind the LDS buffers RED, CE_THREADS partial sums
    __host__ __device__ size_t buf_floats() const { return (size_t)cmax * Tc * 17; }
    __host__ __device__ size_t red_offset() const { return (gmode ? 2 : 3) * buf_floats(); }
    __host__ __device__ size_t lds_floats() const { return red_offset() + CE_THREADS; }
};

struct GenNet { GLayer L[NLAYERS]; int rs_w[4], rs_b[4], we, be; };
struct GenCond { GLayer L[7]; int rs_w[2], rs_b[2], lw, lb; };

}  // namespace mcd

struct mcd_weights {
    mcd_model_cfg_t cfg;
    int device;
    float* dbuf;
    size_t n_floats;
    mcd::CondW cond;
    bool has_cond;
    bool cond_fast;   // shipped condition-encoder architecture -> cond_fast_kernel
    bool cond_unet;   // 'E_unet' condition encoder -> cond_unet_kernel
    bool fast_unet;   // a specialised score_kernel<T,...> exists for cfg.t_unet (score_has_kernel); otherwise the slab-tiled or the runtime-shape kernel
    mcd::TiledNet tiled;   // tables of score_tiled_kernel (t_unet without a score_kernel), frame count padded to tiled_tp
    int tiled_tp;     // tiled_tp_for(t_unet): 16, 24 or 32; 0 = none
    mcd::TiledNet tiled_cond;   // ... of its COND form: the 'E_unet' condition encoder at 13 .. 32 condition frames
    int tiled_cond_tp;
    mcd::GenNet gen;       // plain (unpacked) folded weights of the U-Net for score_generic_kernel
    mcd::GenCond gcond;    // ... and of the 'E_unet' condition encoder
    int zero_row;     // offset (floats) of 32 zero words in dbuf: an all-zero step_table row for mcd_layer_forward
    int* tune;        // 4 device words: the trajectory kernel's own measurement of its previous launch (ScoreParams::tune)
    int opt[MCD_OPT_COUNT];   // mcd_set_option values (plain ints: set before the calls they affect, like any other argument)
};

namespace mcd {

inline thread_local std::string g_err;
inline int fail(int code, const std::string& m) { g_err = m; return code; }

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(MCD_EDEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)


// Raise a kernel's dynamic-LDS limit once per device.  `done` is the kernel's own device bitmask; two host threads racing
// here both make the (idempotent) call, nobody launches before it has been made on its device.
inline int ensure_lds_limit(const void* fn, size_t bytes, std::atomic<unsigned long long>& done) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return MCD_OK;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (dev < 64) done.fetch_or(1ull << dev, std::memory_order_release);
    return MCD_OK;
}
#define LDS_LIMIT(kernel_expr, bytes) do { static std::atomic<unsigned long long> done_{0}; \
    int rc_ = ensure_lds_limit(reinterpret_cast<const void*>(kernel_expr), (bytes), done_); if (rc_ != MCD_OK) return rc_; } while (0)

// Workgroup slots of the device for a kernel (resident workgroups per CU x CUs), asked once per (kernel, device).
inline int wg_slots(const void* fn, size_t lds, std::atomic<int> (&cache)[64], int threads) {      // (threads: the caller's NTHREADS -- a translation-unit constant)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 512;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    v = per_cu * cus;
    cache[dev].store(v, std::memory_order_relaxed);
    return v;
}
// How a scoring call is cut into workgroups.  A workgroup owns NB windows and runs S / split of their samples in sequence.
// split = 1 (window-major) lets the condition encoder and the aggregation run inside the workgroup -- ONE launch per call,
// no workspace -- split = S (chain-major) is one trajectory per workgroup with the encoder and the aggregation as their own
// small launches.
inline int choose_split(int n_groups, int S, int slots) {
    // estimated makespan in units of one trajectory: rounds of workgroups x trajectories per workgroup; chain-major pays its
    // two extra launches (~0.05 trajectories).  (Round 2 charged window-major 2 %: what it lost was the tail of the YOUNGER
    // of the two co-resident workgroups, which the alternating wave priority of score_kernel removes -- the one-launch form is
    // now the faster one at equal rounds, profiles/r03s_prio_slices.txt.)
    auto rounds = [&](long long wgs) { return (double)((wgs + slots - 1) / slots); };
    const double window_major = rounds(n_groups) * S;
    const double chain_major = rounds((long long)n_groups * S) + 0.05;
    return S > 1 && chain_major < window_major ? S : 1;
}

// NWAVES / NTHREADS are constants of the TRANSLATION UNIT (-DMCD_NWAVES of a unit's flags, mcd_instances.hpp), and Plan, MixCfg,
// Tiling, TlStage and the kernels depend on them: every kernel and launcher is instantiated in exactly one unit (the others see
// `extern template`), the launchers below refuse to be instantiated with another wave count than the shipped one of their
// frame count, and mcd_api.hip -- which is built with the default and only CALLS launchers -- poisons the two names.
constexpr int shipped_waves_score(int t) { return t >= 9 && t <= 12 ? 12 : 8; }
constexpr int shipped_waves_tiled(int tp) { return tp > 16 ? 12 : 8; }
#if defined(MCD_FAST_T) || defined(MCD_ANY_NWAVES)      // developer builds measure other wave counts
#define MCD_WAVES_CHECK(expected) static_assert(true, "")
#else
#define MCD_WAVES_CHECK(expected) static_assert(NWAVES == (expected), "this unit's MCD_NWAVES is not the wave count the kernel ships with (MCD_UNIT_FLAGS_<n> in mcd_instances.hpp)")
#endif

// MCD_OPT_PHASE (a tuning option; the table of its values is at the enum in mocodad_hip.h), decoded for the host here and nowhere
// else.  The kernels read the raw value (ScoreParams::phase): score_kernel for start_delay and hashed_start.
struct PhaseOpt {
    int start_delay;      // > 0: score_kernel starts the second half of its grid that many x 1024 cycles late (the kernel's own read)
    bool slices;          // the launchers give co-resident workgroups their priority time slices (-1: off)
    bool self_tune;       // score_kernel corrects the host's slice estimate by its previous launch's measurement (-2: off)
    int forced_shift;     // < -15, score_tiled_kernel: slice length 2^(-value - 16) ticks instead of the estimate; -1: none
    bool hashed_start;    // < -15, score_kernel: every workgroup starts at its own hashed offset (the kernel's own read)
};
inline PhaseOpt decode_phase(int phase) {
    return PhaseOpt{phase > 0 ? phase : 0, phase != -1, phase != -2, phase < -15 ? -phase - 16 : -1, phase < -15};
}
// log2 of the priority time slice of co-resident workgroups in ticks of the 100 MHz clock: about a sixth of the launch's
// expected duration `ticks` (or the length the option forces), within 2^10 .. 2^26
inline int prio_slice_shift(double ticks, int forced_shift = -1) {
    const int sh = forced_shift >= 0 ? forced_shift : (int)floor(log2(ticks / 6.0) + 0.5);
    return sh < 10 ? 10 : (sh > 26 ? 26 : sh);
}

template <int T, int NB, int MINW, bool LT = false>
int launch_score_t(ScoreParams& P, hipStream_t st, bool* fused) {
    MCD_WAVES_CHECK(shipped_waves_score(T));
    using PL = Plan<T, NB>;
    LDS_LIMIT((&score_kernel<T, NB, MINW, LT>), PL::BYTES);
    static std::atomic<int> slots_cache[64];
    const int groups = (P.B + NB - 1) / NB;
    const int slots = wg_slots(reinterpret_cast<const void*>(&score_kernel<T, NB, MINW, LT>), PL::BYTES, slots_cache, NTHREADS);
    if (P.plan_only || P.mode != 0) {
        P.split = P.mode == 0 ? choose_split(groups, P.S, slots) : 1;
        if (P.mode == 0 && P.force_split > 0) P.split = P.force_split < P.S ? P.force_split : P.S;
        if (P.plan_only) return MCD_OK;
    }
    // the in-kernel condition encoder / aggregation need the workgroup to see all samples of its windows; its LDS holds 64
    // per-sample losses per window: more samples are aggregated by aggregate_kernel from the (B,S) losses
    const bool whole = P.split == 1 && P.mode == 0;
    if (!(whole && P.S <= 64)) P.loss_agg = nullptr;
    if (fused) *fused = P.loss_agg != nullptr;
    if (P.loss_agg && P.loss_out_optional) P.loss_out = nullptr;
    if (P.mode == 0 && !P.loss_agg && !P.loss_out) return fail(MCD_EINVAL, "workspace required (mcd_score_workspace_bytes): per-sample losses of an unfused aggregation");
    P.prio_shift = 0;
    if (MINW >= 4 && P.mode == 0 && decode_phase(P.phase).slices) {
        // priority time slice of the co-resident workgroups (see score_kernel): about 1/6 of the launch's expected duration --
        // rounds of workgroups x trajectories per workgroup x passes x ~7.5 us per (chain, frame) of a pass
        const double rounds = (double)(((long long)groups * P.split + slots - 1) / slots);
        const double traj = (double)((P.S + P.split - 1) / P.split);
        const double ticks = rounds * traj * (double)(P.ns > 2 ? P.ns - 1 : 1) * 7.5 * NB * T * 100.0;
        P.prio_shift = prio_slice_shift(ticks);
        P.prio_rounds = (int)rounds;
    }
    hipLaunchKernelGGL((score_kernel<T, NB, MINW, LT>), dim3(groups * P.split), dim3(NTHREADS), PL::BYTES, st, P);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}


// MFMA encoder of the shipped architecture: its four 17-joint layers need 112 floats of LDS per column (20 frames: 158 KB)
template <int T, int NB>
int launch_cond_fast_t(const mcd_weights* w, const DataView& data, const FrameIdx& fi, int seg_len, float* emb, int B, hipStream_t st) {
    constexpr size_t bytes = (size_t)CondFastLds<T, NB>::FLOATS * 4;
    LDS_LIMIT((&cond_fast_kernel<T, NB>), bytes);
    hipLaunchKernelGGL((cond_fast_kernel<T, NB>), dim3((B + NB - 1) / NB), dim3(NTHREADS), bytes, st, w->dbuf, data, fi, seg_len, emb, B);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

template <int T, int NB>
int launch_cond_unet_t(const mcd_weights* w, const DataView& data, const FrameIdx& fi, int seg_len, float* emb, int B, hipStream_t st) {
    constexpr size_t lds = (size_t)CondUnetLds<T, NB>::FLOATS * 4;
    LDS_LIMIT((&cond_unet_kernel<T, NB>), lds);
    hipLaunchKernelGGL((cond_unet_kernel<T, NB>), dim3((B + NB - 1) / NB), dim3(NTHREADS), lds, st, w->dbuf, data, fi, seg_len, emb, B);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

// MFMA kernel of the long windows (12 < T <= 32); slabs: tl_slab_floats(TP) floats per workgroup
// chains per workgroup of the slab-tiled kernel: one -- at 16 frames two workgroups per CU instead of two chains in one: +10.6 %
// (profiles/r04v_tl16_nb1_ab.txt)
constexpr int tl_nb(int) { return 1; }
// workgroups per CU: a single 16-frame chain leaves room for two (75 KB of LDS each, 128 registers)
constexpr int tl_wgs_per_cu(int TP) { return TP * tl_nb(TP) <= 16 ? 2 : 1; }
template <int TP, int NB, bool LT = false, bool COND = false>
int launch_score_tiled_t(const mcd_weights* w, const ScoreParams& P, const FrameMaps& M, float* scratch, int wgs, hipStream_t st) {
    MCD_WAVES_CHECK(COND ? NWAVES : shipped_waves_tiled(TP));      // (the COND form -- the 'E_unet' encoder on the tiled stages -- runs on eight or twelve)
    using LD = TiledLds<TP, NB>;
    // the three shipped shapes (one chain, the shipped wave count), pinned: a change of the plan shows up here
    static_assert(NB != 1 || NTHREADS != 64 * shipped_waves_tiled(TP) || LD::BYTES == (TP == 16 ? 81824 : TP == 24 ? 148704 : 154656),
                  "TiledLds: the LDS of a shipped shape changed");
    constexpr size_t lds = LD::BYTES;
    LDS_LIMIT((&score_tiled_kernel<TP, NB, LT, COND>), lds);
    ScoreParams Q = P;
    Q.prio_shift = 0;
    const PhaseOpt ph = decode_phase(P.phase);
    if (LD::TF <= 16 && !LT && !COND && P.mode == 0 && ph.slices && wgs > 0) {
        // priority time slice of the two co-resident workgroups: about 1/6 of the launch -- chains per workgroup x passes x
        // ~190 us per pass of a 16-frame chain sharing its CU (2.4 GHz), in ticks of the 100 MHz clock
        const double per_wg = (double)((P.n_chains + (long long)wgs * NB - 1) / ((long long)wgs * NB));
        const double ticks = per_wg * (double)(P.ns > 2 ? P.ns - 1 : 1) * 190.0 * 100.0;
        Q.prio_shift = prio_slice_shift(ticks, ph.forced_shift);
    }
    hipLaunchKernelGGL((score_tiled_kernel<TP, NB, LT, COND>), dim3(wgs), dim3(NTHREADS), lds, st, Q, M, COND ? w->tiled_cond : w->tiled,
                       COND ? w->cond.Tc : w->cfg.t_unet, scratch);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}


// Every instantiation lives in exactly one unit of mcd_inst.hip; everywhere else it is only declared.  (A row whose unit no
// compilation selects would be declared here and defined nowhere: refused.)
#define MCD_UNIT_OK(unit) static_assert((unit) >= 1 && (unit) <= MCD_INST_UNITS, "mcd_instances.hpp: a row names a unit above MCD_INST_UNITS");
#define MCD_DECL_SCORE(unit, T, NB, MINW, LT) MCD_UNIT_OK(unit) extern template int launch_score_t<T, NB, MINW, LT>(ScoreParams&, hipStream_t, bool*);
#define MCD_DECL_VARIANT(unit, variant, T, NB, MINW) MCD_DECL_SCORE(unit, T, NB, MINW, false)
#define MCD_DECL_COND_FAST(unit, T, NB) \
    MCD_UNIT_OK(unit) extern template int launch_cond_fast_t<T, NB>(const mcd_weights*, const DataView&, const FrameIdx&, int, float*, int, hipStream_t);
#define MCD_DECL_COND_UNET(unit, T, NB) \
    MCD_UNIT_OK(unit) extern template int launch_cond_unet_t<T, NB>(const mcd_weights*, const DataView&, const FrameIdx&, int, float*, int, hipStream_t);
#define MCD_DECL_TILED(unit, TP, NB, LT) \
    MCD_UNIT_OK(unit) extern template int launch_score_tiled_t<TP, NB, LT>(const mcd_weights*, const ScoreParams&, const FrameMaps&, float*, int, hipStream_t);
#define MCD_DECL_TILED_COND(unit, TP, NB) \
    MCD_UNIT_OK(unit) extern template int launch_score_tiled_t<TP, NB, false, true>(const mcd_weights*, const ScoreParams&, const FrameMaps&, float*, int, hipStream_t);
MCD_SCORE_INSTANCES(MCD_DECL_SCORE)
MCD_SCORE_VARIANT_INSTANCES(MCD_DECL_VARIANT)
MCD_COND_FAST_INSTANCES(MCD_DECL_COND_FAST)
MCD_COND_UNET_INSTANCES(MCD_DECL_COND_UNET)
MCD_TILED_INSTANCES(MCD_DECL_TILED)
MCD_TILED_COND_INSTANCES(MCD_DECL_TILED_COND)

}  // namespace mcd

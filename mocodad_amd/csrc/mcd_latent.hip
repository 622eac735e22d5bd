// mcd_latent.hip — the translation unit of the MoCoDADlatent kernels (mcd_latent_kernel.hpp, and latent_encode_kernel of
// mcd_encode_kernel.hpp, which mcd_launch.hpp brings) and their launchers; built with
// the default eight waves per workgroup (the chain kernel has its own four).  Compiled once as it is (unit 0: the dispatch, the
// chain, projection and Philox kernels, the encode kernels of the rows of unit 0) and once per unit n = 1 .. MCD_LATENT_UNITS
// with -DMCD_LATENT_UNIT=n (the encode / decode kernels of that unit's rows only); see MCD_LATENT_ENCODE_INSTANCES and
// MCD_LATENT_DECODE_INSTANCES / MCD_LATENT_DECODE_SAMPLES_INSTANCES in mcd_instances.hpp.  Unit 0 also holds latent_unproject_kernel.
#undef MCD_NWAVES      // (a developer build may name another wave count for its trajectory kernel)
#ifndef MCD_LATENT_UNIT
#define MCD_LATENT_UNIT 0
#endif
#include "mcd_launch.hpp"
#if MCD_LATENT_UNIT == 0
#include "mcd_latent_kernel.hpp"
#endif

namespace mcd {

static_assert(MCD_LATENT_UNIT >= 0 && MCD_LATENT_UNIT <= MCD_LATENT_UNITS, "compile with -DMCD_LATENT_UNIT=<n>, n = 1 .. MCD_LATENT_UNITS, or without");

// MCD_LATENT_ENCODE_INSTANCES (mcd_instances.hpp): X(unit, T, NB, COND_IN_KERNEL, PROJECT_IN_KERNEL).  A developer build holds the
// 3-frame rows and the row of its frame count, in unit 0.  (That rule compares a row's T with MCD_FAST_T, a value: the token-pasting
// probe MCD_IN_UNIT of mcd_inst.hip cannot state it, so the rows reach their unit through one held-here / not-here template.)
#ifdef MCD_FAST_T
constexpr bool latent_row_held(int t) { return t == 3 || t == MCD_FAST_T; }
constexpr int latent_row_unit(int) { return 0; }
#else
constexpr bool latent_row_held(int) { return true; }
constexpr int latent_row_unit(int unit) { return unit; }
#endif

// A row of a table: its argument struct, which calls it serves, its launch.  Only launch() names the kernel, and only the unit that
// holds the row calls it (RowIn below).
template <int T, int NB, bool CI, bool PIK>
struct EncodeRow {
    using Args = LatentEncodeArgs;
    static bool serves(int t, const Args& a) { return t == T && a.cond_in_kernel == CI; }
    static int launch(const Args& a) {
        static_assert(NWAVES == 8, "the latent encode launch ships with eight waves per workgroup");
        static_assert(PIK || !CI, "the rows that project in a launch of their own take cond_emb from a launch of its own as well");
        constexpr size_t lds = (size_t)LatentEncLds<T, NB, PIK>::FLOATS * 4;
        static_assert(lds <= 160 * 1024, "latent encode: more than 160 KB of LDS");
        LDS_LIMIT((&latent_encode_kernel<T, NB, CI, PIK>), lds);
        hipLaunchKernelGGL((latent_encode_kernel<T, NB, CI, PIK>), dim3((a.B + NB - 1) / NB), dim3(NTHREADS), lds, a.st, a.wbuf, a.call.dv, a.call.cond_fi,
                           a.call.fi, a.call.seg_len, a.call.pe_row, a.cond_out, a.out, a.D, a.B);
        HIP_TRY(hipGetLastError());
        return MCD_OK;
    }
};
// MCD_LATENT_DECODE_INSTANCES (mcd_instances.hpp): X(unit, T), the decode launch of the autoencoder
template <int T>
struct DecodeRow {
    using Args = LatentDecodeArgs;
    static bool serves(int t, const Args&) { return t == T; }
    static int launch(const Args& a) {
        static_assert(NWAVES == 8, "the latent decode launch ships with eight waves per workgroup");
        constexpr size_t lds = (size_t)LatentDecLds<T>::FLOATS * 4;
        static_assert(lds <= 160 * 1024, "latent decode: more than 160 KB of LDS");
        LDS_LIMIT((&latent_decode_kernel<T>), lds);
        hipLaunchKernelGGL((latent_decode_kernel<T>), dim3(a.B), dim3(NTHREADS), lds, a.st, a.wbuf, a.call.dv, a.call.fi, a.call.seg_len, a.call.pe_row,
                           a.cond, a.G, a.pose_out, a.loss_out, a.loss_fn, a.B);
        HIP_TRY(hipGetLastError());
        return MCD_OK;
    }
};
// How many of a window's S samples one workgroup of latent_decode_samples_kernel takes (the ONE statement of the rule; a heuristic,
// measured at two batch sizes only: DESIGN.md 2.6c).  The stem is per workgroup, so a window's samples are split only while the
// windows alone leave workgroup slots of the device empty: the fewest groups g <= S with nb g >= slots, spw = ceil(S / g).  nb >= slots:
// g = 1, one workgroup per window and the stem once.
inline int latent_samples_per_wg(int nb, int S, int slots) {
    int g = (slots + nb - 1) / nb;
    g = g < 1 ? 1 : (g > S ? S : g);
    return (S + g - 1) / g;
}
// MCD_LATENT_DECODE_SAMPLES_INSTANCES (mcd_instances.hpp): X(unit, T), the decode launch for all samples of a window
template <int T>
struct DecodeSamplesRow {
    using Args = LatentDecodeSamplesArgs;
    static bool serves(int t, const Args&) { return t == T; }
    static int launch(const Args& a) {
        static_assert(NWAVES == 8, "the latent decode launch ships with eight waves per workgroup");
        constexpr size_t lds = (size_t)LatentDecLds<T>::FLOATS * 4;
        static_assert(lds <= 160 * 1024, "latent decode: more than 160 KB of LDS");
        LDS_LIMIT((&latent_decode_samples_kernel<T>), lds);
        static std::atomic<int> slots_cache[64];
        const int slots = wg_slots(reinterpret_cast<const void*>(&latent_decode_samples_kernel<T>), lds, slots_cache, NTHREADS);
        const int spw = a.force_spw > 0 ? (a.force_spw < a.S ? a.force_spw : a.S) : latent_samples_per_wg(a.nb, a.S, slots);
        hipLaunchKernelGGL((latent_decode_samples_kernel<T>), dim3(a.nb, (a.S + spw - 1) / spw), dim3(NTHREADS), lds, a.st, a.wbuf, a.call.dv,
                           a.call.fi, a.call.seg_len, a.call.pe_row, a.cond, a.G, a.pose_all, a.loss_all, a.loss_fn, a.b0, a.B, a.S, spw);
        HIP_TRY(hipGetLastError());
        return MCD_OK;
    }
};
// the tables as MCD_ROW(unit, T, row type)
#define MCD_ENCODE_ROW(unit, T, NB, CI, PIK) MCD_ROW(unit, T, EncodeRow<T, NB, CI, PIK>)
#define MCD_DECODE_ROW(unit, T) MCD_ROW(unit, T, DecodeRow<T>)
#define MCD_DECODE_SAMPLES_ROW(unit, T) MCD_ROW(unit, T, DecodeSamplesRow<T>)

// a row's launcher in the unit that holds the row; elsewhere nothing of it is instantiated
template <bool HERE, class Row>
struct RowIn {
    static int go(const typename Row::Args& a) { return Row::launch(a); }
};
template <class Row>
struct RowIn<false, Row> {
    static int go(const typename Row::Args&) { return fail(MCD_EUNSUPPORTED, "latent launch: the row is not part of this unit"); }
};

// the dispatch over the rows of unit U that take Args: defined by the translation unit compiled as that unit
template <int U, class Args>
int launch_latent_unit(int t, const Args& a);
#define MCD_ROW(unit, T, ...) template <> int launch_latent_unit<latent_row_unit(unit), __VA_ARGS__::Args>(int, const __VA_ARGS__::Args&);
MCD_LATENT_ENCODE_INSTANCES(MCD_ENCODE_ROW)
MCD_LATENT_DECODE_INSTANCES(MCD_DECODE_ROW)
MCD_LATENT_DECODE_SAMPLES_INSTANCES(MCD_DECODE_SAMPLES_ROW)
#undef MCD_ROW

#define MCD_ROW(unit, T, ...) \
    if (__VA_ARGS__::serves(t, a)) return RowIn<latent_row_held(T) && latent_row_unit(unit) == MCD_LATENT_UNIT, __VA_ARGS__>::go(a);
template <>
int launch_latent_unit<MCD_LATENT_UNIT, LatentEncodeArgs>(int t, const LatentEncodeArgs& a) {
    MCD_LATENT_ENCODE_INSTANCES(MCD_ENCODE_ROW)
    return fail(MCD_EUNSUPPORTED, "latent encode: no such row");
}
template <>
int launch_latent_unit<MCD_LATENT_UNIT, LatentDecodeArgs>(int t, const LatentDecodeArgs& a) {
    MCD_LATENT_DECODE_INSTANCES(MCD_DECODE_ROW)
    return fail(MCD_EUNSUPPORTED, "latent decode: no such row");
}
template <>
int launch_latent_unit<MCD_LATENT_UNIT, LatentDecodeSamplesArgs>(int t, const LatentDecodeSamplesArgs& a) {
    MCD_LATENT_DECODE_SAMPLES_INSTANCES(MCD_DECODE_SAMPLES_ROW)
    return fail(MCD_EUNSUPPORTED, "latent decode (samples): no such row");
}
#undef MCD_ROW

#if MCD_LATENT_UNIT == 0

bool latent_decode_has_kernel(int t) {
#define MCD_ROW(unit, T) if (latent_row_held(T) && t == (T)) return true;
    MCD_LATENT_DECODE_INSTANCES(MCD_ROW)
#undef MCD_ROW
    return false;
}

int launch_latent_unproject(int t, const float* wbuf, const float* z, float* G, int D, int B, hipStream_t st) {
    hipLaunchKernelGGL(latent_unproject_kernel, dim3((B + UNPROJ_NC - 1) / UNPROJ_NC, t), dim3(UNPROJ_THREADS), 0, st, wbuf, z, G, D / 16,
                       LAT_ENC_C * t * 10, B);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

bool latent_encode_has_kernel(int t, bool cond_in_kernel) {
#define MCD_ROW(unit, T, NB, CI, PIK) if (latent_row_held(T) && t == (T) && cond_in_kernel == (CI)) return true;
    MCD_LATENT_ENCODE_INSTANCES(MCD_ROW)
#undef MCD_ROW
    return false;
}

bool latent_project_in_kernel(int t) {
#define MCD_ROW(unit, T, NB, CI, PIK) if (latent_row_held(T) && t == (T) && !(CI)) return PIK;
    MCD_LATENT_ENCODE_INSTANCES(MCD_ROW)
#undef MCD_ROW
    return true;
}

std::string latent_encode_counts() {
    std::string s;
    for (int t = 1; t <= MCD_MAX_FRAMES; ++t)
        if (latent_encode_has_kernel(t, false)) s += (s.empty() ? "" : ", ") + std::to_string(t);
    return s;
}

// the outer dispatch: a row this library holds -> the unit that holds it
#define MCD_ROW(unit, T, ...) \
    if (latent_row_held(T) && __VA_ARGS__::serves(t, a)) return launch_latent_unit<latent_row_unit(unit), __VA_ARGS__::Args>(t, a);
int launch_latent_decode(int t, const LatentDecodeArgs& a) {
    MCD_LATENT_DECODE_INSTANCES(MCD_DECODE_ROW)
    return fail(MCD_EUNSUPPORTED, "the latent decode launch has no kernel for " + std::to_string(t) + " frames");
}

int launch_latent_decode_samples(int t, const LatentDecodeSamplesArgs& a) {
    MCD_LATENT_DECODE_SAMPLES_INSTANCES(MCD_DECODE_SAMPLES_ROW)
    return fail(MCD_EUNSUPPORTED, "the latent decode launch has no kernel for " + std::to_string(t) + " frames");
}

int launch_latent_encode(int t, const LatentEncodeArgs& a) {
    MCD_LATENT_ENCODE_INSTANCES(MCD_ENCODE_ROW)
    return fail(MCD_EUNSUPPORTED, "the latent encode launch has no kernel for " + std::to_string(t) + " frames (instantiated: " + latent_encode_counts() + " corrupt frames)");
}
#undef MCD_ROW

int launch_latent_project(int t, const float* wbuf, const float* H, float* z0_out, int D, int B, hipStream_t st) {
    hipLaunchKernelGGL(latent_project_kernel, dim3((B + PROJ_NC - 1) / PROJ_NC, D / 16), dim3(PROJ_THREADS), 0, st, wbuf, H, z0_out,
                       LAT_ENC_C * t * 10 / 16, D, B);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int launch_latent_chain(const LatentChainParams& P, hipStream_t st) {
    const int per_wg = P.mode == 1 ? LAT_NC : P.wpg * P.S;
    const size_t lds = (size_t)LatentChainLds(P.net.D, per_wg).floats() * 4;
    LDS_LIMIT((&latent_chain_kernel), 160 * 1024);
    const int grid = P.mode == 1 ? (P.B + LAT_NC - 1) / LAT_NC : (P.B + P.wpg - 1) / P.wpg;
    hipLaunchKernelGGL(latent_chain_kernel, dim3(grid), dim3(LAT_THREADS), lds, st, P);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int launch_latent_philox(unsigned long long seed, long long first_window, int B, int S, int K, int D, float* out, hipStream_t st) {
    const long long n = (long long)S * K * B * (D / 4);
    hipLaunchKernelGGL(latent_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, seed, first_window, B, S, K, D, out);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

#endif  // MCD_LATENT_UNIT == 0

}  // namespace mcd

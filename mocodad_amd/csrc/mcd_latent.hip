// mcd_latent.hip — the translation unit of the MoCoDADlatent kernels (mcd_latent_kernel.hpp) and their launchers; built with
// the default eight waves per workgroup (the chain kernel has its own four).
#undef MCD_NWAVES      // (a developer build may name another wave count for its trajectory kernel)
#include "mcd_launch.hpp"
#include "mcd_latent_kernel.hpp"

namespace mcd {

// MCD_LATENT_ENCODE_INSTANCES (mcd_instances.hpp): X(T, NB, COND_IN_KERNEL) -- T corrupt frames; the fused form also T condition frames
bool latent_encode_has_kernel(int t, bool cond_in_kernel) {
#define MCD_ROW(T, NB, CI) if (t == (T) && cond_in_kernel == (CI)) return true;
    MCD_LATENT_ENCODE_INSTANCES(MCD_ROW)
#undef MCD_ROW
    return false;
}

template <int T, int NB, bool CI>
static int launch_latent_encode_t(const float* wbuf, const DataView& dv, const FrameIdx& cond_fi, const FrameIdx& fi, int seg_len,
                                  const float* pe_row, float* cond_out, float* z0_out, int D, int B, hipStream_t st) {
    static_assert(NWAVES == 8, "the latent encode launch ships with eight waves per workgroup");
    constexpr size_t lds = (size_t)LatentEncLds<T, NB>::FLOATS * 4;
    static_assert(lds <= 160 * 1024, "latent encode: more than 160 KB of LDS");
    LDS_LIMIT((&latent_encode_kernel<T, NB, CI>), lds);
    hipLaunchKernelGGL((latent_encode_kernel<T, NB, CI>), dim3((B + NB - 1) / NB), dim3(NTHREADS), lds, st, wbuf, dv, cond_fi, fi, seg_len,
                       pe_row, cond_out, z0_out, D, B);
    HIP_TRY(hipGetLastError());
    return MCD_OK;
}

int launch_latent_encode(int t, bool cond_in_kernel, const float* wbuf, const DataView& dv, const FrameIdx& cond_fi, const FrameIdx& fi,
                         int seg_len, const float* pe_row, float* cond_out, float* z0_out, int D, int B, hipStream_t st) {
#define MCD_ROW(T, NB, CI) \
    if (t == (T) && cond_in_kernel == (CI)) return launch_latent_encode_t<T, NB, CI>(wbuf, dv, cond_fi, fi, seg_len, pe_row, cond_out, z0_out, D, B, st);
    MCD_LATENT_ENCODE_INSTANCES(MCD_ROW)
#undef MCD_ROW
    return fail(MCD_EUNSUPPORTED, "the latent encode launch has no kernel for " + std::to_string(t) + " frames (instantiated: 3 corrupt frames)");
}

int launch_latent_chain(const LatentChainParams& P, hipStream_t st) {
    const int per_wg = P.mode == 1 ? LAT_NC : P.wpg * P.S;
    const size_t lds = (size_t)latent_chain_lds_floats(P.net.D, per_wg) * 4;
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

}  // namespace mcd

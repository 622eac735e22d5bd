// mcd_chain.hpp — what a reverse-diffusion chain IS, stated once for every kernel that runs one: the call's parameters
// (ScoreParams, DataView, FrameMaps), the frame layout of a window (fm_*), the draws (Philox4x32-10 + Box-Muller: chain_xT,
// chain_step_noise4, latent_philox4), the loss element and the aggregation over the samples.  A chain is one (window b, sample s)
// pair: x_T, ns - 1 DDPM steps (the last without noise), a loss against the window.  Three kernels keep text of their own where a call
// moved their code (profiles/chain_contract_codeobj.json): score_kernel and score_tiled_kernel state their draws and their corrupt-frame loop
// themselves (and the Philox rounds are a macro, not a function); latent_chain_kernel takes its key from latent_philox4 but reads the parity
// tensor in place (profiles/chain_contract_ab.json).  Each such site names the statement here it must agree with, and
// tests/test_chain_bits_gpu.py holds the copies together.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mocodad_hip.h"

namespace mcd {

constexpr int C0 = 2;        // num_coords

// where the windows live: a dense (B,C,T,V) tensor, or a view into trajectory buffers with an optional affine
// test-time transform applied on load (mcd_window_view_t)
struct DataView {
    const float* data;
    const long long* base;
    long long sc, st;
    const int* trans;
    const float* aff;
};
__device__ __forceinline__ float load_coord(const DataView& dv, int b, int c, int t, int v, int seg_len) {
    const long long sc = dv.base ? dv.sc : (long long)seg_len * 17;
    const long long st = dv.base ? dv.st : 17;
    const float* p = dv.data + (dv.base ? dv.base[b] : (long long)b * C0 * seg_len * 17) + t * st + v;
    if (!dv.trans) return p[c * sc];
    const float x = p[0], y = p[sc];
    const float* a = dv.aff + dv.trans[b] * 6 + c * 3;
    return (a[0] * x + a[1] * y) + a[2];
}

struct ScoreParams {
    unsigned long long* prof; // stage timing accumulators (MCD_PROFILE builds) or null
    const float* wbuf;        // packed weights; first TAB_FLOATS words = offset table
    DataView dv;              // windows: (B,C,T,V) tensor or a trajectory view
    const float* noise;       // (S,K,B,C,Tx,V) or null
    const float* cond_emb;    // (B,16) or null
    const float* step_table;  // (ns, 4+16)
    const float* x_in;        // single-pass mode: (B,C,Tu,V)
    float* loss_out;          // (B,S)
    float* pose_out;          // (B,S,C,Tx,V) or null
    float* eps_out;           // single-pass mode
    unsigned long long seed;
    long long first_window;
    int B, S, ns, seg_len, n_corrupt, loss_fn, mode, step_single, n_chains;
    // A workgroup owns NB WINDOWS (group g = blockIdx / split) and runs the samples s = part, part + split, ... of both
    // (part = blockIdx % split) one trajectory after the other.  split = 1: it sees every sample of its windows, so the
    // condition encoder runs once per workgroup in its own LDS (cond_inkernel) and the aggregation over the samples
    // (loss_agg, aggr, aggr_q) happens here too: ONE launch per scoring call.
    int split, aggr, cond_inkernel;
    int force_split;          // host only (MCD_OPT_SPLIT): 0 = choose
    int loss_out_optional;    // host only: loss_out is the library's own scratch, not wanted when the aggregation is fused
    int plan_only;            // host only: choose `split`, do not launch
    int phase;                // MCD_OPT_PHASE, raw (its table: mocodad_hip.h; the host's reading: decode_phase, mcd_launch.hpp)
    int prio_shift;           // host: log2 of the priority time slice in 100 MHz ticks (see the top of the step loop); 0 = off
                              // (an ESTIMATE from the shapes; the kernel replaces it by a sixth of the measured duration of the
                              // previous launch of the same grid when `tune` holds one)
    int prio_rounds;          // host: rounds of workgroups of this launch (grid / resident slots, rounded up)
    int* tune;                // per-handle device words: [0] signature (grid, S, ns) of the launch that wrote [1] = lifetime of its
                              // workgroup 0 in 100 MHz ticks; or null
    float aggr_q;
    float* loss_agg;          // (B,) aggregated loss, or null
    int cond_idx[12];         // cond_inkernel: data frames the condition encoder reads
    int upd_shift;            // some prediction updates a frame other than the one it is read at (element-wise tail: barrier between reads and writes)
    unsigned fixed_mask;      // bit t: U-Net frame t is a condition frame copied from the window (concat / imputation)
    int src_frame[12];        // data frame feeding U-Net frame t (condition frame, or ground truth of a denoised one)
    int tx_of[12];            // denoised U-Net frame t -> its index among the corrupt frames
    int pos_of[12];           // corrupt frame k -> its U-Net frame
    int upd_of[12];           // U-Net frame t -> corrupt frame whose eps-prediction is read at t (-1: none)
    const int* win_mask;      // random_imp: (B,) per-window bitmask of the condition frames (frames in natural order;
                              // replaces fixed_mask and the four maps above, which are then derived from the mask)
    // layer-test instantiation only (mcd_layer_forward): stage id (0..10 ST-GCN layer, 11 down1, 12 down2, 13 up3, 14 up2),
    // its input (B,Cin,T,Vin) and output (B,Cout,T,Vout)
    int lt_stage;
    const float* lt_in;
    float* lt_out;
    const float* lt_skip;     // slab-tiled kernel, stages 7 / 9: the U-Net skip tensor added behind the fused resampler (or null)
};
// data frames a condition encoder reads, in order
struct FrameIdx { int idx[MCD_MAX_FRAMES]; };
// U-Net frame layout of a scoring call for the kernels that take it at run time (more than 12 frames)
struct FrameMaps { int src_frame[MCD_MAX_FRAMES], tx_of[MCD_MAX_FRAMES], pos_of[MCD_MAX_FRAMES], upd_of[MCD_MAX_FRAMES]; };

// Frame layout of one window.  `fixed` = its condition-frame bitmask (P.fixed_mask, or the window's own for random_imp: frames in
// natural order, maps derived from the mask).  M holds the maps: ScoreParams (score_kernel, 12 entries) or FrameMaps -- same member names.
// denoised U-Net frame t -> its index among the corrupt frames
template <class PS, class MS>
__device__ __forceinline__ int fm_tx(const PS& P, const MS& M, unsigned fixed, int t) { return P.win_mask ? __popc(~fixed & ((1u << t) - 1u)) : M.tx_of[t]; }
// data frame feeding U-Net frame t (a condition frame, or the ground truth of a denoised one)
template <class PS, class MS>
__device__ __forceinline__ int fm_src(const PS& P, const MS& M, int t) { return P.win_mask ? t : M.src_frame[t]; }
// U-Net frame whose chain state the eps-prediction read at frame t updates, or -1 (mocodad.py:829-838)
template <class PS, class MS>
__device__ __forceinline__ int fm_upd(const PS& P, const MS& M, unsigned fixed, int t) {
    if (P.win_mask) return ((fixed >> t) & 1u) ? -1 : t;
    const int k = M.upd_of[t];
    return k >= 0 ? M.pos_of[k] : -1;
}
// U-Net frame of the tx-th corrupt frame among T: the tx-th clear bit of the window's mask.  (A mask with fewer than tx + 1 clear
// bits keeps M.pos_of[tx]; nth_set_bit would return -1 there.)
template <class PS, class MS>
__device__ __forceinline__ int fm_corrupt_frame(const PS& P, const MS& M, unsigned fixed, int tx, int T) {
    int tu = M.pos_of[tx];
    if (P.win_mask) { int cnt = 0; for (int t = 0; t < T; ++t) if (!((fixed >> t) & 1u)) { if (cnt == tx) tu = t; ++cnt; } }
    return tu;
}
// today's callers that hold their maps in ScoreParams
__device__ __forceinline__ int fm_tx(const ScoreParams& P, int fixed, int t) { return fm_tx(P, P, (unsigned)fixed, t); }
__device__ __forceinline__ int fm_src(const ScoreParams& P, int t) { return fm_src(P, P, t); }

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= 3.0e38f); }      // NaN / Inf

// Philox4x32-10 + Box-Muller (perf mode noise; parity mode reads the caller's noise tensor)
// The ten rounds over the counter words c0 .. c3 in place.  A macro, not a function: the same rounds behind a call moved
// score_kernel's code objects (profiles/chain_contract_codeobj.json); as text they compile to what the written-out copies did.
#define MCD_PHILOX_ROUNDS(seed, c0, c1, c2, c3)                                            \
    unsigned k0 = (unsigned)(seed), k1 = (unsigned)((seed) >> 32);                         \
    _Pragma("unroll") for (int r = 0; r < 10; ++r) {                                       \
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;                \
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;                \
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;             \
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;             \
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;                                                \
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;                                              \
    }
// all four output words: two Box-Muller pairs = four normals per call
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                               float (&z)[4]) {
    MCD_PHILOX_ROUNDS(seed, c0, c1, c2, c3)
    const unsigned w[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(w[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u2 = ((float)(w[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float r = __fsqrt_rn(-1.38629436111989f * __log2f(u1));       // hardware log2 / sqrt / sin / cos, as below
        z[2 * h] = r * __cosf(6.28318530717958647692f * u2);
        z[2 * h + 1] = r * __sinf(6.28318530717958647692f * u2);
    }
}
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
    MCD_PHILOX_ROUNDS(seed, c0, c1, c2, c3)
    const float u1 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    // Box-Muller on the hardware transcendental units (v_log_f32, v_cos_f32, v_sqrt_f32): this is a noise source,
    // ~1e-6 relative accuracy is irrelevant to its distribution
    return __fsqrt_rn(-1.38629436111989f * __log2f(u1)) * __cosf(6.28318530717958647692f * u2);
}
// the four raw words of one call (integer draws: random_imp_masks_kernel)
__device__ __forceinline__ void philox_words4(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned (&w)[4]) {
    MCD_PHILOX_ROUNDS(seed, c0, c1, c2, c3)
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// position of the r-th (0-based, ascending) set bit of m; PRECONDITION: r < popcount(m).  Clears the r lowest set bits: no
// per-thread array, nothing for scratch memory.
__device__ __forceinline__ int nth_set_bit(unsigned m, int r) {
    for (int i = 0; i < r; ++i) m &= m - 1u;
    return __ffs(m) - 1;
}
__device__ __forceinline__ unsigned low_bits(int n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

// The draws of a chain.  KEY LAYOUT (the only statement of it): a Philox call is keyed (seed; c0, c1, c2, c3) with
//   c1 = noise slot k (0 = x_T, k >= 1 = the z of step ns - k), c2 = sample s, c3 = global window id first_window + b, and
//   c0 = x_T:        the element (c * Tx + tx) * 17 + v            -- one call per element, its first normal (philox_normal)
//        step noise: the joint pair tx * 9 + v0 / 2 of frame tx    -- one call per pair, four normals (philox_normal4):
//                    z[0], z[1] = coordinates 0, 1 of joint v0; z[2], z[3] = of joint v0 + 1 (unused at v0 = 16)
//        latent:     the element group d0 / 4 (latent_philox4)     -- one call per group of four latent elements, any slot
// (random_imp_masks_kernel draws with c1 = c2 = ~0: no call coincides with a noise call.)  Parity mode reads the same element of
// the caller's tensor instead: (S, K, B, C, Tx, V) for poses, (S, K, B, D) for latents, K = max(ns - 1, 1), per = C * Tx * V.
__device__ __forceinline__ float chain_xT_philox(unsigned long long seed, long long first_window, int b, int s, int Tx, int c, int tx, int v) {
    return philox_normal(seed, (unsigned)((c * Tx + tx) * 17 + v), 0u, (unsigned)s, (unsigned)(first_window + b));
}
__device__ __forceinline__ void chain_step_philox4(unsigned long long seed, long long first_window, int b, int s, int k, int tx, int v0, float (&z)[4]) {
    philox_normal4(seed, (unsigned)(tx * 9 + (v0 >> 1)), (unsigned)k, (unsigned)s, (unsigned)(first_window + b), z);
}
__device__ __forceinline__ void latent_philox4(unsigned long long seed, long long first_window, int b, int s, int k, int d0, float (&z)[4]) {
    philox_normal4(seed, (unsigned)(d0 >> 2), (unsigned)k, (unsigned)s, (unsigned)(first_window + b), z);
}
// x_T element of (window b, sample s, corrupt frame tx, coordinate c, joint v)
template <class PS>
__device__ __forceinline__ float chain_xT(const PS& P, int b, int s, int K, int per, int c, int tx, int v) {
    const int Tx = P.n_corrupt;
    return P.noise ? P.noise[((size_t)(s * K + 0) * P.B + b) * per + (c * Tx + tx) * 17 + v]
                   : chain_xT_philox(P.seed, P.first_window, b, s, Tx, c, tx, v);
}
// step-k noise of the joint pair (v0, v0 + 1), v0 even, of corrupt frame tx
template <class PS>
__device__ __forceinline__ void chain_step_noise4(const PS& P, int b, int s, int k, int K, int per, int Tx, int tx, int v0, float (&z)[4]) {
    if (P.noise) {
        const float* zp = P.noise + ((size_t)(s * K + k) * P.B + b) * per + tx * 17 + v0;
        z[0] = zp[0]; z[1] = zp[Tx * 17];
        if (v0 + 1 < 17) { z[2] = zp[1]; z[3] = zp[Tx * 17 + 1]; }
    } else {
        chain_step_philox4(P.seed, P.first_window, b, s, k, tx, v0, z);
    }
}
__device__ __forceinline__ float loss_elem(float a, float b, int fn) {
    const float d = fabsf(a - b);
    if (fn == MCD_LOSS_SMOOTH_L1) return d < 1.f ? 0.5f * d * d : d - 0.5f;
    if (fn == MCD_LOSS_L1) return d;
    return d * d;
}

// aggregation of one window's S per-sample losses (mocodad.py:504-512 best / worst with strict comparisons from 1e10 / -1,
// :489-492 mean / median, :513-516 quantile): torch's conventions -- median = lower middle, quantile = linear interpolation
// (torch.lerp).  Sorts L in place for the order statistics.
__device__ __forceinline__ float aggregate_losses(float* L, int S, int strategy, float q) {
    if (strategy == MCD_AGGR_BEST || strategy == MCD_AGGR_WORST) {
        const bool best = strategy == MCD_AGGR_BEST;
        float cur = best ? 1e10f : -1.f;
        for (int s = 0; s < S; ++s) if (best ? (L[s] < cur) : (L[s] > cur)) cur = L[s];
        return cur;
    }
    if (strategy == MCD_AGGR_MEAN) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += L[s];
        return sum / (float)S;
    }
    for (int s = 0; s < S; ++s)            // torch.median / torch.quantile return NaN when a sample is NaN (a diverged chain);
        if (L[s] != L[s]) return L[s];     // a comparison sort would leave an arbitrary finite value at the rank instead
    for (int i = 1; i < S; ++i) {          // insertion sort (S <= 64)
        const float x = L[i];
        int k = i - 1;
        while (k >= 0 && L[k] > x) { L[k + 1] = L[k]; --k; }
        L[k + 1] = x;
    }
    if (strategy == MCD_AGGR_MEDIAN) return L[(S - 1) / 2];
    const float pos = fminf(fmaxf(q, 0.f), 1.f) * (float)(S - 1);      // (q is validated on the host; the clamp is a backstop)
    const int lo = (int)floorf(pos);
    const int hi = lo + 1 < S ? lo + 1 : S - 1;
    const float wgt = pos - (float)lo;
    const float a = L[lo], c = L[hi];
    return wgt < 0.5f ? a + wgt * (c - a) : c - (c - a) * (1.f - wgt);
}

}  // namespace mcd

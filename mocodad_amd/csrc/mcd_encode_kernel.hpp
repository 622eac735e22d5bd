// mcd_encode_kernel.hpp — the encoder family: the MFMA condition encoders of the pose model, cond_fast_kernel<T, NB> (shipped
// channel list) and cond_unet_kernel<T, NB> ('E_unet'), and the latent model's encode launch latent_encode_kernel<T, NB,
// COND_IN_KERNEL, PROJECT_IN_KERNEL>, and the decode launches of its pretrain stage, latent_decode_kernel<T> and
// latent_decode_samples_kernel<T> (at the end of the file; they share latent_decode_stem and latent_decode_row).
// The first three are a window loader, stage functions of mcd_device.hpp on an LDS plan and a Linear over the (c,t,v) flattening;
// the decode launch is the same loader and the same down stem, capturing the skips, in front of the up path.  The shared pieces are
// stated here once: load_window_frames (all four), unet_down_stem (the 'E_unet' encoder, the encode and the decode launch; with layer
// 5 it is unet_down_path), step_embedding (the encode and the decode launch), flatten_linear (the two encoders' tails)
// (DESIGN.md 2.1-2.2, 2.6).  cond_fast_body, also the trajectory kernel's prologue (score_kernel, P.cond_inkernel), keeps its own
// loader and tail.
#pragma once
#include "mcd_device.hpp"
#include "mcd_latent.hpp"

namespace mcd {

constexpr int TABC = 128;                  // cond table: second 128 words of the weight buffer
constexpr int TABC_LW = 40, TABC_LB = 41;  // bottleneck Linear weight [16][32*T*17] / bias
constexpr int TABC_URS = 56;               // down1 / down2 fragments + bias: 4 words
constexpr int TABC_ULW = 60, TABC_ULB = 61;  // to_time_dim weight [16][6*T*10] / bias
constexpr int CU_OUT = 6;                  // unet_down_channels[6] of STSE_Unet

// ------------------------------------------------------------------------------------------------
// Window isolation: the NB windows of a workgroup are columns of the same MFMA tiles, and the padded k-steps of the
// mixes and resamplers read the NEXT window's rows against zero coefficients -- NaN x 0 = NaN, so a window with a non-finite pose
// (or whose encoding overflows) reaches its neighbours' results, where the reference's windows are independent
// (mocodad.py:155-180).  A window's columns never see a neighbour's FINITE values, so: every encoder below runs its windows
// jointly, tests the joint RESULT once (the NB x 16 embeddings, a flag per window set by the threads that store z0), and behind a
// result that is not finite runs again once per such window ALONE (`solo`: the other slots load zeros and store nothing) on a
// region cleared again.  A finite window gets the bits of the joint run back; a non-finite one what it yields as the only window
// of a call.  Slots past the end of the batch repeat the last window, are never tested and never run alone.
// The solo runs are a second, cold instance of the same functions (OPAQUE = true: thread id and weight pointer are made opaque
// per run, or every per-lane address of the pass is hoisted in front of the loop and kept live -- as in score_kernel's step
// loop); the joint run keeps the straight-line text it had, plus the test.  score_kernel's prologue, where a second instance of
// cond_fast_body would double the trajectory kernels' encoder text, loops over the opaque one instead.
// (Which stages do it: the 12- / 10-joint mixes and the resamplers of the down path -- cond_unet_kernel, latent_encode_kernel.  A
// 17-joint mix does not: its trailing k-step holds joint 16 alone and every lane group reads that joint again, mix_stage's load_x --
// so cond_fast_body's four 17-joint layers cannot leak as they stand; its result is tested all the same, so that the guarantee
// does not rest on that detail of the mix.)
// ------------------------------------------------------------------------------------------------
// the barrier between the joint run's last stores and the test: behind the workgroup's LDS traffic (the flags) alone -- nothing
// here needs the results just stored to global memory to have arrived, which __syncthreads(), a release fence as well, waits for
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the first slot behind `solo` of the workgroup's windows b0 .. whose 16 embeddings ce[n][16] (LDS) are not all finite; -1: none.
// Every thread reads the same words: the answer is uniform.
template <int NB>
__device__ __forceinline__ int next_nonfinite_slot(const float* ce, int solo, int b0, int B) {
    int nxt = -1;
#pragma unroll
    for (int n = NB - 1; n >= 0; --n) {
        bool bad = false;
#pragma unroll
        for (int k = 0; k < EDIM; ++k) bad |= not_finite(ce[n * EDIM + k]);
        if (bad && n > solo && b0 + n < B) nxt = n;
    }
    return __builtin_amdgcn_readfirstlane(nxt);
}
// ... the same from one flag per slot (set while the joint run stored its results)
template <int NB>
__device__ __forceinline__ int next_flagged_slot(const int* bad, int solo) {
    int nxt = -1;
#pragma unroll
    for (int n = NB - 1; n >= 0; --n)
        if (bad[n] && n > solo) nxt = n;
    return __builtin_amdgcn_readfirstlane(nxt);
}

// condition / corrupt frames of windows b0 .. b0 + NB - 1 -> dst[col = (n,t,v)][20], channels 0, 1; frame_of(t) = data frame of
// frame t.  A window past the end repeats the last one.  solo >= 0: that slot alone, the others hold zeros.
template <int T, int NB, bool OPAQUE = false, class FrameOf>
__device__ __forceinline__ void load_window_frames(float* dst, const DataView& dv, FrameOf&& frame_of, int seg_len, int b0, int B, int solo = -1) {
    constexpr int TV = T * 17, COLS = NB * TV;
    int tid = threadIdx.x;
    if constexpr (OPAQUE) asm volatile("" : "+v"(tid));
    for (int u = tid; u < COLS * C0; u += NTHREADS) {
        const int c = u % C0, col = u / C0;
        const int n = col / TV, t = (col / 17) % T, v = col % 17;
        const int b = b0 + n < B ? b0 + n : B - 1;
        dst[col * 20 + c] = (NB == 1 || solo < 0 || n == solo) ? load_coord(dv, b, c, frame_of(t), v, seg_len) : 0.f;
    }
}

// The U-Net's down stem 2->16->32->32 | 17->12 | 32->64->64 | 12->10 on Plan<T, NB> (layers 0 .. 4 and the two down-samplers, each
// with its barrier), input at RG + L0_in, output at RG + DN2_out.  tab: the layer table (layer l at l * F_STRIDE); rs: the table
// words, relative to wb, of down1 / down2's fragments and biases.  HASEMB: the embedding EMB + emb_off(l) is added in each layer's
// GEMM epilogue as in score_kernel.  CAPTURE: the down-samplers keep their B operands -- the skip tensors d1 / d2 -- in the caller's
// skip1 / skip2 (resample_stage; rs then names fragments in the capture k order); without it the two arrays are not touched.
struct RsWords { int w1, b1, w2, b2; };
template <int T, int NB, bool HASEMB, bool CAPTURE, int NS1, int NS2>
__device__ __forceinline__ void unet_down_stem(const float* wb, const float* tab, const RsWords rs, float* RG, const float* EMB,
                                               float (&skip1)[NS1], float (&skip2)[NS2], int wave, int lane, Prof& prof) {
    using PL = Plan<T, NB>;
    auto emb = [&](int l) { return HASEMB ? EMB + emb_off(l) : nullptr; };
    layer_generic<16, 16, 17, true, HASEMB, T, NB>(wb, layer_w(tab, 0), RG + PL::L0_in, RG + PL::L0_z, RG + PL::L0_out, emb(0), wave, lane, prof, 0);
    layer_generic<16, 32, 17, true, HASEMB, T, NB>(wb, layer_w(tab, 1), RG + PL::L1_in, RG + PL::L1_z, RG + PL::L1_out, emb(1), wave, lane, prof, 0);
    layer_generic<32, 32, 17, false, HASEMB, T, NB>(wb, layer_w(tab, 2), RG + PL::L2_in, RG + PL::L2_z, RG + PL::L2_out, emb(2), wave, lane, prof, 0);
    {
        RsCoef<32, 17, 12, T, NB, CAPTURE> rc;
        rc.load(wb + tab_i(wb, rs.w1), wb + tab_i(wb, rs.b1), lane);
        resample_stage<32, 17, 12, T, NB, CAPTURE, false>(RG + PL::L2_out, 36, RG + PL::DN1_out, 36, rc, skip1, wave, lane);
        __syncthreads();
    }
    layer_generic<32, 64, 12, true, HASEMB, T, NB>(wb, layer_w(tab, 3), RG + PL::L3_in, RG + PL::L3_z, RG + PL::L3_out, emb(3), wave, lane, prof, 0);
    layer_generic<64, 64, 12, false, HASEMB, T, NB>(wb, layer_w(tab, 4), RG + PL::L4_in, RG + PL::L4_z, RG + PL::L4_out, emb(4), wave, lane, prof, 0);
    {
        RsCoef<64, 12, 10, T, NB, CAPTURE> rc;
        rc.load(wb + tab_i(wb, rs.w2), wb + tab_i(wb, rs.b2), lane);
        resample_stage<64, 12, 10, T, NB, CAPTURE, false>(RG + PL::L4_out, 68, RG + PL::DN2_out, 68, rc, skip2, wave, lane);
        __syncthreads();
    }
}
// The down path of the encoders: the stem without capture, then 64->128 (layer 5), output at RG + L5_out.  The last layer differs
// per kernel: the caller's.
template <int T, int NB, bool HASEMB>
__device__ __forceinline__ void unet_down_path(const float* wb, const float* tab, const RsWords rs, float* RG, const float* EMB,
                                               int wave, int lane, Prof& prof) {
    using PL = Plan<T, NB>;
    float nosk[1] = {0.f};
    unet_down_stem<T, NB, HASEMB, false>(wb, tab, rs, RG, EMB, nosk, nosk, wave, lane, prof);
    layer_generic<64, 128, 10, true, HASEMB, T, NB>(wb, layer_w(tab, 5), RG + PL::L5_in, RG + PL::L5_z, RG + PL::L5_out, HASEMB ? EMB + emb_off(5) : nullptr, wave, lane, prof, 0);
}

// The step embedding of the latent U-Net at its constant time step: SEN[n][16] = SiLU(pe_row + ce[n]) for the workgroup's NB
// windows (solo >= 0: the other slots hold zeros, so that their rows are the bias alone), then rows [0, n_rows) of W_e / b_e:
// EMB[n * stride + o] = b_e[o] + sum_k W_e[o][k] SEN[n][k], one fmaf chain from the bias, k = 0 .. 15.  The barrier between
// the two halves is also the one behind the caller's clearing of its region (in front of the call: the window is loaded behind it);
// the rows are published by the caller's next barrier.  (With the caller's clearing and loading handed in as a callback between the
// halves -- the order the two kernels had -- latent_encode_kernel<3, 2, true, true> spilled 13 SGPRs where it spills 3, and its
// launch left the bar by 1 %: profiles/README.md, "Latent family".)
template <int NB>
__device__ __forceinline__ void step_embedding(const float* wb, const float* __restrict__ pe_row, const float* ce, float* SEN, float* EMB,
                                               int stride, int n_rows, int tid, int solo) {
    if (tid < NB * EDIM) {
        const float e = pe_row[tid % EDIM] + ce[tid];
        SEN[tid] = (solo >= 0 && tid / EDIM != solo) ? 0.f : e / (1.f + expf(-e));
    }
    __syncthreads();
    gfloat* we = as_global(wb + tab_i(wb, TAB_WE));
    gfloat* be = as_global(wb + tab_i(wb, TAB_BE));
    for (int o = tid; o < n_rows; o += NTHREADS) {
        float w[EDIM];
#pragma unroll
        for (int k = 0; k < EDIM; ++k) w[k] = we[o * EDIM + k];
        const float bo = be[o];
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            float a = bo;
#pragma unroll
            for (int k = 0; k < EDIM; ++k) a = fmaf(w[k], SEN[n * EDIM + k], a);
            EMB[n * stride + o] = a;
        }
    }
}

// Linear over the (c, tv) flattening of H[(n TV + tv) CS + c]: out[n][j] = bias[j] + sum_k W[j][k] H[n][k], k = c TV + tv, for the
// NB windows of the workgroup and n_out outputs; store(n, j, value) takes the result.  A thread owns one (output, part of 16) --
// the 16 parts of an output are the 16 lanes of a DPP row -- of one window, or with SHARE_W of all NB windows, which then share
// every weight load.  (c, tv) loops instead of k % TV, k / TV per element, with compile-time trip counts (the ragged last
// 16-block is predicated): the loops unroll (UNROLL channels at a time) and the weight loads of several channels are in flight
// together -- with the data-dependent bound `tv + part < TV` every load waited for the FMA before it (one L2 round trip per
// element: 100 .. 400 of them per thread, the whole encoder's time).  An output is one fmaf chain in c-then-i order per part, the
// 16-lane sum, then the bias.
template <int C, int CS, int TV, int NB, bool SHARE_W, int UNROLL, bool OPAQUE = false, class Store>
__device__ __forceinline__ void flatten_linear(const float* H, gfloat* W, gfloat* bias, int n_out, Store&& store) {
    constexpr int F = C * TV, NT16 = (TV + 15) / 16, NW = SHARE_W ? NB : 1;
    int tid = threadIdx.x;
    if constexpr (OPAQUE) asm volatile("" : "+v"(tid));
    for (int u = tid; u < (NB / NW) * n_out * 16; u += NTHREADS) {
        const int part = u & 15, jo = SHARE_W ? u >> 4 : (u >> 4) % n_out, n0 = SHARE_W ? 0 : u / (16 * n_out);
        float a[NW];
#pragma unroll
        for (int n = 0; n < NW; ++n) a[n] = 0.f;
        gfloat* wr = W + (size_t)jo * F + part;
        const float* hr = H + (n0 * TV + part) * CS;
#pragma unroll UNROLL
        for (int c = 0; c < C; ++c) {
            float wv[NT16];
#pragma unroll
            for (int i = 0; i < NT16; ++i) wv[i] = (i * 16 + part < TV) ? wr[c * TV + i * 16] : 0.f;
#pragma unroll
            for (int n = 0; n < NW; ++n)
#pragma unroll
                for (int i = 0; i < NT16; ++i) a[n] = fmaf(wv[i], (i * 16 + part < TV) ? hr[(n * TV + i * 16) * CS + c] : 0.f, a[n]);
        }
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            const float r = row16_sum(a[n]);
            if (part == 0) store(n0 + n, jo, r + bias[jo]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// condition encoder, fast path for the shipped architecture (channels [32,16,32] + h_dim 32, latent 16):
// the same MFMA mix / GEMM stages as the U-Net, NB windows per 512-thread workgroup, followed by the
// bottleneck Linear over the (c,t,v) flattening (stsae.py:73-89).  Reads the condition frames straight from the
// window tensor (no gather pass).  Other channel lists use cond_encode_kernel (mcd_generic_kernel.hpp).
// ------------------------------------------------------------------------------------------------
template <int T, int NB>
struct CondFastLds {     // cond_fast_body's region: X0, Z0 [P17][20] | Y0, Z1 [P17][36]
    static constexpr int P17 = ceil16(NB * T * 17);
    static constexpr int FLOATS = P17 * (2 * 20 + 2 * 36);
};

// body shared by cond_fast_kernel, the trajectory kernel's prologue (P.cond_inkernel) and the latent encode launch: windows
// b0 .. b0 + NB - 1, frame_of(t) = data frame of condition frame t; the embeddings go to emb_lds[n][16] (LDS) and / or emb_out (B,16).
// smem: CondFastLds<T, NB>::FLOATS floats, zeroed by the caller.  solo >= 0: that slot alone (window isolation, above) -- the other
// slots load zeros and store nothing; OPAQUE: the instance a caller runs in a loop.
// Its loader and tail are its own copies of load_window_frames / flatten_linear<32, 36, T * 17, NB, false, 4>: the body is inlined
// into every score_kernel row, and the trajectory kernels' text does not move for a refactor.
template <int T, int NB, bool OPAQUE = false, class FrameOf>
__device__ __forceinline__ void cond_fast_body(const float* wbuf, const DataView& dv, FrameOf&& frame_of, int seg_len, float* smem,
                                               int b0, int B, float* emb_lds, float* __restrict__ emb_out, int solo = -1) {
    constexpr int P17 = ceil16(NB * T * 17);
    constexpr int s16 = P17 * 20, s32 = P17 * 36;
    constexpr int TV = T * 17, COLS = NB * TV;
    float* const X0 = smem;                   // [P17][20]  in of layers 0, 2 ; out of layer 1
    float* const Z0 = smem + s16;             // [P17][20]
    float* const Y0 = smem + 2 * s16;         // [P17][36]  out of layers 0, 2 ; in of layers 1, 3
    float* const Z1 = smem + 2 * s16 + s32;   // [P17][36]
    float* const H = smem;                    // [P17][36]  out of layer 3 (over X0/Z0: 36 <= 40)
    int tid = threadIdx.x;
    if constexpr (OPAQUE) asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    Prof prof;
    prof.off();
    for (int u = tid; u < COLS * C0; u += NTHREADS) {
        const int c = u % C0, col = u / C0;
        const int n = col / TV, t = (col / 17) % T, v = col % 17;
        const int b = b0 + n < B ? b0 + n : B - 1;
        X0[col * 20 + c] = (NB == 1 || solo < 0 || n == solo) ? load_coord(dv, b, c, frame_of(t), v, seg_len) : 0.f;
    }
    bsync();
    const float* wb = wbuf;
    if constexpr (OPAQUE) asm volatile("" : "+s"(wb));
    layer_generic<16, 32, 17, true, false, T, NB>(wb, layer_w(wb + TABC, 0), X0, Z0, Y0, nullptr, wave, lane, prof, 0);   // 2(16) -> 32
    layer_generic<32, 16, 17, true, false, T, NB>(wb, layer_w(wb + TABC, 1), Y0, Z1, X0, nullptr, wave, lane, prof, 0);   // 32 -> 16
    layer_generic<16, 32, 17, true, false, T, NB>(wb, layer_w(wb + TABC, 2), X0, Z0, Y0, nullptr, wave, lane, prof, 0);   // 16 -> 32
    layer_generic<32, 32, 17, false, false, T, NB>(wb, layer_w(wb + TABC, 3), Y0, Z1, H, nullptr, wave, lane, prof, 0);   // 32 -> 32
    // bottleneck Linear: emb[n][j] = b[j] + sum_k W[j][k] H[n][k], k = c*TV + tv.  thread = (n, j, part of 16)
    constexpr int F = 32 * TV;
    gfloat* W = as_global(wb + tab_i(wb, TABC + TABC_LW));
    gfloat* bb = as_global(wb + tab_i(wb, TABC + TABC_LB));
    for (int u = tid; u < NB * EDIM * 16; u += NTHREADS) {
        const int part = u & 15, jo = (u >> 4) % EDIM, n = u / (16 * EDIM);
        constexpr int NT16 = (TV + 15) / 16;      // (compile-time trip counts: see flatten_linear)
        float a = 0.f;
        gfloat* wr = W + jo * F + part;
        const float* hr = H + (n * TV + part) * 36;
#pragma unroll 4
        for (int c = 0; c < 32; ++c) {
            float wv[NT16];
#pragma unroll
            for (int i = 0; i < NT16; ++i) wv[i] = (i * 16 + part < TV) ? wr[c * TV + i * 16] : 0.f;
#pragma unroll
            for (int i = 0; i < NT16; ++i) a = fmaf(wv[i], (i * 16 + part < TV) ? hr[i * 16 * 36 + c] : 0.f, a);
        }
        a = row16_sum(a);
        if (part == 0 && (NB == 1 || solo < 0 || n == solo)) {
            const float e = a + bb[jo];
            if (emb_lds) emb_lds[n * EDIM + jo] = e;
            if (emb_out && b0 + n < B) emb_out[(size_t)(b0 + n) * EDIM + jo] = e;
        }
    }
}

template <int T, int NB>
__global__ __launch_bounds__(NTHREADS, 2) void cond_fast_kernel(const float* wbuf, const DataView dv, const FrameIdx fi,
                                                                int seg_len, float* __restrict__ emb_out, int B) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b0 = blockIdx.x * NB;
    __shared__ float CE[NB > 1 ? NB * EDIM : 1];      // the embeddings once more in LDS, for the isolation test (unused with one window)
    for (int u = threadIdx.x; u < CondFastLds<T, NB>::FLOATS; u += NTHREADS) smem[u] = 0.f;
    __syncthreads();
    cond_fast_body<T, NB>(wbuf, dv, [&](int t) { return fi.idx[t]; }, seg_len, smem, b0, B, NB > 1 ? CE : nullptr, emb_out);
    if constexpr (NB > 1) {      // window isolation (top of this file): every window whose embedding is not finite, alone
        lds_barrier();
        for (int solo = next_nonfinite_slot<NB>(CE, -1, b0, B); solo >= 0; solo = next_nonfinite_slot<NB>(CE, solo, b0, B)) {
            for (int u = threadIdx.x; u < CondFastLds<T, NB>::FLOATS; u += NTHREADS) smem[u] = 0.f;
            __syncthreads();
            cond_fast_body<T, NB, true>(wbuf, dv, [&](int t) { return fi.idx[t]; }, seg_len, smem, b0, B, CE, emb_out, solo);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// condition encoder 'E_unet' (STSE_Unet with set_out_layer, stsae_unet.py:62-146,182-251): the U-Net's down path
// 2->16->32->32 | 17->12 | 32->64->64 | 12->10 | 64->128->6 without embeddings (t = None), then
// Linear(6*T*10 -> latent) over the (c,t,v) flattening.  Same MFMA stages and LDS plan as the scoring kernel.
// ------------------------------------------------------------------------------------------------
template <int T, int NB>
struct DownPathLds {     // the scoring kernel's work region, with the [P10][cs] output of the last layer behind its (in, z) = 2 x s128
    using PL = Plan<T, NB>;
    static constexpr int H_OFF = 2 * PL::s128;
    static constexpr int work(int cs) { return cmax(PL::R, H_OFF + PL::P10 * cs); }
};
template <int T, int NB>
struct CondUnetLds : DownPathLds<T, NB> {
    static constexpr int FLOATS = DownPathLds<T, NB>::work(20);
};

// one run of the encoder over the workgroup's region: all windows (solo < 0; the joint run raises bad[n] for a window whose result
// is not finite) or window `solo` alone
template <int T, int NB, bool OPAQUE>
__device__ __forceinline__ void cond_unet_pass(const float* wbuf, const DataView& dv, const FrameIdx& fi, int seg_len,
                                               float* __restrict__ emb_out, int b0, int B, float* smem, int* bad, int solo) {
    using PL = Plan<T, NB>;
    using LD = CondUnetLds<T, NB>;
    float* const RG = smem;
    int tid = threadIdx.x;
    if constexpr (OPAQUE) asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    Prof prof;
    prof.off();
    for (int u = tid; u < LD::FLOATS; u += NTHREADS) smem[u] = 0.f;
    __syncthreads();
    load_window_frames<T, NB, OPAQUE>(RG + PL::L0_in, dv, [&](int t) { return fi.idx[t]; }, seg_len, b0, B, solo);
    __syncthreads();
    const float* wb = wbuf;
    if constexpr (OPAQUE) asm volatile("" : "+s"(wb));
    unet_down_path<T, NB, false>(wb, wb + TABC, RsWords{TABC + TABC_URS + 0, TABC + TABC_URS + 1, TABC + TABC_URS + 2, TABC + TABC_URS + 3},
                                 RG, nullptr, wave, lane, prof);
    layer_generic<128, 16, 10, true, false, T, NB>(wb, layer_w(wb + TABC, 6), RG + PL::L6_in, RG + PL::L6_p, RG + LD::H_OFF, nullptr, wave, lane, prof, 0);
    // to_time_dim: emb[n][j] = b[j] + sum_k W[j][k] H[n][k], k = c*T*10 + t*10 + v
    flatten_linear<CU_OUT, 20, T * 10, NB, false, CU_OUT, OPAQUE>(RG + LD::H_OFF, as_global(wb + tab_i(wb, TABC + TABC_ULW)),
                                                                  as_global(wb + tab_i(wb, TABC + TABC_ULB)), EDIM, [&](int n, int j, float e) {
        if (b0 + n < B && (solo < 0 || n == solo)) {
            emb_out[(size_t)(b0 + n) * EDIM + j] = e;
            if (NB > 1 && solo < 0 && not_finite(e)) bad[n] = 1;
        }
    });
}

template <int T, int NB>
__global__ __launch_bounds__(NTHREADS, 2) void cond_unet_kernel(const float* wbuf, const DataView dv, const FrameIdx fi,
                                                                int seg_len, float* __restrict__ emb_out, int B) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b0 = blockIdx.x * NB;
    __shared__ int BAD[NB];      // window isolation (top of this file): slot n's joint result is not finite
    if (NB > 1 && threadIdx.x < NB) BAD[threadIdx.x] = 0;      // (the pass's barriers lie before the first store)
    cond_unet_pass<T, NB, false>(wbuf, dv, fi, seg_len, emb_out, b0, B, smem, BAD, -1);
    if constexpr (NB > 1) {
        lds_barrier();
        for (int solo = next_flagged_slot<NB>(BAD, -1); solo >= 0; solo = next_flagged_slot<NB>(BAD, solo)) {
            cond_unet_pass<T, NB, true>(wbuf, dv, fi, seg_len, emb_out, b0, B, smem, BAD, solo);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Encode launch of the latent model: windows b0 .. b0 + NB - 1 of a workgroup.  cond_fast_body (the shipped condition encoder) ->
// cond_emb; the embeddings Linear(SiLU(pos_encoding(-1) + cond_emb)) of the seven down-path layers; the down path as in
// cond_unet_kernel, with the embedding added in the GEMM epilogue as in score_kernel; to_time_dim over the (c,t,v) flattening.
// Table of the packed buffer: layers 0 .. 6 at l * F_STRIDE (all mix-first [W_t' | W_r']), TAB_WE / TAB_BE = W_e [400][16] / b_e,
// TAB_RSW / TAB_RSB + 0, 1 = down1 / down2 (non-capturing fragments), TAB_LAT_LW / TAB_LAT_LB = to_time_dim; the condition
// encoder's table at TABC as cond_fast_body expects it.
// ------------------------------------------------------------------------------------------------

// PROJECT_IN_KERNEL = false: the last layer runs as two halves of 32 output channels, each [P10][36] at H_OFF and copied to global
// memory before the next (12 frames: 332 P10 floats for the whole output would be 168 KB)
template <int T, int NB, bool PROJECT_IN_KERNEL = true>
struct LatentEncLds : DownPathLds<T, NB> {
    static constexpr int WORK = cmax(DownPathLds<T, NB>::work(PROJECT_IN_KERNEL ? 68 : 36), CondFastLds<T, NB>::FLOATS);
    static constexpr int EMB = NB * EMB_STRIDE;
    static constexpr int FLAGS = WORK + EMB + 2 * NB * EDIM;     // + cond_emb [NB][16] + SiLU(pe + cond_emb) [NB][16]
    static constexpr int FLOATS = FLAGS + 4;                     // + one word per window: its joint z0 is not finite (window isolation)
};

// COND_IN_KERNEL = false (the three-launch form: any other condition encoder, 1 .. 12 condition frames): a condition-encoder
// kernel of the pose model (cond_fast_kernel / cond_unet_kernel / cond_encode_kernel) has written cond_emb (B,16) to cond_out in a
// launch of its own; the prologue is skipped, CE is read from there and the remainder is the same code.
// PROJECT_IN_KERNEL = false (5 .. 12 corrupt frames): no to_time_dim tail; z0_out is H (B, 640 T), the last layer's output of window b
// at H[b][(t 10 + v) 64 + c] -- the order the LDS holds, so the copy is 16-byte stores -- for latent_project_kernel.
// one run of everything behind cond_emb -- embedding rows, down path, last layer, to_time_dim (or the copy of H) -- over the
// workgroup's region: all windows (solo < 0; the joint run raises bad[n] for a window whose z0 is not finite) or window `solo`
// alone, the other slots on zero poses and bias-only embedding rows
template <int T, int NB, bool PROJECT_IN_KERNEL, bool OPAQUE>
__device__ __forceinline__ void latent_down_pass(const float* wbuf, const DataView& dv, const FrameIdx& fi, int seg_len,
                                                 const float* __restrict__ pe_row, float* __restrict__ z0_out, int D, int b0, int B,
                                                 float* smem, int* bad, int solo) {
    using PL = Plan<T, NB>;
    using LD = LatentEncLds<T, NB, PROJECT_IN_KERNEL>;
    constexpr int TV10 = T * 10;
    float* const RG = smem;
    float* const EMB = smem + LD::WORK;
    float* const CE = EMB + LD::EMB;
    float* const SEN = CE + NB * EDIM;
    int tid = threadIdx.x;
    if constexpr (OPAQUE) asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    Prof prof;
    prof.off();
    const float* wb = wbuf;
    if constexpr (OPAQUE) asm volatile("" : "+s"(wb));
    for (int u = tid; u < LD::WORK; u += NTHREADS) smem[u] = 0.f;      // pad columns / pad channels must hold finite values
    step_embedding<NB>(wb, pe_row, CE, SEN, EMB, EMB_STRIDE, LAT_EMB, tid, solo);
    load_window_frames<T, NB, OPAQUE>(RG + PL::L0_in, dv, [&](int t) { return fi.idx[t]; }, seg_len, b0, B, solo);
    __syncthreads();
    unet_down_path<T, NB, true>(wb, wb, RsWords{TAB_RSW + 0, TAB_RSB + 0, TAB_RSW + 1, TAB_RSB + 1}, RG, EMB, wave, lane, prof);
    constexpr int F = LAT_ENC_C * TV10;
    if constexpr (!PROJECT_IN_KERNEL) {
        // the last layer as two halves of 32 output channels: m-tiles 2 h, 2 h + 1 of its fragments are one contiguous block, so a
        // half is the same layer with its weight, bias and embedding pointers moved on.  (The mix runs again for the second half;
        // the copy of a half has finished in every thread before the next half's GEMM writes: the mix's barrier lies between.)
        const LayerW l6 = layer_w(wb, 6);
        const float* HL = RG + LD::H_OFF;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            LayerW lh = l6;
            lh.wp += h * 2 * (2 * 128 / 16) * 256;
            lh.bias += h * 32;
            layer_generic<128, 32, 10, true, true, T, NB>(wb, lh, RG + PL::L6_in, RG + PL::L6_p, RG + LD::H_OFF, EMB + emb_off(6) + h * 32, wave, lane, prof, 0);
            for (int u = tid; u < NB * TV10 * 8; u += NTHREADS) {
                const int col = u >> 3, q = u & 7, n = col / TV10;
                if (b0 + n < B)
                    store_global4(z0_out + (size_t)(b0 + n) * F + (col - n * TV10) * LAT_ENC_C + h * 32 + 4 * q, lds_load4(lds_addr(HL + col * 36 + 4 * q)));
            }
        }
        return;
    }
    layer_generic<128, 64, 10, true, true, T, NB>(wb, layer_w(wb, 6), RG + PL::L6_in, RG + PL::L6_p, RG + LD::H_OFF, EMB + emb_off(6), wave, lane, prof, 0);
    // to_time_dim: z0[n][j] = b[j] + sum_k W[j][k] H[n][k], k = c*T*10 + t*10 + v; a thread serves every window of the workgroup
    flatten_linear<LAT_ENC_C, 68, TV10, NB, true, 4, OPAQUE>(RG + LD::H_OFF, as_global(wb + tab_i(wb, TAB_LAT_LW)), as_global(wb + tab_i(wb, TAB_LAT_LB)),
                                                             D, [&](int n, int j, float z) {
        if (b0 + n < B && (solo < 0 || n == solo)) {
            z0_out[(size_t)(b0 + n) * D + j] = z;
            if (NB > 1 && solo < 0 && not_finite(z)) bad[n] = 1;
        }
    });
}

template <int T, int NB, bool COND_IN_KERNEL = true, bool PROJECT_IN_KERNEL = true>
__global__ __launch_bounds__(NTHREADS, 1) void latent_encode_kernel(const float* wbuf, const DataView dv, const FrameIdx cond_fi,
                                                                    const FrameIdx fi, int seg_len, const float* __restrict__ pe_row,
                                                                    float* __restrict__ cond_out, float* __restrict__ z0_out, int D, int B) {
    using LD = LatentEncLds<T, NB, PROJECT_IN_KERNEL>;
    static_assert(NB == 1 || PROJECT_IN_KERNEL, "the rows without the to_time_dim tail hold one window per workgroup: nothing tests their result");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const CE = smem + LD::WORK + LD::EMB;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * NB;
    if constexpr (COND_IN_KERNEL) {
        for (int u = tid; u < LD::WORK; u += NTHREADS) smem[u] = 0.f;
        __syncthreads();
        cond_fast_body<T, NB>(wbuf, dv, [&](int t) { return cond_fi.idx[t]; }, seg_len, smem, b0, B, CE, cond_out);
        __syncthreads();
    } else {
        if (tid < NB * EDIM) {
            const int n = tid / EDIM, b = b0 + n < B ? b0 + n : B - 1;      // (a window past the end repeats the last one, as load_window_frames)
            CE[tid] = cond_out[(size_t)b * EDIM + tid % EDIM];
        }
        __syncthreads();
    }
    // Window isolation (top of this file), tested ONCE, on z0: a non-finite corrupt frame leaves cond_emb finite and reaches the
    // neighbour's z0 through the shared down path; a cond_emb that is not finite -- its window's own, or (were a condition-encoder
    // stage to hand it on) a neighbour's -- makes that window's embedding rows and with them its z0 non-finite as well.  So no
    // second test sits between the two phases, where it cost the launch 1.1 % (profiles/nonfinite_windows.txt); a flagged window
    // runs BOTH again alone, the condition encoder first.
    int* const BAD = reinterpret_cast<int*>(smem + LD::FLAGS);
    if (NB > 1 && tid < NB) BAD[tid] = 0;      // (the pass's barriers lie before the first store)
    latent_down_pass<T, NB, PROJECT_IN_KERNEL, false>(wbuf, dv, fi, seg_len, pe_row, z0_out, D, b0, B, smem, BAD, -1);
    if constexpr (NB > 1) {
        lds_barrier();
        for (int solo = next_flagged_slot<NB>(BAD, -1); solo >= 0; solo = next_flagged_slot<NB>(BAD, solo)) {
            if constexpr (COND_IN_KERNEL) {
                for (int u = tid; u < LD::WORK; u += NTHREADS) smem[u] = 0.f;
                __syncthreads();
                cond_fast_body<T, NB, true>(wbuf, dv, [&](int t) { return cond_fi.idx[t]; }, seg_len, smem, b0, B, CE, cond_out, solo);
                __syncthreads();
            }
            latent_down_pass<T, NB, PROJECT_IN_KERNEL, true>(wbuf, dv, fi, seg_len, pe_row, z0_out, D, b0, B, smem, BAD, solo);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Decode launch of the latent autoencoder (stage 'pretrain': STSAE_Unet with use_bottleneck, stsae_unet.py:365-438, behind
// rev_to_time_dim): ONE window per workgroup, so window isolation (top of this file) holds by construction.
//   G (B, 640 T) = rev_to_time_dim(z) from latent_unproject_kernel, in H's order -> up3 + d2 -> layers 7, 8 -> up2 + d1 ->
//   layers 9, 10 -> + X -> pose (B,2,T,17) and the window's mean loss against X (mocodad_latent.py:131, 218)
// The skip tensors d1 / d2 do not cross the launch boundary: the kernel runs layers 0 .. 4 and down1 again on the window's corrupt
// frames -- with the embedding rows the encode launch formed -- and keeps d1 / d2 in registers between the capturing down-samplers
// and the adding up-samplers, as score_kernel does (resample_stage<.., CAPTURE> / <.., ADD>; DESIGN.md 2.6b says why).  Every
// layer runs mix-first through layer_generic on Plan<T, 1>; layer 10's two output channels are one 16-channel m-tile whose other
// rows the packer left zero.
// Table of the packed buffer (pack_latent_ae_model): layers 0 .. 10 at l * F_STRIDE, W_e / b_e with all 530 rows, TAB_LAT_CAPW /
// TAB_LAT_CAPB + 0, 1 = down1 / down2 in the capture k order, TAB_RSW / TAB_RSB + 2, 3 = up3 / up2.
// ------------------------------------------------------------------------------------------------
template <int T>
struct LatentDecLds {
    using PL = Plan<T, 1>;
    static constexpr int G_IN = PL::s64b;                  // G [P10][68]: behind up3's output, where layer 7's z follows
    static constexpr int L8_out = PL::s64b;                // [P12][36]
    static constexpr int L10_z = 0, L10_out = 2 * PL::s32a;      // [P17][36] | [P17][20]
    static constexpr int WORK = PL::R;
    static constexpr int EMB = 560;                        // 530 rows; layer 10's m-tile reads 16 from emb_off(10) = 528: the rest zero
    static constexpr int RED = NTHREADS / 16;              // loss partial sums, one per DPP row
    static constexpr int FLOATS = WORK + EMB + EDIM + RED;
    static_assert(G_IN + PL::P10 * 68 <= PL::R && L10_out + PL::s16 <= PL::R && PL::UP2_out + PL::s32a <= PL::R, "decode LDS plan");
    static_assert(L8_out + PL::s32b <= PL::UP2_out, "decode LDS plan: layer 8's output under up2's");
    static_assert(2 * T * 17 <= NTHREADS, "epilogue: one pose element per thread");
};

// The two pieces of a decode workgroup, stated once for latent_decode_kernel (one G row per window) and latent_decode_samples_kernel
// (a range of a window's G rows, below).
// (1) the region cleared, the rows of all eleven layers as latent_down_pass forms its 400, the window's corrupt frames, and the down
// stem once more for the skips: d1 = layer 2's output, d2 = layer 4's, captured by the down-samplers' B reads.  (down2's own output is
// not needed -- layers 5, 6 and the bottleneck ran in the launches before -- the stage is there for its reads.)  Ends behind a barrier.
template <int T, int NS1, int NS2>
__device__ __forceinline__ void latent_decode_stem(const float* wb, const DataView& dv, const FrameIdx& fi, int seg_len,
                                                   const float* pe_row, const float* cond_row, int b, int B,
                                                   float* smem, float (&skip1)[NS1], float (&skip2)[NS2], int tid, int wave, int lane,
                                                   Prof& prof) {
    using PL = Plan<T, 1>;
    using LD = LatentDecLds<T>;
    float* const RG = smem;
    float* const EMB = smem + LD::WORK;
    float* const SEN = EMB + LD::EMB;
    for (int u = tid; u < LD::WORK + LD::EMB; u += NTHREADS) smem[u] = 0.f;      // pad columns / pad channels must hold finite values
    step_embedding<1>(wb, pe_row, cond_row, SEN, EMB, 0, emb_off(10) + C0, tid, -1);
    load_window_frames<T, 1>(RG + PL::L0_in, dv, [&](int t) { return fi.idx[t]; }, seg_len, b, B);
    __syncthreads();
    unet_down_stem<T, 1, true, true>(wb, wb, RsWords{TAB_LAT_CAPW + 0, TAB_LAT_CAPB + 0, TAB_LAT_CAPW + 1, TAB_LAT_CAPB + 1}, RG, EMB,
                                     skip1, skip2, wave, lane, prof);
}
// (2) row g_row of G (640 T floats each, H's order) -> up3 + d2 -> layers 7, 8 -> up2 + d1 -> layers 9, 10 -> + X -> row o_row of
// pose_out (2, T, 17 each; null: not stored) and loss_out[o_row] (null: not stored).  The skips are read only (resample_stage<..,
// ADD>).  On return RED holds the 32 row sums of the loss, published by the barrier in front of the one thread that adds them.
// OPAQUE: the instance a caller runs in a loop (thread id and weight pointer made opaque per run, as the encoders' solo passes at
// the top of this file); tid / wave / lane: the caller's, used as they are without OPAQUE.
template <int T, bool OPAQUE, int NS1, int NS2>
__device__ __forceinline__ void latent_decode_row(const float* wbuf, const DataView& dv, const FrameIdx& fi, int seg_len,
                                                  const float* G, size_t g_row, float* pose_out, float* loss_out, size_t o_row,
                                                  int loss_fn, int b, float* smem, float (&skip1)[NS1], float (&skip2)[NS2], int tid, int wave,
                                                  int lane, Prof& prof) {
    using PL = Plan<T, 1>;
    using LD = LatentDecLds<T>;
    constexpr int TV = T * 17, TV10 = T * 10, F = LAT_ENC_C * TV10;
    float* const RG = smem;
    float* const EMB = smem + LD::WORK;
    float* const RED = EMB + LD::EMB + EDIM;
    const float* wb = wbuf;
    if constexpr (OPAQUE) {      // (the caller's ids serve the other instance: latent_decode_kernel's text stays what it was)
        tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        asm volatile("" : "+s"(wb));
    }
    // ---- G -> [P10][68]; the pad rows behind the last frame hold zeros (up3's trailing k-step reads two rows past a frame)
    for (int u = tid; u < PL::P10 * 16; u += NTHREADS) {
        const int col = u >> 4, q = u & 15;
        const float4 v = col < TV10 ? load_global4(G + g_row * F + col * LAT_ENC_C + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        lds_store4(lds_addr(RG + LD::G_IN + col * 68 + 4 * q), v.x, v.y, v.z, v.w);
    }
    __syncthreads();
    {
        RsCoef<64, 10, 12, T, 1, false> rc;
        rc.load(wb + tab_i(wb, TAB_RSW + 2), wb + tab_i(wb, TAB_RSB + 2), lane);
        resample_stage<64, 10, 12, T, 1, false, true>(RG + LD::G_IN, 68, RG + PL::UP3_out, 68, rc, skip2, wave, lane);      // up3 (+ d2)
        __syncthreads();
    }
    layer_generic<64, 64, 12, false, true, T, 1>(wb, layer_w(wb, 7), RG + PL::L7_in, RG + PL::L7_z, RG + PL::L7_out, EMB + emb_off(7), wave, lane, prof, 0);
    layer_generic<64, 32, 12, true, true, T, 1>(wb, layer_w(wb, 8), RG + PL::L8_in, RG + PL::L8_z, RG + LD::L8_out, EMB + emb_off(8), wave, lane, prof, 0);
    {
        RsCoef<32, 12, 17, T, 1, false> rc;
        rc.load(wb + tab_i(wb, TAB_RSW + 3), wb + tab_i(wb, TAB_RSB + 3), lane);
        resample_stage<32, 12, 17, T, 1, false, true>(RG + LD::L8_out, 36, RG + PL::UP2_out, 36, rc, skip1, wave, lane);     // up2 (+ d1)
        __syncthreads();
    }
    layer_generic<32, 32, 17, false, true, T, 1>(wb, layer_w(wb, 9), RG + PL::L9_in, RG + PL::L9_z, RG + PL::L9_out, EMB + emb_off(9), wave, lane, prof, 0);
    layer_generic<32, 16, 17, true, true, T, 1>(wb, layer_w(wb, 10), RG + PL::L10_in, RG + LD::L10_z, RG + LD::L10_out, EMB + emb_off(10), wave, lane, prof, 0);
    // ---- + X, the pose, and the loss in a fixed order: one element per thread, the 16 lanes of a DPP row, then the 32 row sums one
    // after the other by one thread
    float l = 0.f;
    if (tid < C0 * TV) {
        const int c = tid / TV, tv = tid - c * TV, t = tv / 17, v = tv - t * 17;
        const float x = load_coord(dv, b, c, fi.idx[t], v, seg_len);
        const float p = RG[LD::L10_out + tv * 20 + c] + x;
        if (pose_out) pose_out[(o_row * C0 + c) * TV + tv] = p;
        l = loss_elem(p, x, loss_fn);
    }
    l = row16_sum(l);
    if ((lane & 15) == 0) RED[tid >> 4] = l;
    __syncthreads();
    if (tid == 0 && loss_out) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < LD::RED; ++i) s += RED[i];
        loss_out[o_row] = s / (float)(C0 * TV);
    }
}

template <int T>
__global__ __launch_bounds__(NTHREADS, 1) void latent_decode_kernel(const float* wbuf, const DataView dv, const FrameIdx fi, int seg_len,
                                                                    const float* __restrict__ pe_row, const float* __restrict__ cond,
                                                                    const float* __restrict__ G, float* __restrict__ pose_out,
                                                                    float* __restrict__ loss_out, int loss_fn, int B) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    Prof prof;
    prof.off();
    float skip1[RsCfg<32, 17, 12, T, 1, true>::PER * RsCfg<32, 17, 12, T, 1, true>::SK];
    float skip2[RsCfg<64, 12, 10, T, 1, true>::PER * RsCfg<64, 12, 10, T, 1, true>::SK];
    latent_decode_stem<T>(wbuf, dv, fi, seg_len, pe_row, cond + (size_t)b * EDIM, b, B, smem, skip1, skip2, tid, wave, lane, prof);
    latent_decode_row<T, false>(wbuf, dv, fi, seg_len, G, (size_t)b, pose_out, loss_out, (size_t)b, loss_fn, b, smem, skip1, skip2, tid, wave, lane, prof);
}

// ------------------------------------------------------------------------------------------------
// Decode launch for the S generated latents of a window (mcd_latent_decode_samples): workgroup (x, y) = window
// b0 + x of the call and its samples y spw .. min(S, (y + 1) spw) - 1.  The stem above runs ONCE per workgroup -- the skips depend on
// the window alone and stay in registers -- then latent_decode_row once per sample on row x S + s of G (the chunk's rows, from
// latent_unproject_kernel over the chunk's latent rows) -> pose_all[b, s] (B,S,2,T,17; null: not stored) and loss_all[b, s].
// Samples are independent: a generated latent may be non-finite (a diverged chain), and the pad rows and pad channels of the region
// meet zero coefficients (NaN x 0 = NaN).  A sample leaves the next one nothing but such pads -- every value a stage reads with a
// non-zero coefficient was written by that sample's own stages -- so behind a sample whose loss is not finite the work region is
// cleared again, as it is in front of the first; behind a finite one the pads hold finite values, as they do behind the stem.  (The
// test is on the 32 row sums of the loss: every element of the pose is in one of them.)  The embedding rows are not written by a
// sample and are not cleared.  A sample's bits therefore do not depend on spw, nor on the samples in front of it.
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(NTHREADS, 1) void latent_decode_samples_kernel(const float* wbuf, const DataView dv, const FrameIdx fi, int seg_len,
                                                                            const float* __restrict__ pe_row, const float* __restrict__ cond,
                                                                            const float* __restrict__ G, float* __restrict__ pose_all,
                                                                            float* __restrict__ loss_all, int loss_fn, int b0, int B,
                                                                            int S, int spw) {
    using LD = LatentDecLds<T>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const float* const RED = smem + LD::WORK + LD::EMB + EDIM;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = b0 + blockIdx.x;
    const int s0 = blockIdx.y * spw, s1 = s0 + spw < S ? s0 + spw : S;
    Prof prof;
    prof.off();
    float skip1[RsCfg<32, 17, 12, T, 1, true>::PER * RsCfg<32, 17, 12, T, 1, true>::SK];
    float skip2[RsCfg<64, 12, 10, T, 1, true>::PER * RsCfg<64, 12, 10, T, 1, true>::SK];
    latent_decode_stem<T>(wbuf, dv, fi, seg_len, pe_row, cond + (size_t)b * EDIM, b, B, smem, skip1, skip2, tid, wave, lane, prof);
#pragma unroll 1
    for (int s = s0; s < s1; ++s) {
        latent_decode_row<T, true>(wbuf, dv, fi, seg_len, G, (size_t)blockIdx.x * S + s, pose_all, loss_all, (size_t)b * S + s, loss_fn, b, smem, skip1, skip2, tid, wave, lane, prof);
        // every thread reads the same 32 row sums (behind the row's barrier; the next stores to RED lie behind the next row's): uniform
        if (s + 1 < s1 && __ballot(not_finite(RED[lane & (LD::RED - 1)])) != 0ull) {
            for (int u = tid; u < LD::WORK; u += NTHREADS) smem[u] = 0.f;
            __syncthreads();
        }
    }
}

}  // namespace mcd

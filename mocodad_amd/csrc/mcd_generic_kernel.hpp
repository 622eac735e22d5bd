// mcd_generic_kernel.hpp — the runtime-shape kernels of libmocodad_hip.so: plain fp32 FMAs, shapes read from the handle's tables
// (GLayer rows of mcd_launch.hpp), none of them on a default path of the shipped configurations.  Included by mcd_api.hip alone.
//   cond_encode_kernel          STSE.encode for any channel list / 21 .. 31 condition frames   models/stsae/stsae.py:59-92
//   cond_unet_generic_kernel    'E_unet' condition encoder at any frame count (cross-check)    models/stsae/stsae_unet.py:62-146
//   score_generic_kernel        runtime-shape trajectory kernel: the CROSS-CHECK of the MFMA kernels (MCD_OPT_GENERIC_UNET)
// All three run their ST-GCN layers through g_layer.
#pragma once
#include "mcd_launch.hpp"

namespace mcd {
namespace {

constexpr int GEN_THREADS = 256;     // block size of the two generic kernels (CE_THREADS, cond_encode_kernel's, is mcd_launch.hpp's: the packer sizes LDS by it)
constexpr int GEN_BUF = 1280;        // floats per frame of the three rotating buffers: 128 ch x 10 joints (>= 32 x 17, 64 x 12)
constexpr int GEN_D1 = 32 * 17, GEN_D2 = 64 * 12;
constexpr int GEN_SLAB = 3 * GEN_BUF + GEN_D1 + GEN_D2;      // per frame and workgroup
// LDS plan of score_generic_kernel at T U-Net frames, offsets in floats (the kernel carves at them, the launcher asks for floats())
struct GenericLds {
    int CTV;                                                          // C0 x T x 17: one [c][t][v] tensor over the U-Net frames
    __host__ __device__ explicit GenericLds(int T) : CTV(C0 * T * 17) {}
    __host__ __device__ int xt() const { return 0; }                  // chain state
    __host__ __device__ int eps() const { return xt() + CTV; }        // layer 10's output (+ x)
    __host__ __device__ int zn() const { return eps() + CTV; }        // this step's noise at the U-Net frames
    __host__ __device__ int emb() const { return zn() + CTV; }        // [EMB_TOTAL + 4]
    __host__ __device__ int se() const { return emb() + EMB_TOTAL + 4; }   // [16]
    __host__ __device__ int red() const { return se() + EDIM; }       // [GEN_THREADS]
    __host__ __device__ int floats() const { return red() + GEN_THREADS; }
};

// one ST-GCN layer (stsgcn.py:94-116, BatchNorm folded): X [cin][T][V] -> O [cout][T][V]; Y (>= cin T V floats, may be O) and
// Z are scratch.  THREADS: the caller's block size; VC: the joint count when the caller knows it (its joint-mix loop is then
// unrolled), 0 = read L.V.  EMB: the layer output takes an embedding term -- emb[L.embo + channel] of the pass's embedding outputs
// (LDS), 0.f where emb is null or L.embo < 0; without EMB (a caller that has no embeddings) the output is the PReLU itself.
// Each stage as wave tasks of (8 channels, 64 columns) with 8 accumulators per thread: the time mix (Y = X . Tq per joint), the joint
// mix (Z = Y . A), the channel GEMM + residual + PReLU.  A column's activation (or coefficient) is loaded once for 8 multiply-adds,
// and the GEMM's weight rows are wave-uniform scalar loads.  (The first version ran the two mixes as one 17 x (T + 1) loop per
// output element: 8x the multiplies, 0.45 TFLOP/s; at 16 condition frames it was a quarter of the whole scoring step.)
template <int THREADS, int VC, bool EMB>
__device__ void g_layer(const float* wb, const GLayer& L, int T, const float* X, float* Y, float* Z, float* O, const float* emb) {
    const int V = VC ? VC : L.V, TV = T * V, cin = L.cin, cout = L.cout, nblk = (TV + 63) / 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    constexpr int NW = THREADS / 64;
    const float* Tq = wb + L.tq;      // [q][v][t]
    const float* Am = wb + L.am;      // [q][v][w]
    const int ngi = (cin + 7) / 8, ngo = (cout + 7) / 8;
    for (int task = wave; task < ngi * nblk; task += NW) {          // time mix: Y[c][q, v] = sum_t X[c][t, v] Tq[q, v][t]
        const int c0 = (task / nblk) * 8, p = (task % nblk) * 64 + lane;
        if (p < TV) {
            const float* tq = Tq + (size_t)p * T;
            const float* xb = X + p % V;
            int co[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) co[i] = (c0 + i < cin ? c0 + i : cin - 1) * TV;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < T; ++t) {
                const float tv = tq[t];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(xb[co[i] + t * V], tv, acc[i]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (c0 + i < cin) Y[(c0 + i) * TV + p] = acc[i];
        }
    }
    __syncthreads();
    for (int task = wave; task < ngi * nblk; task += NW) {          // joint mix: Z[c][q, w] = sum_v Y[c][q, v] A[q, v][w]
        const int c0 = (task / nblk) * 8, p = (task % nblk) * 64 + lane;
        if (p < TV) {
            const int q = p / V, w = p % V;
            const float* am = Am + (size_t)q * V * V + w;
            const float* yb = Y + q * V;
            int co[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) co[i] = (c0 + i < cin ? c0 + i : cin - 1) * TV;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            auto mac = [&](int v) {
                const float a = am[v * V];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(yb[co[i] + v], a, acc[i]);
            };
            if constexpr (VC != 0) {
#pragma unroll
                for (int v = 0; v < VC; ++v) mac(v);
            } else {
                for (int v = 0; v < V; ++v) mac(v);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (c0 + i < cin) Z[(c0 + i) * TV + p] = acc[i];
        }
    }
    __syncthreads();
    const float* wt = wb + L.wt;
    const float* wr = L.wr >= 0 ? wb + L.wr : nullptr;
    const float* bias = wb + L.bias;
    const float slope = L.slope;
    [[maybe_unused]] const bool has_emb = emb && L.embo >= 0;
    for (int task = wave; task < ngo * nblk; task += NW) {          // channel GEMM + residual + PReLU (+ embedding)
        const int o0 = (task / nblk) * 8, p = (task % nblk) * 64 + lane;
        int row[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = o0 + i < cout ? o0 + i : cout - 1;
        if (p < TV) {
            float acc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = bias[row[i]];
            for (int c = 0; c < cin; ++c) {
                const float z = Z[c * TV + p];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(wt[row[i] * cin + c], z, acc[i]);
            }
            if (wr) {
                for (int c = 0; c < cin; ++c) {
                    const float x = X[c * TV + p];
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] = fmaf(wr[row[i] * cin + c], x, acc[i]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += X[row[i] * TV + p];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (o0 + i < cout) {
                    if constexpr (EMB) O[(o0 + i) * TV + p] = prelu(acc[i], slope) + (has_emb ? emb[L.embo + row[i]] : 0.f);
                    else O[(o0 + i) * TV + p] = prelu(acc[i], slope);
                }
        }
    }
    __syncthreads();
}
// joint resampler (stsgcn.py:187-199 over the joint axis): X [C][T][vin] -> O [C][T][vout] (+ skip)
__device__ void g_resample(const float* wb, int wo, int bo, int C, int T, int vin, int vout, const float* X, float* O, const float* skip) {
    const float* W = wb + wo;
    const float* bb = wb + bo;
    for (int u = threadIdx.x; u < C * T * vout; u += GEN_THREADS) {
        const int vo = u % vout, ct = u / vout;
        float a = bb[vo];
        for (int v = 0; v < vin; ++v) a = fmaf(W[vo * vin + v], X[ct * vin + v], a);
        if (skip) a += skip[u];
        O[u] = a;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// Runtime-shape form of the trajectory kernel: ANY U-Net frame count 1..MCD_MAX_FRAMES (the reference is generic in
// n_frames, mocodad.py:780-796, stsgcn.py:134-141), every strategy.  Plain fp32 FMAs, one 256-thread workgroup per chain
// at a time (persistent grid), activations [channel][frame][joint] in a per-workgroup global scratch slab.  Correct, not fast,
// and since round 3 off every default path (score_kernel<T,...> covers 1 .. 12 frames, score_tiled_kernel 13 .. 32): it is the
// independent implementation MCD_OPT_GENERIC_UNET switches to, which the tests compare the MFMA kernels with.
// The chain -- draws, frame maps, update, loss -- is mcd_chain.hpp's.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GEN_THREADS) void score_generic_kernel(const ScoreParams P, const FrameMaps M, const GenNet N, int T,
                                                                    float* __restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const GenericLds LD(T);
    const int TV = T * 17, CTV = LD.CTV, tid = threadIdx.x;
    float* XT = gsm + LD.xt();
    float* EPS = gsm + LD.eps();
    float* ZN = gsm + LD.zn();
    float* EMB = gsm + LD.emb();
    float* SE = gsm + LD.se();
    float* RED = gsm + LD.red();
    float* slab = scratch + (size_t)blockIdx.x * GEN_SLAB * T;
    float* A = slab;
    float* Bb = A + GEN_BUF * T;
    float* Zb = Bb + GEN_BUF * T;
    float* D1 = Zb + GEN_BUF * T;
    float* D2 = D1 + GEN_D1 * T;
    const float* wb = P.wbuf;
    const int Tx = P.n_corrupt, K = P.ns > 2 ? P.ns - 1 : 1, per = C0 * Tx * 17;
    for (long long chain = blockIdx.x; chain < P.n_chains; chain += gridDim.x) {
        const int b = (int)(chain / P.S), s = (int)(chain % P.S);
        const unsigned fixed = (unsigned)(P.win_mask ? P.win_mask[b] : P.fixed_mask);
        __syncthreads();
        for (int u = tid; u < CTV; u += GEN_THREADS) {
            const int c = u / TV, t = (u % TV) / 17, v = u % 17;
            float x;
            if (P.mode == 1) x = P.x_in[((size_t)b * C0 + c) * TV + t * 17 + v];
            else if ((fixed >> t) & 1u) x = load_coord(P.dv, b, c, fm_src(P, M, t), v, P.seg_len);
            else x = chain_xT(P, b, s, K, per, c, fm_tx(P, M, fixed, t), v);
            XT[u] = x;
        }
        const int i_first = P.mode == 1 ? P.step_single : P.ns - 1;
        const int i_last = P.mode == 1 ? P.step_single : 1;
        for (int sidx = i_first; sidx >= i_last; --sidx) {
            const float* srow = P.step_table + sidx * (4 + EDIM);
            __syncthreads();
            if (tid < EDIM) {
                float e = srow[4 + tid];
                if (P.cond_emb) e += P.cond_emb[(size_t)b * EDIM + tid];
                SE[tid] = e / (1.f + expf(-e));
            }
            // this step's noise, one thread per (frame, joint pair)
            if (P.mode == 0 && sidx > 1) {
                const int k = P.ns - sidx;
                for (int gi = tid; gi < T * 9; gi += GEN_THREADS) {
                    const int t = gi / 9, v0 = (gi % 9) * 2;
                    float z[4] = {0.f, 0.f, 0.f, 0.f};
                    if (!((fixed >> t) & 1u)) chain_step_noise4(P, b, s, k, K, per, Tx, fm_tx(P, M, fixed, t), v0, z);
                    ZN[t * 17 + v0] = z[0]; ZN[TV + t * 17 + v0] = z[1];
                    if (v0 + 1 < 17) { ZN[t * 17 + v0 + 1] = z[2]; ZN[TV + t * 17 + v0 + 1] = z[3]; }
                }
            }
            __syncthreads();
            for (int o = tid; o < EMB_TOTAL; o += GEN_THREADS) {
                const float* we = wb + N.we + o * EDIM;
                float a = wb[N.be + o];
                for (int k = 0; k < EDIM; ++k) a = fmaf(we[k], SE[k], a);
                EMB[o] = a;
            }
            __syncthreads();
            // ---- the U-Net (stsae_unet.py:406-438)
            g_layer<GEN_THREADS, 0, true>(wb, N.L[0], T, XT, A, Zb, A, EMB);
            g_layer<GEN_THREADS, 0, true>(wb, N.L[1], T, A, Bb, Zb, Bb, EMB);
            g_layer<GEN_THREADS, 0, true>(wb, N.L[2], T, Bb, D1, Zb, D1, EMB);                                         // d1
            g_resample(wb, N.rs_w[0], N.rs_b[0], 32, T, 17, 12, D1, A, nullptr);                  // down1
            g_layer<GEN_THREADS, 0, true>(wb, N.L[3], T, A, Bb, Zb, Bb, EMB);
            g_layer<GEN_THREADS, 0, true>(wb, N.L[4], T, Bb, D2, Zb, D2, EMB);                                         // d2
            g_resample(wb, N.rs_w[1], N.rs_b[1], 64, T, 12, 10, D2, A, nullptr);                  // down2
            g_layer<GEN_THREADS, 0, true>(wb, N.L[5], T, A, Bb, Zb, Bb, EMB);
            g_layer<GEN_THREADS, 0, true>(wb, N.L[6], T, Bb, A, Zb, A, EMB);
            g_resample(wb, N.rs_w[2], N.rs_b[2], 64, T, 10, 12, A, Bb, D2);                       // up3 + d2
            g_layer<GEN_THREADS, 0, true>(wb, N.L[7], T, Bb, A, Zb, A, EMB);
            g_layer<GEN_THREADS, 0, true>(wb, N.L[8], T, A, Bb, Zb, Bb, EMB);
            g_resample(wb, N.rs_w[3], N.rs_b[3], 32, T, 12, 17, Bb, A, D1);                       // up2 + d1
            g_layer<GEN_THREADS, 0, true>(wb, N.L[9], T, A, Bb, Zb, Bb, EMB);
            g_layer<GEN_THREADS, 0, true>(wb, N.L[10], T, Bb, A, Zb, EPS, EMB);
            // ---- eps = U-Net output + its input; DDPM update of the frame each prediction drives (mocodad.py:172-178,829-838)
            const float ca = srow[0], cb = srow[1], csg = srow[2];
            const bool zadd = sidx > 1;
            float xn[(C0 * MCD_MAX_FRAMES * 17 + GEN_THREADS - 1) / GEN_THREADS];
            int dst[(C0 * MCD_MAX_FRAMES * 17 + GEN_THREADS - 1) / GEN_THREADS];
            int it = 0;
            for (int u = tid; u < CTV; u += GEN_THREADS, ++it) {
                const int c = u / TV, t = (u % TV) / 17, v = u % 17;
                const float eps = EPS[u] + XT[u];
                dst[it] = -1; xn[it] = 0.f;
                if (P.mode == 1) {
                    P.eps_out[((size_t)b * C0 + c) * TV + t * 17 + v] = eps;
                } else {
                    const int tp = fm_upd(P, M, fixed, t);
                    if (tp >= 0) {
                        const int up = c * TV + tp * 17 + v;
                        xn[it] = ca * (XT[up] - cb * eps) + csg * (zadd ? ZN[up] : 0.f);
                        dst[it] = up;
                    }
                }
            }
            __syncthreads();
            it = 0;
            for (int u = tid; u < CTV; u += GEN_THREADS, ++it)
                if (dst[it] >= 0) XT[dst[it]] = xn[it];
        }
        if (P.mode == 1) continue;
        __syncthreads();
        // ---- loss over the corrupt frames (mocodad.py:484)
        float part = 0.f;
        for (int e = tid; e < per; e += GEN_THREADS) {
            const int c = e / (Tx * 17), tx = (e / 17) % Tx, v = e % 17;
            const int tu = fm_corrupt_frame(P, M, fixed, tx, T);
            const float x0 = XT[c * TV + tu * 17 + v];
            const float gt = load_coord(P.dv, b, c, fm_src(P, M, tu), v, P.seg_len);
            part += loss_elem(x0, gt, P.loss_fn);
            if (P.pose_out) P.pose_out[(size_t)(b * P.S + s) * per + e] = x0;
        }
        RED[tid] = part;
        __syncthreads();
        for (int o = GEN_THREADS / 2; o > 0; o >>= 1) { if (tid < o) RED[tid] += RED[tid + o]; __syncthreads(); }
        if (tid == 0) P.loss_out[chain] = RED[0] / (float)per;
    }
}

// 'E_unet' condition encoder at any frame count (the U-Net's down path without embeddings + to_time_dim), same scratch scheme
__global__ __launch_bounds__(GEN_THREADS) void cond_unet_generic_kernel(const float* wb, const GenCond N, const DataView dv, const FrameIdx fi,
                                                                        int seg_len, int T, int B, float* __restrict__ emb_out,
                                                                        float* __restrict__ scratch) {
    __shared__ float RED[GEN_THREADS];
    const int TV = T * 17, tid = threadIdx.x;
    float* slab = scratch + (size_t)blockIdx.x * GEN_SLAB * T;
    float* A = slab;
    float* Bb = A + GEN_BUF * T;
    float* Zb = Bb + GEN_BUF * T;
    float* D1 = Zb + GEN_BUF * T;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        for (int u = tid; u < C0 * TV; u += GEN_THREADS) {
            const int c = u / TV, t = (u % TV) / 17, v = u % 17;
            D1[u] = load_coord(dv, b, c, fi.idx[t], v, seg_len);
        }
        __syncthreads();
        g_layer<GEN_THREADS, 0, true>(wb, N.L[0], T, D1, A, Zb, A, nullptr);
        g_layer<GEN_THREADS, 0, true>(wb, N.L[1], T, A, Bb, Zb, Bb, nullptr);
        g_layer<GEN_THREADS, 0, true>(wb, N.L[2], T, Bb, A, Zb, A, nullptr);
        g_resample(wb, N.rs_w[0], N.rs_b[0], 32, T, 17, 12, A, Bb, nullptr);
        g_layer<GEN_THREADS, 0, true>(wb, N.L[3], T, Bb, A, Zb, A, nullptr);
        g_layer<GEN_THREADS, 0, true>(wb, N.L[4], T, A, Bb, Zb, Bb, nullptr);
        g_resample(wb, N.rs_w[1], N.rs_b[1], 64, T, 12, 10, Bb, A, nullptr);
        g_layer<GEN_THREADS, 0, true>(wb, N.L[5], T, A, Bb, Zb, Bb, nullptr);
        g_layer<GEN_THREADS, 0, true>(wb, N.L[6], T, Bb, A, Zb, A, nullptr);            // -> A [6][T][10]
        const int F = CU_OUT * T * 10;
        for (int jo = 0; jo < EDIM; ++jo) {
            float a = 0.f;
            for (int k = tid; k < F; k += GEN_THREADS) a = fmaf(wb[N.lw + (size_t)jo * F + k], A[k], a);
            RED[tid] = a;
            __syncthreads();
            for (int o = GEN_THREADS / 2; o > 0; o >>= 1) { if (tid < o) RED[tid] += RED[tid + o]; __syncthreads(); }
            if (tid == 0) emb_out[(size_t)b * EDIM + jo] = RED[0] + wb[N.lb + jo];
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// condition encoder (runtime channel list; 0.3 % of the work): one workgroup per window, VALU only, activations in LDS.
// gbuf (W.gmode): one buffer of cmax x Tc x 17 floats per workgroup in global scratch -- the buffers rotate, so a different one of
// the three is the global one in every layer.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CE_THREADS) void cond_encode_kernel(const CondW W, const float* __restrict__ cond,
                                                                 float* __restrict__ emb_out, int B, float* __restrict__ gbuf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Tc = W.Tc, TV = Tc * 17, tid = threadIdx.x;
    const int BF = (int)W.buf_floats();
    float* RED = smem + (int)W.red_offset();           // CE_THREADS partial sums
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
    float* X = smem;
    float* Z = X + BF;
    float* O = W.gmode ? gbuf + (size_t)blockIdx.x * BF : Z + BF;      // (the launcher passes gbuf exactly when W.gmode is set)
    __syncthreads();
    for (int u = tid; u < C0 * TV; u += CE_THREADS) X[u] = cond[(size_t)b * C0 * TV + u];  // (c, t, v) row-major
    __syncthreads();
    for (int l = 0; l < W.n_layers; ++l) {
        g_layer<CE_THREADS, 17, false>(W.base, W.L[l], Tc, X, O, Z, O, nullptr);      // (the time mix's Y in the output buffer)
        float* tmp = X; X = O; O = tmp;
    }
    // bottleneck Linear over the (c,t,v) flattening (stsae.py:73-89)
    const int hd = W.L[W.n_layers - 1].cout;
    const int F = hd * TV;
    const int jj = tid / 16, part = tid % 16;  // 16 partial sums per output
    for (int j0 = 0; j0 < W.latent; j0 += CE_THREADS / 16) {
        const int jo = j0 + jj;
        float a = 0.f;
        if (jo < W.latent) {
            const float* wrow = W.base + W.lw + (size_t)jo * F;
            for (int k = part; k < F; k += 16) a = fmaf(wrow[k], X[k], a);
        }
        RED[tid] = a;
        __syncthreads();
        if (part == 0 && jo < W.latent) {
            float s = W.base[W.lb + jo];
            for (int k = 0; k < 16; ++k) s += RED[jj * 16 + k];
            emb_out[(size_t)b * W.latent + jo] = s;
        }
        __syncthreads();
    }
    }
}

}  // namespace
}  // namespace mcd

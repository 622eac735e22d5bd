// mcd_latent_kernel.hpp — MoCoDADlatent (models/mocodad_latent.py:69-132, stage 'diffusion'): the launches of a latent scoring
// call behind its encode launch (latent_encode_kernel, mcd_encode_kernel.hpp) and their test / replay companions.
//   latent_chain_kernel           every reverse-diffusion chain of the call: S (ns-1) denoiser passes (components.py:203-291) as
//                                 v_mfma_f32_16x16x4_f32 products with the chains as the N dimension, the DDPM updates, the loss
//                                 against z0 and the loss-based aggregation over the samples
//   latent_philox_kernel          the perf mode's draws in the parity layout
//   latent_project_kernel         to_time_dim for all windows of a call as MFMA products (5 .. 12 corrupt frames, whose encode launch
//                                 stops at the last layer's output)
//   latent_unproject_kernel       stage 'pretrain' (mcd_latent_reconstruct): rev_to_time_dim for all windows of a call as
//                                 MFMA products, feeding latent_decode_kernel (mcd_encode_kernel.hpp)
#pragma once
#include "mcd_device.hpp"
#include "mcd_latent.hpp"

namespace mcd {

__device__ __forceinline__ f32x4 lat_mfma4(const float4 a, const float4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

__global__ __launch_bounds__(LAT_THREADS) void latent_chain_kernel(const LatentChainParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int D = P.net.D, L = P.net.n_layers;
    const int per_wg = P.mode == 1 ? LAT_NC : P.wpg * P.S;      // chains of this workgroup
    const LatentChainLds LD(D, per_wg);           // (what each region holds: at the struct)
    const int XS = LD.XS;
    float* const HA = smem + LD.ha();
    float* const HB = smem + LD.hb();
    float* const X = smem + LD.x();
    float* const Z0 = smem + LD.z0();
    float* const E = smem + LD.e();
    float* const CE = smem + LD.ce();
    float* const RED = smem + LD.red();
    int* const COLB = reinterpret_cast<int*>(smem + LD.colb());
    int* const COLS = reinterpret_cast<int*>(smem + LD.cols());
    float* const LOSS = smem + LD.loss();
    const int tid = threadIdx.x, lane = tid & 63, n16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = P.ns > 2 ? P.ns - 1 : 1;
    const int i_first = P.mode == 1 ? P.step_single : P.ns - 1;
    const int i_last = P.mode == 1 ? P.step_single : 1;
    const int n_chunks = (per_wg + LAT_NC - 1) / LAT_NC;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        // ---- the columns of this pass: chain q of the workgroup = (window q / S, sample q % S); mode 1: row
        if (tid < LAT_NC) {
            const int q = chunk * LAT_NC + tid;
            int b = -1, s = 0;
            if (P.mode == 1) {
                b = blockIdx.x * LAT_NC + tid;
                if (b >= P.B) b = -1;
            } else if (q < per_wg) {
                b = blockIdx.x * P.wpg + q / P.S;
                s = q % P.S;
                if (b >= P.B) b = -1;
            }
            COLB[tid] = b;
            COLS[tid] = s;
        }
        __syncthreads();
        for (int u = tid; u < LAT_NC * 16; u += LAT_THREADS) {
            const int col = u >> 4, b = COLB[col];
            CE[u] = b >= 0 ? P.cond[(size_t)b * EDIM + (u & 15)] : 0.f;
        }
        // x_T (slot 0 of the noise layout) or the given rows; z0.  One Philox call = the four normals of an element group.
        for (int u = tid; u < LAT_NC * (D >> 2); u += LAT_THREADS) {
            const int col = u / (D >> 2), d0 = (u % (D >> 2)) * 4, b = COLB[col], s = COLS[col];
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            float4 zc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b >= 0) {
                if (P.mode == 1) {
                    const float4 v = load_global4(P.x_in + (size_t)b * D + d0);
                    z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
                } else {
                    if (P.noise) {
                        const float4 v = load_global4(P.noise + ((size_t)(s * K) * P.B + b) * D + d0);
                        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
                    } else {
                        latent_philox4(P.seed, P.first_window, b, s, 0, d0, z);
                    }
                    zc = load_global4(P.z0 + (size_t)b * D + d0);
                }
            }
            lds_store4(lds_addr(X + col * XS + d0), z[0], z[1], z[2], z[3]);
            lds_store4(lds_addr(Z0 + col * XS + d0), zc.x, zc.y, zc.z, zc.w);
        }
        __syncthreads();

        for (int step = i_first; step >= i_last; --step) {
            const float* srow = P.step_table + step * (4 + EDIM);
            for (int u = tid; u < LAT_NC * 16; u += LAT_THREADS) E[(u >> 4) * 20 + (u & 15)] = srow[4 + (u & 15)] + CE[u];
            if (L == 1)      // the only layer reads x while its own epilogue rewrites it: from a copy
                for (int u = tid; u < LAT_NC * D; u += LAT_THREADS) HB[(u / D) * LAT_HS + u % D] = X[(u / D) * XS + u % D];
            __syncthreads();
            const float t0 = srow[0], t1 = srow[1], t2 = srow[2];
            for (int l = 0; l < L; ++l) {
                const bool last = l == L - 1;
                const float* in = l == 0 ? (L == 1 ? HB : X) : ((l & 1) ? HA : HB);
                const int in_s = (l == 0 && L > 1) ? XS : LAT_HS;
                float* out = (l & 1) ? HB : HA;
                const int KQh = P.net.in[l] >> 4, KQ = KQh + 1, MT = P.net.out[l] >> 4;
                const float* wb = P.wbuf;
                const unsigned in_a = lds_addr(in) + 4u * (unsigned)(n16 * in_s + 4 * g);
                const unsigned e_a = lds_addr(E) + 4u * (unsigned)(n16 * 20 + 4 * g);
                for (int mt = wave; mt < MT; mt += LAT_WAVES) {
                    const float* wp = wb + P.net.wp[l] + ((size_t)mt * KQ * 64 + lane) * 4;
                    float4 a[LAT_MAX_DIM / 16 + 1];
#pragma unroll
                    for (int k = 0; k <= LAT_MAX_DIM / 16; ++k) a[k] = k < KQ ? load_global4(wp + k * 256) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const int c0 = mt * 16 + 4 * g;      // the lane's four output rows
                    const float4 b1 = load_global4(wb + P.net.bias[l] + c0), bc = load_global4(wb + P.net.cbias[l] + c0);
                    f32x4 acc[2], accc[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[nt] = f32x4{b1.x, b1.y, b1.z, b1.w};
                        accc[nt] = lat_mfma4(a[0], lds_load4(e_a + 4u * (unsigned)(nt * 16 * 20)), f32x4{bc.x, bc.y, bc.z, bc.w});
                    }
#pragma unroll
                    for (int k = 1; k <= LAT_MAX_DIM / 16; ++k) {
                        if (k <= KQh) {
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt)
                                acc[nt] = lat_mfma4(a[k], lds_load4(in_a + 4u * (unsigned)(nt * 16 * in_s + (k - 1) * 16)), acc[nt]);
                        }
                    }
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int col = nt * 16 + n16;
                        f32x4 v = acc[nt];
                        if (!last) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                        v += accc[nt];
                        if (!last) {
                            lds_store4(lds_addr(out + col * LAT_HS + c0), v[0], v[1], v[2], v[3]);
                        } else if (P.mode == 1) {
                            const int b = COLB[col];
                            if (b >= 0) store_global4(P.eps_out + (size_t)b * D + c0, make_float4(v[0], v[1], v[2], v[3]));
                        } else {
                            // DDPM update (mocodad_latent.py:117-123); z = 0 at step 1.  The lane's four rows are one element group.
                            const int b = COLB[col], s = COLS[col];
                            float z[4] = {0.f, 0.f, 0.f, 0.f};
                            if (step > 1 && b >= 0) {
                                const int k = P.ns - step;
                                if (P.noise) {
                                    const float4 zv = load_global4(P.noise + ((size_t)(s * K + k) * P.B + b) * D + c0);
                                    z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
                                } else {
                                    latent_philox4(P.seed, P.first_window, b, s, k, c0, z);
                                }
                            }
                            const unsigned xa = lds_addr(X + col * XS + c0);
                            const float4 x = lds_load4(xa);
                            lds_store4(xa, t0 * (x.x - t1 * v[0]) + t2 * z[0], t0 * (x.y - t1 * v[1]) + t2 * z[1],
                                       t0 * (x.z - t1 * v[2]) + t2 * z[2], t0 * (x.w - t1 * v[3]) + t2 * z[3]);
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (P.mode == 1) return;
        // ---- loss of every chain of the pass against its window's latent code: mean over D (mocodad.py:484)
        {
            const int col = tid >> 3, part = tid & 7;
            float sum = 0.f;
            for (int d = part; d < D; d += 8) sum += loss_elem(X[col * XS + d], Z0[col * XS + d], P.loss_fn);
            RED[tid] = sum;
        }
        __syncthreads();
        if (tid < LAT_NC && COLB[tid] >= 0) {
            float sum = 0.f;
#pragma unroll
            for (int p = 0; p < 8; ++p) sum += RED[tid * 8 + p];
            const float loss = sum / (float)D;
            LOSS[chunk * LAT_NC + tid] = loss;
            if (P.loss_all) P.loss_all[(size_t)COLB[tid] * P.S + COLS[tid]] = loss;
        }
        if (P.latent_all || P.latent_code) {
            for (int u = tid; u < LAT_NC * D; u += LAT_THREADS) {
                const int col = u / D, d = u % D, b = COLB[col], s = COLS[col];
                if (b < 0) continue;
                if (P.latent_all) P.latent_all[((size_t)b * P.S + s) * D + d] = X[col * XS + d];
                if (P.latent_code && s == 0) P.latent_code[(size_t)b * D + d] = Z0[col * XS + d];
            }
        }
        __syncthreads();
    }
    // ---- aggregation over the samples of every window of the workgroup (mocodad.py:489-516), as aggregate_kernel does it
    if (P.loss_agg && tid < P.wpg) {
        const int b = blockIdx.x * P.wpg + tid;
        if (b < P.B) P.loss_agg[b] = aggregate_losses(LOSS + tid * P.S, P.S, P.aggr, P.aggr_q);
    }
}

// The draws of the perf mode in the parity layout (S, max(ns-1,1), B, D): slot 0 = x_T, slot k = z of step ns - k.
__global__ __launch_bounds__(256) void latent_philox_kernel(unsigned long long seed, long long first_window, int B, int S, int K, int D,
                                                            float* __restrict__ out) {
    const long long n = (long long)S * K * B * (D >> 2);
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    const int grp = (int)(u % (D >> 2));
    const int b = (int)((u / (D >> 2)) % B);
    const int k = (int)((u / ((long long)(D >> 2) * B)) % K);
    const int s = (int)(u / ((long long)(D >> 2) * B * K));
    float z[4];
    latent_philox4(seed, first_window, b, s, k, grp * 4, z);
    store_global4(out + (((size_t)(s * K + k) * B + b) * D + grp * 4), make_float4(z[0], z[1], z[2], z[3]));
}

// to_time_dim of the rows that project in a launch of their own: z0[b][j] = bias[j] + sum_k W'[j][k] H[b][k] with H (B, K = 640 T)
// as the encode launch left it (k = (t 10 + v) 64 + c) and W' = to_time_dim.weight with its columns in that order, in
// pack_gemm_frags order (M = D, K).  Workgroup (x, y): windows 32 x .. 32 x + 31 as two n-tiles, m-tile y of the D / 16.  Wave w
// accumulates the 16-wide k-groups w, w + 8, ...; the eight partial tiles are summed through LDS in wave order, so a window's z0
// is one fixed sequence of operations on its own column: columns of an MFMA never mix, and the columns past the batch hold zeros.
// Every workgroup streams W' once per 32 windows (the in-kernel tail of the 3-frame rows: once per workgroup of NB windows).
constexpr int PROJ_WAVES = 8, PROJ_THREADS = PROJ_WAVES * 64, PROJ_NC = 32;
__global__ __launch_bounds__(PROJ_THREADS) void latent_project_kernel(const float* __restrict__ wbuf, const float* __restrict__ H,
                                                                      float* __restrict__ z0_out, int KQ, int D, int B) {
    __shared__ __attribute__((aligned(16))) float RED[PROJ_WAVES * 2 * 64 * 4];
    const int tid = threadIdx.x, lane = tid & 63, n16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = blockIdx.y, b_first = blockIdx.x * PROJ_NC;
    const size_t K = (size_t)KQ * 16;
    const int bA = b_first + n16, bB = bA + 16;
    // (a column past the batch reads the last window's row, inside H, and is replaced by zeros)
    const float* hA = H + (size_t)(bA < B ? bA : B - 1) * K + 4 * g;
    const float* hB = H + (size_t)(bB < B ? bB : B - 1) * K + 4 * g;
    const float* wp = wbuf + tab_i(wbuf, TAB_LAT_LW) + ((size_t)mt * KQ * 64 + lane) * 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int kq = wave; kq < KQ; kq += PROJ_WAVES) {
        const float4 a = load_global4(wp + (size_t)kq * 256);
        float4 xA = load_global4(hA + kq * 16), xB = load_global4(hB + kq * 16);
        if (bA >= B) xA = zero;
        if (bB >= B) xB = zero;
        accA = lat_mfma4(a, xA, accA);
        accB = lat_mfma4(a, xB, accB);
    }
    lds_store4(lds_addr(RED + ((wave * 2 + 0) * 64 + lane) * 4), accA[0], accA[1], accA[2], accA[3]);
    lds_store4(lds_addr(RED + ((wave * 2 + 1) * 64 + lane) * 4), accB[0], accB[1], accB[2], accB[3]);
    __syncthreads();
    if (tid < 2 * 64) {      // thread = (n-tile, lane): the lane's four output rows of one window
        const int nt = tid >> 6, c0 = mt * 16 + 4 * g, b = b_first + nt * 16 + n16;
        float4 s = lds_load4(lds_addr(RED + (nt * 64 + lane) * 4));
#pragma unroll
        for (int w = 1; w < PROJ_WAVES; ++w) {
            const float4 v = lds_load4(lds_addr(RED + ((w * 2 + nt) * 64 + lane) * 4));
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const float4 bb = load_global4(wbuf + tab_i(wbuf, TAB_LAT_LB) + c0);
        if (b < B) store_global4(z0_out + (size_t)b * D + c0, make_float4(s.x + bb.x, s.y + bb.y, s.z + bb.z, s.w + bb.w));
    }
}

// rev_to_time_dim of the autoencoder (stsae_unet.py:433-434) for all windows of a call: G[b][r] = bias'[r] + sum_k W'[r][k] z[b][k]
// with the 640 T outputs r in H's order [(t 10 + v) 64 + c] -- the rows of W' and bias' are permuted by the packer, so that
// latent_decode_kernel copies a window's G into its LDS region with 16-byte loads -- and W' in pack_gemm_frags order (M = 640 T,
// K = D).  Workgroup (x, y): windows 32 x .. 32 x + 31 as two n-tiles, the 40 m-tiles (one corrupt frame's 640 outputs) 40 y ..;
// wave w takes the m-tiles w, w + 4, ...  A window is a column: its z stays in the wave's registers for all m-tiles, the k-chain of an
// output starts from the bias and runs over k in ascending groups, and columns of an MFMA never mix -- a non-finite z row reaches
// its own G row only.  The columns past the batch read the last window's z (inside the buffer), compute on zeros and store nothing.
// Every workgroup streams its 40 D-wide row tiles of W' once per 32 windows.
constexpr int UNPROJ_WAVES = 4, UNPROJ_THREADS = UNPROJ_WAVES * 64, UNPROJ_NC = 32, UNPROJ_MT = 40;
__global__ __launch_bounds__(UNPROJ_THREADS) void latent_unproject_kernel(const float* __restrict__ wbuf, const float* __restrict__ z,
                                                                          float* __restrict__ G, int KQ, int F, int B) {
    const int tid = threadIdx.x, lane = tid & 63, n16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = KQ * 16;
    const int bA = blockIdx.x * UNPROJ_NC + n16, bB = bA + 16;
    const float* zpA = z + (size_t)(bA < B ? bA : B - 1) * D + 4 * g;
    const float* zpB = z + (size_t)(bB < B ? bB : B - 1) * D + 4 * g;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 zA[LAT_MAX_DIM / 16], zB[LAT_MAX_DIM / 16];
#pragma unroll
    for (int k = 0; k < LAT_MAX_DIM / 16; ++k) {
        zA[k] = (k < KQ && bA < B) ? load_global4(zpA + k * 16) : zero;
        zB[k] = (k < KQ && bB < B) ? load_global4(zpB + k * 16) : zero;
    }
    const float* wtab = wbuf + tab_i(wbuf, TAB_LAT_RW);
    const float* btab = wbuf + tab_i(wbuf, TAB_LAT_RB);
#pragma unroll 1
    for (int i = 0; i < UNPROJ_MT / UNPROJ_WAVES; ++i) {
        const int mt = blockIdx.y * UNPROJ_MT + wave + i * UNPROJ_WAVES;
        const float* wp = wtab + ((size_t)mt * KQ * 64 + lane) * 4;
        float4 a[LAT_MAX_DIM / 16];
#pragma unroll
        for (int k = 0; k < LAT_MAX_DIM / 16; ++k) a[k] = k < KQ ? load_global4(wp + k * 256) : zero;
        const int c0 = mt * 16 + 4 * g;      // the lane's four output rows
        const float4 bb = load_global4(btab + c0);
        f32x4 accA = {bb.x, bb.y, bb.z, bb.w}, accB = accA;
#pragma unroll
        for (int k = 0; k < LAT_MAX_DIM / 16; ++k) {
            if (k < KQ) {
                accA = lat_mfma4(a[k], zA[k], accA);
                accB = lat_mfma4(a[k], zB[k], accB);
            }
        }
        if (bA < B) store_global4(G + (size_t)bA * F + c0, make_float4(accA[0], accA[1], accA[2], accA[3]));
        if (bB < B) store_global4(G + (size_t)bB * F + c0, make_float4(accB[0], accB[1], accB[2], accB[3]));
    }
}

}  // namespace mcd

// mcd_pack.hpp — the weight packer of libmocodad_hip.so, host only: no kernel and no HIP runtime call.  Included by mcd_api.hip.
//   fold    BatchNorm folded into the 1x1 convolutions in double, once per layer (fold_layer) / resampler (fold_conv_bn) and handle
//   emit    small emitters write a folded layer into the Builder in one of the layouts the kernels read: plain rows (GLayer, the
//           runtime-shape kernels), MFMA fragments [W_t' | W_r'] or [W_t' ; W_r'], 16-padded biases, resampler fragments
//   model   pack_pose_model / pack_latent_model / pack_latent_ae_model call the emitters in the order the buffer is laid out in and return the host
//           buffer with every table the handle keeps (PackedModel); mcd_pack_weights / mcd_pack_latent_weights upload it.
// The allocation ORDER of a call site is the buffer's layout: tests/test_pack_layout_host.py pins it (mcd_debug_pack_digest).
#pragma once
#include "mcd_launch.hpp"
#include "mcd_latent.hpp"

namespace {

using namespace mcd;

struct TensorMap {
    std::unordered_map<std::string, std::pair<const float*, int64_t>> m;
    std::string missing;
    const float* get(const std::string& name, int64_t numel) {
        auto it = m.find(name);
        if (it == m.end()) { if (missing.empty()) missing = "missing tensor " + name; return nullptr; }
        if (it->second.second != numel) {
            if (missing.empty()) missing = "tensor " + name + " has " + std::to_string(it->second.second) + " elements, expected " + std::to_string(numel);
            return nullptr;
        }
        return it->second.first;
    }
    bool has(const std::string& name) const { return m.count(name) != 0; }
};

struct Folded { std::vector<double> w, b; };  // BN-folded 1x1 conv: w[cout][cin], b[cout]

// conv (cout,cin,1,1)+bias followed by eval BatchNorm2d (eps 1e-5): W' = s W, b' = s (b - mu) + beta
bool fold_conv_bn(TensorMap& tm, const std::string& conv, const std::string& bn, int cout, int cin, Folded& f) {
    const float* w = tm.get(conv + ".weight", (int64_t)cout * cin);
    const float* b = tm.get(conv + ".bias", cout);
    const float* g = tm.get(bn + ".weight", cout);
    const float* be = tm.get(bn + ".bias", cout);
    const float* mu = tm.get(bn + ".running_mean", cout);
    const float* var = tm.get(bn + ".running_var", cout);
    if (!w || !b || !g || !be || !mu || !var) return false;
    f.w.resize((size_t)cout * cin); f.b.resize(cout);
    for (int o = 0; o < cout; ++o) {
        const double s = (double)g[o] / sqrt((double)var[o] + 1e-5);
        for (int i = 0; i < cin; ++i) f.w[(size_t)o * cin + i] = s * (double)w[(size_t)o * cin + i];
        f.b[o] = s * ((double)b[o] - (double)mu[o]) + (double)be[o];
    }
    return true;
}

struct Builder {
    std::vector<float> buf;
    int alloc(size_t n) { size_t o = (buf.size() + 3) & ~size_t(3); buf.resize(o + n, 0.f); return (int)o; }
};

// Tq[q][v][t] = T[v][t][q]; A copied
bool pack_mix(TensorMap& tm, const std::string& p, int T, int V, Builder& B, int& tq, int& am) {
    const float* Tm = tm.get(p + ".gcn.T", (int64_t)V * T * T);
    const float* A = tm.get(p + ".gcn.A", (int64_t)T * V * V);
    if (!Tm || !A) return false;
    tq = B.alloc((size_t)T * V * T);
    for (int q = 0; q < T; ++q) for (int v = 0; v < V; ++v) for (int t = 0; t < T; ++t)
        B.buf[tq + (q * V + v) * T + t] = Tm[(v * T + t) * T + q];
    am = B.alloc((size_t)T * V * V);
    memcpy(&B.buf[am], A, sizeof(float) * T * V * V);
    return true;
}

// fragment-order coefficients for the MFMA mix (see mix_stage)
// (TP > T: the tables of a frame count padded to TP -- score_tiled_kernel -- with zero coefficients for the pad frames)
bool pack_mix_mfma(TensorMap& tm, const std::string& p, int T, int V, Builder& B, int& tqf, int& af, int TP = 0) {
    const float* Tm = tm.get(p + ".gcn.T", (int64_t)V * T * T);
    const float* A = tm.get(p + ".gcn.A", (int64_t)T * V * V);
    if (!Tm || !A) return false;
    if (TP < T) TP = T;
    const int KS = (V + 3) / 4, MT = (V + 15) / 16;
    const int NR = (KS * TP + 15) / 16;
    // (+ MIX_QPAD zero rows: the ragged frame groups of 5 / 7 / 11 frames compute up to one output frame beyond the last)
    tqf = B.alloc((size_t)(TP + MIX_QPAD) * NR * 64);
    af = B.alloc((size_t)(TP + MIX_QPAD) * MT * KS * 64);
    for (int q = 0; q < T; ++q) for (int r = 0; r < NR; ++r) for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 15, g = lane >> 4, idx = r * 16 + i, s = idx / TP, t = idx % TP, v = mix_vmap(V, s, g);
        B.buf[tqf + (q * NR + r) * 64 + lane] = (idx < KS * TP && v < V && t < T) ? Tm[(v * T + t) * T + q] : 0.f;
    }
    for (int q = 0; q < T; ++q) for (int s = 0; s < KS; ++s) for (int lane = 0; lane < 64; ++lane) {
        const int j = lane & 15, g = lane >> 4, v = mix_vmap(V, s, g);
        for (int mt = 0; mt < MT; ++mt) {
            // m-tile 0: MFMA A fragment (output joint 16mt + j).  V = 17: the one joint beyond it is mixed on the VALU
            // (mix_stage), its coefficient A_q[v][16] replicated over the 16 lanes of the group
            const int w = (V == 17 && mt == 1) ? 16 : mt * 16 + j;
            B.buf[af + ((q * MT + mt) * KS + s) * 64 + lane] = (v < V && w < V) ? A[(q * V + v) * V + w] : 0.f;
        }
    }
    return true;
}

// time-mix coefficients of one layer as the A fragments of tl_time_mix: [joint v][frame tile of a chain][k-step][lane], lane
// (i, g) = gcn.T[v][t = 4 ks + g][q], q = row i of the tile (tiles follow the layer's frame groups, TlGroups)
int pack_time_mfma(const float* Tm, int T, int V, int TP, int NB, Builder& B) {
    const int ngrp = tl_ngrp(V), nch = NB >= ngrp ? NB / ngrp : 1, fgc = NB * TP / ngrp / nch;
    const int mtg = (fgc + 15) / 16, ntc = mtg * (TP / fgc), kt = TP / 4;
    const int off = B.alloc((size_t)V * ntc * kt * 64);
    for (int v = 0; v < V; ++v) for (int tile = 0; tile < ntc; ++tile) for (int ks = 0; ks < kt; ++ks) for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 15, g = lane >> 4, t = 4 * ks + g, r = (tile % mtg) * 16 + i, q = (tile / mtg) * fgc + r;
        B.buf[off + ((size_t)(v * ntc + tile) * kt + ks) * 64 + lane] = (r < fgc && q < T && t < T) ? Tm[((size_t)v * T + t) * T + q] : 0.f;
    }
    return off;
}

// MFMA A-operand fragment order of a logical [M][K] matrix (M, K multiples of 16) with the K permutation that lets
// one ds_read_b128 of the B operand feed four k-steps (see gemm_tiles): element e of lane (i, g) in group kq is
// W[16 mt + i][16 kq + 4 g + e]  (k-step e of the group covers channels {16 kq + 4 g + e : g = 0..3}).
template <class F>
int pack_gemm_frags(Builder& B, int M, int K, F&& w) {
    const int MTn = M / 16, KQ = K / 16;
    const int off = B.alloc((size_t)MTn * KQ * 64 * 4);
    for (int mt = 0; mt < MTn; ++mt) for (int kq = 0; kq < KQ; ++kq) for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 4; ++e) {
            const int row = mt * 16 + (lane & 15), g = lane >> 4;
            B.buf[off + ((size_t)(mt * KQ + kq) * 64 + lane) * 4 + e] = (float)w(row, kq * 16 + 4 * g + e);
        }
    return off;
}

// Linear (out,in) + bias, optionally followed by an eval-mode BatchNorm1d (eps 1e-5): W' = s W, b' = s (b - mu) + beta, in double
bool fold_linear_bn(TensorMap& tm, const std::string& lin, const std::string& bn, int out, int in, Folded& f) {
    const float* w = tm.get(lin + ".weight", (int64_t)out * in);
    const float* b = tm.get(lin + ".bias", out);
    if (!w || !b) return false;
    f.w.resize((size_t)out * in); f.b.resize(out);
    const float *g = nullptr, *be = nullptr, *mu = nullptr, *var = nullptr;
    if (!bn.empty()) {
        g = tm.get(bn + ".weight", out); be = tm.get(bn + ".bias", out);
        mu = tm.get(bn + ".running_mean", out); var = tm.get(bn + ".running_var", out);
        if (!g || !be || !mu || !var) return false;
    }
    for (int o = 0; o < out; ++o) {
        const double s = g ? (double)g[o] / sqrt((double)var[o] + 1e-5) : 1.0;
        for (int i = 0; i < in; ++i) f.w[(size_t)o * in + i] = s * (double)w[(size_t)o * in + i];
        f.b[o] = g ? s * ((double)b[o] - (double)mu[o]) + (double)be[o] : (double)b[o];
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// fold: one ST-GCN layer (stsgcn.py:94-116) -- tcn and residual conv + BatchNorm, the PReLU slope, the combined bias
// ------------------------------------------------------------------------------------------------
struct FoldedLayer {
    int cin, cout;                 // real channels (the fragments pad cin to the caller's cinp)
    bool res;                      // residual conv (cin != cout); otherwise the identity
    Folded ft, fr;
    float slope;
    std::vector<double> bias;      // b_t' (+ b_r')
};
// Reads tcn, residual, prelu in this order (the first missing tensor is the one reported).  Allocates nothing in the buffer.
bool fold_layer(TensorMap& tm, const std::string& p, int cin, int cout, bool res, FoldedLayer& f) {
    f.cin = cin; f.cout = cout; f.res = res;
    if (!fold_conv_bn(tm, p + ".tcn.0", p + ".tcn.1", cout, cin, f.ft)) return false;
    if (res && !fold_conv_bn(tm, p + ".residual.0", p + ".residual.1", cout, cin, f.fr)) return false;
    const float* sl = tm.get(p + ".prelu.weight", 1);
    if (!sl) return false;
    f.slope = sl[0];
    f.bias.resize(cout);
    for (int o = 0; o < cout; ++o) f.bias[o] = f.ft.b[o] + (res ? f.fr.b[o] : 0.0);
    return true;
}
// joint resampler (stsgcn.py:187-199): conv over the joint axis + BatchNorm, w[vout][vin]
bool fold_resampler(TensorMap& tm, const std::string& p, int vin, int vout, Folded& f) {
    return fold_conv_bn(tm, p + ".block.0", p + ".block.1", vout, vin, f);
}

// ------------------------------------------------------------------------------------------------
// emit: a folded layer / resampler into the buffer
// ------------------------------------------------------------------------------------------------
int emit_doubles(Builder& B, const std::vector<double>& v, size_t padded = 0) {
    const int off = B.alloc(padded ? padded : v.size());
    for (size_t i = 0; i < v.size(); ++i) B.buf[off + i] = (float)v[i];
    return off;
}
// plain rows for g_layer: W_t', W_r' (when the layer has one), bias; tq / am are the caller's pack_mix
void emit_plain(const FoldedLayer& f, int V, int embo, Builder& B, GLayer& g) {
    g.cin = f.cin; g.cout = f.cout; g.V = V; g.slope = f.slope; g.embo = embo;
    g.wt = emit_doubles(B, f.ft.w);
    g.wr = f.res ? emit_doubles(B, f.fr.w) : -1;
    g.bias = emit_doubles(B, f.bias);
}
int emit_bias16(const FoldedLayer& f, Builder& B) { return emit_doubles(B, f.bias, ceil16(f.cout)); }
// mix-first fragments of [W_t' | W_r'] (M = cout padded to 16, K = cinp, twice with a residual conv; cinp = cin padded to 16)
int emit_mix_first(const FoldedLayer& f, int cinp, Builder& B) {
    return pack_gemm_frags(B, ceil16(f.cout), cinp * (f.res ? 2 : 1), [&](int r, int k) -> double {
        const bool second = k >= cinp;
        const int kk = second ? k - cinp : k;
        if (r >= f.cout || kk >= f.cin) return 0.0;
        return second ? f.fr.w[(size_t)r * f.cin + kk] : f.ft.w[(size_t)r * f.cin + kk];
    });
}
// [W_t' ; W_r'] stacked, the W-first product of score_kernel's layers 6 and 8 (M = 2 cout, K = cin) as fragments ...
double w_first_at(const FoldedLayer& f, int r, int k) {
    return r < f.cout ? f.ft.w[(size_t)r * f.cin + k] : f.fr.w[(size_t)(r - f.cout) * f.cin + k];
}
int emit_w_first(const FoldedLayer& f, Builder& B) {
    return pack_gemm_frags(B, 2 * f.cout, f.cin, [&](int r, int k) { return w_first_at(f, r, k); });
}
// ... and of layer 10 as its 4 useful rows (2 + 2), plain, for the FMA path
int emit_w_first_rows(const FoldedLayer& f, Builder& B) {
    const int off = B.alloc((size_t)2 * f.cout * f.cin);
    for (int r = 0; r < 2 * f.cout; ++r) for (int k = 0; k < f.cin; ++k) B.buf[off + r * f.cin + k] = (float)w_first_at(f, r, k);
    return off;
}
// MFMA A fragments of a joint resampler, WF[mt][ks][64]: lane (i, g) = W'[16 mt + i][rs_vmap(capture, vin, ks, g)].  capture: the
// k order of the down-samplers whose B operands double as the skip tensors (see resample_stage).  17 output joints: the second
// fragment holds joint 16's weights replicated over each lane group (VALU path).  The bias, padded to 32: behind the fragments
// in the same allocation (bias_off == nullptr: the RsCoef chunks of the tiled kernel) or an allocation of its own.
int emit_resampler(const Folded& f, int vin, int vout, bool capture, Builder& B, int* bias_off) {
    const int KS = capture ? (vin > 16 ? 5 : 4) : (vin + 3) / 4, MTr = (vout + 15) / 16;
    const int wf = B.alloc((size_t)MTr * KS * 64 + (bias_off ? 0 : 32));
    const int bo = bias_off ? (*bias_off = B.alloc(32)) : wf + MTr * KS * 64;
    for (int mt = 0; mt < MTr; ++mt) for (int ks = 0; ks < KS; ++ks) for (int lane = 0; lane < 64; ++lane) {
        const int vo = (vout == 17 && mt == 1) ? 16 : mt * 16 + (lane & 15), v = rs_vmap(capture, vin, ks, lane >> 4);
        B.buf[wf + (mt * KS + ks) * 64 + lane] = (vo < vout && v < vin) ? (float)f.w[(size_t)vo * vin + v] : 0.f;
    }
    for (int vo = 0; vo < vout; ++vo) B.buf[bo + vo] = (float)f.b[vo];
    return wf;
}
// plain rows of a resampler for g_resample
void emit_resampler_plain(const Folded& f, Builder& B, int& w, int& b) { w = emit_doubles(B, f.w); b = emit_doubles(B, f.b); }
// a tensor copied as it is
int emit_copy(Builder& B, const float* src, size_t n) {
    const int off = B.alloc(n);
    memcpy(&B.buf[off], src, sizeof(float) * n);
    return off;
}
void set_layer_row(int* row, int tq, int am, int wp, int bias, float slope) {      // one F_STRIDE row of an offset table
    row[F_TQ] = tq; row[F_AM] = am; row[F_WP] = wp; row[F_BIAS] = bias;
    memcpy(&row[F_SLOPE], &slope, sizeof(float));
}
// mix coefficients of one layer for score_tiled_kernel: the frame count padded to TP
bool emit_tiled_mix(TensorMap& tm, const std::string& p, int T, int V, int TP, Builder& B, TiledNet& TN, int l) {
    if (!pack_mix_mfma(tm, p, T, V, B, TN.tq[l], TN.am[l], TP)) return false;
    const float* Tm = tm.get(p + ".gcn.T", (int64_t)V * T * T);
    if (!Tm) return false;
    TN.tqm[l] = pack_time_mfma(Tm, T, V, TP, tl_nb(TP), B);
    return true;
}

const char* const UNET_LAYER_NAMES[NLAYERS] = {"st_gcnnsp1a.0", "st_gcnnsd1.0", "st_gcnnsd1.1", "st_gcnnsd2.0", "st_gcnnsd2.1", "st_gcnnsd3.0",
                                                "st_gcnnsd3.1", "st_gcnnsu4.0", "st_gcnnsu4.1", "st_gcnnsu3.0", "st_gcnnsu3.1"};
const char* const RS_NAMES[4] = {"down1", "down2", "up3", "up2"};
constexpr int RS_IN[4] = {17, 12, 10, 12}, RS_OUT[4] = {12, 10, 12, 17};

// ------------------------------------------------------------------------------------------------
// The condition encoder of a handle (pose model and latent model alike): folded weights, mix tables and GEMM fragments appended to
// the builder, and where they went.  has: strategy inject; unet: the 'E_unet' architecture; fast: the shipped channel list at a
// frame count cond_fast_kernel is instantiated for.  The table words are written by write_cond_table once the buffer is complete.
// ------------------------------------------------------------------------------------------------
struct CondPack {
    CondW Cw;
    bool has, unet, fast;
    bool fast_table;                // cond_fast_body's table is packed: fast, or asked for by the caller that runs the body itself
    int ctab[4][F_STRIDE];          // cond_fast_body's table
    int utab[TABC_ULB + 1];         // cond table of the 'E_unet' encoder: 7 layers, 2 resamplers, Linear
    TiledNet TNc;                   // ... and its tables for score_tiled_kernel<.., COND> (13 .. 32 condition frames)
    int tiled_cond_tp;
    GenCond GC;                     // plain layout for cond_unet_generic_kernel
};
// want_fast_table: pack cond_fast_body's table for the shipped channel list even where this library holds no cond_fast_kernel for
// the frame count (the latent encode launch runs the body itself)
int pack_cond_encoder(TensorMap& tm, const mcd_model_cfg_t* cfg, Builder& B, CondPack& cp, bool want_fast_table = false) {
    memset(&cp, 0, sizeof(cp));
    CondW& Cw = cp.Cw;
    cp.has = cfg->strategy == MCD_STRATEGY_INJECT;
    cp.unet = cp.has && cfg->cond_layers == MCD_COND_UNET;
    if (cp.unet) {
        const int Tc = cfg->t_cond;
        if (Tc < 1 || Tc > MCD_MAX_FRAMES) return fail(MCD_EUNSUPPORTED, "condition frames must be in 1.." + std::to_string(MCD_MAX_FRAMES));
        Cw.Tc = Tc; Cw.latent = EDIM;
        static const int ucin[7] = {C0, 16, 32, 32, 64, 64, 128}, ucout[7] = {16, 32, 32, 64, 64, 128, CU_OUT}, uv[7] = {17, 17, 17, 12, 12, 10, 10};
        int* utab = cp.utab;
        for (int l = 0; l < 7; ++l) {
            const std::string p = std::string("condition_encoder.") + UNET_LAYER_NAMES[l];
            FoldedLayer f;
            if (!fold_layer(tm, p, ucin[l], ucout[l], ucin[l] != ucout[l], f)) return fail(MCD_EMISSING, tm.missing);
            int tq = 0, am = 0;
            if (!pack_mix_mfma(tm, p, Tc, uv[l], B, tq, am)) return fail(MCD_EMISSING, tm.missing);
            const int wp = emit_mix_first(f, ceil16(f.cin), B);
            set_layer_row(&utab[l * F_STRIDE], tq, am, wp, emit_bias16(f, B), f.slope);
            GLayer& g = cp.GC.L[l];      // plain layout for cond_unet_generic_kernel
            if (!pack_mix(tm, p, Tc, uv[l], B, g.tq, g.am)) return fail(MCD_EMISSING, tm.missing);
            emit_plain(f, uv[l], -1, B, g);
        }
        Folded rs[2];
        for (int r = 0; r < 2; ++r) {
            if (!fold_resampler(tm, std::string("condition_encoder.") + RS_NAMES[r], RS_IN[r], RS_OUT[r], rs[r])) return fail(MCD_EMISSING, tm.missing);
            utab[TABC_URS + 2 * r] = emit_resampler(rs[r], RS_IN[r], RS_OUT[r], false, B, &utab[TABC_URS + 2 * r + 1]);
            emit_resampler_plain(rs[r], B, cp.GC.rs_w[r], cp.GC.rs_b[r]);
        }
        const int64_t F = (int64_t)CU_OUT * Tc * 10;
        const float* lw = tm.get("condition_encoder.to_time_dim.weight", F * EDIM);
        const float* lb = tm.get("condition_encoder.to_time_dim.bias", EDIM);
        if (!lw || !lb) return fail(MCD_EMISSING, tm.missing);
        cp.GC.lw = utab[TABC_ULW] = emit_copy(B, lw, F * EDIM);
        cp.GC.lb = utab[TABC_ULB] = emit_copy(B, lb, EDIM);
        cp.tiled_cond_tp = cond_unet_has_kernel(Tc) ? 0 : tiled_cond_tp_for(Tc);
        if (cp.tiled_cond_tp) {      // the slab-tiled MFMA stages: mix tables for the padded frame count; GEMM fragments, biases, slopes as above
            TiledNet& TNc = cp.TNc;
            for (int l = 0; l < 7; ++l) {
                if (!emit_tiled_mix(tm, std::string("condition_encoder.") + UNET_LAYER_NAMES[l], Tc, uv[l], cp.tiled_cond_tp, B, TNc, l))
                    return fail(MCD_EMISSING, tm.missing);
                TNc.wp[l] = utab[l * F_STRIDE + F_WP]; TNc.bias[l] = utab[l * F_STRIDE + F_BIAS];
                memcpy(&TNc.slope[l], &utab[l * F_STRIDE + F_SLOPE], sizeof(float));
            }
            for (int r = 0; r < 2; ++r) TNc.rsw[r] = emit_resampler(rs[r], RS_IN[r], RS_OUT[r], false, B, nullptr);
            TNc.we = utab[TABC_ULW]; TNc.be = utab[TABC_ULB];
        }
    } else if (cp.has) {
        if (cfg->cond_layers < 1 || cfg->cond_layers > MCD_MAX_COND_LAYERS) return fail(MCD_EINVAL, "bad cond_layers");
        if (cfg->t_cond < 1 || cfg->t_cond > MCD_MAX_FRAMES) return fail(MCD_EUNSUPPORTED, "condition frames must be in 1.." + std::to_string(MCD_MAX_FRAMES));
        Cw.n_layers = cfg->cond_layers; Cw.Tc = cfg->t_cond; Cw.latent = EDIM; Cw.cmax = C0;
        FoldedLayer fl[MCD_MAX_COND_LAYERS];
        int cin = C0;
        for (int l = 0; l < Cw.n_layers; ++l) {
            const int cout = cfg->cond_channels[l];
            if (cout < 1 || cout > 128) return fail(MCD_EUNSUPPORTED, "condition-encoder channels must be in 1..128");
            const std::string p = "condition_encoder.encoder.model_layers." + std::to_string(l);
            if (cout > Cw.cmax) Cw.cmax = cout;
            if (!pack_mix(tm, p, Cw.Tc, 17, B, Cw.L[l].tq, Cw.L[l].am)) return fail(MCD_EMISSING, tm.missing);
            if (!fold_layer(tm, p, cin, cout, cin != cout, fl[l])) return fail(MCD_EMISSING, tm.missing);
            emit_plain(fl[l], 17, -1, B, Cw.L[l]);
            cin = cout;
        }
        const int64_t F = (int64_t)cin * Cw.Tc * 17;
        const float* lw = tm.get("condition_encoder.btlnk.weight", F * EDIM);
        const float* lb = tm.get("condition_encoder.btlnk.bias", EDIM);
        if (!lw || !lb) return fail(MCD_EMISSING, tm.missing);
        Cw.lw = emit_copy(B, lw, F * EDIM);
        Cw.lb = emit_copy(B, lb, EDIM);
        // fast path (cond_fast_kernel): the shipped architecture at a frame count the MFMA stages are instantiated for
        const bool shipped_list = Cw.n_layers == 4 && Cw.L[0].cout == 32 && Cw.L[1].cout == 16 && Cw.L[2].cout == 32 && Cw.L[3].cout == 32;
        cp.fast = shipped_list && cond_fast_has_kernel(Cw.Tc);
        cp.fast_table = cp.fast || (shipped_list && want_fast_table);
        if (cp.fast_table) {
            for (int l = 0; l < 4; ++l) {
                int tq = 0, am = 0;
                if (!pack_mix_mfma(tm, "condition_encoder.encoder.model_layers." + std::to_string(l), Cw.Tc, 17, B, tq, am)) return fail(MCD_EMISSING, tm.missing);
                const int wp = emit_mix_first(fl[l], ceil16(fl[l].cin), B);
                set_layer_row(cp.ctab[l], tq, am, wp, emit_bias16(fl[l], B), fl[l].slope);
            }
        }
        Cw.gmode = 0;      // three buffers in LDS if they fit, else two (CondW::lds_floats)
        if (Cw.lds_floats() * 4 > 160 * 1024) Cw.gmode = 1;
        if (Cw.lds_floats() * 4 > 160 * 1024) return fail(MCD_EUNSUPPORTED, "condition encoder activations exceed LDS");
    }
    return MCD_OK;
}
void write_cond_table(int* tab, const CondPack& cp) {
    if (cp.unet) for (int i = 0; i <= TABC_ULB; ++i) tab[TABC + i] = cp.utab[i];
    if (cp.fast_table) {
        for (int l = 0; l < 4; ++l) for (int f = 0; f < F_STRIDE; ++f) tab[TABC + l * F_STRIDE + f] = cp.ctab[l][f];
        tab[TABC + TABC_LW] = cp.Cw.lw; tab[TABC + TABC_LB] = cp.Cw.lb;
    }
}

// ------------------------------------------------------------------------------------------------
// the two models
// ------------------------------------------------------------------------------------------------
// What a packer returns: the host buffer and every table the handle keeps (the tables zero where a model has no such part).
struct PackedModel {
    std::vector<float> buf;
    GenNet gen;            // pose model: plain layout of the U-Net for score_generic_kernel
    TiledNet tiled;        // ... and the tables of score_tiled_kernel (t_unet without a score_kernel), frame count padded to tiled_tp
    CondPack cond;
    LatentNet net;         // latent model: the denoiser
    int fast_unet;         // pose model: score_has_kernel(t_unet)
    int tiled_tp;
    int zero_row;          // pose model: offset of 32 zero words (an all-zero step_table row for mcd_layer_forward)
    int fused_ok;          // latent model: cond_fast_body's table is packed and t_cond = t_unet
    PackedModel() : fast_unet(0), tiled_tp(0), zero_row(0), fused_ok(0) {
        memset(&gen, 0, sizeof(gen)); memset(&tiled, 0, sizeof(tiled)); memset(&cond, 0, sizeof(cond)); memset(&net, 0, sizeof(net));
    }
};
TensorMap tensor_map(const mcd_tensor_t* tensors, int32_t n_tensors) {
    TensorMap tm;
    for (int i = 0; i < n_tensors; ++i) tm.m[tensors[i].name] = {tensors[i].data, tensors[i].numel};
    return tm;
}
int check_common_cfg(const mcd_model_cfg_t* cfg) {
    if (cfg->num_coords != C0) return fail(MCD_EUNSUPPORTED, "num_coords must be 2");
    if (cfg->n_joints != 17) return fail(MCD_EUNSUPPORTED, "n_joints must be 17 (the reference U-Net hard-wires 17/12/10 joints)");
    if (cfg->emb_dim != EDIM) return fail(MCD_EUNSUPPORTED, "embedding_dim must be 16");
    return MCD_OK;
}
// the embedding Linear of U-Net layer l into the stacked WeAll / beAll
bool copy_emb_linear(TensorMap& tm, const std::string& p, int l, int cout, Builder& B, int we_off, int be_off) {
    const float* we = tm.get(p + ".emb_layer.1.weight", (int64_t)cout * EDIM);
    const float* be = tm.get(p + ".emb_layer.1.bias", cout);
    if (!we || !be) return false;
    memcpy(&B.buf[we_off + (size_t)emb_off(l) * EDIM], we, sizeof(float) * cout * EDIM);
    memcpy(&B.buf[be_off + emb_off(l)], be, sizeof(float) * cout);
    return true;
}

// MoCoDAD: the U-Net (stsae_unet.py:406-438) in the layouts of score_kernel, score_tiled_kernel and score_generic_kernel, + the condition encoder
int pack_pose_model(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, PackedModel& m) {
    const int rc0 = check_common_cfg(cfg);
    if (rc0 != MCD_OK) return rc0;
    const int T = cfg->t_unet;
    if (T < 1 || T > MCD_MAX_FRAMES) return fail(MCD_EUNSUPPORTED, "U-Net frame count must be in 1.." + std::to_string(MCD_MAX_FRAMES));
    m.fast_unet = score_has_kernel(T);     // the instantiated score_kernel<T,...>
    GenNet& G = m.gen;
    TensorMap tm = tensor_map(tensors, n_tensors);
    Builder B;
    std::vector<int> tab(TAB_FLOATS, 0);
    B.alloc(TAB_FLOATS);  // offset table lives at the start of the buffer
    const int we_off = B.alloc((size_t)EMB_TOTAL * EDIM), be_off = B.alloc(EMB_TOTAL + 28);
    FoldedLayer F[NLAYERS];
    for (int l = 0; l < NLAYERS; ++l) {
        const LDesc D = layer_desc(l);
        const std::string p = std::string("model.") + UNET_LAYER_NAMES[l];
        int tq = 0, am = 0;
        if (!pack_mix_mfma(tm, p, T, D.V, B, tq, am)) return fail(MCD_EMISSING, tm.missing);
        // (layer 0: 2 real input channels, zero-padded to one 16-channel block in the fragments)
        if (!fold_layer(tm, p, l == 0 ? C0 : D.cin, D.cout, D.res != 0, F[l])) return fail(MCD_EMISSING, tm.missing);
        if (!copy_emb_linear(tm, p, l, D.cout, B, we_off, be_off)) return fail(MCD_EMISSING, tm.missing);
        if (!pack_mix(tm, p, T, D.V, B, G.L[l].tq, G.L[l].am)) return fail(MCD_EMISSING, tm.missing);
        emit_plain(F[l], D.V, emb_off(l), B, G.L[l]);      // plain layout for the runtime-shape kernel
        const int bias = emit_bias16(F[l], B);
        // score_kernel runs layers 6, 8 and 10 W-first ([W_t' ; W_r'] stacked; layer 10: plain rows), the others mix-first
        const int wp = l == 10 ? emit_w_first_rows(F[l], B) : (l == 6 || l == 8) ? emit_w_first(F[l], B) : emit_mix_first(F[l], D.cin, B);
        set_layer_row(&tab[l * F_STRIDE], tq, am, wp, bias, F[l].slope);
    }
    Folded rs[4];
    for (int r = 0; r < 4; ++r) {
        if (!fold_resampler(tm, std::string("model.") + RS_NAMES[r], RS_IN[r], RS_OUT[r], rs[r])) return fail(MCD_EMISSING, tm.missing);
        // the down-samplers capture the skip tensors (see resample_stage)
        tab[TAB_RSW + r] = emit_resampler(rs[r], RS_IN[r], RS_OUT[r], r < 2, B, &tab[TAB_RSB + r]);
        emit_resampler_plain(rs[r], B, G.rs_w[r], G.rs_b[r]);
    }
    tab[TAB_WE] = G.we = we_off; tab[TAB_BE] = G.be = be_off;
    // tables of score_tiled_kernel (frame counts without a score_kernel, up to its largest padded one): mix coefficients for the
    // padded frame count, non-capture resampler packs; GEMM fragments, biases, slopes and the embedding Linear are the specialised
    // kernels' own -- but for layers 6 and 8, which this kernel runs mix-first like the others
    TiledNet& TN = m.tiled;
    m.tiled_tp = m.fast_unet ? 0 : tiled_tp_for(T);
    if (m.tiled_tp) {
        for (int l = 0; l < NLAYERS; ++l) {
            if (!emit_tiled_mix(tm, std::string("model.") + UNET_LAYER_NAMES[l], T, layer_desc(l).V, m.tiled_tp, B, TN, l)) return fail(MCD_EMISSING, tm.missing);
            TN.wp[l] = (l == 6 || l == 8) ? emit_mix_first(F[l], F[l].cin, B) : tab[l * F_STRIDE + F_WP];
            TN.bias[l] = tab[l * F_STRIDE + F_BIAS]; TN.slope[l] = F[l].slope;
        }
        for (int r = 0; r < 4; ++r) TN.rsw[r] = emit_resampler(rs[r], RS_IN[r], RS_OUT[r], false, B, nullptr);
        TN.we = we_off; TN.be = be_off;
    }
    const int rc = pack_cond_encoder(tm, cfg, B, m.cond);
    if (rc != MCD_OK) return rc;
    write_cond_table(tab.data(), m.cond);
    memcpy(B.buf.data(), tab.data(), sizeof(int) * TAB_FLOATS);
    m.zero_row = B.alloc(32);
    m.buf = std::move(B.buf);
    return MCD_OK;
}

bool latent_dim_ok(int d) { return d >= 16 && d <= LAT_MAX_DIM && d % 16 == 0; }

// layer l of the latent U-Net: its mix, its embedding rows into W_e / b_e, its bias, its fragments mix-first, its table row
int pack_latent_layer(TensorMap& tm, int l, int T, Builder& B, std::vector<int>& tab, int we_off, int be_off) {
    const LDesc Dl = layer_desc(l);
    const std::string p = std::string("model.") + UNET_LAYER_NAMES[l];
    int tq = 0, am = 0;
    if (!pack_mix_mfma(tm, p, T, Dl.V, B, tq, am)) return fail(MCD_EMISSING, tm.missing);
    FoldedLayer f;
    if (!fold_layer(tm, p, l == 0 ? C0 : Dl.cin, Dl.cout, Dl.res != 0, f)) return fail(MCD_EMISSING, tm.missing);
    if (!copy_emb_linear(tm, p, l, Dl.cout, B, we_off, be_off)) return fail(MCD_EMISSING, tm.missing);
    const int bias = emit_bias16(f, B);
    set_layer_row(&tab[l * F_STRIDE], tq, am, emit_mix_first(f, Dl.cin, B), bias, f.slope);
    return MCD_OK;
}
// The part both latent handles share, behind the offset table: the embedding table W_e / b_e with room for emb_rows rows (the rows
// of layers 0 .. 6 filled), the down path's seven layers, every one mix-first, [W_t' | W_r'] (layer 6 too, as in cond_unet_kernel),
// down1 / down2 (non-capturing fragments), to_time_dim for the encode launch's tail or for latent_project_kernel.
int pack_latent_down(TensorMap& tm, int T, int D, int emb_rows, Builder& B, std::vector<int>& tab, int& we_off, int& be_off) {
    we_off = B.alloc((size_t)emb_rows * EDIM); be_off = B.alloc(emb_rows);
    for (int l = 0; l < LAT_DOWN_LAYERS; ++l)
        if (int rc = pack_latent_layer(tm, l, T, B, tab, we_off, be_off)) return rc;
    tab[TAB_WE] = we_off; tab[TAB_BE] = be_off;
    for (int r = 0; r < 2; ++r) {
        Folded f;
        if (!fold_resampler(tm, std::string("model.") + RS_NAMES[r], RS_IN[r], RS_OUT[r], f)) return fail(MCD_EMISSING, tm.missing);
        tab[TAB_RSW + r] = emit_resampler(f, RS_IN[r], RS_OUT[r], false, B, &tab[TAB_RSB + r]);
    }
    const int64_t F = (int64_t)LAT_ENC_C * T * 10;
    const float* lw = tm.get("model.to_time_dim.weight", F * D);
    const float* lb = tm.get("model.to_time_dim.bias", D);
    if (!lw || !lb) return fail(MCD_EMISSING, tm.missing);
    if (latent_project_in_kernel(T)) {
        tab[TAB_LAT_LW] = emit_copy(B, lw, F * D);
    } else {
        // latent_project_kernel: A fragments of W' [D][K], column k' = (t 10 + v) 64 + c of W' = column c T 10 + (t 10 + v) of the
        // weight -- the order in which the encode launch leaves H
        const int TV = T * 10;
        tab[TAB_LAT_LW] = pack_gemm_frags(B, D, (int)F, [&](int r, int k) -> double { return lw[(size_t)r * F + (size_t)(k % LAT_ENC_C) * TV + k / LAT_ENC_C]; });
    }
    tab[TAB_LAT_LB] = emit_copy(B, lb, D);
    return MCD_OK;
}

// The configurations both latent handles refuse.  rows_ok: the handle's launches have kernels for t_unet corrupt frames; head: how
// its message for the frame counts opens
int check_latent_cfg(const mcd_model_cfg_t* cfg, int D, bool rows_ok, const char* head) {
    const int rc0 = check_common_cfg(cfg);
    if (rc0 != MCD_OK) return rc0;
    if (cfg->strategy != MCD_STRATEGY_INJECT) return fail(MCD_EINVAL, "the latent model conditions by 'inject' only (mocodad_latent.py:32)");
    const int T = cfg->t_unet;
    if (T < 1 || T > MCD_MAX_FRAMES || cfg->t_cond < 1 || cfg->t_cond > MCD_MAX_FRAMES)
        return fail(MCD_EUNSUPPORTED, "frame counts must be in 1.." + std::to_string(MCD_MAX_FRAMES));
    if (!rows_ok || cfg->t_cond > 12)
        return fail(MCD_EUNSUPPORTED, std::string(head) + std::to_string(T) + " corrupt + " + std::to_string(cfg->t_cond) +
                                      " condition frames (instantiated: " + latent_encode_counts() + " corrupt frames with 1 .. 12 condition frames)");
    if (cfg->cond_layers != MCD_COND_UNET && (cfg->cond_layers < 1 || cfg->cond_layers > MCD_MAX_COND_LAYERS))
        return fail(MCD_EINVAL, "cond_layers must be 1 .. " + std::to_string(MCD_MAX_COND_LAYERS) + " or MCD_COND_UNET");
    if (cfg->cond_layers == MCD_COND_UNET && !cond_unet_has_kernel(cfg->t_cond))
        return fail(MCD_EUNSUPPORTED, "this library holds no cond_unet_kernel for " + std::to_string(cfg->t_cond) + " condition frames (MCD_COND_UNET_INSTANCES)");
    if (!latent_dim_ok(D)) return fail(MCD_EUNSUPPORTED, "latent_embedding_dim " + std::to_string(D) + ": must be a multiple of 16 in 16..128");
    return MCD_OK;
}
// The condition encoder of a latent handle, packed as the pose model's (the AE decoder is dead work at evaluation and is not read).
// The fused form runs cond_fast_body itself: its table is packed in every build, whatever cond_fast_kernel rows the library holds
int pack_latent_cond(TensorMap& tm, const mcd_model_cfg_t* cfg, Builder& B, std::vector<int>& tab, PackedModel& m) {
    const bool fusable = cfg->t_cond == cfg->t_unet && latent_encode_has_kernel(cfg->t_unet, true);
    const int rc = pack_cond_encoder(tm, cfg, B, m.cond, fusable);
    if (rc != MCD_OK) return rc;
    write_cond_table(tab.data(), m.cond);
    m.fused_ok = m.cond.fast_table && fusable;
    return MCD_OK;
}

// MoCoDADlatent, stage 'pretrain' (mocodad_latent.py:59-64): STSAE_Unet with use_bottleneck -- the down path and to_time_dim as in
// the diffusion stage's handle, then rev_to_time_dim and the up path (stsae_unet.py:365-438) for latent_unproject_kernel and
// latent_decode_kernel -- and the condition encoder.  No denoiser.  The decoder tables exist in this kind of handle only.
int pack_latent_ae_model(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, int latent_dim, PackedModel& m) {
    const int T = cfg->t_unet, D = latent_dim;
    if (int rc = check_latent_cfg(cfg, D, latent_encode_has_kernel(T, false) && latent_decode_has_kernel(T), "the latent autoencoder has no kernels for ")) return rc;

    TensorMap tm = tensor_map(tensors, n_tensors);
    Builder B;
    B.alloc(TAB_FLOATS);
    std::vector<int> tab(TAB_FLOATS, 0);
    int we_off = 0, be_off = 0;
    if (int rc = pack_latent_down(tm, T, D, EMB_TOTAL, B, tab, we_off, be_off)) return rc;
    if (int rc = pack_latent_cond(tm, cfg, B, tab, m)) return rc;
    // ---- the up path: layers 7 .. 10 mix-first like the others (layer 10: its 2 output channels in one 16-row m-tile), their
    // embedding rows behind those of the down path
    for (int l = LAT_DOWN_LAYERS; l < NLAYERS; ++l)
        if (int rc = pack_latent_layer(tm, l, T, B, tab, we_off, be_off)) return rc;
    // up3 / up2, and down1 / down2 once more in the capture k order: the decode launch's down-samplers hold d1 / d2 in registers
    for (int r = 0; r < 4; ++r) {
        Folded f;
        if (!fold_resampler(tm, std::string("model.") + RS_NAMES[r], RS_IN[r], RS_OUT[r], f)) return fail(MCD_EMISSING, tm.missing);
        if (r < 2) tab[TAB_LAT_CAPW + r] = emit_resampler(f, RS_IN[r], RS_OUT[r], true, B, &tab[TAB_LAT_CAPB + r]);
        else tab[TAB_RSW + r] = emit_resampler(f, RS_IN[r], RS_OUT[r], false, B, &tab[TAB_RSB + r]);
    }
    {
        // latent_unproject_kernel: A fragments of W' [640 T][D] and bias', row r' = (t 10 + v) 64 + c = row c T 10 + (t 10 + v) of
        // rev_to_time_dim (the view of stsae_unet.py:434) -- H's order, which the decode launch copies into its LDS region as it lies
        const int TV = T * 10, F = LAT_ENC_C * TV;
        const float* rw = tm.get("model.rev_to_time_dim.weight", (int64_t)F * D);
        const float* rb = tm.get("model.rev_to_time_dim.bias", F);
        if (!rw || !rb) return fail(MCD_EMISSING, tm.missing);
        auto src_row = [&](int r) { return (size_t)(r % LAT_ENC_C) * TV + r / LAT_ENC_C; };
        tab[TAB_LAT_RW] = pack_gemm_frags(B, F, D, [&](int r, int k) -> double { return rw[src_row(r) * D + k]; });
        tab[TAB_LAT_RB] = B.alloc(F);
        for (int r = 0; r < F; ++r) B.buf[tab[TAB_LAT_RB] + r] = rb[src_row(r)];
    }
    memset(&m.net, 0, sizeof(m.net));
    m.net.D = D;
    memcpy(B.buf.data(), tab.data(), sizeof(int) * TAB_FLOATS);
    m.buf = std::move(B.buf);
    return MCD_OK;
}

// MoCoDADlatent: the U-Net's down path (stsae_unet.py:182-219) with its embedding Linears, to_time_dim, the condition encoder,
// the denoiser (components.py:228-241)
int pack_latent_model(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, const mcd_latent_cfg_t* lcfg, PackedModel& m) {
    const int T = cfg->t_unet, D = lcfg->latent_dim, NL = lcfg->n_layers;
    if (int rc = check_latent_cfg(cfg, D, latent_encode_has_kernel(T, false), "the latent encode launch has no kernel for ")) return rc;
    if (NL < 1 || NL > LAT_MAX_LAYERS) return fail(MCD_EUNSUPPORTED, "the denoiser has " + std::to_string(NL) + " layers: 1.." + std::to_string(LAT_MAX_LAYERS) + " are supported");
    for (int l = 0; l < NL; ++l)
        if (!latent_dim_ok(lcfg->hidden[l])) return fail(MCD_EUNSUPPORTED, "denoiser hidden size " + std::to_string(lcfg->hidden[l]) + ": must be a multiple of 16 in 16..128");
    if (lcfg->hidden[NL - 1] != D) return fail(MCD_EINVAL, "the last denoiser hidden size must equal latent_embedding_dim (it predicts the latent's noise)");

    TensorMap tm = tensor_map(tensors, n_tensors);
    Builder B;
    B.alloc(TAB_FLOATS);
    std::vector<int> tab(TAB_FLOATS, 0);
    int we_off = 0, be_off = 0;
    if (int rc = pack_latent_down(tm, T, D, LAT_EMB, B, tab, we_off, be_off)) return rc;
    if (int rc = pack_latent_cond(tm, cfg, B, tab, m)) return rc;
    // ---- the denoiser: Linear -> BatchNorm1d -> ReLU, the last layer a plain Linear; cond_layers apart
    LatentNet& N = m.net;
    N.D = D; N.n_layers = NL;
    for (int l = 0; l < NL; ++l) {
        const int in = l == 0 ? D : lcfg->hidden[l - 1], outc = lcfg->hidden[l];
        const bool last = l == NL - 1;
        const std::string p = "denoiser.net." + std::to_string(l), pc = "denoiser.cond_layers." + std::to_string(l);
        Folded f, fc;
        if (!fold_linear_bn(tm, last ? p : p + ".0", last ? "" : p + ".1", outc, in, f)) return fail(MCD_EMISSING, tm.missing);
        if (!fold_linear_bn(tm, pc, "", outc, EDIM, fc)) return fail(MCD_EMISSING, tm.missing);
        N.in[l] = in; N.out[l] = outc;
        N.wp[l] = pack_gemm_frags(B, outc, EDIM + in, [&](int r, int k) -> double {
            return k < EDIM ? fc.w[(size_t)r * EDIM + k] : f.w[(size_t)r * in + (k - EDIM)];
        });
        N.bias[l] = B.alloc(outc);
        N.cbias[l] = B.alloc(outc);
        for (int o = 0; o < outc; ++o) { B.buf[N.bias[l] + o] = (float)f.b[o]; B.buf[N.cbias[l] + o] = (float)fc.b[o]; }
    }
    memcpy(B.buf.data(), tab.data(), sizeof(int) * TAB_FLOATS);
    m.buf = std::move(B.buf);
    return MCD_OK;
}

// The layout digest of mcd_debug_pack_digest: 64-bit FNV-1a over the buffer, then over the tables as they lie in memory (every
// table was zeroed before it was filled, CondW::base is null), then over the flags as eight int32
uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
uint64_t pack_digest(const PackedModel& m) {
    uint64_t h = 14695981039346656037ull;
    h = fnv1a(h, m.buf.data(), m.buf.size() * sizeof(float));
    h = fnv1a(h, &m.gen, sizeof(m.gen)); h = fnv1a(h, &m.cond.GC, sizeof(m.cond.GC));
    h = fnv1a(h, &m.tiled, sizeof(m.tiled)); h = fnv1a(h, &m.cond.TNc, sizeof(m.cond.TNc));
    h = fnv1a(h, &m.cond.Cw, sizeof(m.cond.Cw)); h = fnv1a(h, &m.net, sizeof(m.net));
    const int32_t flags[8] = {m.fast_unet, m.tiled_tp, m.cond.has, m.cond.unet, m.cond.fast, m.cond.tiled_cond_tp, m.zero_row, m.fused_ok};
    return fnv1a(h, flags, sizeof(flags));
}

}  // namespace

// mcd_stage_table.hpp — the per-wave stage table of score_kernel<3, 2, MINW> (3 U-Net frames x 2 chains per workgroup) and of its
// layer-test twin: for every stage whose unit map is not a shift of the wave index -- the 6-unit mixes (layers 0, 1, 10: unit ->
// (chain, frame) is a division by 3), the 12-unit SAMEQ mixes (layers 2, 3, 8, 9) and the resamplers that follow their map
// (down1, up2) -- the LDS byte offsets of a wave's units and the mixes' offsets into their coefficient tables, generated at compile time from the types that define them (Plan,
// MixCfg, emb_off) and checked against the stage code's own expressions below.  The kernel reads a row (32 bytes: s_load_dwordx4 +
// dwordx2) where the stage's coefficient prefetch is issued (StageRow, stage_row: mcd_device.hpp); the stage then runs none of the
// wave -> unit -> (chain, block, frame) -> offset arithmetic, which it used to repeat for every unit and use.
// The table lives in the constant memory of the translation unit that instantiates the kernel; the packed weight buffer is unchanged.
#pragma once
#include "mcd_device.hpp"

namespace mcd {

// rows of a wave; a two-round stage has its second round's row right behind the first (a wave without a unit there: unit 0's addresses, read and never stored to)
namespace srow { enum { L0 = 0, L1 = 1, L2 = 2, DN1 = 4, L3 = 6, L8 = 8, UP2 = 10, L9 = 12, L10 = 14, NROWS = 16 }; }

template <int T, int NB>
struct StageTabGen {
    static_assert(T == 3 && NB == 2 && NWAVES == 8, "the stage table is generated for the 3-frame x 2-chain kernel of 8 waves");
    using PL = Plan<T, NB>;
    using M16 = MixCfg<16, 17, T, NB>;      // layers 0, 1, 10: 6 units, one round
    using M17 = MixCfg<32, 17, T, NB>;      // layers 2, 9: 12 units, SAMEQ
    using M12 = MixCfg<32, 12, T, NB>;      // layers 3, 8 and the unit map of down1 / up2 (SQMAP): 12 units, SAMEQ
    static_assert(M16::QC == 1 && M16::UNITS == 6 && M16::PER == 1 && M17::SAMEQ && M12::SAMEQ && M17::PER == 2 && M12::PER == 2, "unit maps the rows are generated for");
    enum { L0 = srow::L0, L1 = srow::L1, L2 = srow::L2, DN1 = srow::DN1, L3 = srow::L3, L8 = srow::L8, UP2 = srow::UP2, L9 = srow::L9, L10 = srow::L10, NROWS = srow::NROWS };
    struct Tab { StageRow r[NWAVES][NROWS]; };

    struct Unit { int n, cb, q; };          // chain, 16-channel block, output frame
    template <class M>
    static constexpr Unit unit(int wave, int round) {      // (the decomposition of mix_stage / resample_stage's unit_at)
        const int um = M::unit_of(wave, round);
        const int u = um < 0 ? 0 : um;      // (a wave without a unit there reads unit 0's rows and stores nothing, as in mix_stage)
        const int rest = u / M::NQ;
        return Unit{rest / M::CB, rest % M::CB, (u % M::NQ) * M::QC};
    }
    // a mix: load_x reads in + n (T V) cs_in + 16 cb; the store functor writes out + n (T V) cs_out + q (V cs_out) + 16 cb
    template <class M>
    static constexpr StageRow mix_row(int wave, int round, int V, int in, int cs_in, int out, int cs_out, int aux = 0, int aux2 = 0) {
        const Unit u = unit<M>(wave, round);
        // (MixCoef::load_unit: tqd[(q NR + r) 64 + lane], af[((q MT + mt) KS + ks) 64 + lane])
        return StageRow{4u * (unsigned)(in + u.n * (T * V) * cs_in + u.cb * 16),
                        4u * (unsigned)(out + u.n * (T * V) * cs_out + u.q * (V * cs_out) + u.cb * 16),
                        4u * (unsigned)(aux + u.n * EMB_STRIDE + u.cb * 16), 4u * (unsigned)(aux2 + u.cb * 16),
                        4u * (unsigned)(u.q * M::NR * 64), 4u * (unsigned)(u.q * M::MT * M::KS * 64), 0u, 0u};
    }
    // a resampler on the SAMEQ map: frame nt = n T + q, reads in + nt VIN cs_in + 16 cb, writes out + nt VOUT cs_out + 16 cb
    static constexpr StageRow rs_row(int wave, int slot, int in, int vin, int cs_in, int out, int vout, int cs_out) {
        const Unit u = unit<M12>(wave, slot);
        const int nt = u.n * T + u.q;
        return StageRow{4u * (unsigned)(in + nt * vin * cs_in + u.cb * 16), 4u * (unsigned)(out + nt * vout * cs_out + u.cb * 16), 0u, 0u, 0u, 0u, 0u, 0u};
    }
    static constexpr Tab make() {
        Tab t{};
        for (int w = 0; w < NWAVES; ++w) {
            StageRow* r = t.r[w];
            r[L0] = mix_row<M16>(w, 0, 17, PL::O_XT, 4, PL::L0_z, 20);                     // layer 0 reads the chain state XT[col][4] in place
            r[L1] = mix_row<M16>(w, 0, 17, PL::L1_in, 20, PL::L1_z, 20);
            r[L10] = mix_row<M16>(w, 0, 17, PL::L10_p, 20, PL::O_ZO, 2);                   // W-first: mixes P[col][20], stores ZO[col][2 coordinates]
            for (int k = 0; k < 2; ++k) {
                r[L2 + k] = mix_row<M17>(w, k, 17, PL::L2_in, 36, PL::L2_z, 36);
                r[L9 + k] = mix_row<M17>(w, k, 17, PL::L9_in, 36, PL::L9_z, 36);
                r[L3 + k] = mix_row<M12>(w, k, 12, PL::L3_in, 36, PL::L3_z, 36);
                // W-first layer 8: mixes P_t of P[col][68], seeds from / stores to P_r (+ 32); its embedding row and folded bias
                r[L8 + k] = mix_row<M12>(w, k, 12, PL::L8_p, 68, PL::L8_p + 32, 68, PL::O_EMB + emb_off(8), PL::O_BIA + 80);
                r[DN1 + k] = rs_row(w, k, PL::L2_out, 17, 36, PL::DN1_out, 12, 36);
                r[UP2 + k] = rs_row(w, k, PL::L8_p + 32, 12, 68, PL::UP2_out, 17, 36);
            }
        }
        return t;
    }
};
template <int T, int NB>
struct StageTab : StageTabGen<T, NB> {
    using G = StageTabGen<T, NB>;
    using typename G::Tab;
    using typename G::Unit;
    using typename G::PL;
    using typename G::M12;
    using typename G::M17;
    static constexpr Tab tab = G::make();

    // ---- compile-time checks (stage_tab_checked below): the unit maps in closed form, every unit of a stage owned by exactly one
    //      (wave, round) with the addresses the stage code's expressions give it, rows inside the plan
    static constexpr bool sameq_closed_form() {     // waves 0-3: frame w/2, chain w&1, block = round; waves 4-7: frame 2, chain (w-4)/2, block w&1
        for (int w = 0; w < NWAVES; ++w)
            for (int k = 0; k < 2; ++k) {
                if (w >= 4 && k == 1) { if (M12::unit_of(w, k) >= 0 || M17::unit_of(w, k) >= 0) return false; continue; }
                const Unit a = G::template unit<M12>(w, k), b = G::template unit<M17>(w, k);
                const Unit c = w < 4 ? Unit{w & 1, k, w >> 1} : Unit{(w - 4) >> 1, w & 1, 2};
                if (a.n != c.n || a.cb != c.cb || a.q != c.q || b.n != c.n || b.cb != c.cb || b.q != c.q) return false;
            }
        return true;
    }
    // rows `row` (+ round) of the waves that have a unit there hold, for every (chain n, block cb, frame q) exactly once,
    // in_b = in0 + n in_n + q in_q + 64 cb and out_b = out0 + n out_n + q out_q + 64 cb (bytes)
    static constexpr bool covers(int row, int rounds, int ncb, unsigned in0, unsigned in_n, unsigned in_q, unsigned out0, unsigned out_n, unsigned out_q, unsigned tq_q = 0u, unsigned af_q = 0u) {
        for (int n = 0; n < NB; ++n)
            for (int cb = 0; cb < ncb; ++cb)
                for (int q = 0; q < T; ++q) {
                    int hits = 0;
                    for (int w = 0; w < NWAVES; ++w)
                        for (int k = 0; k < rounds; ++k) {
                            if (rounds == 1 ? w >= 6 : (k == 1 && w >= 4)) continue;      // (no unit there)
                            const StageRow& r = tab.r[w][row + k];
                            if (r.in_b == in0 + n * in_n + q * in_q + cb * 64u && r.out_b == out0 + n * out_n + q * out_q + cb * 64u &&
                                (tq_q == 0u || (r.tq_o == q * tq_q && r.af_o == q * af_q))) ++hits;
                        }
                    if (hits != 1) return false;
                }
        return true;
    }
    static constexpr bool in_plan() {
        for (int w = 0; w < NWAVES; ++w)
            for (int i = 0; i < G::NROWS; ++i) {
                const StageRow& r = tab.r[w][i];
                if (r.in_b % 16 || r.out_b % 8 || r.aux_b % 16 || r.aux2_b % 16) return false;
                if (r.in_b >= PL::BYTES || r.out_b >= PL::BYTES || r.aux_b >= PL::BYTES || r.aux2_b >= PL::BYTES) return false;
            }
        return true;
    }
};
template <int T, int NB>
constexpr bool stage_tab_checked() {
    using S = StageTab<T, NB>;
    using PL = Plan<T, NB>;
    constexpr unsigned TV17 = T * 17, TV12 = T * 12;
    static_assert(S::sameq_closed_form(), "SAMEQ unit map: not the closed form the rows were checked against");
    static_assert(S::in_plan(), "a stage-table row points outside the LDS plan or is misaligned");
    // mixes (mix_stage's load_x, the layers' store functors): in = region + n (T V) cs_in + 16 cb, out = region + n (T V) cs_out + q V cs_out + 16 cb
    static_assert(S::covers(S::L0, 1, 1, 4u * PL::O_XT, 4u * TV17 * 4, 0u, 4u * PL::L0_z, 4u * TV17 * 20, 4u * 17 * 20, 256u, 4u * 2 * 5 * 64), "layer 0 rows");
    static_assert(S::covers(S::L1, 1, 1, 4u * PL::L1_in, 4u * TV17 * 20, 0u, 4u * PL::L1_z, 4u * TV17 * 20, 4u * 17 * 20, 256u, 4u * 2 * 5 * 64), "layer 1 rows");
    static_assert(S::covers(S::L10, 1, 1, 4u * PL::L10_p, 4u * TV17 * 20, 0u, 4u * PL::O_ZO, 4u * TV17 * 2, 4u * 17 * 2, 256u, 4u * 2 * 5 * 64), "layer 10 rows");
    static_assert(S::covers(S::L2, 2, 2, 4u * PL::L2_in, 4u * TV17 * 36, 0u, 4u * PL::L2_z, 4u * TV17 * 36, 4u * 17 * 36, 256u, 4u * 2 * 5 * 64), "layer 2 rows");
    static_assert(S::covers(S::L9, 2, 2, 4u * PL::L9_in, 4u * TV17 * 36, 0u, 4u * PL::L9_z, 4u * TV17 * 36, 4u * 17 * 36, 256u, 4u * 2 * 5 * 64), "layer 9 rows");
    static_assert(S::covers(S::L3, 2, 2, 4u * PL::L3_in, 4u * TV12 * 36, 0u, 4u * PL::L3_z, 4u * TV12 * 36, 4u * 12 * 36, 256u, 4u * 1 * 3 * 64), "layer 3 rows");
    static_assert(S::covers(S::L8, 2, 2, 4u * PL::L8_p, 4u * TV12 * 68, 0u, 4u * (PL::L8_p + 32), 4u * TV12 * 68, 4u * 12 * 68, 256u, 4u * 1 * 3 * 64), "layer 8 rows");
    // resamplers (resample_stage): in = region + (n T + q) VIN cs_in + 16 cb, out = region + (n T + q) VOUT cs_out + 16 cb
    static_assert(S::covers(S::DN1, 2, 2, 4u * PL::L2_out, 4u * TV17 * 36, 4u * 17 * 36, 4u * PL::DN1_out, 4u * TV12 * 36, 4u * 12 * 36), "down1 rows");
    static_assert(S::covers(S::UP2, 2, 2, 4u * (PL::L8_p + 32), 4u * TV12 * 68, 4u * 12 * 68, 4u * PL::UP2_out, 4u * TV17 * 36, 4u * 17 * 36), "up2 rows");
    return true;
}

}  // namespace mcd

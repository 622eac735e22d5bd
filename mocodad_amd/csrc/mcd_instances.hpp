// mcd_instances.hpp — every kernel instantiation of libmocodad_hip.so and the translation unit that holds it.
//
// The library is built from mcd_api.hip (C ABI, dispatch; it includes the packer, mcd_pack.hpp, and the runtime-shape kernels,
// mcd_generic_kernel.hpp) plus mcd_inst.hip compiled once
// per unit with -DMCD_INST_UNIT_<n>: a unit explicitly instantiates the launcher templates of its rows (and with them the
// kernels); every other translation unit sees them as `extern template` and compiles none of that device code.  The units
// build in parallel (mocodad_amd/build.py); their number and the assignment below only balance compile times.
// These tables are the ONLY list: the instantiations (mcd_inst.hip), the `extern template` declarations (mcd_launch.hpp), the
// dispatch switches (mcd_api.hip) and the "is there a kernel for this frame count" predicates at the end of this file all
// expand them.  A new frame count or workgroup shape is a row here (and, for a new unit, MCD_INST_UNITS); nothing else.
//   X(unit, T_u, NB, MINW, LT)   score_kernel<T_u, NB, MINW, LT>      (LT: the layer-test form behind mcd_layer_forward)
//   X(unit, variant, T_u, NB, MINW)  ... an alternative workgroup shape of T_u frames, taken when MCD_OPT_VARIANT == variant
//   X(unit, T_c, NB)             cond_fast_kernel / cond_unet_kernel<T_c, NB>
//   X(unit, TP, NB, LT)          score_tiled_kernel<TP, NB, LT>
//   X(unit, TP, NB)              score_tiled_kernel<TP, NB, false, true>: the 'E_unet' condition encoder at 13 .. 32 condition frames
//   X(unit, T, NB, COND_IN_KERNEL, PROJECT_IN_KERNEL)   latent_encode_kernel (at the end of this file; its translation unit is mcd_latent.hip)
//   X(unit, T)                   latent_decode_kernel<T>, latent_decode_samples_kernel<T> (likewise)
#pragma once

#ifndef MCD_FAST_T      // the shipped library

#define MCD_INST_UNITS 25

// Per-unit compile flags (mocodad_amd/build.py reads these lines).  The wave count of a workgroup is a translation-unit constant
// (MCD_NWAVES): units 3, 5, 23, 11 and 12 hold ONLY the 12-frame, the 9- / 10- / 11-frame and the 24- / 32-frame (slab-tiled) trajectory kernels and build them with twelve waves per workgroup -- three per SIMD,
// 168 registers, 12 mix units per stage, n-thirds in the 64-channel GEMMs: +2.6 % over eight waves (profiles/r04ak_t12_w12_ab.txt).
// Its launcher (the same translation unit) launches 768 threads; nothing outside the unit depends on the wave count.
#define MCD_UNIT_FLAGS_3 "-DMCD_NWAVES=12"      // (round 4 added -mllvm -amdgpu-sched-strategy=iterative-minreg: 25 -> 19 spilled registers, +0.6 %; the kernel has spilled nothing since round 5, and the default strategy is +0.3 .. 0.4 % now: profiles/r06j_switch_sweep_ab.txt)
#define MCD_UNIT_FLAGS_23 "-DMCD_NWAVES=12 -mllvm -amdgpu-sched-strategy=iterative-minreg"     // 9 frames: +1.3 % with it (11 frames -2.4 %, 24 / 32 frames -0.7 / -3.2 %: default strategy, profiles/r04at_minreg_ab.txt)
#define MCD_UNIT_FLAGS_11 "-DMCD_NWAVES=12"     // the slab-tiled kernel at 24 frames: +4.5 % (profiles/r04aq_tiled_w12_ab.txt)
#define MCD_UNIT_FLAGS_12 "-DMCD_NWAVES=12"     // ... and at 32 frames: +2.0 %
#define MCD_UNIT_FLAGS_5 "-DMCD_NWAVES=12"      // 9, 10 and 11 frames (profiles/r04al_w12_shapes_ab.txt, r04an_t10_w12_ab.txt)
// The layer-test (LT) forms behind mcd_layer_forward are built with the flags AND the template arguments of their production
// twins, so that the stage tests run the shipped stage code (the twelve-wave mix tables, n-thirds tiling, skip-round branches):
#define MCD_UNIT_FLAGS_24 "-DMCD_NWAVES=12 -mllvm -amdgpu-sched-strategy=iterative-minreg"     // LT of 9 frames (= unit 23)
#define MCD_UNIT_FLAGS_25 "-DMCD_NWAVES=12"     // LT of 10, 11 and 12 frames (= units 5, 3)
#define MCD_UNIT_FLAGS_15 "-DMCD_NWAVES=12"     // LT of the slab-tiled kernel at 24 frames (= unit 11)
#define MCD_UNIT_FLAGS_16 "-DMCD_NWAVES=12"     // ... and at 32 frames (= unit 12)

#ifdef MCD_TUNING_VARIANTS      // alternative workgroup shapes (MCD_OPT_VARIANT, bench.py --variant): developer builds only
#define MCD_SCORE_VARIANT_INSTANCES(X) \
    X(1, 1, 3, 4, 2)      /* 4 chains / WG, 1 WG per CU */ \
    X(1, 3, 3, 1, 4)      /* 1 chain / WG */ \
    X(1, 2, 3, 2, 2)      /* the default shape without the register cap */ \
    X(2, 1, 6, 2, 2)      /* 2 chains / WG, 1 WG per CU (no register cap) */
#else
#define MCD_SCORE_VARIANT_INSTANCES(X)
#endif

#define MCD_SCORE_INSTANCES(X) \
    X(1, 3, 2, 4, false)  /* HR-Avenue / HR-STC: 2 chains per workgroup, 2 workgroups per CU (<= 128 VGPRs) */ \
    X(1, 1, 4, 4, false)  /* (4 chains / WG, 2 WGs per CU) */ \
    X(1, 2, 2, 4, false)  /* e.g. seg_len 4 split in halves (2 chains / WG, 2 WGs per CU: every mix is one round of units; +31 % over <2,3,4>, profiles/r04aa_t2_nb_ab.txt) */ \
    X(2, 6, 1, 4, false)  /* concat over 6 frames: 1 chain / WG, 2 WGs per CU */ \
    X(2, 4, 1, 4, false)  /* e.g. seg_len 8 split in halves */ \
    X(3, 12, 1, 3, false) /* seg_len 24 split in halves: 1 workgroup of TWELVE waves per CU (unit 3 is compiled with MCD_UNIT_FLAGS_3), 168 registers */ \
    X(22, 8, 1, 2, false) /* e.g. seg_len 8 concat / seg_len 12 with 4 condition frames */ \
    X(4, 5, 1, 4, false)  /* e.g. seg_len 10 split in halves (1 chain / WG, 2 WGs per CU: +4.7 % over <5,2,2>, profiles/r04r_t5_shape_ab.txt) */ \
    X(4, 7, 1, 2, false)  /* odd frame counts: one output frame per mix unit */ \
    X(23, 9, 1, 3, false) X(5, 10, 1, 3, false) X(5, 11, 1, 3, false) /* twelve waves as well (unit 5): +3.7 / +0.9 / +0.9 %; 7 and 8 frames measured -1 % / +0.2 %: eight waves */ \
    X(9, 3, 2, 4, true) X(9, 6, 1, 4, true) X(25, 12, 1, 3, true) X(24, 9, 1, 3, true)     /* the layer-test forms: the template arguments of their production twins */ \
    X(13, 5, 1, 4, true) X(13, 7, 1, 2, true) X(25, 10, 1, 3, true) X(25, 11, 1, 3, true)

#define MCD_COND_FAST_INSTANCES(X) \
    X(7, 1, 4) X(7, 2, 3) X(7, 3, 2) X(7, 4, 2) X(7, 5, 2) X(7, 6, 2) X(7, 7, 1) X(7, 8, 1) X(7, 9, 1) X(7, 10, 1) X(7, 11, 1) X(7, 12, 1) \
    X(20, 13, 1) X(20, 14, 1) X(20, 15, 1) X(20, 16, 1) X(21, 17, 1) X(21, 18, 1) X(21, 19, 1) X(21, 20, 1)   /* 13 .. 20 frames: one window per workgroup, up to 158 KB of LDS */

#define MCD_COND_UNET_INSTANCES(X) \
    X(8, 1, 4) X(8, 2, 2) X(8, 3, 2) X(8, 4, 2) X(8, 5, 2) X(8, 6, 1) X(8, 7, 1) X(10, 8, 1) X(10, 9, 1) X(10, 10, 1) X(10, 11, 1) X(10, 12, 1)

#define MCD_TILED_INSTANCES(X) X(6, 16, 1, false) X(11, 24, 1, false) X(12, 32, 1, false) X(14, 16, 1, true) X(15, 24, 1, true) X(16, 32, 1, true)

#define MCD_TILED_COND_INSTANCES(X) X(17, 16, 1) X(18, 24, 1) X(19, 32, 1)

#else
// Developer builds (python -m mocodad_amd.build --fast-t T [-D MCD_FAST_NB= -D MCD_FAST_MINW= -D MCD_FAST_TILED=16|24|32
// -D MCD_FAST_TILED_COND=16|24|32]): the same tables with only the requested rows, all in unit 1, and one flag set for every
// file.  Everything generated from the tables follows: such a library answers a frame count it does not hold the way the
// shipped one answers a frame count IT does not hold.
#define MCD_INST_UNITS 1
#ifndef MCD_FAST_NB
#define MCD_FAST_NB (MCD_FAST_T == 3 ? 2 : 1)
#endif
#ifndef MCD_FAST_MINW
#define MCD_FAST_MINW (MCD_NWAVES == 12 ? 3 : MCD_FAST_T >= 7 ? 2 : 4)
#endif
#define MCD_SCORE_INSTANCES(X) X(1, MCD_FAST_T, MCD_FAST_NB, MCD_FAST_MINW, false)
#define MCD_SCORE_VARIANT_INSTANCES(X)
#define MCD_COND_FAST_INSTANCES(X) X(1, MCD_FAST_T, MCD_FAST_NB)
#define MCD_COND_UNET_INSTANCES(X) X(1, MCD_FAST_T, MCD_FAST_NB)
#ifdef MCD_FAST_TILED
#define MCD_TILED_INSTANCES(X) X(1, MCD_FAST_TILED, 1, false)
#else
#define MCD_TILED_INSTANCES(X)
#endif
#ifdef MCD_FAST_TILED_COND
#define MCD_TILED_COND_INSTANCES(X) X(1, MCD_FAST_TILED_COND, 1)
#else
#define MCD_TILED_COND_INSTANCES(X)
#endif
#endif  // MCD_FAST_T

// The encode launch of the latent model (mcd_latent.hip, built in shipped and developer libraries alike):
//   X(unit, T, NB, COND_IN_KERNEL, PROJECT_IN_KERNEL)   latent_encode_kernel<T, NB, COND_IN_KERNEL, PROJECT_IN_KERNEL>: T corrupt frames
//       COND_IN_KERNEL     true = the shipped condition encoder at T condition frames inside the launch, false = cond_emb from a
//                          condition-encoder launch of the rows above
//       PROJECT_IN_KERNEL  true = to_time_dim as the kernel's tail; false = the kernel writes the last layer's output H (B, 640 T)
//                          and latent_project_kernel (one MFMA launch for all windows) computes z0 from it
//       unit               0 = mcd_latent.hip as it is compiled for the chain, projection and Philox kernels; n = 1 .. MCD_LATENT_UNITS:
//                          the same file compiled once more with -DMCD_LATENT_UNIT=n (mocodad_amd/build.py does), holding only the
//                          encode kernels of its rows.  The assignment only balances compile times.
// A developer build (MCD_FAST_T) keeps the 3-frame rows and the row of MCD_FAST_T if there is one, all in unit 0.
#define MCD_LATENT_ENCODE_INSTANCES(X) \
    X(0, 3, 2, true, true) X(0, 3, 2, false, true) \
    X(1, 5, 1, false, false) X(1, 12, 1, false, false) X(2, 6, 1, false, false) X(2, 11, 1, false, false) \
    X(3, 7, 1, false, false) X(3, 10, 1, false, false) X(4, 8, 1, false, false) X(4, 9, 1, false, false)
// The decode launch of the latent autoencoder (stage 'pretrain'; latent_decode_kernel<T> of mcd_encode_kernel.hpp, one window per
// workgroup), in units of mcd_latent.hip like the encode rows -- units of their own, so that no object of the rows above changes:
//   X(unit, T)   latent_decode_kernel<T>: T corrupt frames, the frame counts of the encode rows
// A developer build keeps the 3-frame row and the row of MCD_FAST_T, in unit 0.
#define MCD_LATENT_DECODE_INSTANCES(X) \
    X(5, 3) X(5, 5) X(5, 6) X(6, 7) X(6, 8) X(7, 9) X(7, 10) X(8, 11) X(8, 12)
// The decode launch for all generated latents of a window (mcd_latent_decode_samples; latent_decode_samples_kernel<T>, one window and
// a range of its samples per workgroup), again in units of its own:
//   X(unit, T)   latent_decode_samples_kernel<T>: the frame counts of the rows above
#define MCD_LATENT_DECODE_SAMPLES_INSTANCES(X) \
    X(9, 3) X(9, 5) X(9, 6) X(10, 7) X(10, 8) X(11, 9) X(11, 10) X(12, 11) X(12, 12)
#ifndef MCD_FAST_T
#define MCD_LATENT_UNITS 12
#else
#define MCD_LATENT_UNITS 0
#endif

// What the tables hold, for the packer and the dispatch of mcd_api.hip (a frame count outside them takes the next more general
// kernel: slab-tiled, then runtime-shape).
namespace mcd {
#define MCD_ROW_IS_T(unit, T, ...) || t == (T)
#define MCD_ROW_IS_T_LT(unit, T, NB, MINW, LT) || (t == (T) && lt == (LT))
#define MCD_ROW_TP(unit, TP, NB, LT) if (!(LT) && (TP) >= t && (tp == 0 || (TP) < tp)) tp = (TP);
#define MCD_ROW_TP_COND(unit, TP, NB) if ((TP) >= t && (tp == 0 || (TP) < tp)) tp = (TP);
constexpr bool score_has_kernel(int t, bool lt = false) { return false MCD_SCORE_INSTANCES(MCD_ROW_IS_T_LT); }   // score_kernel<t, ..., lt>
constexpr bool cond_fast_has_kernel(int t) { return false MCD_COND_FAST_INSTANCES(MCD_ROW_IS_T); }
constexpr bool cond_unet_has_kernel(int t) { return false MCD_COND_UNET_INSTANCES(MCD_ROW_IS_T); }
// padded frame count of the slab-tiled kernel (and of its COND form) that holds t frames: the smallest one instantiated; 0 = none
constexpr int tiled_tp_for(int t) { int tp = 0; MCD_TILED_INSTANCES(MCD_ROW_TP) return tp; }
constexpr int tiled_cond_tp_for(int t) { int tp = 0; MCD_TILED_COND_INSTANCES(MCD_ROW_TP_COND) return tp; }
#define MCD_ROW_COUNT(...) +1
constexpr bool score_has_variants() { return (0 MCD_SCORE_VARIANT_INSTANCES(MCD_ROW_COUNT)) > 0; }
#undef MCD_ROW_IS_T
#undef MCD_ROW_IS_T_LT
#undef MCD_ROW_TP
#undef MCD_ROW_TP_COND
#undef MCD_ROW_COUNT
}  // namespace mcd

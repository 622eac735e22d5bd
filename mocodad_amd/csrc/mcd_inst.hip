// mcd_inst.hip — one unit of kernel instantiations (see mcd_instances.hpp); compiled once per unit n = 1 .. MCD_INST_UNITS with
// -DMCD_INST_UNIT_<n> (mocodad_amd/build.py does).
#include "mcd_launch.hpp"

// MCD_IN_UNIT(u)(code) is `code` in the unit that is being compiled and nothing elsewhere: MCD_INST_UNIT_<u> is defined (as 1, by
// -D) only there, and an undefined name pastes to an identifier that no MCD_PROBE_ macro answers.
#define MCD_PROBE_1 ~, MCD_KEEP
#define MCD_KEEP(...) __VA_ARGS__
#define MCD_DROP(...)
#define MCD_SECOND(a, b, ...) b
#define MCD_PROBE(...) MCD_SECOND(__VA_ARGS__, MCD_DROP, ~)
#define MCD_PASTE(a, b) a##b
#define MCD_PROBE_OF(x) MCD_PROBE(MCD_PASTE(MCD_PROBE_, x))
#define MCD_IN_UNIT(u) MCD_PROBE_OF(MCD_INST_UNIT_##u)

namespace mcd {

#define MCD_DEF_SCORE(unit, T, NB, MINW, LT) MCD_IN_UNIT(unit)(template int launch_score_t<T, NB, MINW, LT>(ScoreParams&, hipStream_t, bool*);)
#define MCD_DEF_VARIANT(unit, variant, T, NB, MINW) MCD_DEF_SCORE(unit, T, NB, MINW, false)
#define MCD_DEF_COND_FAST(unit, T, NB) \
    MCD_IN_UNIT(unit)(template int launch_cond_fast_t<T, NB>(const mcd_weights*, const DataView&, const FrameIdx&, int, float*, int, hipStream_t);)
#define MCD_DEF_COND_UNET(unit, T, NB) \
    MCD_IN_UNIT(unit)(template int launch_cond_unet_t<T, NB>(const mcd_weights*, const DataView&, const FrameIdx&, int, float*, int, hipStream_t);)
#define MCD_DEF_TILED(unit, TP, NB, LT) \
    MCD_IN_UNIT(unit)(template int launch_score_tiled_t<TP, NB, LT>(const mcd_weights*, const ScoreParams&, const FrameMaps&, float*, int, hipStream_t);)
#define MCD_DEF_TILED_COND(unit, TP, NB) \
    MCD_IN_UNIT(unit)(template int launch_score_tiled_t<TP, NB, false, true>(const mcd_weights*, const ScoreParams&, const FrameMaps&, float*, int, hipStream_t);)
MCD_SCORE_INSTANCES(MCD_DEF_SCORE)
MCD_SCORE_VARIANT_INSTANCES(MCD_DEF_VARIANT)
MCD_COND_FAST_INSTANCES(MCD_DEF_COND_FAST)
MCD_COND_UNET_INSTANCES(MCD_DEF_COND_UNET)
MCD_TILED_INSTANCES(MCD_DEF_TILED)
MCD_TILED_COND_INSTANCES(MCD_DEF_TILED_COND)

// every unit 1 .. MCD_INST_UNITS holds rows (mcd_launch.hpp refuses a row outside that range): a unit without any was compiled without its -D
#define MCD_COUNT(unit, ...) MCD_IN_UNIT(unit)(+1)
static_assert((0 MCD_SCORE_INSTANCES(MCD_COUNT) MCD_SCORE_VARIANT_INSTANCES(MCD_COUNT) MCD_COND_FAST_INSTANCES(MCD_COUNT) MCD_COND_UNET_INSTANCES(MCD_COUNT)
               MCD_TILED_INSTANCES(MCD_COUNT) MCD_TILED_COND_INSTANCES(MCD_COUNT)) > 0,
              "compile with -DMCD_INST_UNIT_<n>, n = 1 .. MCD_INST_UNITS (mocodad_amd/build.py does)");

}  // namespace mcd

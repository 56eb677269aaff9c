// engine_tuning.h -- the settings of an engine that oc_hip_set_tuning, set_self_adaptive and set_damping write and that a device
// group's members share with their leader (EngineTuning: one assignment makes a member), and THE statement of the tuning keys:
// one row per key with its field, its default (the field's initialiser), its rule, the engine kinds that may set a non-zero value
// and the values only the A/B build of the library accepts.  What a key does is told in include/opencorr_hip.h.  No HIP calls
// (tests/cpp/engine_tuning_check.cpp runs tuning_set on a CPU; tests/engine_tuning_model.py restates the rules independently).
#pragma once
#include <cstring>
#include <type_traits>

#include "../../../include/opencorr_hip.h"
#include "icgn2d_plan.h"

namespace ochip_host {

struct EngineTuning {
    // kernel selection; every choice but the three arith_* keys computes the same bits
    int icgn2d_variant = -1;  // -1 = automatic (icgn2d_plan.h; MI355X sweeps)
    int icgn2d_xcd = 1;
    int icgn2d_tile_px = 128;  // (64 until round 3; 128 suits the lockstep sweeps: 3.29 vs 3.34 ms)
    int icgn2d_setup_cache = 1;
    int icgn2d_int_first = 1;
    int icgn2d_split_chunks = 0;
    // 0 = every multiply and add of the solver rounds on its own (oracle OC_ORDER_LANES; the reference built for baseline x86-64),
    // 1 = the per-sample multiply-adds are fused (oc_device.h OC_FMA; oracle OC_ORDER_LANES_FMA): by rounding, inside north_star's
    // tolerance
    int arith_fma = 0;
    int arith_onepass = 0;    // the one-pass arithmetic contract of ICGN2D1 / ICGN2D2, icgn2d_onepass.hip
    int arith_onepass3d = 0;  // ... of ICGN3D1, icgn3d_onepass.hip
    int fftcc2d_fused = 1;
    int fftcc3d_fused = 1;
    int fftcc3d_planes_blocks = 0;
    int fftcc3d_tile_vox = 64;
    int icgn3d_tile_vox = 64;  // (config E: 78.8 -> 75.5 ms, profiles/r4g_icgn3d1_ab_block_schedule.txt)
    int icgn3d_mapping = 0;    // 1 = one half-wave per subvolume row (icgn3d_rows.hip; OC_ORDER_ROWS): 12 - 25 % SLOWER
    int mt_splits = 0;         // "match_splits"
    int single_combine = 1;
    int host_chunk = 65536;
    int group_allgather = 0;
    int group_force_rccl = 0;
    bool self_adaptive = false;                                // DIC::setSelfAdaptive
    float lm_lambda = 100.f, lm_alpha = 0.1f, lm_beta = 10.f;  // DampingParameter defaults, src/oc_iclm.h:33-38
};
static_assert(std::is_trivially_copyable<EngineTuning>::value, "a group member takes its leader's settings by one assignment");

constexpr int kTuningMatchMaxSplits = 64;  // == ochip::kMatchMaxSplits (oc_kernels.h; asserted in capi.hip)

enum class TuningRule {
    Bool,           // value != 0
    Range,          // lo <= value <= hi
    ZeroOrAtLeast,  // 0, or >= lo
    Fused2d,        // 2 ... 5 kept, anything else value != 0
    Fused3d,        // 2 kept (A/B build only), anything else value != 0
    Variant         // -1 ... kIcgn2dVariantCount - 1; from 0 on the build must contain the launch shape (icgn2d_variant_built)
};
enum class TuningAbOnly { Nothing, NonZero, Two };  // the values only the A/B build accepts
enum class TuningRefusal { None, UnknownKey, WrongKind, OnePassOf3d, AbOnly, OutOfRange };

constexpr unsigned tuning_kind(int kind) { return kind < 1 || kind > 31 ? 0u : 1u << kind; }
constexpr unsigned kEveryKind = ~0u;
constexpr unsigned kIcgn2dKinds = tuning_kind(OC_HIP_ICGN2D1) | tuning_kind(OC_HIP_ICGN2D2) | tuning_kind(OC_HIP_ICLM2D1) | tuning_kind(OC_HIP_ICLM2D2);

struct TuningKey {
    const char* name;
    int EngineTuning::*field;
    TuningRule rule;
    int lo, hi;
    const char* range_words;              // what the refusal OutOfRange says ...
    const char* refused_words = nullptr;  // ... and what WrongKind / AbOnly say: printf formats that are handed `value`
    unsigned kinds = kEveryKind;          // engine kinds that may set a non-zero value; every kind may set 0 ...
    bool owners_only = false;             // ... unless this says that the other kinds are refused whatever the value
    TuningAbOnly ab_only = TuningAbOnly::Nothing;  // checked after the kind and before the range (Variant: after the range)
};

#define OC_AB_WORDS " that only the A/B build of the library contains (python -m opencorr_amd.build --ab)"
inline constexpr TuningKey kTuningKeys[] = {
    {"icgn2d_variant", &EngineTuning::icgn2d_variant, TuningRule::Variant, -1, kIcgn2dVariantCount - 1, "icgn2d_variant %d out of range [-1 (automatic), 12)",
     "icgn2d_variant %d is an A/B partner" OC_AB_WORDS},
    {"icgn2d_xcd", &EngineTuning::icgn2d_xcd, TuningRule::Bool, 0, 1, nullptr},
    {"icgn2d_tile_px", &EngineTuning::icgn2d_tile_px, TuningRule::ZeroOrAtLeast, 16, 0, "icgn2d_tile_px must be 0 (off) or >= 16"},
    {"icgn2d_setup_cache", &EngineTuning::icgn2d_setup_cache, TuningRule::Bool, 0, 1, nullptr},
    {"icgn2d_int_first", &EngineTuning::icgn2d_int_first, TuningRule::Bool, 0, 1, nullptr},
    // (the split launch shape, variant 8, exists in the A/B build only: the key would have no effect in the product build)
    {"icgn2d_split_chunks", &EngineTuning::icgn2d_split_chunks, TuningRule::Range, 0, 256, "icgn2d_split_chunks must be 0 (back to back) ... 256",
     "icgn2d_split_chunks belongs to icgn2d_variant 8, an A/B partner" OC_AB_WORDS, kEveryKind, false, TuningAbOnly::NonZero},
    {"arith_fma", &EngineTuning::arith_fma, TuningRule::Bool, 0, 1, nullptr,
     "arith_fma: only the ICGN2D1 / ICGN2D2 / ICLM2D1 / ICLM2D2 / ICGN3D1 engines, the descriptor matcher and the SIFT3D scale space have a fused-arithmetic build",
     kIcgn2dKinds | tuning_kind(OC_HIP_ICGN3D1) | tuning_kind(OC_HIP_MATCHER) | tuning_kind(OC_HIP_SIFT3D)},
    // (ICGN3D1 is refused in words of its own, OnePassOf3d: kTuningOnePassOf3dWords)
    {"arith_onepass", &EngineTuning::arith_onepass, TuningRule::Bool, 0, 1, nullptr, "arith_onepass: only the ICGN2D1 / ICGN2D2 engines have a one-pass build",
     tuning_kind(OC_HIP_ICGN2D1) | tuning_kind(OC_HIP_ICGN2D2)},
    {"arith_onepass3d", &EngineTuning::arith_onepass3d, TuningRule::Bool, 0, 1, nullptr,
     "arith_onepass3d: only the ICGN3D1 engine has this one-pass build (ICGN2D1 / ICGN2D2: arith_onepass)", tuning_kind(OC_HIP_ICGN3D1)},
    {"fftcc2d_fused", &EngineTuning::fftcc2d_fused, TuningRule::Fused2d, 0, 5, nullptr},
    {"fftcc3d_fused", &EngineTuning::fftcc3d_fused, TuningRule::Fused3d, 0, 2, nullptr, "fftcc3d_fused = 2 (the 32^3 kernel of rounds 1 - 5) is an A/B partner" OC_AB_WORDS,
     kEveryKind, false, TuningAbOnly::Two},
    {"fftcc3d_planes_blocks", &EngineTuning::fftcc3d_planes_blocks, TuningRule::Range, 0, 4096, "fftcc3d_planes_blocks must be 0 (default) ... 4096"},
    {"fftcc3d_tile_vox", &EngineTuning::fftcc3d_tile_vox, TuningRule::ZeroOrAtLeast, 8, 0, "fftcc3d_tile_vox must be 0 (off) or >= 8"},
    {"icgn3d_tile_vox", &EngineTuning::icgn3d_tile_vox, TuningRule::ZeroOrAtLeast, 8, 0, "icgn3d_tile_vox must be 0 (off) or >= 8"},
    {"icgn3d_mapping", &EngineTuning::icgn3d_mapping, TuningRule::Bool, 0, 1, nullptr,
     "icgn3d_mapping = 1 (the row mapping, measured 12 - 25 %% slower) is an A/B partner" OC_AB_WORDS, kEveryKind, false, TuningAbOnly::NonZero},
    // parts the candidate range of the descriptor matcher's distance kernel is cut into
    {"match_splits", &EngineTuning::mt_splits, TuningRule::Range, 0, kTuningMatchMaxSplits, "match_splits must be 0 (automatic) ... 64",
     "match_splits: the key of the descriptor matcher", tuning_kind(OC_HIP_MATCHER), true},
    {"single_combine", &EngineTuning::single_combine, TuningRule::Bool, 0, 1, nullptr},
    {"host_chunk", &EngineTuning::host_chunk, TuningRule::ZeroOrAtLeast, 16384, 0, "host_chunk must be 0 (off) or >= 16384 POIs"},
    {"group_allgather", &EngineTuning::group_allgather, TuningRule::Bool, 0, 1, nullptr},
    {"group_force_rccl", &EngineTuning::group_force_rccl, TuningRule::Bool, 0, 1, nullptr},
};
#undef OC_AB_WORDS
static_assert(kIcgn2dVariantCount == 12 && kTuningMatchMaxSplits == 64, "the words of icgn2d_variant and match_splits name these bounds");
constexpr bool tuning_refusals_have_words() {
    for (const TuningKey& k : kTuningKeys) {
        const bool range = k.rule == TuningRule::Range || k.rule == TuningRule::ZeroOrAtLeast || k.rule == TuningRule::Variant;
        const bool refused = k.kinds != kEveryKind || k.ab_only != TuningAbOnly::Nothing || k.rule == TuningRule::Variant;
        if ((range && !k.range_words) || (refused && !k.refused_words)) return false;
    }
    return true;
}
static_assert(tuning_refusals_have_words(), "every refusal a row can give has its words");
inline constexpr const char* kTuningOnePassOf3dWords =
    "arith_onepass: the key of the ICGN2D1 / ICGN2D2 engines; the one-pass build of ICGN3D1 has a key of its own, arith_onepass3d";

struct TuningResult {
    int status = OC_HIP_OK;
    TuningRefusal refusal = TuningRefusal::None;
    const TuningKey* key = nullptr;  // the row (null: UnknownKey)
    const char* words() const {      // of a refusal that has a row
        return refusal == TuningRefusal::OnePassOf3d ? kTuningOnePassOf3dWords : refusal == TuningRefusal::OutOfRange ? key->range_words : key->refused_words;
    }
};

inline const TuningKey* tuning_key(const char* name) {
    if (std::strcmp(name, "xcd") == 0) name = "icgn2d_xcd";
    for (const TuningKey& k : kTuningKeys)
        if (std::strcmp(name, k.name) == 0) return &k;
    return nullptr;
}

// One key of oc_hip_set_tuning on an engine of `kind`: the status, which refusal it was, and the row.  A refusal leaves `t` as it was.
inline TuningResult tuning_set(EngineTuning& t, int kind, const char* key, int value, bool ab_build) {
    const TuningKey* k = tuning_key(key);
    if (!k) return {OC_HIP_ERR_INVALID, TuningRefusal::UnknownKey, nullptr};
    const bool owner = (k->kinds & tuning_kind(kind)) != 0;
    if (!owner && (value != 0 || k->owners_only))
        return {OC_HIP_ERR_UNSUPPORTED, kind == OC_HIP_ICGN3D1 && k->field == &EngineTuning::arith_onepass ? TuningRefusal::OnePassOf3d : TuningRefusal::WrongKind, k};
    if (!ab_build && ((k->ab_only == TuningAbOnly::NonZero && value != 0) || (k->ab_only == TuningAbOnly::Two && value == 2)))
        return {OC_HIP_ERR_UNSUPPORTED, TuningRefusal::AbOnly, k};
    int stored = value;
    switch (k->rule) {
    case TuningRule::Bool: stored = value != 0; break;
    case TuningRule::Fused2d: stored = value >= 2 && value <= 5 ? value : value != 0; break;
    case TuningRule::Fused3d: stored = value == 2 ? 2 : value != 0; break;
    case TuningRule::ZeroOrAtLeast:
        if (value < 0 || (value > 0 && value < k->lo)) return {OC_HIP_ERR_INVALID, TuningRefusal::OutOfRange, k};
        break;
    case TuningRule::Range:
    case TuningRule::Variant:
        if (value < k->lo || value > k->hi) return {OC_HIP_ERR_INVALID, TuningRefusal::OutOfRange, k};
        if (k->rule == TuningRule::Variant && value >= 0 && !icgn2d_variant_built(value, ab_build)) return {OC_HIP_ERR_UNSUPPORTED, TuningRefusal::AbOnly, k};
        break;
    }
    t.*(k->field) = stored;
    return {OC_HIP_OK, TuningRefusal::None, k};
}

}  // namespace ochip_host

// icgn2d_plan.h -- what run_icgn2d (capi.hip) decides before it enqueues anything, without the engine: the table of ICGN2D launch
// shapes ("icgn2d_variant"), the dynamic LDS a workgroup of a shape asks for, and the rules that map a call to the variant, the
// launch path and the use of the set-up cache -- or to a refusal.  Standard headers only (tests/cpp/icgn2d_plan_check.cpp runs
// the rules on a CPU; tests/icgn2d_plan_model.py restates them independently).
#pragma once
#include <cstddef>

// gathers in flight and register budget (waves per SIMD) of variant 5 (experiments: tools/ab_build.py; A/B build only)
#ifndef OC_V5_G
#define OC_V5_G 2
#endif
#ifndef OC_V5_OCC
#define OC_V5_OCC 6
#endif
// The launch shapes, once (what each id is for: the comment above launch_dof in icgn2d.hip, which instantiates a kernel per row
// of the first list and, in the A/B build of the library, of the second).
//        id  G mode pipe wpb occ
#define OC_ICGN2D_VARIANTS_PRODUCT(X) \
    X(1, 3, 1, 0, 1, 4)       \
    X(2, 3, 1, 0, 4, 4)       \
    X(3, 4, 1, 0, 1, 3)       \
    X(4, 3, 4, 0, 8, 4)       \
    X(5, OC_V5_G, 4, 0, 8, OC_V5_OCC) \
    X(7, 3, 2, 0, 4, 4)       \
    X(10, 2, 6, 0, 4, 6)      \
    X(11, 3, 6, 0, 4, 4)
#define OC_ICGN2D_VARIANTS_AB(X) \
    X(0, 3, 0, 0, 1, 1)       \
    X(6, 2, 4, 0, 4, 4)
// A/B partners with launch code of their own: 8 = the split launch shape (set-up kernel + iteration kernel; the row is the
// iteration kernel's shape at 6 DoF), 9 = icgn2d_band.hip (table + LDS band, subset in registers)
#define OC_ICGN2D_VARIANTS_OWN_LAUNCH(X) \
    X(8, OC_V5_G, 4, 0, 8, OC_V5_OCC) \
    X(9, 1, 5, 0, 8, 6)

namespace ochip_host {

constexpr int kIcgn2dWave = 64;
constexpr int kIcgn2dLdsBudget = 160 * 1024 - 2048;  // dynamic LDS; 2 KB stay free for the static area of the cooperative inverse
constexpr int kIcgn2dVariantCount = 12;              // ids 0 ... 11
constexpr size_t kIcgn2dBigQueue = 32768;            // fills the chip often enough for the 8-wave / lockstep shapes
constexpr size_t kIcgn2dMaxGrid = 1u << 30;          // one wave per POI; grid.x is limited to 2^31-1: longer queues take several launches
constexpr size_t kIcgn2dSplitMinPois = 16384;        // the split shape's two-stream pipeline: launches from this many POIs on

struct Icgn2dShape {
    int id, g, mode, pipe, wpb, occ;
    bool ab_only;  // a measured loser that only the A/B build of the library (-DOC_BUILD_AB=1) contains
};
inline constexpr Icgn2dShape kIcgn2dShapes[] = {
#define X(ID, GG, MM, PP, WW, OO) {ID, GG, MM, PP, WW, OO, false},
    OC_ICGN2D_VARIANTS_PRODUCT(X)
#undef X
#define X(ID, GG, MM, PP, WW, OO) {ID, GG, MM, PP, WW, OO, true},
    OC_ICGN2D_VARIANTS_AB(X) OC_ICGN2D_VARIANTS_OWN_LAUNCH(X)
#undef X
};
// the launch shape of a variant id, whether a build contains it or not; id = -1: no such variant
constexpr Icgn2dShape icgn2d_shape(int variant) {
    for (const Icgn2dShape& s : kIcgn2dShapes)
        if (s.id == variant) return s;
    return {-1, 0, 0, 0, 0, 0, false};
}
static_assert(icgn2d_shape(kIcgn2dVariantCount - 1).id >= 0 && icgn2d_shape(kIcgn2dVariantCount).id < 0, "ids end at kIcgn2dVariantCount");
constexpr bool icgn2d_variant_built(int variant, bool ab_build) { return icgn2d_shape(variant).id >= 0 && (ab_build || !icgn2d_shape(variant).ab_only); }
// variants with a per-workgroup coordinate table (mode >= 3) need one subset radius per launch
constexpr bool icgn2d_variant_uses_table(int variant) { return icgn2d_shape(variant).mode >= 3; }

// Dynamic LDS of one workgroup: `wpb` waves with their [pass][lane] float arrays -- four in mode 0, one in modes 2, 4 and 6 (the
// target subset only), two otherwise; none in the set-up kernel of the split shape (phase 1) -- plus the workgroup's coordinate
// table: 12 bytes per sample slot from mode 3 up, 6 in mode 6 (the compact table).  nt = passes of 64 samples.
constexpr size_t icgn2d_lds_bytes(int mode, int wpb, size_t nt, int phase) {
    const size_t arrays = phase == 1 ? 0 : mode == 0 ? 4 : (mode == 4 || mode == 6 || mode == 2) ? 1 : 2;
    return (arrays * wpb * sizeof(float) + (mode == 6 ? 6 : mode >= 3 ? 12 : 0)) * nt * kIcgn2dWave;
}
// the one-pass kernel (icgn2d_onepass.hip) keeps nothing but a table of three floats per sample slot
constexpr size_t icgn2d_onepass_lds_bytes(size_t nt) { return 3 * sizeof(float) * nt * kIcgn2dWave; }
constexpr int icgn2d_onepass_max_samples() { return (int)(kIcgn2dLdsBudget / icgn2d_onepass_lds_bytes(1)) * kIcgn2dWave; }
constexpr long long icgn2d_samples(int rx, int ry) { return (2LL * rx + 1) * (2LL * ry + 1); }
constexpr size_t icgn2d_passes(int rx, int ry) { return (size_t)((icgn2d_samples(rx, ry) + kIcgn2dWave - 1) / kIcgn2dWave); }
// largest (2rx+1)*(2ry+1) a variant accepts: whole passes that one workgroup holds (0 for variant 9: the band kernel has its
// own rule, icgn2d_band_supported)
constexpr int icgn2d_max_samples(int variant) {
    const Icgn2dShape s = icgn2d_shape(variant);
    return s.id < 0 || variant == 9 ? 0 : (int)(kIcgn2dLdsBudget / icgn2d_lds_bytes(s.mode, s.wpb, 1, 0)) * kIcgn2dWave;
}
// `per_cu` workgroups of a variant's shape, each holding subsets of nt passes, fit a CU's LDS
constexpr bool icgn2d_fit_cu(int variant, int per_cu, size_t nt) {
    return per_cu * icgn2d_lds_bytes(icgn2d_shape(variant).mode, icgn2d_shape(variant).wpb, nt, 0) <= (size_t)kIcgn2dLdsBudget;
}
// Workgroups a CU holds by registers, which the big-queue shapes want all inside its LDS as well: three 8-wave workgroups of
// variant 5 (6 waves per SIMD), two of variant 4, six / four 4-wave ones of variants 10 / 11 -- subsets up to 19 passes (35 x 34)
// for ICGN2D1, 28 (41 x 41) for ICGN2D2
constexpr int icgn2d_per_cu(int variant) { return variant == 5 ? 3 : variant == 4 ? 2 : variant == 10 ? 6 : 4; }
static_assert(icgn2d_fit_cu(5, 3, 19) && !icgn2d_fit_cu(5, 3, 20) && icgn2d_fit_cu(10, 6, 19) && !icgn2d_fit_cu(10, 6, 20), "ICGN2D1: 19 passes");
static_assert(icgn2d_fit_cu(4, 2, 28) && !icgn2d_fit_cu(4, 2, 29) && icgn2d_fit_cu(11, 4, 28) && !icgn2d_fit_cu(11, 4, 29), "ICGN2D2: 28 passes");
// Variants 10 / 11 (4-wave workgroups on the compact coordinate table): whether a launch with ONE radius pair can run them -- at
// most 256 columns and 256 rows (the table keeps them as bytes) and all their workgroups of a CU inside its LDS.  Self-adaptive
// radii and IC-LM are the caller's to exclude.  A queue named through the tuning key runs them at any length.
constexpr bool icgn2d_compact_fits(int variant, int rx, int ry) {
    return (variant == 10 || variant == 11) && rx >= 0 && ry >= 0 && 2 * rx + 1 <= 256 && 2 * ry + 1 <= 256 &&
           icgn2d_fit_cu(variant, icgn2d_per_cu(variant), icgn2d_passes(rx, ry));
}

// ---- the decision ----------------------------------------------------------------------------------------------------------
struct Icgn2dRequest {
    int dof = 6;                                       // 6: ICGN2D1 / ICLM2D1, 12: ICGN2D2 / ICLM2D2
    bool lm = false, onepass = false;                  // an IC-LM engine; "arith_onepass" (honoured by the ICGN engines only)
    bool self_adaptive = false, has_offsets = false;   // per-POI radii (rx, ry: the largest of the batch); centre offsets
    int variant = -1, rx = 0, ry = 0;                  // "icgn2d_variant" (-1 = automatic); the radii the on-chip arrays are sized for
    size_t count = 0;                                  // POIs
    bool setup_cache = true;                           // "icgn2d_setup_cache"
    int split_chunks = 0;                              // "icgn2d_split_chunks"
    bool ab_build = false, band_supported = false;     // the A/B build; there: icgn2d_band.hip has an instantiation for (dof, rx, ry)
};
enum class Icgn2dPath { Plain, OnePass, Lm, Band, SplitPipelined };
enum class Icgn2dRefusal { None, OnePassOffsets, OnePassSelfAdaptive, OnePassTooLarge, TooLarge };
struct Icgn2dPlan {
    Icgn2dRefusal refusal = Icgn2dRefusal::None;
    int limit = 0;                        // OnePassTooLarge, TooLarge: the largest sample count that would have run
    int variant = 0;                      // the launch shape (OnePass, Lm and Band have one each: it does not reach their launchers)
    Icgn2dPath path = Icgn2dPath::Plain;  // SplitPipelined: every launch of at least kIcgn2dSplitMinPois POIs; a shorter last one is Plain
    bool uses_setup_cache = false;        // the launch keeps { reference mean, norm, H^-1 } per POI from call to call
    bool needs_setup_records = false;     // the split shape's per-call records (set-up kernel -> iteration kernel)
};

// What is refused whatever the radii are (run_icgn2d asks before the self-adaptive radius query touches the device): the one-pass
// contract runs one radius per launch on integer local coordinates, and is never replaced by another contract.
constexpr Icgn2dRefusal icgn2d_refused_before_radii(const Icgn2dRequest& q) {
    if (!q.onepass || q.lm) return Icgn2dRefusal::None;
    return q.has_offsets ? Icgn2dRefusal::OnePassOffsets : q.self_adaptive ? Icgn2dRefusal::OnePassSelfAdaptive : Icgn2dRefusal::None;
}
// Per-POI radii: no shared coordinate table, and the per-wave arrays are sized for the LARGEST subset of the batch.  The
// target-array-only shape (variant 7) keeps four workgroups on a CU where variant 2 holds two (bench.py paths_8f_row1): it takes
// over when three workgroups of variant 2 no longer fit a CU (subsets from 27 passes = 41 x 41 up; the measured case, radii 12 ...
// 20: 4.91 -> 3.98 ms); smaller batches keep the table-less default, which is 4 % ahead at equal occupancy (3.49 vs 3.61 ms on
// a uniform r = 16: one image read per sample fewer).
constexpr int icgn2d_per_poi_radius_variant(const Icgn2dRequest& q) {
    return !icgn2d_fit_cu(2, 3, icgn2d_passes(q.rx, q.ry)) ? 7 : q.dof == 12 ? 3 : 2;
}
// The automatic choice (MI355X sweeps).  Big queues of subsets whose workgroups all fit a CU: the lockstep sweeps
// on a coordinate table -- in 4-wave workgroups on the compact table where that applies (interleaved,
// profiles/r11a_icgn2d_4wave_compact_table_ab.json: config B 2.49 against 2.59 ms and config C 2.30 against 2.42 ms per launch
// served by the set-up cache, 2.86 / 2.91 and 3.25 / 3.41 without it), else in the 8-wave workgroups of variant 5 (ICGN2D1) / 4
// (ICGN2D2: 3.65 against 3.81 ms for variant 3 on config C, profiles/r03q_icgn2d2_variant_ab_configC.json).  Everything else: the
// LDS-light table-less shapes, variant 2 / 3 (config A, 10 000 POIs: 0.33 ms in variant 2's 4-wave workgroups against 0.38).
constexpr bool kIcgn2dCompactDefault[2] = {true, true};  // [0] ICGN2D1: 10 for 5, [1] ICGN2D2: 11 for 4
constexpr int icgn2d_automatic_variant(const Icgn2dRequest& q) {
    if (q.self_adaptive) return icgn2d_per_poi_radius_variant(q);
    const int table = q.dof == 12 ? 4 : 5, compact = q.dof == 12 ? 11 : 10;
    if (q.count < kIcgn2dBigQueue || !icgn2d_fit_cu(table, icgn2d_per_cu(table), icgn2d_passes(q.rx, q.ry))) return q.dof == 12 ? 3 : 2;
    return kIcgn2dCompactDefault[q.dof == 12] && icgn2d_compact_fits(compact, q.rx, q.ry) ? compact : table;
}
// The shape a launch of the ordinary ICGN kernel (not one-pass, not IC-LM) starts from: the named variant where it can serve
// this call, otherwise what replaces it -- silently and with the same bits.
constexpr int icgn2d_named_or_automatic_variant(const Icgn2dRequest& q) {
    const int named = q.variant;
    if (named < 0) return icgn2d_automatic_variant(q);
    // 10 / 11 need one radius per launch and every workgroup of a CU inside its LDS
    if ((named == 10 || named == 11) && (q.self_adaptive || !icgn2d_compact_fits(named, q.rx, q.ry))) return icgn2d_automatic_variant(q);
    if (q.self_adaptive && icgn2d_variant_uses_table(named)) return icgn2d_per_poi_radius_variant(q);
    // 9 = icgn2d_band.hip (A/B build only, measured 1.7 x slower than variant 5): at most the passes it unrolls
    if (named == 9 && !(q.ab_build && q.band_supported)) return q.dof == 12 ? 3 : 2;
    return named;
}

inline Icgn2dPlan icgn2d_plan(const Icgn2dRequest& q) {
    if (icgn2d_refused_before_radii(q) != Icgn2dRefusal::None) return {icgn2d_refused_before_radii(q)};
    const long long N = icgn2d_samples(q.rx, q.ry);
    if (q.onepass && !q.lm) {
        // one launch shape, its own kernel, around the set-up cache (the variant is what the big-queue default would be)
        if (N > icgn2d_onepass_max_samples()) return {Icgn2dRefusal::OnePassTooLarge, icgn2d_onepass_max_samples()};
        return {Icgn2dRefusal::None, 0, q.dof == 6 ? 5 : 4, Icgn2dPath::OnePass};
    }
    // the IC-LM launch shape has the LDS footprint of variant 1
    int variant = q.lm ? 1 : icgn2d_named_or_automatic_variant(q);
    const bool band = variant == 9;
    // what the shape cannot hold falls back to the LDS-light single-wave variant, and what that cannot hold is refused
    if (!band && N > icgn2d_max_samples(variant)) {
        variant = 1;
        if (N > icgn2d_max_samples(1)) return {Icgn2dRefusal::TooLarge, icgn2d_max_samples(1)};
    }
    const Icgn2dPath path = q.lm ? Icgn2dPath::Lm : band ? Icgn2dPath::Band
                            : variant == 8 && q.split_chunks >= 2 && q.count >= kIcgn2dSplitMinPois ? Icgn2dPath::SplitPipelined : Icgn2dPath::Plain;
    // Set-up cache: the big-queue table variants, one launch, nothing per POI but its coordinates.  Centre offsets, self-adaptive
    // radii, IC-LM and the small-queue variants go around it.
    const bool cached = q.setup_cache && !q.lm && !q.has_offsets && !q.self_adaptive && q.count <= kIcgn2dMaxGrid &&
                        (variant == 4 || variant == 5 || variant == 10 || variant == 11);
    return {Icgn2dRefusal::None, 0, variant, path, cached, /* needs_setup_records */ variant == 8};
}

}  // namespace ochip_host

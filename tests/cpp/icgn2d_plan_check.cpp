// icgn2d_plan_check.cpp -- runs opencorr_amd/csrc/host/icgn2d_plan.h on a CPU (tests/test_icgn2d_plan_cpu.py).
//
// stdin, one request per line:  dof lm onepass self_adaptive offsets variant rx ry count setup_cache split_chunks ab_build band_supported
// stdout, one plan per line:    run <variant> <path> <uses_setup_cache> <needs_setup_records>   |   refuse <which> <limit>
// With the argument "limits": one line per variant id, "<id> <built in product> <built in A/B> <uses table> <max samples>", then the
// one-pass limit.
#include <cstdio>
#include <cstring>

#include "../../opencorr_amd/csrc/host/icgn2d_plan.h"

using namespace ochip_host;

static const char* path_name(Icgn2dPath p) {
    switch (p) {
        case Icgn2dPath::Plain: return "plain";
        case Icgn2dPath::OnePass: return "onepass";
        case Icgn2dPath::Lm: return "lm";
        case Icgn2dPath::Band: return "band";
        case Icgn2dPath::SplitPipelined: return "split_pipelined";
    }
    return "?";
}

static const char* refusal_name(Icgn2dRefusal r) {
    switch (r) {
        case Icgn2dRefusal::None: return "none";
        case Icgn2dRefusal::OnePassOffsets: return "onepass_offsets";
        case Icgn2dRefusal::OnePassSelfAdaptive: return "onepass_self_adaptive";
        case Icgn2dRefusal::OnePassTooLarge: return "onepass_too_large";
        case Icgn2dRefusal::TooLarge: return "too_large";
    }
    return "?";
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "limits")) {
        for (int v = 0; v < kIcgn2dVariantCount; v++)
            std::printf("%d %d %d %d %d\n", v, (int)icgn2d_variant_built(v, false), (int)icgn2d_variant_built(v, true),
                        (int)icgn2d_variant_uses_table(v), icgn2d_max_samples(v));
        std::printf("onepass %d\n", icgn2d_onepass_max_samples());
        return 0;
    }
    int dof, lm, onepass, sa, offsets, variant, rx, ry, cache, split, ab, band;
    unsigned long long count;
    int got;
    while ((got = std::scanf("%d %d %d %d %d %d %d %d %llu %d %d %d %d", &dof, &lm, &onepass, &sa, &offsets, &variant, &rx, &ry, &count, &cache,
                             &split, &ab, &band)) == 13) {
        Icgn2dRequest q;
        q.dof = dof;
        q.lm = lm != 0;
        q.onepass = onepass != 0;
        q.self_adaptive = sa != 0;
        q.has_offsets = offsets != 0;
        q.variant = variant;
        q.rx = rx;
        q.ry = ry;
        q.count = (size_t)count;
        q.setup_cache = cache != 0;
        q.split_chunks = split;
        q.ab_build = ab != 0;
        q.band_supported = band != 0;
        const Icgn2dPlan plan = icgn2d_plan(q);
        if (plan.refusal != Icgn2dRefusal::None)
            std::printf("refuse %s %d\n", refusal_name(plan.refusal), plan.limit);
        else
            std::printf("run %d %s %d %d\n", plan.variant, path_name(plan.path), (int)plan.uses_setup_cache, (int)plan.needs_setup_records);
    }
    if (got != EOF) {
        std::fprintf(stderr, "malformed request line (%d of 13 fields)\n", got);
        return 2;
    }
    return 0;
}

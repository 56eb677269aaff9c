// engine_tuning_check.cpp -- runs opencorr_amd/csrc/host/engine_tuning.h on a CPU (tests/test_engine_tuning_cpu.py).
//
// stdin, one request per line, the four fields separated by ONE blank each (the key may be empty):
//   kind key value ab_build  ->  <status> <refusal> <the whole EngineTuning after the call, which started from the defaults>
// With the argument "defaults": the EngineTuning of a new engine, in the same form.  With "keys": the keys of the table.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../opencorr_amd/csrc/host/engine_tuning.h"

using namespace ochip_host;

static const char* name(TuningRefusal r) {
    switch (r) {
        case TuningRefusal::None: return "none";
        case TuningRefusal::UnknownKey: return "unknown_key";
        case TuningRefusal::WrongKind: return "wrong_kind";
        case TuningRefusal::OnePassOf3d: return "onepass_of_3d";
        case TuningRefusal::AbOnly: return "ab_only";
        case TuningRefusal::OutOfRange: return "out_of_range";
    }
    return "?";
}

static void print(const EngineTuning& t) {
    std::printf("variant=%d xcd=%d tile_px=%d setup_cache=%d int_first=%d split_chunks=%d arith_fma=%d arith_onepass=%d arith_onepass3d=%d "
                "fftcc2d_fused=%d fftcc3d_fused=%d planes_blocks=%d fftcc3d_tile_vox=%d icgn3d_tile_vox=%d mapping=%d match_splits=%d "
                "single_combine=%d host_chunk=%d group_allgather=%d group_force_rccl=%d self_adaptive=%d lm=%g,%g,%g\n",
                t.icgn2d_variant, t.icgn2d_xcd, t.icgn2d_tile_px, t.icgn2d_setup_cache, t.icgn2d_int_first, t.icgn2d_split_chunks, t.arith_fma,
                t.arith_onepass, t.arith_onepass3d, t.fftcc2d_fused, t.fftcc3d_fused, t.fftcc3d_planes_blocks, t.fftcc3d_tile_vox, t.icgn3d_tile_vox,
                t.icgn3d_mapping, t.mt_splits, t.single_combine, t.host_chunk, t.group_allgather, t.group_force_rccl, (int)t.self_adaptive,
                (double)t.lm_lambda, (double)t.lm_alpha, (double)t.lm_beta);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "defaults")) {
        print(EngineTuning{});
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "keys")) {
        for (const TuningKey& k : kTuningKeys) std::printf("%s\n", k.name);
        return 0;
    }
    char line[256];
    while (std::fgets(line, sizeof(line), stdin)) {
        line[std::strcspn(line, "\n")] = 0;
        char* key = std::strchr(line, ' ');
        char* value = key ? std::strchr(key + 1, ' ') : nullptr;
        char* ab = value ? std::strchr(value + 1, ' ') : nullptr;
        if (!ab) {
            std::fprintf(stderr, "malformed request line '%s'\n", line);
            return 2;
        }
        *key++ = *value++ = *ab++ = 0;
        EngineTuning t;
        const TuningResult r = tuning_set(t, std::atoi(line), key, std::atoi(value), std::atoi(ab) != 0);
        // a refusal with a row has words, an accepted key and an unknown one have none to ask for
        if ((r.refusal != TuningRefusal::None && r.refusal != TuningRefusal::UnknownKey) && !(r.key && r.words())) {
            std::fprintf(stderr, "'%s': a refusal without words\n", key);
            return 3;
        }
        std::printf("%d %s ", r.status, name(r.refusal));
        print(t);
    }
    return 0;
}

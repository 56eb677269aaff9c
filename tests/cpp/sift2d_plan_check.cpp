// sift2d_plan_check.cpp -- prints what opencorr_amd/csrc/host/sift2d_plan.h decides for one request, on a CPU
// (tests/test_sift2d_plan_cpu.py compares it with the float64 model's plan).
//   argv: width height n_features n_octave_layers contrast_threshold edge_threshold sigma
//   ->    "status <code> <why>"; on success "octaves <n> layers <n> threshold <n>", then per Gaussian layer
//         "layer <i> dims <cols> <rows> octave <o> index <i> sigma <bits> source <i> blurred <0|1> radius <R>"
//         and per blurred layer "w <i> <bits> ..." (float32 bit patterns in hex); at the end "reflect <n> <i...>" for n = 1, 2, 8
//         over i = -30 ... 30, "nearest <src> <dst> <i...>" and "pow2 <bits of t> <bits of 2^t> ..."
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host/sift2d_plan.h"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s width height n_features n_octave_layers contrast_threshold edge_threshold sigma\n", argv[0]);
        return 2;
    }
    ochip_host::Sift2dSettings cfg;
    cfg.n_features = std::atoi(argv[3]);
    cfg.n_octave_layers = std::atoi(argv[4]);
    cfg.contrast_threshold = (float)std::atof(argv[5]);
    cfg.edge_threshold = (float)std::atof(argv[6]);
    cfg.sigma = (float)std::atof(argv[7]);
    const ochip_host::Sift2dPlan p = ochip_host::sift2d_plan(cfg, std::atoi(argv[1]), std::atoi(argv[2]));
    std::printf("status %d %s\n", p.status, p.why.c_str());
    if (p.status != OC_HIP_OK) return 0;
    std::printf("octaves %d layers %zu threshold %d\n", p.n_octave, p.gauss.size(), p.threshold);
    for (size_t i = 0; i < p.gauss.size(); i++) {
        const ochip_host::Sift2dLayer& g = p.gauss[i];
        std::printf("layer %zu dims %d %d octave %d index %d sigma %08x source %d blurred %d radius %d\n", i, g.cols, g.rows, g.octave, g.index, bits(g.sigma),
                    g.source, g.blurred ? 1 : 0, g.radius);
        if (!g.blurred) continue;
        std::printf("w %zu", i);
        for (float w : g.weight) std::printf(" %08x", bits(w));
        std::printf("\n");
    }
    for (int n : {1, 2, 8}) {
        std::printf("reflect %d", n);
        for (int i = -30; i <= 30; i++) std::printf(" %d", ochip_host::sift2d_reflect(i, n));
        std::printf("\n");
    }
    for (int src : {37, 74, 9}) {
        std::printf("nearest %d %d", src, src / 2);
        for (int i = 0; i < src / 2; i++) std::printf(" %d", ochip_host::sift2d_nearest(i, src, src / 2));
        std::printf("\n");
    }
    std::printf("pow2");
    for (int k = 0; k <= 4000; k++) {
        const float t = 0.05f + k * 0.002137f;
        std::printf(" %08x %08x", bits(t), bits(ochip_host::sift2d_pow2(t)));
    }
    std::printf("\n");
    return 0;
}

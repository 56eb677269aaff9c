// sift3d_plan_check.cpp -- prints what opencorr_amd/csrc/host/sift3d_plan.h decides for one request, on a CPU
// (tests/test_sift3d_plan_cpu.py compares it with the float64 model's plan and, bit for bit, with the twin's weights).
//   argv: dim_z dim_y dim_x n_octave_layers min_dimension sigma_source sigma_base unit_x unit_y unit_z
//   ->    "status <code> <why>"; on success "octaves <n> layers <n>", then per Gaussian layer
//         "layer <i> dims <x> <y> <z> units <bits x3> octave <m> scale <bits> sigma <bits> source <i> blurred <0|1> radius <x> <y> <z>"
//         and per axis of a blurred layer "w <i> <axis> <bits> ..." (float32 bit patterns in hex)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host/sift3d_plan.h"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: %s dim_z dim_y dim_x n_octave_layers min_dimension sigma_source sigma_base unit_x unit_y unit_z\n", argv[0]);
        return 2;
    }
    ochip_host::Sift3dSettings cfg;
    cfg.n_octave_layers = std::atoi(argv[4]);
    cfg.min_dimension = std::atoi(argv[5]);
    cfg.sigma_source = (float)std::atof(argv[6]);
    cfg.sigma_base = (float)std::atof(argv[7]);
    const ochip_host::Sift3dPlan p = ochip_host::sift3d_plan(cfg, std::atoi(argv[3]), std::atoi(argv[2]), std::atoi(argv[1]), (float)std::atof(argv[8]),
                                                             (float)std::atof(argv[9]), (float)std::atof(argv[10]));
    std::printf("status %d %s\n", p.status, p.why.c_str());
    if (p.status != OC_HIP_OK) return 0;
    std::printf("octaves %d layers %zu\n", p.n_octave, p.gauss.size());
    for (size_t i = 0; i < p.gauss.size(); i++) {
        const ochip_host::Sift3dLayer& g = p.gauss[i];
        std::printf("layer %zu dims %d %d %d units %08x %08x %08x octave %d scale %08x sigma %08x source %d blurred %d radius %d %d %d\n", i, g.dim[0],
                    g.dim[1], g.dim[2], bits(g.unit[0]), bits(g.unit[1]), bits(g.unit[2]), g.octave, bits(g.scale), bits(g.sigma), g.source,
                    g.blurred ? 1 : 0, g.radius[0], g.radius[1], g.radius[2]);
        if (!g.blurred) continue;
        for (int a = 0; a < 3; a++) {
            std::printf("w %zu %d", i, a);
            for (float w : g.weight[a]) std::printf(" %08x", bits(w));
            std::printf("\n");
        }
    }
    return 0;
}

// sift3d_feature_plan_check.cpp -- checks, on a CPU, what opencorr_amd/csrc/host/sift3d_feature_plan.h decides for one request
// (tests/test_sift3d_features_cpu.py drives it): every table entry against the reference's expression written inline with pow
// (src/oc_sift.cpp:902, :1129), bit for bit at every offset; the sentinel exactly where norm > radius; the grid exponent; the verdict.
//   argv: dim_z dim_y dim_x n_octave_layers unit_x unit_y unit_z max_abs
//   ->    "status <code> <why>"; on success "exponent <E>", then per table
//         "table <orient|describe> <layer> half <x> <y> <z> entries <n> outside <n> mismatches <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host/sift3d_plan.h"
#include "host/sift3d_feature_plan.h"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s dim_z dim_y dim_x n_octave_layers unit_x unit_y unit_z max_abs\n", argv[0]);
        return 2;
    }
    ochip_host::Sift3dSettings cfg;
    cfg.n_octave_layers = std::atoi(argv[4]);
    const ochip_host::Sift3dPlan ss = ochip_host::sift3d_plan(cfg, std::atoi(argv[3]), std::atoi(argv[2]), std::atoi(argv[1]), (float)std::atof(argv[5]),
                                                              (float)std::atof(argv[6]), (float)std::atof(argv[7]));
    if (ss.status != OC_HIP_OK) {
        std::fprintf(stderr, "the scale space refuses: %s\n", ss.why.c_str());
        return 3;
    }
    const ochip_host::Sift3dFeaturePlan p = ochip_host::sift3d_feature_plan(ss, (float)std::atof(argv[8]));
    std::printf("status %d %s\n", p.status, p.why.c_str());
    if (p.status != OC_HIP_OK) return 0;
    std::printf("exponent %d\n", p.exponent);
    for (size_t i = 0; i < ss.gauss.size(); i++)
        for (int stage = 0; stage < 2; stage++) {
            const ochip_host::Sift3dFeatureTable& t = stage == 0 ? p.orient[i] : p.describe[i];
            if (t.weight.empty()) continue;
            const ochip_host::Sift3dLayer& g = ss.gauss[i];
            long outside = 0, mismatches = 0;
            for (int az = 0; az <= t.half[2]; az++)
                for (int ay = 0; ay <= t.half[1]; ay++)
                    for (int ax = 0; ax <= t.half[0]; ax++) {
                        // the offsets -a and +a give the same entry: (d * unit)^2 has no sign
                        const float x = (float)ax * g.unit[0], y = (float)ay * g.unit[1], z = (float)az * g.unit[2];
                        const float xn = (float)-ax * g.unit[0], yn = (float)-ay * g.unit[1], zn = (float)-az * g.unit[2];
                        const float norm = sqrtf(x * x + y * y + z * z), norm_n = sqrtf(xn * xn + yn * yn + zn * zn);
                        float want;
                        if (norm > t.radius) {
                            want = ochip_host::kSiftFeatureOutside;
                            outside++;
                        } else if (stage == 0) {
                            want = expf(-0.5f * powf(norm / t.sigma, 2.f));
                        } else {
                            want = (float)exp(-0.5 * pow((double)(norm / t.sigma), 2));
                        }
                        if (bits(want) != bits(t.weight[t.at(ax, ay, az)]) || bits(norm) != bits(norm_n)) mismatches++;
                    }
            std::printf("table %s %zu half %d %d %d entries %zu outside %ld mismatches %ld\n", stage == 0 ? "orient" : "describe", i, t.half[0], t.half[1],
                        t.half[2], t.weight.size(), outside, mismatches);
        }
    return 0;
}

// sift3d_feature_plan.h -- the host scalars of SIFT3D's orientation and descriptor stages (capi_sift3d.hip, sift3d_features.hip;
// SIFT3D::assignOrientation and constructDescriptor, src/oc_sift.cpp:849-1049, 1051-1249): the Gaussian weight tables, the grid of
// the exact sums and the verdict on what is refused.  Nothing else computes these.  No HIP calls
// (tests/cpp/sift3d_feature_plan_check.cpp runs it on a CPU).  Built with -ffp-contract=off: every float operation rounds on its own.
//
// Weights.  Keypoint coordinates are integers (the reference refines nothing), so within a layer the weight of a voxel depends on
// (|dx|, |dy|, |dz|) alone: (dx * unit)^2 has no sign.  One table per Gaussian layer and stage, made with the host's expf / exp:
//   orientation (:895-902)   n = sqrtf(x x + y y + z z), q = n / sigma_w, w = expf(-0.5f * (q * q)), kept where n <= 3 sigma_w
//   descriptor (:1091-1129)  n likewise, q = (double)(n / sigma), w = (float)exp(-0.5 * (q * q)), kept where n <= 2 sigma
// with kSiftFeatureOutside (-1) where the sphere test fails.  pow(q, 2) of the reference is q * q: GCC and Clang both compile the
// call to the product (in float at :902, exact in double at :1129).
//
// Grid of the exact sums.  A = max |v| of the input volume, E = the smallest integer with 2^E >= 2 A / min(unit) (0 for A = 0).
// Every gradient component is then at most 2^(E-1) in magnitude.  A voxel term t becomes the integer llrintf(ldexpf(t, -q)) with
//   q = E - 40 for the three d sums, 2 E - 40 for the six tensor sums, E - 39 for descriptor bins
// (ldexpf is exact: no term is large enough to overflow, and one that falls below 2^-126 rounds to 0 either way), and the integers
// add up in 64 bits: at most 2^20 voxels of at most 2^42 each.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/opencorr_hip.h"

namespace ochip_host {

constexpr float kSiftFeatureOutside = -1.f;
constexpr int kSiftFeatureMaxHalfExtent = 80;          // table half-extent per axis (the defaults with units down to 0.5: 73)
constexpr long long kSiftFeatureMaxWindow = 1ll << 20;  // voxels of one window, clamped to the layer
constexpr int kSiftFeatureMaxExponent = 60;
constexpr int kSiftDescriptorLength = 768;

// beta, gamma, gradient_threshold, truncate_threshold of Sift3dConfig; defaults of SIFT3D::SIFT3D() (:147-152)
struct Sift3dFeatureSettings {
    float beta = 0.9f;
    float gamma = 0.4f;
    float gradient_threshold = 0.0000000001f;
    float truncate_threshold = 0.2f * 128 / 768;
};

// the window of one stage in one layer, relative to an integer keypoint coordinate, and its weights
struct Sift3dFeatureTable {
    float radius = 0.f;          // window_radius (:860) / sphere_radius (:1062)
    float sigma = 0.f;           // sigma_w (:859) / sigma (:1061)
    float cube_radius = 0.f;     // :1063, descriptor only
    int half[3] = {0, 0, 0};     // |offset| <= half[a] covers every voxel that can pass the sphere test
    std::vector<float> weight;   // [(half[2] + 1)][(half[1] + 1)][(half[0] + 1)]
    size_t at(int ax, int ay, int az) const { return ((size_t)az * (half[1] + 1) + ay) * (half[0] + 1) + ax; }
};

struct Sift3dFeaturePlan {
    int status = OC_HIP_OK;  // OC_HIP_ERR_INVALID / OC_HIP_ERR_UNSUPPORTED: `why` says what; nothing may be launched
    std::string why;
    int exponent = 0;        // E
    std::vector<Sift3dFeatureTable> orient, describe;  // one per Gaussian layer; empty `weight` for layers no keypoint can name
};

inline float sift3d_norm(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }  // Point3D::vectorNorm

inline float sift3d_orient_weight(float norm, float sigma_w) {
    const float q = norm / sigma_w;
    return expf(-0.5f * (q * q));
}

inline float sift3d_describe_weight(float norm, float sigma) {
    const double q = (double)(norm / sigma);
    return (float)exp(-0.5 * (q * q));
}

// E of the grid; false when A is not finite
inline bool sift3d_grid_exponent(float max_abs, float unit_min, int* exponent) {
    *exponent = 0;
    if (!std::isfinite(max_abs)) return false;
    if (max_abs == 0.f) return true;
    int e = 0;
    const double m = frexp(2.0 * (double)max_abs / (double)unit_min, &e);  // the quotient = m 2^e, 0.5 <= m < 1
    *exponent = m == 0.5 ? e - 1 : e;
    return true;
}

// the largest |offset| on one axis at which a voxel can pass the sphere test, one more for the rounding of the products: an
// offset beyond it has |offset * unit| > radius, and sqrtf(x x + y y + z z) >= |y| in IEEE arithmetic.  The loops of :863-876 /
// :1066-1079 reach that far and, on y in :870 (radius * unit_y), possibly further: what lies beyond the table lies outside the sphere.
inline int sift3d_feature_half_extent(float reach) {
    if (!(reach < 1e6f)) return 1 << 30;
    return (int)ceilf(reach) + 1;
}

inline void sift3d_fill_table(Sift3dFeatureTable& t, const float* unit, bool describe) {
    t.weight.assign((size_t)(t.half[0] + 1) * (t.half[1] + 1) * (t.half[2] + 1), kSiftFeatureOutside);
    for (int az = 0; az <= t.half[2]; az++)
        for (int ay = 0; ay <= t.half[1]; ay++)
            for (int ax = 0; ax <= t.half[0]; ax++) {
                const float n = sift3d_norm((float)ax * unit[0], (float)ay * unit[1], (float)az * unit[2]);
                if (n <= t.radius) t.weight[t.at(ax, ay, az)] = describe ? sift3d_describe_weight(n, t.sigma) : sift3d_orient_weight(n, t.sigma);
            }
}

// gauss: the layer table of sift3d_plan(); max_abs: A
inline Sift3dFeaturePlan sift3d_feature_plan(const Sift3dPlan& scale_space, float max_abs) {
    Sift3dFeaturePlan p;
    auto refuse = [&p](int status, const char* fmt, double a, double b) {
        char buf[256];
        std::snprintf(buf, sizeof buf, fmt, a, b);
        p.status = status;
        p.why = buf;
        p.orient.clear();
        p.describe.clear();
        return p;
    };
    if (scale_space.status != OC_HIP_OK || scale_space.gauss.empty()) return refuse(OC_HIP_ERR_INVALID, "sift3d: no layer table", 0, 0);
    const float* u0 = scale_space.gauss[0].unit;
    float unit_min = u0[0] < u0[1] ? u0[0] : u0[1];
    unit_min = unit_min < u0[2] ? unit_min : u0[2];
    if (!sift3d_grid_exponent(max_abs, unit_min, &p.exponent))
        return refuse(OC_HIP_ERR_INVALID, "sift3d: the volume holds non-finite voxels: no orientation, no descriptors", 0, 0);
    if (p.exponent > kSiftFeatureMaxExponent || p.exponent < -kSiftFeatureMaxExponent)
        return refuse(OC_HIP_ERR_UNSUPPORTED, "sift3d: grid exponent %g outside the supported +-%g (max |v| / min unit)", p.exponent, kSiftFeatureMaxExponent);
    const size_t n = scale_space.gauss.size();
    p.orient.resize(n);
    p.describe.resize(n);
    const float sqrt_2 = sqrtf(2.f);  // :1054
    for (size_t i = 0; i < n; i++) {
        const Sift3dLayer& g = scale_space.gauss[i];
        const int in_octave = (int)i % scale_space.gauss_per_octave();
        if (in_octave < 1 || in_octave > scale_space.n_octave_layers) continue;  // detectExtrema visits DoG layers 1 ... n_octave_layers (:797-802)
        Sift3dFeatureTable& o = p.orient[i];
        o.sigma = 1.5f * g.scale;   // :859
        o.radius = 3.f * o.sigma;   // :860
        Sift3dFeatureTable& d = p.describe[i];
        d.sigma = 5.f * sqrt_2 * g.scale;      // :1061
        d.radius = 2.f * d.sigma;              // :1062
        d.cube_radius = d.radius / sqrt_2;     // :1063
        for (int a = 0; a < 3; a++) {
            o.half[a] = sift3d_feature_half_extent(o.radius / g.unit[a]);
            d.half[a] = sift3d_feature_half_extent(d.radius / g.unit[a]);
        }
        for (const Sift3dFeatureTable* t : {&o, &d}) {
            for (int a = 0; a < 3; a++)
                if (t->half[a] > kSiftFeatureMaxHalfExtent)
                    return refuse(OC_HIP_ERR_UNSUPPORTED, "sift3d: a window of half-extent %g voxels exceeds the supported %g", t->half[a], kSiftFeatureMaxHalfExtent);
            long long window = 1;  // clamped to IMG_BORDER ... dim - IMG_BORDER (:864-876)
            for (int a = 0; a < 3; a++) {
                const long long inside = g.dim[a] > 2 ? g.dim[a] - 2 : 0, reach = 2ll * t->half[a] + 1;
                window *= inside < reach ? inside : reach;
            }
            if (window > kSiftFeatureMaxWindow)
                return refuse(OC_HIP_ERR_UNSUPPORTED, "sift3d: a window of %g voxels exceeds the supported %g", (double)window, (double)kSiftFeatureMaxWindow);
        }
        sift3d_fill_table(o, g.unit, false);
        sift3d_fill_table(d, g.unit, true);
    }
    return p;
}

}  // namespace ochip_host

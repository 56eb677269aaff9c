// sift3d_plan.h -- the host scalars of SIFT3D's scale space (capi_sift3d.hip, sift3d.hip): the layer table of
// SIFT3D::createGaussianPyramid (src/oc_sift.cpp:679-739: dims, units, octave, scale, sigma, the layer each one is made from),
// the three weight arrays of SIFT3D::gaussianBlur per blurred layer (:367-399, :438-454, :490-506) and the support verdict.
// Nothing else computes these.  No HIP calls (tests/cpp/sift3d_plan_check.cpp runs it on a CPU; tests/sift3d_model.py restates
// the table independently).  Built with -ffp-contract=off like the rest of the library: every float operation below rounds on its own.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/opencorr_hip.h"

namespace ochip_host {

constexpr int kSift3dMaxRadius = 32;       // every axis radius the blur kernels take (the defaults with unit ratios up to 4)
constexpr int kSift3dMaxOctaveLayers = 16;
constexpr long long kSift3dMaxVoxels = 0x7fffffffll;

// the members of the reference's Sift3dConfig (src/oc_sift.h:71-83) that the scale space reads; defaults of SIFT3D::SIFT3D() (:142-159)
struct Sift3dSettings {
    int n_octave_layers = 3;
    int min_dimension = 8;
    float alpha = 0.1f;
    float sigma_source = 1.15f;
    float sigma_base = 1.6f;
};

struct Sift3dLayer {
    int dim[3] = {0, 0, 0};          // { dim_x, dim_y, dim_z } like Layer3D::dim_xyz
    float unit[3] = {1.f, 1.f, 1.f};
    int octave = 0;
    float scale = 0.f;
    float sigma = 0.f;               // 0 for the bottom layer of octave m > 0 (the reference leaves it unset: that layer is not blurred)
    int source = -1;                 // Gaussian layer this one is made from; -1 = the input volume
    bool blurred = true;             // false: downsampled (dst[i][j][k] = src[2i][2j][2k], :549-562)
    int radius[3] = {0, 0, 0};       // per axis x, y, z
    std::vector<float> weight[3];    // radius + 1 entries each
    size_t voxels() const { return (size_t)dim[0] * dim[1] * dim[2]; }
};

struct Sift3dPlan {
    int status = OC_HIP_OK;          // OC_HIP_ERR_INVALID / OC_HIP_ERR_UNSUPPORTED: `why` says what; nothing may be launched
    std::string why;
    int n_octave = 0, n_octave_layers = 0;
    std::vector<Sift3dLayer> gauss;  // n_octave * (n_octave_layers + 3)
    int gauss_per_octave() const { return n_octave_layers + 3; }
    int dog_per_octave() const { return n_octave_layers + 2; }
    int dog_layers() const { return n_octave * dog_per_octave(); }
    // DoG layer d = g[n + 1] - g[n] (:766-785) carries dims, units, octave and scale of this Gaussian layer
    int dog_gauss(int d) const { return (d / dog_per_octave()) * gauss_per_octave() + d % dog_per_octave(); }
};

// kernel_radius of :372-381 and the sigma the weights are made with (0 when sigma is not > 0, a NaN included)
inline float sift3d_kernel_radius(float& sigma) {
    if (sigma > 0) {
        const float c = ceilf(3.f * sigma);
        return c > 1 ? c : 1.f;
    }
    sigma = 0.f;
    return 1.f;
}

// the weights of one axis (:386-399): w[0] = 1 / (1 + sum of 2 w[i], ascending), w[i] = expf(-0.5 x^2) * w[0]
inline std::vector<float> sift3d_weights(float sigma, int radius) {
    std::vector<float> w((size_t)radius + 1);
    w[0] = 1.f;
    for (int i = 1; i <= radius; i++) {
        const float x = i / (sigma + FLT_EPSILON);
        w[i] = expf(-0.5f * x * x);
        w[0] += (w[i] * 2.f);
    }
    w[0] = 1.f / w[0];
    for (int i = 1; i <= radius; i++) w[i] *= w[0];
    return w;
}

inline Sift3dPlan sift3d_refuse(int status, const char* fmt, double a = 0, double b = 0, double c = 0) {
    Sift3dPlan p;
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b, c);
    p.status = status;
    p.why = buf;
    return p;
}

inline Sift3dPlan sift3d_plan(const Sift3dSettings& cfg, int dim_x, int dim_y, int dim_z, float unit_x, float unit_y, float unit_z) {
    if (dim_x < 1 || dim_y < 1 || dim_z < 1) return sift3d_refuse(OC_HIP_ERR_INVALID, "sift3d: volume dimensions must be >= 1 (got %g x %g x %g)", dim_x, dim_y, dim_z);
    if (cfg.n_octave_layers < 1 || cfg.min_dimension < 1)
        return sift3d_refuse(OC_HIP_ERR_INVALID, "sift3d: n_octave_layers and min_dimension must be >= 1 (got %g, %g)", cfg.n_octave_layers, cfg.min_dimension);
    if (!(unit_x > 0) || !(unit_y > 0) || !(unit_z > 0) || !std::isfinite(unit_x) || !std::isfinite(unit_y) || !std::isfinite(unit_z))
        return sift3d_refuse(OC_HIP_ERR_INVALID, "sift3d: physical units must be positive and finite (got %g, %g, %g)", unit_x, unit_y, unit_z);
    if (cfg.n_octave_layers > kSift3dMaxOctaveLayers)
        return sift3d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift3d: at most %g layers per octave (got %g)", kSift3dMaxOctaveLayers, cfg.n_octave_layers);
    if ((long long)dim_x * dim_y * dim_z > kSift3dMaxVoxels) return sift3d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift3d: volumes of at most 2^31-1 voxels");

    Sift3dPlan p;
    p.n_octave_layers = cfg.n_octave_layers;
    int dim_min = dim_x < dim_y ? dim_x : dim_y;
    dim_min = dim_min < dim_z ? dim_min : dim_z;
    const int n_octave = (int)(floorf(log2f((float)dim_min) - log2f((float)cfg.min_dimension)) + 1);  // :683-684
    p.n_octave = n_octave > 0 ? n_octave : 1;
    const int per = p.gauss_per_octave(), layer_number = p.n_octave * per;
    p.gauss.resize((size_t)layer_number);
    const float kappa = powf(2.f, 1.f / cfg.n_octave_layers);  // :696

    int len[3] = {dim_x, dim_y, dim_z};
    float unit[3] = {unit_x, unit_y, unit_z};
    for (int i = 0; i < layer_number; i++) {
        Sift3dLayer& g = p.gauss[(size_t)i];
        g.octave = i / per;
        const int layer_in_octave = i % per;
        if (i == 0) {
            g.scale = 1.f / kappa * cfg.sigma_base;                                              // :705
            g.sigma = sqrtf(g.scale * g.scale - cfg.sigma_source * cfg.sigma_source);            // :706
        } else if (layer_in_octave == 0) {
            for (int a = 0; a < 3; a++) {
                len[a] /= 2;
                unit[a] *= 2;
            }
            g.source = (g.octave - 1) * per + cfg.n_octave_layers;                               // :723 and the `i - 3` of :747
            g.scale = p.gauss[(size_t)g.source].scale;
            g.blurred = false;
        } else {
            g.source = i - 1;
            g.scale = kappa * p.gauss[(size_t)i - 1].scale;                                      // :727
            g.sigma = sqrtf(kappa * kappa - 1.f) * p.gauss[(size_t)layer_in_octave - 1].scale;   // :728: the index is into octave 0
        }
        for (int a = 0; a < 3; a++) {
            g.dim[a] = len[a];
            g.unit[a] = unit[a];
        }
        if (len[0] < 1 || len[1] < 1 || len[2] < 1) return sift3d_refuse(OC_HIP_ERR_INVALID, "sift3d: an octave without voxels");
        if (!g.blurred) continue;
        float unit_max = unit[0] > unit[1] ? unit[0] : unit[1];  // :368-369
        unit_max = unit_max > unit[2] ? unit_max : unit[2];
        float sigma = g.sigma;
        const float kernel_radius = sift3d_kernel_radius(sigma);
        for (int a = 0; a < 3; a++) {
            const float r = kernel_radius * floorf(unit_max / unit[a] + 0.5f);  // :384
            if (!(r <= (float)kSift3dMaxRadius))
                return sift3d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift3d: blur radius %g on axis %g exceeds the supported %g", r, a, kSift3dMaxRadius);
            g.radius[a] = (int)r;
            g.weight[a] = sift3d_weights(sigma, g.radius[a]);
        }
    }
    return p;
}

// s[lo(c - r)] and s[hi(c + r)] of :1505-1517 as one index map (c - r never passes n - 1, c + r never falls below 0, so one
// function serves both sides), then clamped into [0, n - 1]: the reference's single reflection leaves the array when
// r > n - 1, where it is undefined; wherever it is defined the clamp changes nothing.
inline int sift3d_mirror(int i, int n) {
    if (i < 0) i = -i;
    else if (i > n - 1) i = 2 * (n - 1) - i;
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

}  // namespace ochip_host

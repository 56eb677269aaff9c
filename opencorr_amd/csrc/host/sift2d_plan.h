// sift2d_plan.h -- the host scalars of SIFT2D's detector (capi_sift2d.hip, sift2d.hip): cv::SIFT as the reference's
// SIFT2D::compute() creates it (src/oc_sift.cpp:22-30, 60-93), restated in DESIGN.md section 4.13.  The octave count, the
// dims of every layer, the sigmas, radii and weights of every blur, the extrema threshold and every refusal.  Nothing else computes
// these: the kernel launcher, tests/cpp/sift2d_twin.cpp and tests/cpp/sift2d_plan_check.cpp read them here (tests/sift2d_model.py
// restates them independently).  No HIP calls.  Built with -ffp-contract=off: every float operation below rounds on its own.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/opencorr_hip.h"

namespace ochip_host {

constexpr int kSift2dMaxRadius = 32;        // every radius the blur kernel takes
constexpr int kSift2dMaxOctaveLayers = 8;
constexpr long long kSift2dMaxPixels = 0x7fffffffll;  // of the doubled base image
constexpr int kSift2dBorder = 5;            // SIFT_IMG_BORDER
constexpr int kSift2dMaxSteps = 5;          // SIFT_MAX_INTERP_STEPS

// the members of the reference's Sift2dConfig (src/oc_sift.h:30-37); defaults of SIFT2D::SIFT2D() (src/oc_sift.cpp:22-30)
struct Sift2dSettings {
    int n_features = 0;
    int n_octave_layers = 3;
    float contrast_threshold = 0.04f;
    float edge_threshold = 10.f;
    float sigma = 1.6f;
};

struct Sift2dLayer {
    int cols = 0, rows = 0;
    int octave = 0;                  // 0 = the doubled base (cv::KeyPoint's octave -1)
    int index = 0;                   // layer within the octave
    float sigma = 0.f;               // of the blur that makes this layer; 0: resampled from `source`
    int source = -1;                 // Gaussian layer this one is made from; -1: the upscaled input
    bool blurred = true;
    int radius = 0;
    std::vector<float> weight;       // radius + 1 entries
    size_t pixels() const { return (size_t)cols * rows; }
};

struct Sift2dPlan {
    int status = OC_HIP_OK;          // OC_HIP_ERR_INVALID / OC_HIP_ERR_UNSUPPORTED: `why` says what; nothing may be launched
    std::string why;
    int n_octave = 0, n_octave_layers = 0;
    int base_cols = 0, base_rows = 0;
    int threshold = 0;               // fabsf(v) > threshold
    std::vector<Sift2dLayer> gauss;  // n_octave * (n_octave_layers + 3)
    int gauss_per_octave() const { return n_octave_layers + 3; }
    int dog_per_octave() const { return n_octave_layers + 2; }
    int dog_layers() const { return n_octave * dog_per_octave(); }
    // DoG layer d = g[i + 1] - g[i] has the dims and the octave of this Gaussian layer
    int dog_gauss(int d) const { return (d / dog_per_octave()) * gauss_per_octave() + d % dog_per_octave(); }
};

// cvRound: to nearest, halves to even (the default rounding mode)
inline int sift2d_round(double v) { return (int)std::nearbyint(v); }

// ksize = cvRound(sig * 8 + 1) | 1, R = ksize / 2; -1 for a sigma that is not finite or not > 0
inline int sift2d_radius(float sigma) {
    if (!(sigma > 0) || !std::isfinite(sigma)) return -1;
    const double k = (double)sigma * 8 + 1;
    if (k > 4.0 * kSift2dMaxRadius + 8) return kSift2dMaxRadius + 1;
    return (sift2d_round(k) | 1) / 2;
}

// exp(-x^2 / (2 sig^2)) in double, normalised to sum 1 in double (the taps summed in index order -R ... R), rounded to float32
inline std::vector<float> sift2d_weights(float sigma, int radius) {
    std::vector<double> t((size_t)radius + 1);
    const double s2 = 2.0 * (double)sigma * (double)sigma;
    for (int i = 0; i <= radius; i++) t[(size_t)i] = std::exp(-((double)i * i) / s2);
    double sum = 0;
    for (int i = -radius; i <= radius; i++) sum += t[(size_t)(i < 0 ? -i : i)];
    std::vector<float> w((size_t)radius + 1);
    for (int i = 0; i <= radius; i++) w[(size_t)i] = (float)(t[(size_t)i] / sum);
    return w;
}

// reflect-101 (-1 -> 1, n -> n - 2), repeated until the index is inside: period 2 (n - 1); n == 1: always 0
inline int sift2d_reflect(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// nearest-neighbour source index of the half-size resample
inline int sift2d_nearest(int x, int src, int dst) {
    const int s = (int)std::floor(x * ((double)src / dst));
    return s < src - 1 ? s : src - 1;
}

// 2^t for the keypoint size: host and device run these same double operations (no contraction), so the kernel and its CPU twin
// agree in every bit whatever either libm does.  n = nearest integer, z = (t - n) ln 2 in [-0.35, 0.35], exp(z) by its series to
// z^14 (remainder below 2e-17 relative), rounded to float32 once.  On the arguments tried (tests/test_sift2d_plan_cpu.py: 4 001
// values of t in [0.05, 8.6] against a float64 exp2) the result is the correctly rounded float32 of 2^t; nothing is claimed beyond
// that sample -- a double result within some 1e-16 of a float32 rounding boundary may round the other way.
#if defined(__HIPCC__)
#define OC_SIFT2D_HD __host__ __device__
#else
#define OC_SIFT2D_HD
#endif
OC_SIFT2D_HD inline float sift2d_pow2(float t) {
    const double td = (double)t;
    const double n = td < 0 ? (double)(long long)(td - 0.5) : (double)(long long)(td + 0.5);
    const double z = (td - n) * 0.6931471805599453;
    double e = 1.0;
    for (int k = 14; k >= 1; k--) e = 1.0 + e * z / (double)k;
    int m = (int)n;
    for (; m > 0; m--) e = e * 2.0;
    for (; m < 0; m++) e = e * 0.5;
    return (float)e;
}

inline Sift2dPlan sift2d_refuse(int status, const char* fmt, double a = 0, double b = 0) {
    Sift2dPlan p;
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b);
    p.status = status;
    p.why = buf;
    return p;
}

inline Sift2dPlan sift2d_plan(const Sift2dSettings& cfg, int width, int height) {
    if (width < 2 || height < 2) return sift2d_refuse(OC_HIP_ERR_INVALID, "sift2d: image sides must be >= 2 (got %g x %g)", width, height);
    if (cfg.n_octave_layers < 1 || cfg.n_octave_layers > kSift2dMaxOctaveLayers)
        return sift2d_refuse(OC_HIP_ERR_INVALID, "sift2d: n_octave_layers must be in [1, %g] (got %g)", kSift2dMaxOctaveLayers, cfg.n_octave_layers);
    if (!(cfg.sigma > 0) || !std::isfinite(cfg.sigma)) return sift2d_refuse(OC_HIP_ERR_INVALID, "sift2d: sigma must be finite and > 0 (got %g)", cfg.sigma);
    if (!std::isfinite(cfg.contrast_threshold) || !std::isfinite(cfg.edge_threshold))
        return sift2d_refuse(OC_HIP_ERR_INVALID, "sift2d: contrast_threshold and edge_threshold must be finite");
    if (cfg.n_features != 0)
        return sift2d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift2d: n_features = %g: trimming to the best features is not part of the detector (0 keeps all)", cfg.n_features);
    if (4ll * width * height > kSift2dMaxPixels) return sift2d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift2d: doubled base images of at most 2^31-1 pixels");

    Sift2dPlan p;
    p.n_octave_layers = cfg.n_octave_layers;
    p.base_cols = 2 * width, p.base_rows = 2 * height;
    const int side = p.base_cols < p.base_rows ? p.base_cols : p.base_rows;
    const int n_octave = sift2d_round(std::log((double)side) / std::log(2.0) - 2);
    p.n_octave = n_octave > 0 ? n_octave : 1;
    p.threshold = (int)std::floor(0.5 * cfg.contrast_threshold / cfg.n_octave_layers * 255);
    const int per = p.gauss_per_octave();
    p.gauss.resize((size_t)p.n_octave * per);

    // sig[0] = sigma, sig[i] = sqrt((sigma k^i)^2 - (sigma k^(i-1))^2), in double, rounded to float32 once
    std::vector<float> sig((size_t)per);
    const double k = std::pow(2.0, 1.0 / cfg.n_octave_layers);
    sig[0] = cfg.sigma;
    for (int i = 1; i < per; i++) {
        const double prev = std::pow(k, (double)(i - 1)) * cfg.sigma, total = prev * k;
        sig[(size_t)i] = (float)std::sqrt(total * total - prev * prev);
    }
    const float base_sigma = sqrtf(fmaxf(cfg.sigma * cfg.sigma - 4 * 0.5f * 0.5f, 0.01f));

    int cols = p.base_cols, rows = p.base_rows;
    for (int o = 0; o < p.n_octave; o++) {
        if (o > 0) cols /= 2, rows /= 2;
        if (cols < 1 || rows < 1) return sift2d_refuse(OC_HIP_ERR_INVALID, "sift2d: an octave without pixels");
        for (int i = 0; i < per; i++) {
            Sift2dLayer& g = p.gauss[(size_t)o * per + i];
            g.cols = cols, g.rows = rows, g.octave = o, g.index = i;
            if (i == 0 && o > 0) {
                g.source = (o - 1) * per + cfg.n_octave_layers;
                g.blurred = false;
                continue;
            }
            g.source = o * per + i - 1;  // (-1 for the first layer: the upscaled input)
            g.sigma = i == 0 ? base_sigma : sig[(size_t)i];
            g.radius = sift2d_radius(g.sigma);
            // (a blur sigma below 0.0625 has a single tap, R = 0: cv::SIFT would copy the layer; the kernels take R >= 1, so it is refused)
            if (g.radius < 1)
                return sift2d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift2d: the blur sigma %g of layer %g gives a blur radius below 1", g.sigma, i);
            if (g.radius > kSift2dMaxRadius)
                return sift2d_refuse(OC_HIP_ERR_UNSUPPORTED, "sift2d: sigma %g gives a blur radius beyond the supported %g", g.sigma, kSift2dMaxRadius);
            g.weight = sift2d_weights(g.sigma, g.radius);
        }
    }
    return p;
}

}  // namespace ochip_host

// sift2d_twin.cpp -- CPU restatement, in float32, of the arithmetic contract of SIFT2D's detector (DESIGN.md section 4.13;
// opencorr_amd/csrc/sift2d.hip, include/opencorr_hip.h "SIFT2D's detector"): the 2x upscale, the Gaussian and DoG pyramids, the
// 26-neighbour extrema scan and the sub-pixel localisation with its contrast and edge rejections -- cv::SIFT as the reference's
// SIFT2D::compute() creates it (src/oc_sift.cpp:22-30, 60-93).  The octave count, dims, sigmas, radii, weights and the threshold
// come from host/sift2d_plan.h, like the library's; the arithmetic on pixels is written here a second time.  The kernels are
// compared with it bit for bit (tests/test_gpu_sift2d.py) and a float64 model pins it (tests/test_sift2d_twin_cpu.py).
//
// Build: g++ -O2 -ffp-contract=off -fopenmp (tests/sift2d_twin.py).  OpenMP runs over rows and candidates only: one pixel's sum
// is one thread's, r ascending; the list is in scan order of the starting extremum whatever the thread count.
//
// oc_twin_sift2d_set_slip plants ONE deliberate error (tests/test_sift2d_twin_cpu.py shows that the model catches each):
//   1 = strict comparisons with the 26 neighbours, 2 = the 18 neighbours of the layers below and above skipped, 3 = border 4,
//   4 = plain reflection (-1 -> 0) in place of reflect-101, 5 = truncation in place of cvRound in the localisation steps,
//   6 = threshold not floored, 7 = the 0.5 of x and y missing, 8 = edge test inverted.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../opencorr_amd/csrc/host/sift2d_plan.h"

namespace {

using namespace ochip_host;

int g_slip = 0;

struct Keypoint {  // oc_hip_sift2d_keypoint
    float x, y, size, response;
    int octave, layer, row, col;
    float xc, xr, xi;
    int packed_octave;
};
static_assert(sizeof(Keypoint) == 48, "a keypoint is 48 bytes");

struct Start {
    int octave, layer, row, col, accepted;
};

struct Twin {
    Sift2dSettings cfg;
    Sift2dPlan plan;
    std::vector<std::vector<float>> gauss, dog;
};

int reflect(int i, int n) {
    if (g_slip != 4) return sift2d_reflect(i, n);
    while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
    return i;
}

// rows first, then columns; acc = w[0] s[c], then acc = acc + w[r] (s[lo] + s[hi]) for r = 1 ... R
void blur(const std::vector<float>& src, std::vector<float>& dst, int cols, int rows, const std::vector<float>& w, int R) {
    std::vector<float> tmp((size_t)cols * rows);
    dst.resize((size_t)cols * rows);
#pragma omp parallel for schedule(static)
    for (int y = 0; y < rows; y++) {
        const float* s = &src[(size_t)y * cols];
        for (int x = 0; x < cols; x++) {
            float acc = w[0] * s[x];
            for (int r = 1; r <= R; r++) acc = acc + w[(size_t)r] * (s[reflect(x - r, cols)] + s[reflect(x + r, cols)]);
            tmp[(size_t)y * cols + x] = acc;
        }
    }
#pragma omp parallel for schedule(static)
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            float acc = w[0] * tmp[(size_t)y * cols + x];
            for (int r = 1; r <= R; r++)
                acc = acc + w[(size_t)r] * (tmp[(size_t)reflect(y - r, rows) * cols + x] + tmp[(size_t)reflect(y + r, rows) * cols + x]);
            dst[(size_t)y * cols + x] = acc;
        }
}

// destination x samples the source at (x + 0.5) * 0.5 - 0.5: even x = 2k between k - 1 (0.25) and k (0.75), odd x = 2k + 1 between
// k (0.75) and k + 1 (0.25), indices clamped to the edge; along x first in both source rows (a = w0 s[x0] + w1 s[x1]), then w0 a + w1 b along y
void upscale(const float* img, int w, int h, std::vector<float>& dst) {
    dst.resize((size_t)4 * w * h);
#pragma omp parallel for schedule(static)
    for (int y = 0; y < 2 * h; y++) {
        const int ky = y >> 1;
        const int y0 = (y & 1) ? ky : (ky > 0 ? ky - 1 : 0), y1 = (y & 1) ? (ky + 1 < h ? ky + 1 : h - 1) : ky;
        const float wy0 = (y & 1) ? 0.75f : 0.25f, wy1 = (y & 1) ? 0.25f : 0.75f;
        for (int x = 0; x < 2 * w; x++) {
            const int kx = x >> 1;
            const int x0 = (x & 1) ? kx : (kx > 0 ? kx - 1 : 0), x1 = (x & 1) ? (kx + 1 < w ? kx + 1 : w - 1) : kx;
            const float wx0 = (x & 1) ? 0.75f : 0.25f, wx1 = (x & 1) ? 0.25f : 0.75f;
            const float a = wx0 * img[(size_t)y0 * w + x0] + wx1 * img[(size_t)y0 * w + x1];
            const float b = wx0 * img[(size_t)y1 * w + x0] + wx1 * img[(size_t)y1 * w + x1];
            dst[(size_t)y * 2 * w + x] = wy0 * a + wy1 * b;
        }
    }
}

int round_step(float v) { return g_slip == 5 ? (int)v : (int)nearbyintf(v); }

// X of H X = b by elimination with partial pivoting (the first largest magnitude of a column wins); a zero pivot: X = 0
void solve3(float A[3][4], float X[3]) {
    X[0] = X[1] = X[2] = 0.f;
    for (int k = 0; k < 3; k++) {
        int p = k;
        for (int i = k + 1; i < 3; i++)
            if (fabsf(A[i][k]) > fabsf(A[p][k])) p = i;
        if (A[p][k] == 0.f) return;
        if (p != k)
            for (int j = 0; j < 4; j++) {
                const float t = A[k][j];
                A[k][j] = A[p][j];
                A[p][j] = t;
            }
        for (int i = k + 1; i < 3; i++) {
            const float f = A[i][k] / A[k][k];
            for (int j = k + 1; j < 4; j++) A[i][j] = A[i][j] - f * A[k][j];
        }
    }
    X[2] = A[2][3] / A[2][2];
    X[1] = (A[1][3] - A[1][2] * X[2]) / A[1][1];
    X[0] = ((A[0][3] - A[0][1] * X[1]) - A[0][2] * X[2]) / A[0][0];
}

bool localize(const Twin& t, int o, int layer, int r, int c, Keypoint& kp) {
    const Sift2dPlan& p = t.plan;
    const int n = p.n_octave_layers, border = g_slip == 3 ? 4 : kSift2dBorder;
    const Sift2dLayer& g = p.gauss[(size_t)o * p.gauss_per_octave()];
    const int cols = g.cols, rows = g.rows;
    const float img_scale = 1.f / 255, deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    float xc = 0, xr = 0, xi = 0, dD[3] = {0, 0, 0};
    int step = 0;
    for (; step < kSift2dMaxSteps; step++) {
        const float* img = t.dog[(size_t)o * p.dog_per_octave() + layer].data();
        const float* prev = t.dog[(size_t)o * p.dog_per_octave() + layer - 1].data();
        const float* next = t.dog[(size_t)o * p.dog_per_octave() + layer + 1].data();
#define AT(a, rr, cc) a[(size_t)(rr) * cols + (cc)]
        dD[0] = (AT(img, r, c + 1) - AT(img, r, c - 1)) * deriv_scale;
        dD[1] = (AT(img, r + 1, c) - AT(img, r - 1, c)) * deriv_scale;
        dD[2] = (AT(next, r, c) - AT(prev, r, c)) * deriv_scale;
        const float v2 = AT(img, r, c) * 2;
        const float dxx = (AT(img, r, c + 1) + AT(img, r, c - 1) - v2) * second_scale;
        const float dyy = (AT(img, r + 1, c) + AT(img, r - 1, c) - v2) * second_scale;
        const float dss = (AT(next, r, c) + AT(prev, r, c) - v2) * second_scale;
        const float dxy = (AT(img, r + 1, c + 1) - AT(img, r + 1, c - 1) - AT(img, r - 1, c + 1) + AT(img, r - 1, c - 1)) * cross_scale;
        const float dxs = (AT(next, r, c + 1) - AT(next, r, c - 1) - AT(prev, r, c + 1) + AT(prev, r, c - 1)) * cross_scale;
        const float dys = (AT(next, r + 1, c) - AT(next, r - 1, c) - AT(prev, r + 1, c) + AT(prev, r - 1, c)) * cross_scale;
        float A[3][4] = {{dxx, dxy, dxs, dD[0]}, {dxy, dyy, dys, dD[1]}, {dxs, dys, dss, dD[2]}};
        float X[3];
        solve3(A, X);
        xc = -X[0], xr = -X[1], xi = -X[2];
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        const float big = (float)(INT_MAX / 3);
        if (!(fabsf(xi) <= big) || !(fabsf(xr) <= big) || !(fabsf(xc) <= big)) return false;  // (a NaN is rejected here too)
        c += round_step(xc);
        r += round_step(xr);
        layer += round_step(xi);
        if (layer < 1 || layer > n || c < border || c >= cols - border || r < border || r >= rows - border) return false;
    }
    if (step >= kSift2dMaxSteps) return false;
    const float* img = t.dog[(size_t)o * p.dog_per_octave() + layer].data();
    float dot = dD[0] * xc;
    dot = dot + dD[1] * xr;
    dot = dot + dD[2] * xi;
    const float contr = AT(img, r, c) * img_scale + 0.5f * dot;
    if (fabsf(contr) * n < t.cfg.contrast_threshold) return false;
    const float v2 = AT(img, r, c) * 2;
    const float dxx = (AT(img, r, c + 1) + AT(img, r, c - 1) - v2) * second_scale;
    const float dyy = (AT(img, r + 1, c) + AT(img, r - 1, c) - v2) * second_scale;
    const float dxy = (AT(img, r + 1, c + 1) - AT(img, r + 1, c - 1) - AT(img, r - 1, c + 1) + AT(img, r - 1, c - 1)) * cross_scale;
#undef AT
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy, e = t.cfg.edge_threshold;
    const bool edge = det <= 0 || tr * tr * e >= (e + 1) * (e + 1) * det;
    if (g_slip == 8 ? !edge : edge) return false;
    const float pw = (float)(1 << o), half = g_slip == 7 ? 1.f : 0.5f;
    kp.x = (c + xc) * pw * half;
    kp.y = (r + xr) * pw * half;
    kp.size = t.cfg.sigma * sift2d_pow2((layer + xi) / n) * pw * 2 * 0.5f;
    kp.response = fabsf(contr);
    kp.octave = o - 1, kp.layer = layer, kp.row = r, kp.col = c;
    kp.xc = xc, kp.xr = xr, kp.xi = xi;
    kp.packed_octave = ((o - 1) & 255) | (layer << 8) | (sift2d_round(((double)xi + 0.5) * 255) << 16);
    return true;
}

bool is_candidate(const Twin& t, int o, int layer, int r, int c, float threshold) {
    const Sift2dPlan& p = t.plan;
    const int cols = p.gauss[(size_t)o * p.gauss_per_octave()].cols;
    const float* L[3] = {t.dog[(size_t)o * p.dog_per_octave() + layer].data(), t.dog[(size_t)o * p.dog_per_octave() + layer - 1].data(),
                         t.dog[(size_t)o * p.dog_per_octave() + layer + 1].data()};
    const float v = L[0][(size_t)r * cols + c];
    if (!(fabsf(v) > threshold)) return false;
    if (!(v > 0) && !(v < 0)) return false;
    bool ge = true, le = true;
    for (int k = 0; k < (g_slip == 2 ? 1 : 3); k++)
        for (int dr = -1; dr <= 1; dr++)
            for (int dc = -1; dc <= 1; dc++) {
                if (k == 0 && dr == 0 && dc == 0) continue;
                const float q = L[k][(size_t)(r + dr) * cols + (c + dc)];
                ge = ge && (g_slip == 1 ? v > q : v >= q);
                le = le && (g_slip == 1 ? v < q : v <= q);
            }
    return v > 0 ? ge : le;
}

}  // namespace

extern "C" {

void oc_twin_sift2d_set_slip(int which) { g_slip = which; }

// image: w x h, float32 (is_u8 = 0) or uint8 (is_u8 = 1); null when the plan refuses (oc_twin_sift2d_status of a null handle is not asked)
void* oc_twin_sift2d_build(const void* image, int is_u8, int w, int h, int n_features, int n_octave_layers, float contrast_threshold,
                           float edge_threshold, float sigma, int* status) {
    Twin* t = new Twin;
    t->cfg.n_features = n_features, t->cfg.n_octave_layers = n_octave_layers, t->cfg.contrast_threshold = contrast_threshold;
    t->cfg.edge_threshold = edge_threshold, t->cfg.sigma = sigma;
    t->plan = sift2d_plan(t->cfg, w, h);
    if (status) *status = t->plan.status;
    if (t->plan.status != OC_HIP_OK) {
        delete t;
        return nullptr;
    }
    std::vector<float> img((size_t)w * h);
    for (size_t i = 0; i < img.size(); i++) img[i] = is_u8 ? (float)static_cast<const uint8_t*>(image)[i] : static_cast<const float*>(image)[i];
    for (float v : img)
        if (!std::isfinite(v)) {
            if (status) *status = OC_HIP_ERR_INVALID;
            delete t;
            return nullptr;
        }
    const Sift2dPlan& p = t->plan;
    t->gauss.resize(p.gauss.size());
    t->dog.resize((size_t)p.dog_layers());
    std::vector<float> base;
    upscale(img.data(), w, h, base);
    for (size_t i = 0; i < p.gauss.size(); i++) {
        const Sift2dLayer& g = p.gauss[i];
        if (g.blurred) {
            blur(g.source < 0 ? base : t->gauss[(size_t)g.source], t->gauss[i], g.cols, g.rows, g.weight, g.radius);
        } else {
            const Sift2dLayer& s = p.gauss[(size_t)g.source];
            const std::vector<float>& src = t->gauss[(size_t)g.source];
            t->gauss[i].resize(g.pixels());
            for (int y = 0; y < g.rows; y++)
                for (int x = 0; x < g.cols; x++) {
                    const int sx = sift2d_nearest(x, s.cols, g.cols), sy = sift2d_nearest(y, s.rows, g.rows);
                    t->gauss[i][(size_t)y * g.cols + x] = src[(size_t)sy * s.cols + sx];
                }
        }
    }
    for (int d = 0; d < p.dog_layers(); d++) {
        const size_t gi = (size_t)p.dog_gauss(d);
        t->dog[(size_t)d].resize(p.gauss[gi].pixels());
        for (size_t q = 0; q < t->dog[(size_t)d].size(); q++) t->dog[(size_t)d][q] = t->gauss[gi + 1][q] - t->gauss[gi][q];
    }
    return t;
}

void oc_twin_sift2d_free(void* h) { delete static_cast<Twin*>(h); }
int oc_twin_sift2d_layers(void* h, int pyramid) {
    const Twin* t = static_cast<Twin*>(h);
    return pyramid == 0 ? (int)t->plan.gauss.size() : t->plan.dog_layers();
}
int oc_twin_sift2d_octaves(void* h) { return static_cast<Twin*>(h)->plan.n_octave; }
int oc_twin_sift2d_threshold(void* h) { return static_cast<Twin*>(h)->plan.threshold; }

const float* oc_twin_sift2d_info(void* h, int pyramid, int index, int* cols, int* rows, int* octave, float* sigma, int* radius) {
    const Twin* t = static_cast<Twin*>(h);
    const Sift2dLayer& g = t->plan.gauss[(size_t)(pyramid == 0 ? index : t->plan.dog_gauss(index))];
    *cols = g.cols, *rows = g.rows, *octave = g.octave;
    *sigma = pyramid == 0 ? g.sigma : 0.f;
    *radius = pyramid == 0 ? g.radius : 0;
    return pyramid == 0 ? t->gauss[(size_t)index].data() : t->dog[(size_t)index].data();
}

int oc_twin_sift2d_weights(void* h, int index, float* out) {
    const Sift2dLayer& g = static_cast<Twin*>(h)->plan.gauss[(size_t)index];
    std::memcpy(out, g.weight.data(), g.weight.size() * sizeof(float));
    return (int)g.weight.size();
}

// every starting extremum in scan order (octave, layer, row, column) into `starts` (up to start_capacity), the located keypoints in
// the same order into `out` (up to capacity); returns the number of keypoints, *n_starts the number of starts
long oc_twin_sift2d_detect(void* h, void* out, long capacity, void* starts, long start_capacity, long* n_starts) {
    const Twin* t = static_cast<Twin*>(h);
    const Sift2dPlan& p = t->plan;
    const int border = g_slip == 3 ? 4 : kSift2dBorder;
    const float threshold = g_slip == 6 ? (float)(0.5 * t->cfg.contrast_threshold / p.n_octave_layers * 255) : (float)p.threshold;
    std::vector<Start> list;
    for (int o = 0; o < p.n_octave; o++) {
        const Sift2dLayer& g = p.gauss[(size_t)o * p.gauss_per_octave()];
        for (int layer = 1; layer <= p.n_octave_layers; layer++)
            for (int r = border; r < g.rows - border; r++)
                for (int c = border; c < g.cols - border; c++)
                    if (is_candidate(*t, o, layer, r, c, threshold)) list.push_back(Start{o, layer, r, c, 0});
    }
    std::vector<Keypoint> kps(list.size());
#pragma omp parallel for schedule(static)
    for (long i = 0; i < (long)list.size(); i++)
        list[(size_t)i].accepted = localize(*t, list[(size_t)i].octave, list[(size_t)i].layer, list[(size_t)i].row, list[(size_t)i].col, kps[(size_t)i]);
    long n = 0;
    for (size_t i = 0; i < list.size(); i++) {
        if (starts && (long)i < start_capacity) static_cast<Start*>(starts)[i] = list[i];
        if (!list[i].accepted) continue;
        if (out && n < capacity) static_cast<Keypoint*>(out)[n] = kps[i];
        n++;
    }
    if (n_starts) *n_starts = (long)list.size();
    return n;
}

float oc_twin_sift2d_pow2(float t) { return sift2d_pow2(t); }
float oc_twin_sift2d_powf(float t) { return powf(2.f, t); }

}  // extern "C"

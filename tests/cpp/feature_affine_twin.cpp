// feature_affine_twin.cpp -- CPU restatement of the FeatureAffine2D/3D contract (include/opencorr_hip.h) in
// plain C++: brute-force neighbour sets put into the contract's order, the counter-based sample generator, the float32 / double
// operations in the contract's order.  The GPU kernel must equal this in every bit (tests/test_gpu_feature_affine.py); this
// against an independent float64 model: tests/test_feature_affine_twin_cpu.py.  Build with -ffp-contract=off.
//
// Planted slips (oc_twin_fa_set_slip), each of which the CPU test must see:
//   1 consensus with <=          2 radius test with <=          3 sampling with replacement     4 KNN fallback skipped
//   5 diagonal - 1.f dropped     6 local coordinates not subtracted                             7 exit rule on max_set's mean
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <omp.h>
#include <utility>
#include <vector>

namespace {

int g_slip = 0;

struct Grid {
    float x0, y0, z0, inv_pitch;
    int ncx, ncy, ncz;
};

// Strain's grid rule over the reference keypoints: pitch a little above the radius, capped cell count per axis
Grid make_grid(int ndim, const float* ref, long n, float radius) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long i = 0; i < n; i++)
        for (int a = 0; a < ndim; a++) {
            const float c = ref[i * ndim + a];
            if (c < mn[a]) mn[a] = c;
            if (c > mx[a]) mx[a] = c;
        }
    for (int a = 0; a < 3; a++)
        if (!(mn[a] <= mx[a])) mn[a] = mx[a] = 0.f;
    float pitch = radius * 1.001f;
    const float span = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    const float cap = ndim == 2 ? 4096.f : 256.f;
    if (!(pitch > span / cap)) pitch = span / cap;
    if (!(pitch > 0.f)) pitch = 1.f;
    Grid g;
    g.x0 = mn[0];
    g.y0 = mn[1];
    g.z0 = mn[2];
    g.inv_pitch = 1.f / pitch;
    g.ncx = (int)((mx[0] - mn[0]) * g.inv_pitch) + 1;
    g.ncy = (int)((mx[1] - mn[1]) * g.inv_pitch) + 1;
    g.ncz = ndim == 3 ? (int)((mx[2] - mn[2]) * g.inv_pitch) + 1 : 1;
    return g;
}

int cell_axis(float c, float c0, float inv_pitch, int nc) {
    const float t = (c - c0) * inv_pitch;
    return t >= 0.f ? (t < (float)nc ? (int)t : nc - 1) : 0;
}

void cell_of(int ndim, const float* p, const Grid& g, int c[3]) {
    c[0] = cell_axis(p[0], g.x0, g.inv_pitch, g.ncx);
    c[1] = cell_axis(p[1], g.y0, g.inv_pitch, g.ncy);
    c[2] = ndim == 3 ? cell_axis(p[2], g.z0, g.inv_pitch, g.ncz) : 0;
}

float dist2(int ndim, const float* p, const float* k) {
    const float dx = p[0] - k[0], dy = p[1] - k[1];
    float d = dx * dx;
    d = d + dy * dy;
    if (ndim == 3) {
        const float dz = p[2] - k[2];
        d = d + dz * dz;
    }
    return d;
}

uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Cand {
    float r[3], t[3];
};

// least squares of [x y (z) 1] X = [x' y' (z')] over the candidates rows[0 ... count-1], in that order
bool fit(int ndim, const std::vector<Cand>& c, const int* rows, int count, float X[4][3]) {
    const int D = ndim + 1;
    double S[4][4] = {}, B[4][3] = {};
    for (int i = 0; i < count; i++) {
        const Cand& k = c[rows[i]];
        double row[4];
        for (int a = 0; a < ndim; a++) row[a] = (double)k.r[a];
        row[ndim] = 1.0;
        for (int a = 0; a < D; a++)
            for (int b = a; b < D; b++) S[a][b] = S[a][b] + row[a] * row[b];
        for (int a = 0; a < D; a++)
            for (int r = 0; r < ndim; r++) B[a][r] = B[a][r] + row[a] * (double)k.t[r];
    }
    double A[4][7];
    double big = 0.0;
    for (int a = 0; a < D; a++) {
        for (int b = 0; b < D; b++) {
            A[a][b] = a <= b ? S[a][b] : S[b][a];
            if (std::fabs(A[a][b]) > big) big = std::fabs(A[a][b]);
        }
        for (int r = 0; r < ndim; r++) A[a][D + r] = B[a][r];
    }
    const double tiny = big * 0x1p-40;
    double rinv[4];
    for (int k = 0; k < D; k++) {
        int p = k;
        double best = std::fabs(A[k][k]);
        for (int i = k + 1; i < D; i++)
            if (std::fabs(A[i][k]) > best) {
                best = std::fabs(A[i][k]);
                p = i;
            }
        if (!(best >= tiny)) return false;
        if (p != k)
            for (int j = 0; j < D + ndim; j++) std::swap(A[k][j], A[p][j]);
        rinv[k] = 1.0 / A[k][k];
        for (int i = k + 1; i < D; i++) {
            const double f = A[i][k] * rinv[k];
            for (int j = k + 1; j < D + ndim; j++) A[i][j] = A[i][j] - f * A[k][j];
        }
    }
    for (int r = 0; r < ndim; r++) {
        double x[4];
        for (int k = D - 1; k >= 0; k--) {
            double v = A[k][D + r];
            for (int j = k + 1; j < D; j++) v = v - A[k][j] * x[j];
            x[k] = v * rinv[k];
        }
        for (int k = 0; k < D; k++) X[k][r] = (float)x[k];
    }
    return true;
}

float error_of(int ndim, const Cand& k, const float X[4][3]) {
    if (ndim == 2) {
        const float dx = (k.r[0] * X[0][0] + k.r[1] * X[1][0] + X[2][0]) - k.t[0];
        const float dy = (k.r[0] * X[0][1] + k.r[1] * X[1][1] + X[2][1]) - k.t[1];
        return sqrtf(dx * dx + dy * dy);
    }
    const float dx = (k.r[0] * X[0][0] + k.r[1] * X[1][0] + k.r[2] * X[2][0] + X[3][0]) - k.t[0];
    const float dy = (k.r[0] * X[0][1] + k.r[1] * X[1][1] + k.r[2] * X[2][1] + X[3][1]) - k.t[1];
    const float dz = (k.r[0] * X[0][2] + k.r[1] * X[1][2] + k.r[2] * X[2][2] + X[3][2]) - k.t[2];
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

struct Settings {
    int ndim;
    float radius, threshold;
    int nmin, trials, samples;
    uint64_t seed;
    int adaptive, feature_min, radius_min;
    float width, height;
};

// the K nearest keypoints by ascending (d2, index)
std::vector<long> knn(const Settings& s, const float* ref, long nkp, const float* p, int K) {
    std::vector<std::pair<float, long>> all;
    for (long i = 0; i < nkp; i++) {
        const float d = dist2(s.ndim, p, ref + i * s.ndim);
        if (d == d) all.emplace_back(d, i);
    }
    std::sort(all.begin(), all.end());
    std::vector<long> out;
    for (size_t i = 0; i < all.size() && (int)i < K; i++) out.push_back(all[i].second);
    return out;
}

void one_poi(const Settings& s, const Grid& g, const float* ref, const float* tar, long nkp, float* poi) {
    const int ndim = s.ndim, D = ndim + 1;
    const int ZNCC = ndim == 2 ? 16 : 18, ITER = ndim == 2 ? 17 : 19, FEATURE = ndim == 2 ? 19 : 21;
    float p[3] = {poi[0], poi[1], ndim == 3 ? poi[2] : 0.f};
    uint64_t base = splitmix64(s.seed ^ ((uint64_t)bits(p[0]) | ((uint64_t)bits(p[1]) << 32)));
    if (ndim == 3) base = splitmix64(base ^ (uint64_t)bits(p[2]));
    std::vector<long> pick;
    if (ndim == 2 && s.adaptive) {
        pick = knn(s, ref, nkp, p, s.feature_min);
        if ((int)pick.size() < s.samples) {
            poi[ZNCC] = -1.f;
            return;
        }
        float x_min = s.width, x_max = -1.f, y_min = s.height, y_max = -1.f;
        for (long i : pick) {
            const float x = ref[i * 2], y = ref[i * 2 + 1];
            x_min = x < x_min ? x : x_min;
            x_max = x > x_max ? x : x_max;
            y_min = y < y_min ? y : y_min;
            y_max = y > y_max ? y : y_max;
        }
        int srx, sry;
        if (p[0] >= x_min && p[0] <= x_max && p[1] >= y_min && p[1] <= y_max) {
            srx = fabsf(x_max - p[0]) > fabsf(p[0] - x_min) ? (int)fabsf(x_max - p[0]) : (int)fabsf(p[0] - x_min);
            sry = fabsf(y_max - p[1]) > fabsf(p[1] - y_min) ? (int)fabsf(y_max - p[1]) : (int)fabsf(p[1] - y_min);
        } else {
            p[0] = (float)(int)(0.5f * (x_max + x_min));
            p[1] = (float)(int)(0.5f * (y_max + y_min));
            srx = (int)(0.5f * (x_max - x_min));
            sry = (int)(0.5f * (y_max - y_min));
        }
        srx = srx < s.radius_min ? s.radius_min : srx;
        sry = sry < s.radius_min ? s.radius_min : sry;
        poi[0] = p[0];
        poi[1] = p[1];
        poi[23] = (float)srx;
        poi[24] = (float)sry;
    } else {
        // radius search, brute force, then the walk's order: cells of the block row-major, ascending index inside a cell
        const float r2 = s.radius * s.radius;
        int pc[3];
        cell_of(ndim, p, g, pc);
        struct Key {
            int cz, cy, cx;
            long i;
        };
        std::vector<Key> in;
        for (long i = 0; i < nkp; i++) {
            const float d = dist2(ndim, p, ref + i * ndim);
            if (!(g_slip == 2 ? d <= r2 : d < r2)) continue;
            int c[3];
            cell_of(ndim, ref + i * ndim, g, c);
            if (std::abs(c[0] - pc[0]) > 1 || std::abs(c[1] - pc[1]) > 1 || std::abs(c[2] - pc[2]) > 1) continue;  // not in the block
            in.push_back({c[2], c[1], c[0], i});
        }
        std::sort(in.begin(), in.end(), [](const Key& a, const Key& b) {
            if (a.cz != b.cz) return a.cz < b.cz;
            if (a.cy != b.cy) return a.cy < b.cy;
            if (a.cx != b.cx) return a.cx < b.cx;
            return a.i < b.i;
        });
        if ((int)in.size() < s.samples) {
            poi[ZNCC] = -1.f;
            return;
        }
        if ((int)in.size() < s.nmin && g_slip != 4) pick = knn(s, ref, nkp, p, s.nmin);
        else
            for (const Key& k : in) pick.push_back(k.i);
    }
    const int n = (int)pick.size();
    std::vector<Cand> c(n);
    for (int j = 0; j < n; j++)
        for (int a = 0; a < ndim; a++) {
            c[j].r[a] = g_slip == 6 ? ref[pick[j] * ndim + a] : ref[pick[j] * ndim + a] - p[a];
            c[j].t[a] = g_slip == 6 ? tar[pick[j] * ndim + a] : tar[pick[j] * ndim + a] - p[a];
        }
    // RANSAC
    std::vector<int> perm(n), max_set, trial_set;
    int trials = 0;
    float mean = 0.f, max_mean = NAN;
    float X[4][3];
    const float exit_mean = s.threshold / (float)s.nmin;
    do {
        for (int j = 0; j < n; j++) perm[j] = j;
        int smp[8];
        for (int j = 0; j < s.samples; j++) {
            const uint64_t h = splitmix64(base + (((uint64_t)(uint32_t)trials << 8) | (uint64_t)j));
            if (g_slip == 3) {
                smp[j] = (int)(((h >> 32) * (uint64_t)n) >> 32);
                continue;
            }
            const uint32_t k = (uint32_t)j + (uint32_t)(((h >> 32) * (uint64_t)(uint32_t)(n - j)) >> 32);
            std::swap(perm[j], perm[k]);
            smp[j] = perm[j];
        }
        trial_set.clear();
        float part[64];
        for (int l = 0; l < 64; l++) part[l] = 0.f;
        if (fit(ndim, c, smp, s.samples, X))
            for (int j = 0; j < n; j++) {
                const float err = error_of(ndim, c[j], X);
                if (g_slip == 1 ? err <= s.threshold : err < s.threshold) {
                    trial_set.push_back(j);
                    part[j & 63] = part[j & 63] + err;
                }
            }
        for (int off = 1; off < 64; off <<= 1) {  // the xor butterfly, ascending offsets
            float next[64];
            for (int l = 0; l < 64; l++) next[l] = part[l] + part[l ^ off];
            std::memcpy(part, next, sizeof(part));
        }
        mean = part[0] / (float)trial_set.size();
        if (trial_set.size() > max_set.size()) {
            max_set = trial_set;
            max_mean = mean;
        }
        trials++;
    } while (trials < s.trials && ((int)max_set.size() < s.nmin || (g_slip == 7 ? max_mean : mean) > exit_mean));
    const int m = (int)max_set.size();
    if (m < D || !fit(ndim, c, max_set.data(), m, X)) {
        poi[ZNCC] = -2.f;
        return;
    }
    const float one = g_slip == 5 ? 0.f : 1.f;
    if (ndim == 2) {
        poi[2] = X[2][0];
        poi[3] = X[0][0] - one;
        poi[4] = X[1][0];
        poi[8] = X[2][1];
        poi[9] = X[0][1];
        poi[10] = X[1][1] - one;
    } else {
        for (int r = 0; r < 3; r++) {
            poi[3 + 4 * r] = X[3][r];
            for (int a = 0; a < 3; a++) poi[3 + 4 * r + 1 + a] = a == r ? X[a][r] - one : X[a][r];
        }
    }
    poi[ITER] = (float)trials;
    poi[FEATURE] = (float)m;
    poi[ZNCC] = 0.f;
}

}  // namespace

extern "C" {

void oc_twin_fa_set_slip(int slip) { g_slip = slip; }

// pois: count records of stride_f floats (25 / 31 used), updated in place; threads: OpenMP threads (< 1: the runtime's default)
void oc_twin_fa_compute(int ndim, const float* ref, const float* tar, long nkp, float* pois, long count, int stride_f, float radius,
                        int nmin, int trials, int samples, float threshold, unsigned long long seed, int adaptive, int feature_min,
                        int radius_min, int width, int height, int threads) {
    const Settings s = {ndim, radius, threshold, nmin, trials, samples, seed, adaptive, feature_min, radius_min, (float)width, (float)height};
    const Grid g = make_grid(ndim, ref, nkp, radius);
    if (threads < 1) threads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
    for (long i = 0; i < count; i++) one_poi(s, g, ref, tar, nkp, pois + i * stride_f);
}

}  // extern "C"

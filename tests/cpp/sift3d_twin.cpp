// sift3d_twin.cpp -- CPU restatement of the arithmetic contract of SIFT3D's scale space (opencorr_amd/csrc/sift3d.hip,
// include/opencorr_hip.h "SIFT3D's scale space"), written the way the reference writes it: the layer table of
// SIFT3D::createGaussianPyramid (src/oc_sift.cpp:679-739), the three passes of SIFT3D::gaussianBlur with their weights (:365-547),
// downSampling (:549-562), createDogPyramid with max_abs (:756-793) and the scan of detectExtrema (:795-847).  It shares no code
// with the library: the plan header is checked against it (tests/test_sift3d_plan_cpu.py), the kernels are compared with it bit
// for bit (tests/test_gpu_sift3d.py), and a float64 model pins it (tests/test_sift3d_twin_cpu.py).
//
// Build: g++ -O2 -ffp-contract=off -fopenmp (tests/sift3d_twin.py).  fma = 0: product and sum of a tap round separately;
// fma = 1: std::fmaf(w[r], s_lo + s_hi, acc).  OpenMP runs over voxels only: one voxel's sum is one thread's, r ascending.
//
// Defined where the reference is not: a mirrored index that leaves the axis (radius > n - 1) is clamped into [0, n - 1].
//
// oc_twin_sift3d_set_slip plants ONE deliberate error (tests/test_sift3d_twin_cpu.py shows that the model catches each):
//   1 = `>=` / `<=` in place of the strict comparisons, 2 = the two scale neighbours skipped, 3 = border 0 instead of 1 (a
//   neighbour outside the layer is skipped), 4 = the high reflection 2(n-1)-i+1, 5 = taps summed in descending r,
//   6 = threshold `>` in place of `>=`.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

int g_slip = 0;

struct Layer {
    int dim[3];      // x, y, z
    float unit[3];
    int octave;
    float scale, sigma, max_abs;
    int radius[3];
    std::vector<float> weight[3];
    std::vector<float> vol;  // [z][y][x]
};

struct Candidate {
    int x, y, z, octave, layer;
    float scale;
};

struct Twin {
    int n_octave_layers, n_octave;
    float alpha;
    std::vector<Layer> gauss, dog;
};

inline int mirror_low(int i) { return i < 0 ? -i : i; }
inline int mirror_high(int i, int last) {
    if (i > last) return g_slip == 4 ? 2 * last - i + 1 : 2 * last - i;
    return i;
}
inline int clamp_index(int i, int last) { return i < 0 ? 0 : i > last ? last : i; }

std::vector<float> make_weights(float sigma, int radius) {
    std::vector<float> kernel((size_t)radius + 1);
    kernel[0] = 1.f;
    for (int i = 1; i <= radius; i++) {
        float x = i / (sigma + FLT_EPSILON);
        kernel[i] = expf(-0.5f * x * x);
        kernel[0] += (kernel[i] * 2.f);
    }
    kernel[0] = 1.f / kernel[0];
    for (int i = 1; i <= radius; i++) kernel[i] *= kernel[0];
    return kernel;
}

// one pass along `axis` (0 = x, 1 = y, 2 = z) of a [z][y][x] volume
void blur_axis(const std::vector<float>& src, std::vector<float>& dst, const int* dim, int axis, const std::vector<float>& w, int radius, int fma) {
    const long nx = dim[0], ny = dim[1], nz = dim[2];
    const long stride = axis == 0 ? 1 : axis == 1 ? nx : nx * ny;
    const int n = dim[axis], last = n - 1;
#pragma omp parallel for
    for (long v = 0; v < nx * ny * nz; v++) {
        const long k = v % nx, j = (v / nx) % ny, i = v / (nx * ny);
        const int c = axis == 0 ? (int)k : axis == 1 ? (int)j : (int)i;
        const float* line = src.data() + (v - c * stride);
        float acc = w[0] * line[c * stride];
        for (int t = 1; t <= radius; t++) {
            const int r = g_slip == 5 ? radius + 1 - t : t;
            const int lo = clamp_index(mirror_low(c - r), last), hi = clamp_index(mirror_high(c + r, last), last);
            const float pair = line[lo * stride] + line[hi * stride];
            if (fma) acc = std::fmaf(w[r], pair, acc);
            else acc = acc + w[r] * pair;
        }
        dst[(size_t)v] = acc;
    }
}

void gaussian_blur(const std::vector<float>& src, Layer& L, int fma) {
    float unit_max = L.unit[0] > L.unit[1] ? L.unit[0] : L.unit[1];
    unit_max = unit_max > L.unit[2] ? unit_max : L.unit[2];
    float sigma = L.sigma;
    int kernel_radius;
    if (sigma > 0) {
        kernel_radius = ceilf(3.f * sigma) > 1 ? (int)ceilf(3.f * sigma) : 1;
    } else {
        sigma = 0.f;
        kernel_radius = 1;
    }
    for (int a = 0; a < 3; a++) {
        L.radius[a] = (int)(kernel_radius * floorf(unit_max / L.unit[a] + 0.5f));
        L.weight[a] = make_weights(sigma, L.radius[a]);
    }
    std::vector<float> buffer(L.vol.size());
    blur_axis(src, L.vol, L.dim, 0, L.weight[0], L.radius[0], fma);
    blur_axis(L.vol, buffer, L.dim, 1, L.weight[1], L.radius[1], fma);
    blur_axis(buffer, L.vol, L.dim, 2, L.weight[2], L.radius[2], fma);
}

void down_sampling(const Layer& src, Layer& dst) {
    const long sx = src.dim[0], sy = src.dim[1], dx = dst.dim[0], dy = dst.dim[1], dz = dst.dim[2];
#pragma omp parallel for
    for (long i = 0; i < dz; i++)
        for (long j = 0; j < dy; j++)
            for (long k = 0; k < dx; k++) dst.vol[(size_t)((i * dy + j) * dx + k)] = src.vol[(size_t)(((i * 2) * sy + j * 2) * sx + k * 2)];
}

}  // namespace

extern "C" {

void oc_twin_sift3d_set_slip(int slip) { g_slip = slip; }

void* oc_twin_sift3d_build(const float* volume, int dim_x, int dim_y, int dim_z, int n_octave_layers, int min_dimension, float alpha, float sigma_source,
                           float sigma_base, float unit_x, float unit_y, float unit_z, int fma) {
    Twin* T = new Twin;
    T->n_octave_layers = n_octave_layers;
    T->alpha = alpha;
    int dim_min = dim_x < dim_y ? dim_x : dim_y;
    dim_min = dim_min < dim_z ? dim_min : dim_z;
    T->n_octave = (int)(floorf(log2f((float)dim_min) - log2f((float)min_dimension)) + 1);
    T->n_octave = T->n_octave > 0 ? T->n_octave : 1;
    const int layer_per_octave = n_octave_layers + 3, layer_number = T->n_octave * layer_per_octave;
    std::vector<Layer>& g = T->gauss;
    g.resize((size_t)layer_number);
    int len[3] = {dim_x, dim_y, dim_z};
    float unit[3] = {unit_x, unit_y, unit_z};
    const float kappa = powf(2.f, 1.f / n_octave_layers);
    for (int i = 0; i < layer_number; i++) {
        Layer& L = g[(size_t)i];
        L.octave = i / layer_per_octave;
        const int layer_in_octave = i % layer_per_octave;
        L.sigma = 0.f;
        L.max_abs = -1.f;
        L.radius[0] = L.radius[1] = L.radius[2] = 0;
        if (i == 0) {
            L.scale = 1.f / kappa * sigma_base;
            L.sigma = sqrtf(L.scale * L.scale - sigma_source * sigma_source);
        } else if (layer_in_octave == 0) {
            for (int a = 0; a < 3; a++) {
                len[a] /= 2;
                unit[a] *= 2;
            }
            L.scale = g[(size_t)((L.octave - 1) * layer_per_octave + n_octave_layers)].scale;
        } else {
            L.scale = kappa * g[(size_t)i - 1].scale;
            L.sigma = sqrtf(kappa * kappa - 1.f) * g[(size_t)layer_in_octave - 1].scale;
        }
        for (int a = 0; a < 3; a++) {
            L.dim[a] = len[a];
            L.unit[a] = unit[a];
        }
        L.vol.resize((size_t)len[0] * len[1] * len[2]);
    }
    std::vector<float> input(volume, volume + (size_t)dim_x * dim_y * dim_z);
    gaussian_blur(input, g[0], fma);
    for (int i = 1; i < layer_number; i++) {
        if (i % layer_per_octave == 0) down_sampling(g[(size_t)i - 3], g[(size_t)i]);
        else gaussian_blur(g[(size_t)i - 1].vol, g[(size_t)i], fma);
    }
    const int dog_per_octave = n_octave_layers + 2;
    T->dog.resize((size_t)(T->n_octave * dog_per_octave));
    for (int m = 0; m < T->n_octave; m++)
        for (int n = 0; n < dog_per_octave; n++) {
            const Layer &a = g[(size_t)(m * layer_per_octave + n)], &b = g[(size_t)(m * layer_per_octave + n + 1)];
            Layer& D = T->dog[(size_t)(m * dog_per_octave + n)];
            std::memcpy(D.dim, a.dim, sizeof D.dim);
            std::memcpy(D.unit, a.unit, sizeof D.unit);
            D.octave = m;
            D.scale = a.scale;
            D.sigma = 0.f;
            D.radius[0] = D.radius[1] = D.radius[2] = 0;
            D.vol.resize(a.vol.size());
            D.max_abs = -1.f;
            for (size_t v = 0; v < a.vol.size(); v++) {
                D.vol[v] = b.vol[v] - a.vol[v];
                const float dog_abs = fabsf(D.vol[v]);
                D.max_abs = D.max_abs < dog_abs ? dog_abs : D.max_abs;
            }
        }
    return T;
}

void oc_twin_sift3d_free(void* h) { delete static_cast<Twin*>(h); }

int oc_twin_sift3d_layers(const void* h, int pyramid) {
    const Twin* T = static_cast<const Twin*>(h);
    return (int)(pyramid == 0 ? T->gauss.size() : T->dog.size());
}

int oc_twin_sift3d_octaves(const void* h) { return static_cast<const Twin*>(h)->n_octave; }

const float* oc_twin_sift3d_info(const void* h, int pyramid, int index, int* dims, float* units, int* octave, float* scale, float* sigma, float* max_abs,
                                 int* radius) {
    const Twin* T = static_cast<const Twin*>(h);
    const Layer& L = pyramid == 0 ? T->gauss[(size_t)index] : T->dog[(size_t)index];
    for (int a = 0; a < 3; a++) {
        dims[a] = L.dim[a];
        units[a] = L.unit[a];
        radius[a] = L.radius[a];
    }
    *octave = L.octave;
    *scale = L.scale;
    *sigma = L.sigma;
    *max_abs = L.max_abs;
    return L.vol.data();
}

// the weights of one axis of a blurred Gaussian layer: radius + 1 floats into out (room for 64)
int oc_twin_sift3d_weights(const void* h, int index, int axis, float* out) {
    const Layer& L = static_cast<const Twin*>(h)->gauss[(size_t)index];
    for (size_t i = 0; i < L.weight[axis].size() && i < 64; i++) out[i] = L.weight[axis][i];
    return (int)L.weight[axis].size();
}

// the scan of detectExtrema; returns the number of candidates, writes at most `capacity` of them
long oc_twin_sift3d_detect(const void* h, Candidate* out, long capacity) {
    const Twin* T = static_cast<const Twin*>(h);
    const int border = g_slip == 3 ? 0 : 1;
    long count = 0;
    for (int m = 0; m < T->n_octave; m++)
        for (int n = 1; n < T->n_octave_layers + 1; n++) {
            const int layer_idx = m * (T->n_octave_layers + 2) + n;
            const Layer& D = T->dog[(size_t)layer_idx];
            const float *here = D.vol.data(), *below = T->dog[(size_t)layer_idx - 1].vol.data(), *above = T->dog[(size_t)layer_idx + 1].vol.data();
            const long nx = D.dim[0], ny = D.dim[1], nz = D.dim[2];
            for (long i = border; i < nz - border; i++)
                for (long j = border; j < ny - border; j++)
                    for (long k = border; k < nx - border; k++) {
                        const long at = (i * ny + j) * nx + k;
                        const float dog_value = here[at];
                        const float threshold = T->alpha * D.max_abs;
                        const bool large = g_slip == 6 ? fabsf(dog_value) > threshold : fabsf(dog_value) >= threshold;
                        if (!large) continue;
                        float nb[8];
                        int count_nb = 0;
                        if (i - 1 >= 0) nb[count_nb++] = here[at - nx * ny];
                        if (i + 1 < nz) nb[count_nb++] = here[at + nx * ny];
                        if (j - 1 >= 0) nb[count_nb++] = here[at - nx];
                        if (j + 1 < ny) nb[count_nb++] = here[at + nx];
                        if (k - 1 >= 0) nb[count_nb++] = here[at - 1];
                        if (k + 1 < nx) nb[count_nb++] = here[at + 1];
                        if (g_slip != 2) {
                            nb[count_nb++] = below[at];
                            nb[count_nb++] = above[at];
                        }
                        bool greater = true, less = true;
                        for (int q = 0; q < count_nb; q++) {
                            greater = greater && (g_slip == 1 ? dog_value >= nb[q] : dog_value > nb[q]);
                            less = less && (g_slip == 1 ? dog_value <= nb[q] : dog_value < nb[q]);
                        }
                        if (greater || less) {
                            if (count < capacity) out[count] = Candidate{(int)k, (int)j, (int)i, m, n, D.scale};
                            count++;
                        }
                    }
        }
    return count;
}

}  // extern "C"

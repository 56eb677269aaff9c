// sift3d_features_twin.cpp -- CPU restatement of the arithmetic contract of SIFT3D's orientation and descriptor stages
// (opencorr_amd/csrc/sift3d_features.hip, include/opencorr_hip.h "SIFT3D's orientation and descriptor stages"), written the way
// the reference writes them: SIFT3D::assignOrientation (src/oc_sift.cpp:849-1049), constructDescriptor (:1051-1249),
// cartisan2Barycentric (:579-623) on the icosahedron of prepare() (:212-231), as plain sequential loops over the Gaussian layers the
// scale-space twin (sift3d_twin.cpp) made.  It computes every Gaussian weight inline (no table) and shares one text with the
// library: the Jacobi iteration of opencorr_amd/csrc/sift3d_jacobi.h, which the contract names as the eigen-decomposition.
//
// mode 0: the contract -- every voxel term goes to the power-of-two grid (llrintf(ldexpf(t, -q))) and is added as a 64-bit integer.
// mode 1: the reference's accumulation -- sequential float32 `+=` in its loop order.  Used only to measure
//         (tests/test_sift3d_features_cpu.py: its distance to the float64 model sets the bars).
//
// Build: g++ -O2 -ffp-contract=off -fopenmp (tests/sift3d_features_twin.py).  OpenMP runs over keypoints only.
//
// oc_twin_features_set_slip plants ONE deliberate error: 1 = floor for the cube index (:1185-1187), 2 = `/ unit_y` at :870,
// 3 = the last tile that meets the ray wins, 4 = `<` for `<=` in both sphere tests, 5 = no truncation (:1232-1235),
// 6 = the rotation matrix transposed (:1020-1028), 7 = eigenvalues sorted ascending (:970).
#include <cfloat>
#include <cmath>
#include <cstring>

#include "../../opencorr_amd/csrc/sift3d_jacobi.h"

namespace {

int g_slip = 0;
const int IMG_BORDER = 1;

struct Point3D {
    float x, y, z;
    Point3D() : x(0.f), y(0.f), z(0.f) {}
    Point3D(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    float vectorNorm() const { return sqrtf(x * x + y * y + z * z); }
};
inline Point3D operator+(Point3D a, Point3D b) { return Point3D(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Point3D operator-(Point3D a, Point3D b) { return a + Point3D(-b.x, -b.y, -b.z); }
inline Point3D operator*(float f, Point3D p) { return Point3D(f * p.x, f * p.y, f * p.z); }
inline Point3D operator*(Point3D p, float f) { return f * p; }
inline float operator*(Point3D a, Point3D b) { return (a.x * b.x + a.y * b.y + a.z * b.z); }                                        // dot
inline Point3D operator/(Point3D a, Point3D b) { return Point3D((a.y * b.z - a.z * b.y), (a.z * b.x - a.x * b.z), (a.x * b.y - a.y * b.x)); }  // cross

struct TriangleTile {
    Point3D vertices[3];
    int vertex_idx[3];
};

#define TILE(ax, ay, az, ai, bx, by, bz, bi, cx, cy, cz, ci) {{Point3D(ax, ay, az), Point3D(bx, by, bz), Point3D(cx, cy, cz)}, {ai, bi, ci}}
const TriangleTile icosahedron[20] = {
    TILE(0.000000f, -0.525731f, 0.850651f, 1, 0.000000f, 0.525731f, 0.850651f, 0, 0.850651f, 0.000000f, 0.525731f, 8),
    TILE(0.850651f, 0.000000f, 0.525731f, 8, 0.000000f, 0.525731f, 0.850651f, 0, 0.525731f, 0.850651f, 0.000000f, 4),
    TILE(0.525731f, 0.850651f, 0.000000f, 4, 0.000000f, 0.525731f, 0.850651f, 0, -0.525731f, 0.850651f, 0.000000f, 5),
    TILE(-0.525731f, 0.850651f, 0.000000f, 5, 0.000000f, 0.525731f, 0.850651f, 0, -0.850651f, 0.000000f, 0.525731f, 9),
    TILE(-0.850651f, 0.000000f, 0.525731f, 9, 0.000000f, 0.525731f, 0.850651f, 0, 0.000000f, -0.525731f, 0.850651f, 1),
    TILE(0.525731f, -0.850651f, 0.000000f, 6, 0.000000f, -0.525731f, 0.850651f, 1, 0.850651f, 0.000000f, 0.525731f, 8),
    TILE(0.525731f, -0.850651f, 0.000000f, 6, 0.850651f, 0.000000f, 0.525731f, 8, 0.850651f, 0.000000f, -0.525731f, 10),
    TILE(0.850651f, 0.000000f, -0.525731f, 10, 0.850651f, 0.000000f, 0.525731f, 8, 0.525731f, 0.850651f, 0.000000f, 4),
    TILE(0.850651f, 0.000000f, -0.525731f, 10, 0.525731f, 0.850651f, 0.000000f, 4, 0.000000f, 0.525731f, -0.850651f, 2),
    TILE(0.000000f, 0.525731f, -0.850651f, 2, 0.525731f, 0.850651f, 0.000000f, 4, -0.525731f, 0.850651f, 0.000000f, 5),
    TILE(0.000000f, 0.525731f, -0.850651f, 2, -0.525731f, 0.850651f, 0.000000f, 5, -0.850651f, 0.000000f, -0.525731f, 11),
    TILE(-0.850651f, 0.000000f, -0.525731f, 11, -0.525731f, 0.850651f, 0.000000f, 5, -0.850651f, 0.000000f, 0.525731f, 9),
    TILE(-0.850651f, 0.000000f, -0.525731f, 11, -0.850651f, 0.000000f, 0.525731f, 9, -0.525731f, -0.850651f, 0.000000f, 7),
    TILE(-0.525731f, -0.850651f, 0.000000f, 7, -0.850651f, 0.000000f, 0.525731f, 9, 0.000000f, -0.525731f, 0.850651f, 1),
    TILE(-0.525731f, -0.850651f, 0.000000f, 7, 0.000000f, -0.525731f, 0.850651f, 1, 0.525731f, -0.850651f, 0.000000f, 6),
    TILE(0.525731f, -0.850651f, 0.000000f, 6, 0.000000f, -0.525731f, -0.850651f, 3, -0.525731f, -0.850651f, 0.000000f, 7),
    TILE(-0.525731f, -0.850651f, 0.000000f, 7, 0.000000f, -0.525731f, -0.850651f, 3, -0.850651f, 0.000000f, -0.525731f, 11),
    TILE(-0.850651f, 0.000000f, -0.525731f, 11, 0.000000f, -0.525731f, -0.850651f, 3, 0.000000f, 0.525731f, -0.850651f, 2),
    TILE(0.000000f, 0.525731f, -0.850651f, 2, 0.000000f, -0.525731f, -0.850651f, 3, 0.850651f, 0.000000f, -0.525731f, 10),
    TILE(0.850651f, 0.000000f, -0.525731f, 10, 0.000000f, -0.525731f, -0.850651f, 3, 0.525731f, -0.850651f, 0.000000f, 6),
};

int cartisan2Barycentric(const Point3D& cart_coor, Point3D& bary_coor, const TriangleTile& triangle) {
    Point3D e1, e2, t, p, q;
    float k;
    e1 = triangle.vertices[1] - triangle.vertices[0];
    e2 = triangle.vertices[2] - triangle.vertices[0];
    t = -1.f * triangle.vertices[0];
    p = cart_coor / e2;
    q = t / e1;
    float det = e1 * p;
    if (fabsf(det) < FLT_EPSILON * 10.f) return -1;
    float det_inv = 1.f / det;
    bary_coor.z = det_inv * (cart_coor * q);
    bary_coor.y = det_inv * (p * t);
    bary_coor.x = 1.f - bary_coor.y - bary_coor.z;
    k = det_inv * (q * e2);
    if (k < 0) return -1;
    if (bary_coor.x < -FLT_EPSILON * 10.f || bary_coor.y < -FLT_EPSILON * 10.f || bary_coor.z < -FLT_EPSILON * 10.f) return -1;
    Point3D residual = k * cart_coor - bary_coor.x * triangle.vertices[0] - bary_coor.y * triangle.vertices[1] - bary_coor.z * triangle.vertices[2];
    if (residual.vectorNorm() > FLT_EPSILON * 10.f) return -1;
    return 1;
}

struct Candidate {
    int x, y, z, octave, layer;
    float scale;
};

struct Keypoint {
    float coor_layer[3], coor_img[3];
    int octave, layer;
    float scale;
    float rotation_matrix[9];
};

struct Layer {
    const float* vol;  // [z][y][x]
    int dim_xyz[3];
    float unit_xyz[3];
    float at(int i, int j, int k) const { return vol[((size_t)i * dim_xyz[1] + j) * dim_xyz[0] + k]; }
};

struct EigenMatrix {
    float eigen_value;
    float eigen_vector[3];
};

// a sum of voxel terms: the contract's 64-bit integer on the grid 2^quantum, or the reference's float
struct Sum {
    long long exact = 0;
    float sequential = 0.f;
    void add(float term, int quantum, int mode) {
        if (mode == 0) exact += llrintf(ldexpf(term, -quantum));
        else sequential += term;
    }
    float as_float(int quantum, int mode) const { return mode == 0 ? ldexpf((float)exact, quantum) : sequential; }
    double as_double(int quantum, int mode) const { return mode == 0 ? ldexp((double)exact, quantum) : (double)sequential; }
};

Layer layer_of(const float* const* vols, const int* dims, const float* units, int g_idx) {
    Layer L;
    L.vol = vols[g_idx];
    for (int a = 0; a < 3; a++) {
        L.dim_xyz[a] = dims[3 * g_idx + a];
        L.unit_xyz[a] = units[3 * g_idx + a];
    }
    return L;
}

bool in_sphere(float norm, float radius) { return g_slip == 4 ? norm < radius : norm <= radius; }

}  // namespace

extern "C" {

void oc_twin_features_set_slip(int slip) { g_slip = slip; }

// the smallest integer E with 2^E >= 2 A / min(unit) (0 for A = 0); -1000 when A is not finite
int oc_twin_features_grid_exponent(float max_abs, float unit_min) {
    if (!std::isfinite(max_abs)) return -1000;
    if (max_abs == 0.f) return 0;
    const double bound = 2.0 * (double)max_abs / (double)unit_min;
    int E = 0;
    while (ldexp(1.0, E) < bound) E++;
    while (ldexp(1.0, E - 1) >= bound) E--;
    return E;
}

// `0.5 * (a - b) / unit` as the reference writes it (in double, rounded to float on assignment) and as the kernels compute it
void oc_twin_features_gradient_forms(float a, float b, float unit, float* in_double, float* in_float) {
    *in_double = 0.5 * (a - b) / unit;
    *in_float = (0.5f * (a - b)) / unit;
}

// assignOrientation for n candidates.  status[m]: 0 accepted, 1 gradient threshold, 2 eigenvalues, 3 angle; sums[9 m ...]: d_x d_y
// d_z, tensor xx xy xz yy yz zz; slots[m]: the keypoint record (rotation matrix all zero unless accepted)
void oc_twin_features_orient(const float* const* vols, const int* dims, const float* units, int n_octave_layers, const Candidate* candidates, long n,
                             int E, float beta, float gamma, float gradient_threshold, int mode, int* status, float* sums, Keypoint* slots) {
#pragma omp parallel for schedule(dynamic)
    for (long m = 0; m < n; m++) {
        const Candidate& kp = candidates[m];
        const int g_idx = kp.layer + kp.octave * (n_octave_layers + 3);
        const Layer L = layer_of(vols, dims, units, g_idx);
        const Point3D coor_layer((float)kp.x, (float)kp.y, (float)kp.z);

        float sigma_w = 1.5f * kp.scale;
        float window_radius = 3.f * sigma_w;

        int x_min = (int)floorf(coor_layer.x - window_radius / L.unit_xyz[0]);
        x_min = x_min > IMG_BORDER ? x_min : IMG_BORDER;
        int x_max = (int)ceilf(coor_layer.x + window_radius / L.unit_xyz[0]);
        x_max = x_max < L.dim_xyz[0] - IMG_BORDER ? x_max : L.dim_xyz[0] - IMG_BORDER;
        int y_min = (int)floorf(coor_layer.y - window_radius / L.unit_xyz[1]);
        y_min = y_min > IMG_BORDER ? y_min : IMG_BORDER;
        int y_max = g_slip == 2 ? (int)ceilf(coor_layer.y + window_radius / L.unit_xyz[1]) : (int)ceilf(coor_layer.y + window_radius * L.unit_xyz[1]);
        y_max = y_max < L.dim_xyz[1] - IMG_BORDER ? y_max : L.dim_xyz[1] - IMG_BORDER;
        int z_min = (int)floorf(coor_layer.z - window_radius / L.unit_xyz[2]);
        z_min = z_min > IMG_BORDER ? z_min : IMG_BORDER;
        int z_max = (int)ceilf(coor_layer.z + window_radius / L.unit_xyz[2]);
        z_max = z_max < L.dim_xyz[2] - IMG_BORDER ? z_max : L.dim_xyz[2] - IMG_BORDER;

        Sum d_mat[3], tensor[6];
        const int q_d = E - 40, q_t = 2 * E - 40;
        for (int i = z_min; i < z_max; i++)
            for (int j = y_min; j < y_max; j++)
                for (int k = x_min; k < x_max; k++) {
                    Point3D img_coor((float)k, (float)j, (float)i);
                    Point3D phys_corr;
                    phys_corr.x = (img_coor.x - coor_layer.x) * L.unit_xyz[0];
                    phys_corr.y = (img_coor.y - coor_layer.y) * L.unit_xyz[1];
                    phys_corr.z = (img_coor.z - coor_layer.z) * L.unit_xyz[2];
                    if (in_sphere(phys_corr.vectorNorm(), window_radius)) {
                        const float ratio = phys_corr.vectorNorm() / sigma_w;
                        float cur_weight = expf(-0.5f * (ratio * ratio));
                        float grad_x = (0.5f * (L.at(i, j, k + 1) - L.at(i, j, k - 1))) / L.unit_xyz[0];
                        float grad_y = (0.5f * (L.at(i, j + 1, k) - L.at(i, j - 1, k))) / L.unit_xyz[1];
                        float grad_z = (0.5f * (L.at(i + 1, j, k) - L.at(i - 1, j, k))) / L.unit_xyz[2];
                        tensor[0].add(grad_x * grad_x * cur_weight, q_t, mode);
                        tensor[1].add(grad_x * grad_y * cur_weight, q_t, mode);
                        tensor[2].add(grad_x * grad_z * cur_weight, q_t, mode);
                        tensor[3].add(grad_y * grad_y * cur_weight, q_t, mode);
                        tensor[4].add(grad_y * grad_z * cur_weight, q_t, mode);
                        tensor[5].add(grad_z * grad_z * cur_weight, q_t, mode);
                        d_mat[0].add(grad_x * cur_weight, q_d, mode);
                        d_mat[1].add(grad_y * cur_weight, q_d, mode);
                        d_mat[2].add(grad_z * cur_weight, q_d, mode);
                    }
                }
        const float d_mat_x = d_mat[0].as_float(q_d, mode), d_mat_y = d_mat[1].as_float(q_d, mode), d_mat_z = d_mat[2].as_float(q_d, mode);
        float* s = sums + 9 * m;
        s[0] = d_mat_x, s[1] = d_mat_y, s[2] = d_mat_z;
        for (int t = 0; t < 6; t++) s[3 + t] = tensor[t].as_float(q_t, mode);

        Keypoint& out = slots[m];
        std::memset(&out, 0, sizeof out);
        out.coor_layer[0] = coor_layer.x, out.coor_layer[1] = coor_layer.y, out.coor_layer[2] = coor_layer.z;
        float scale_factor = powf(2.f, (float)kp.octave);
        out.coor_img[0] = coor_layer.x * scale_factor, out.coor_img[1] = coor_layer.y * scale_factor, out.coor_img[2] = coor_layer.z * scale_factor;
        out.octave = kp.octave, out.layer = kp.layer, out.scale = kp.scale;

        if ((d_mat_x * d_mat_x + d_mat_y * d_mat_y + d_mat_z * d_mat_z) < gradient_threshold) {
            status[m] = 1;
            continue;
        }
        double a[6], value[3], vector[3][3];
        for (int t = 0; t < 6; t++) a[t] = tensor[t].as_double(q_t, mode);
        ochip_sift::sift3d_jacobi(a, value, vector);
        EigenMatrix e_m[3];
        for (int t = 0; t < 3; t++) {
            e_m[t].eigen_value = (float)value[t];
            for (int c = 0; c < 3; c++) e_m[t].eigen_vector[c] = (float)vector[t][c];
        }
        for (int t = 1; t < 3; t++)  // std::sort by `>` (:970): three elements, an insertion sort
            for (int u = t; u > 0 && (g_slip == 7 ? e_m[u].eigen_value < e_m[u - 1].eigen_value : e_m[u].eigen_value > e_m[u - 1].eigen_value); u--) {
                EigenMatrix tmp = e_m[u];
                e_m[u] = e_m[u - 1];
                e_m[u - 1] = tmp;
            }
        if ((e_m[1].eigen_value / e_m[0].eigen_value) > beta || (e_m[2].eigen_value / e_m[1].eigen_value) > beta ||
            fabsf(e_m[0].eigen_value - e_m[1].eigen_value) < FLT_EPSILON || fabsf(e_m[1].eigen_value - e_m[2].eigen_value) < FLT_EPSILON ||
            fabsf(e_m[2].eigen_value - e_m[0].eigen_value) < FLT_EPSILON) {
            status[m] = 2;
            continue;
        }
        Point3D d_vec(d_mat_x, d_mat_y, d_mat_z);
        float cos_phi = FLT_MAX;
        for (int i = 0; i < 2; i++) {
            Point3D q_vec(e_m[i].eigen_vector[0], e_m[i].eigen_vector[1], e_m[i].eigen_vector[2]);
            float q_d_dot = q_vec * d_vec;
            float abs_cos_phi = fabsf(q_d_dot / (q_vec.vectorNorm() * d_vec.vectorNorm()));
            cos_phi = cos_phi < abs_cos_phi ? cos_phi : abs_cos_phi;
            float sgn = q_d_dot > 0 ? 1.f : -1.f;
            e_m[i].eigen_vector[0] *= sgn;
            e_m[i].eigen_vector[1] *= sgn;
            e_m[i].eigen_vector[2] *= sgn;
        }
        if (cos_phi < gamma) {
            status[m] = 3;
            continue;
        }
        Point3D r1(e_m[0].eigen_vector[0], e_m[0].eigen_vector[1], e_m[0].eigen_vector[2]);
        Point3D r2(e_m[1].eigen_vector[0], e_m[1].eigen_vector[1], e_m[1].eigen_vector[2]);
        Point3D rc = r1 / r2;
        float* R = out.rotation_matrix;
        if (g_slip == 6) {
            R[0] = r1.x, R[1] = r2.x, R[2] = rc.x, R[3] = r1.y, R[4] = r2.y, R[5] = rc.y, R[6] = r1.z, R[7] = r2.z, R[8] = rc.z;
        } else {
            R[0] = r1.x, R[3] = r2.x, R[6] = rc.x, R[1] = r1.y, R[4] = r2.y, R[7] = rc.y, R[2] = r1.z, R[5] = r2.z, R[8] = rc.z;
        }
        status[m] = 0;
    }
}

// constructDescriptor for n keypoints: descriptor[768 m ...]
void oc_twin_features_describe(const float* const* vols, const int* dims, const float* units, int n_octave_layers, const Keypoint* kp_queue, long n, int E,
                               float truncate_threshold, int mode, float* descriptor) {
    float sqrt_2 = sqrtf(2.f);
#pragma omp parallel for schedule(dynamic)
    for (long m = 0; m < n; m++) {
        const Keypoint& kp = kp_queue[m];
        const int g_idx = kp.layer + kp.octave * (n_octave_layers + 3);
        const Layer L = layer_of(vols, dims, units, g_idx);
        const Point3D coor_layer(kp.coor_layer[0], kp.coor_layer[1], kp.coor_layer[2]);
        const float* R = kp.rotation_matrix;
        float* desc = descriptor + 768 * m;
        Sum bins[768];
        const int quantum = E - 39;

        float sigma = 5.f * sqrt_2 * kp.scale;
        float sphere_radius = 2.f * sigma;
        float cube_radius = sphere_radius / sqrt_2;

        int x_min = (int)floorf(coor_layer.x - sphere_radius / L.unit_xyz[0]);
        x_min = x_min > IMG_BORDER ? x_min : IMG_BORDER;
        int x_max = (int)ceilf(coor_layer.x + sphere_radius / L.unit_xyz[0]);
        x_max = x_max < L.dim_xyz[0] - IMG_BORDER ? x_max : L.dim_xyz[0] - IMG_BORDER;
        int y_min = (int)floorf(coor_layer.y - sphere_radius / L.unit_xyz[1]);
        y_min = y_min > IMG_BORDER ? y_min : IMG_BORDER;
        int y_max = (int)ceilf(coor_layer.y + sphere_radius / L.unit_xyz[1]);
        y_max = y_max < L.dim_xyz[1] - IMG_BORDER ? y_max : L.dim_xyz[1] - IMG_BORDER;
        int z_min = (int)floorf(coor_layer.z - sphere_radius / L.unit_xyz[2]);
        z_min = z_min > IMG_BORDER ? z_min : IMG_BORDER;
        int z_max = (int)ceilf(coor_layer.z + sphere_radius / L.unit_xyz[2]);
        z_max = z_max < L.dim_xyz[2] - IMG_BORDER ? z_max : L.dim_xyz[2] - IMG_BORDER;

        for (int i = z_min; i < z_max; i++)
            for (int j = y_min; j < y_max; j++)
                for (int k = x_min; k < x_max; k++) {
                    Point3D img_coor((float)k, (float)j, (float)i);
                    Point3D phys_coor = img_coor - coor_layer;
                    phys_coor.x *= L.unit_xyz[0];
                    phys_coor.y *= L.unit_xyz[1];
                    phys_coor.z *= L.unit_xyz[2];
                    float cur_distance = phys_coor.vectorNorm();
                    if (!in_sphere(cur_distance, sphere_radius)) continue;

                    Point3D rotated_coor;
                    rotated_coor.x = R[0] * phys_coor.x + R[1] * phys_coor.y + R[2] * phys_coor.z;
                    rotated_coor.y = R[3] * phys_coor.x + R[4] * phys_coor.y + R[5] * phys_coor.z;
                    rotated_coor.z = R[6] * phys_coor.x + R[7] * phys_coor.y + R[8] * phys_coor.z;

                    Point3D subregion_coor;
                    subregion_coor.x = 2 * (rotated_coor.x + cube_radius) / cube_radius;
                    subregion_coor.y = 2 * (rotated_coor.y + cube_radius) / cube_radius;
                    subregion_coor.z = 2 * (rotated_coor.z + cube_radius) / cube_radius;
                    subregion_coor.x -= 0.5f;
                    subregion_coor.y -= 0.5f;
                    subregion_coor.z -= 0.5f;
                    if (subregion_coor.x <= -0.5f || subregion_coor.y <= -0.5f || subregion_coor.z <= -0.5f || subregion_coor.x >= 3.5f ||
                        subregion_coor.y >= 3.5f || subregion_coor.z >= 3.5f)
                        continue;

                    const double ratio = (double)(cur_distance / sigma);
                    float cur_weight = (float)exp(-0.5 * (ratio * ratio));
                    Point3D gradient;
                    gradient.x = (0.5f * (L.at(i, j, k + 1) - L.at(i, j, k - 1))) / L.unit_xyz[0];
                    gradient.y = (0.5f * (L.at(i, j + 1, k) - L.at(i, j - 1, k))) / L.unit_xyz[1];
                    gradient.z = (0.5f * (L.at(i + 1, j, k) - L.at(i - 1, j, k))) / L.unit_xyz[2];
                    gradient = gradient * cur_weight;

                    Point3D rotated_gradient;
                    rotated_gradient.x = R[0] * gradient.x + R[1] * gradient.y + R[2] * gradient.z;
                    rotated_gradient.y = R[3] * gradient.x + R[4] * gradient.y + R[5] * gradient.z;
                    rotated_gradient.z = R[6] * gradient.x + R[7] * gradient.y + R[8] * gradient.z;

                    float gradient_magnitude = rotated_gradient.vectorNorm();
                    if (gradient_magnitude * gradient_magnitude < FLT_EPSILON * 10.f) continue;

                    int intersect_idx = -1;
                    Point3D bary_coor;
                    for (int t = 0; t < 20; t++) {
                        Point3D trial;
                        if (cartisan2Barycentric(rotated_gradient, trial, icosahedron[t]) > 0) {
                            intersect_idx = t;
                            bary_coor = trial;
                            if (g_slip != 3) break;
                        }
                    }
                    if (intersect_idx < 0) continue;

                    Point3D decimal_coor;
                    decimal_coor.x = subregion_coor.x - floorf(subregion_coor.x);
                    decimal_coor.y = subregion_coor.y - floorf(subregion_coor.y);
                    decimal_coor.z = subregion_coor.z - floorf(subregion_coor.z);

                    for (int dz = 0; dz < 2; dz++)
                        for (int dy = 0; dy < 2; dy++)
                            for (int dx = 0; dx < 2; dx++) {
                                int local_x = (g_slip == 1 ? (int)floorf(subregion_coor.x) : (int)subregion_coor.x) + dx;
                                int local_y = (g_slip == 1 ? (int)floorf(subregion_coor.y) : (int)subregion_coor.y) + dy;
                                int local_z = (g_slip == 1 ? (int)floorf(subregion_coor.z) : (int)subregion_coor.z) + dz;
                                if (local_x < 0 || local_y < 0 || local_z < 0 || local_x >= 4 || local_y >= 4 || local_z >= 4) continue;
                                int cube_idx = local_x + local_y * 4 + local_z * 16;
                                float interp_weight = ((dx == 0) ? (1.f - decimal_coor.x) : decimal_coor.x) * ((dy == 0) ? (1.f - decimal_coor.y) : decimal_coor.y) *
                                                      ((dz == 0) ? (1.f - decimal_coor.z) : decimal_coor.z);
                                int offset_v1 = cube_idx * 12 + icosahedron[intersect_idx].vertex_idx[0];
                                int offset_v2 = cube_idx * 12 + icosahedron[intersect_idx].vertex_idx[1];
                                int offset_v3 = cube_idx * 12 + icosahedron[intersect_idx].vertex_idx[2];
                                bins[offset_v1].add(gradient_magnitude * interp_weight * bary_coor.x, quantum, mode);
                                bins[offset_v2].add(gradient_magnitude * interp_weight * bary_coor.y, quantum, mode);
                                bins[offset_v3].add(gradient_magnitude * interp_weight * bary_coor.z, quantum, mode);
                            }
                }
        for (int i = 0; i < 768; i++) desc[i] = bins[i].as_float(quantum, mode);

        float sq_sum = 0;
        for (int i = 0; i < 768; i++) sq_sum += desc[i] * desc[i];
        float inv_norm = 1.f / (sqrtf(sq_sum) + FLT_EPSILON);
        for (int i = 0; i < 768; i++) desc[i] *= inv_norm;
        if (g_slip != 5)
            for (int i = 0; i < 768; i++) desc[i] = (desc[i] < truncate_threshold) ? desc[i] : truncate_threshold;
        sq_sum = 0;
        for (int i = 0; i < 768; i++) sq_sum += desc[i] * desc[i];
        inv_norm = 1.f / (sqrtf(sq_sum) + FLT_EPSILON);
        for (int i = 0; i < 768; i++) desc[i] *= inv_norm;
    }
}

}  // extern "C"

// sift3d_features.hip -- SIFT3D's orientation and descriptor stages (SIFT3D::assignOrientation, constructDescriptor;
// src/oc_sift.cpp:849-1049, 1051-1249) on the Gaussian pyramid sift3d.hip leaves on the device.
//
// Contract:    per voxel the reference's float32 expressions in its order, every operation rounding on its own (the file is built
//              with -ffp-contract=off); `0.5 * (a - b) / unit` of :905-907 / :1131-1133 as (0.5f * (a - b)) / unit, which gives the
//              double expression's bits.  The Gaussian weight and the sphere test come from the host's table
//              (host/sift3d_feature_plan.h), never from device expf.  Sums over voxels are exact: every term goes to the grid of
//              that header (__float2ll_rn(ldexpf(term, -q))) and is added as a 64-bit integer, so no result depends on the order,
//              the launch shape or the run.  The eigen-decomposition is sift3d_jacobi.h; everything after it is the reference's
//              float32 code as written.
// Orientation: one wave per candidate; the window's voxels go round the 64 lanes (x fastest), nine int64 partials per lane, a
//              shuffle reduction, and lane 0 finishes.  Accepted records are compacted in candidate order by count / scan / fill.
// Descriptor:  one workgroup of 256 per keypoint, 768 int64 bins in LDS (6 KB) fed by ds_add_u64; voxels outside the sphere or the
//              inscribed cube leave before the triangle search, which tries only the tiles whose centroid lies within 41.4
//              degrees of the ray (no hit is lost: see kTileCone).  The normalise / truncate / normalise sums (:1219-1247) are one
//              lane's sequential float32 additions, like the reference's.
#include <algorithm>
#include <cfloat>

#include "oc_device.h"
#include "oc_kernels.h"
#include "sift3d_jacobi.h"

namespace ochip {

namespace {

// the icosahedron of SIFT3D::prepare (:212-231): three vertices per tile, then their indices among the 12 directions
__constant__ float kIcosaVertex[20][9] = {
    {0.000000f, -0.525731f, 0.850651f, 0.000000f, 0.525731f, 0.850651f, 0.850651f, 0.000000f, 0.525731f},
    {0.850651f, 0.000000f, 0.525731f, 0.000000f, 0.525731f, 0.850651f, 0.525731f, 0.850651f, 0.000000f},
    {0.525731f, 0.850651f, 0.000000f, 0.000000f, 0.525731f, 0.850651f, -0.525731f, 0.850651f, 0.000000f},
    {-0.525731f, 0.850651f, 0.000000f, 0.000000f, 0.525731f, 0.850651f, -0.850651f, 0.000000f, 0.525731f},
    {-0.850651f, 0.000000f, 0.525731f, 0.000000f, 0.525731f, 0.850651f, 0.000000f, -0.525731f, 0.850651f},
    {0.525731f, -0.850651f, 0.000000f, 0.000000f, -0.525731f, 0.850651f, 0.850651f, 0.000000f, 0.525731f},
    {0.525731f, -0.850651f, 0.000000f, 0.850651f, 0.000000f, 0.525731f, 0.850651f, 0.000000f, -0.525731f},
    {0.850651f, 0.000000f, -0.525731f, 0.850651f, 0.000000f, 0.525731f, 0.525731f, 0.850651f, 0.000000f},
    {0.850651f, 0.000000f, -0.525731f, 0.525731f, 0.850651f, 0.000000f, 0.000000f, 0.525731f, -0.850651f},
    {0.000000f, 0.525731f, -0.850651f, 0.525731f, 0.850651f, 0.000000f, -0.525731f, 0.850651f, 0.000000f},
    {0.000000f, 0.525731f, -0.850651f, -0.525731f, 0.850651f, 0.000000f, -0.850651f, 0.000000f, -0.525731f},
    {-0.850651f, 0.000000f, -0.525731f, -0.525731f, 0.850651f, 0.000000f, -0.850651f, 0.000000f, 0.525731f},
    {-0.850651f, 0.000000f, -0.525731f, -0.850651f, 0.000000f, 0.525731f, -0.525731f, -0.850651f, 0.000000f},
    {-0.525731f, -0.850651f, 0.000000f, -0.850651f, 0.000000f, 0.525731f, 0.000000f, -0.525731f, 0.850651f},
    {-0.525731f, -0.850651f, 0.000000f, 0.000000f, -0.525731f, 0.850651f, 0.525731f, -0.850651f, 0.000000f},
    {0.525731f, -0.850651f, 0.000000f, 0.000000f, -0.525731f, -0.850651f, -0.525731f, -0.850651f, 0.000000f},
    {-0.525731f, -0.850651f, 0.000000f, 0.000000f, -0.525731f, -0.850651f, -0.850651f, 0.000000f, -0.525731f},
    {-0.850651f, 0.000000f, -0.525731f, 0.000000f, -0.525731f, -0.850651f, 0.000000f, 0.525731f, -0.850651f},
    {0.000000f, 0.525731f, -0.850651f, 0.000000f, -0.525731f, -0.850651f, 0.850651f, 0.000000f, -0.525731f},
    {0.850651f, 0.000000f, -0.525731f, 0.000000f, -0.525731f, -0.850651f, 0.525731f, -0.850651f, 0.000000f},
};
__constant__ int kIcosaIndex[20][3] = {{1, 0, 8},  {8, 0, 4},  {4, 0, 5},  {5, 0, 9},   {9, 0, 1},  {6, 1, 8},  {6, 8, 10},
                                       {10, 8, 4}, {10, 4, 2}, {2, 4, 5},  {2, 5, 11},  {11, 5, 9}, {11, 9, 7}, {7, 9, 1},
                                       {7, 1, 6},  {6, 3, 7},  {7, 3, 11}, {11, 3, 2},  {2, 3, 10}, {10, 3, 6}};

__device__ __forceinline__ float sift_norm(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }  // Point3D::vectorNorm

__device__ __forceinline__ long long sift_quantise(float term, int shift) { return __float2ll_rn(ldexpf(term, shift)); }

__device__ __forceinline__ bool sift_names_layer(const SiftFeatureParams& p, int octave, int layer, float scale) {
    if (octave < 0 || octave >= p.n_octave || layer < 1 || layer > p.n_octave_layers) return false;
    return __float_as_uint(scale) == __float_as_uint(p.layers[layer + octave * (p.n_octave_layers + 3)].scale);
}

__global__ __launch_bounds__(256) void sift_max_abs_kernel(const float* __restrict__ v, size_t count, unsigned* __restrict__ max_abs_bits) {
    __shared__ unsigned wave_max[4];
    unsigned m = 0;  // (bit patterns of |v|: they order like the values, every NaN above every number)
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (size_t)gridDim.x * 256) m = max(m, __float_as_uint(v[idx]) & 0x7fffffffu);
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_abs_bits, max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3])));
}

__global__ __launch_bounds__(256) void sift_check_candidates_kernel(const SiftCandidate* __restrict__ list, size_t n, SiftFeatureParams p,
                                                                    unsigned* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const SiftCandidate c = list[i];
    bool ok = sift_names_layer(p, c.octave, c.layer, c.scale);
    if (ok) {
        const SiftFeatureLayer& L = p.layers[c.layer + c.octave * (p.n_octave_layers + 3)];
        ok = c.x >= 0 && c.x < L.dim[0] && c.y >= 0 && c.y < L.dim[1] && c.z >= 0 && c.z < L.dim[2];
    }
    if (!ok) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void sift_check_keypoints_kernel(const SiftKeypoint* __restrict__ list, size_t n, SiftFeatureParams p,
                                                                   unsigned* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const SiftKeypoint k = list[i];
    bool ok = sift_names_layer(p, k.octave, k.layer, k.scale);
    if (ok) {
        const SiftFeatureLayer& L = p.layers[k.layer + k.octave * (p.n_octave_layers + 3)];
        for (int a = 0; a < 3; a++) {
            const float c = k.coor_layer[a];
            ok = ok && c >= 0.f && c <= (float)(L.dim[a] - 1) && c == floorf(c);  // (a NaN fails every comparison)
        }
        for (int t = 0; t < 9; t++) ok = ok && fabsf(k.rotation_matrix[t]) <= 2.f;
    }
    if (!ok) atomicOr(flag, 1u);
}

// the loops of :863-876 / :1066-1079 on one axis, [lo, lo + n), cut to the table's half-extent: beyond it no voxel passes the
// sphere test (host/sift3d_feature_plan.h)
__device__ __forceinline__ void sift_window_axis(float c, float below, float above, int dim, int centre, int half, int& lo, int& n) {
    int mn = (int)floorf(c - below);
    mn = mn > 1 ? mn : 1;
    int mx = (int)ceilf(c + above);
    mx = mx < dim - 1 ? mx : dim - 1;
    mn = max(mn, centre - half);
    mx = min(mx, centre + half + 1);
    lo = mn;
    n = mx > mn ? mx - mn : 0;
}

// everything of :929-1031 after the sums: the verdict and, for an accepted candidate, the rotation matrix
__device__ int sift_orient_finish(const SiftFeatureParams& p, const float* d, const double* tensor, float* rotation) {
    if ((d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < p.gradient_threshold) return 1;
    double value[3], vector[3][3];
    ochip_sift::sift3d_jacobi(tensor, value, vector);
    float ev[3], q[3][3];
    for (int i = 0; i < 3; i++) {
        ev[i] = (float)value[i];
        for (int k = 0; k < 3; k++) q[i][k] = (float)vector[i][k];
    }
    for (int i = 1; i < 3; i++)  // descending (:970, sortByEigenvalue)
        for (int j = i; j > 0 && ev[j] > ev[j - 1]; j--) {
            const float e = ev[j];
            ev[j] = ev[j - 1];
            ev[j - 1] = e;
            for (int k = 0; k < 3; k++) {
                const float t = q[j][k];
                q[j][k] = q[j - 1][k];
                q[j - 1][k] = t;
            }
        }
    if ((ev[1] / ev[0]) > p.beta || (ev[2] / ev[1]) > p.beta || fabsf(ev[0] - ev[1]) < FLT_EPSILON || fabsf(ev[1] - ev[2]) < FLT_EPSILON ||
        fabsf(ev[2] - ev[0]) < FLT_EPSILON)
        return 2;
    float cos_phi = FLT_MAX;
    const float d_norm = sift_norm(d[0], d[1], d[2]);
    for (int i = 0; i < 2; i++) {
        const float q_d = q[i][0] * d[0] + q[i][1] * d[1] + q[i][2] * d[2];
        const float abs_cos_phi = fabsf(q_d / (sift_norm(q[i][0], q[i][1], q[i][2]) * d_norm));
        cos_phi = cos_phi < abs_cos_phi ? cos_phi : abs_cos_phi;
        const float sgn = q_d > 0 ? 1.f : -1.f;
        for (int k = 0; k < 3; k++) q[i][k] *= sgn;
    }
    if (cos_phi < p.gamma) return 3;
    const float* r1 = q[0];
    const float* r2 = q[1];
    const float rc[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    for (int k = 0; k < 3; k++) {  // :1020-1028
        rotation[k] = r1[k];
        rotation[3 + k] = r2[k];
        rotation[6 + k] = rc[k];
    }
    return 0;
}

__global__ __launch_bounds__(64) void sift_orient_kernel(const SiftCandidate* __restrict__ list, unsigned n, SiftFeatureParams p,
                                                         int* __restrict__ status, float* __restrict__ sums, SiftKeypoint* __restrict__ slots) {
    const unsigned m = blockIdx.x;
    if (m >= n) return;
    const int lane = threadIdx.x;
    const SiftCandidate cand = list[m];
    const SiftFeatureLayer L = p.layers[cand.layer + cand.octave * (p.n_octave_layers + 3)];
    const float c[3] = {(float)cand.x, (float)cand.y, (float)cand.z};
    const int centre[3] = {cand.x, cand.y, cand.z};
    int lo[3], len[3];
    for (int a = 0; a < 3; a++)  // :870 multiplies by unit_y where the other five bounds divide
        sift_window_axis(c[a], L.orient_radius / L.unit[a], a == 1 ? L.orient_radius * L.unit[a] : L.orient_radius / L.unit[a], L.dim[a], centre[a],
                         L.orient_half[a], lo[a], len[a]);
    const unsigned total = (unsigned)len[0] * (unsigned)len[1] * (unsigned)len[2];
    const unsigned plane = (unsigned)len[0] * (unsigned)len[1];
    const size_t row = (size_t)L.dim[0], slab = (size_t)L.dim[0] * L.dim[1];
    const int shift_d = 40 - p.exponent, shift_t = 40 - 2 * p.exponent;
    long long acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned v = lane; v < total; v += 64) {
        const unsigned zi = v / plane, rem = v - zi * plane, yi = rem / (unsigned)len[0], xi = rem - yi * (unsigned)len[0];
        const int k = lo[0] + (int)xi, j = lo[1] + (int)yi, i = lo[2] + (int)zi;
        const int ax = abs(k - centre[0]), ay = abs(j - centre[1]), az = abs(i - centre[2]);
        if (ax > L.orient_half[0] || ay > L.orient_half[1] || az > L.orient_half[2]) continue;  // (beyond the table is beyond the sphere)
        const float w = L.orient[((size_t)az * (L.orient_half[1] + 1) + ay) * (L.orient_half[0] + 1) + ax];
        if (w < 0.f) continue;  // :900
        const float* at = L.vol + ((size_t)i * slab + (size_t)j * row + (size_t)k);
        const float gx = (0.5f * (at[1] - at[-1])) / L.unit[0];
        const float gy = (0.5f * (at[row] - at[-(ptrdiff_t)row])) / L.unit[1];
        const float gz = (0.5f * (at[slab] - at[-(ptrdiff_t)slab])) / L.unit[2];
        acc[0] += sift_quantise(gx * w, shift_d);
        acc[1] += sift_quantise(gy * w, shift_d);
        acc[2] += sift_quantise(gz * w, shift_d);
        acc[3] += sift_quantise(gx * gx * w, shift_t);
        acc[4] += sift_quantise(gx * gy * w, shift_t);
        acc[5] += sift_quantise(gx * gz * w, shift_t);
        acc[6] += sift_quantise(gy * gy * w, shift_t);
        acc[7] += sift_quantise(gy * gz * w, shift_t);
        acc[8] += sift_quantise(gz * gz * w, shift_t);
    }
    for (int t = 0; t < 9; t++)
        for (int off = 32; off > 0; off >>= 1) acc[t] += __shfl_down(acc[t], off);
    if (lane != 0) return;
    float out[9], d[3];
    double tensor[6];
    for (int t = 0; t < 3; t++) out[t] = d[t] = ldexpf(__ll2float_rn(acc[t]), -shift_d);
    for (int t = 0; t < 6; t++) {
        out[3 + t] = ldexpf(__ll2float_rn(acc[3 + t]), -shift_t);
        tensor[t] = ldexp(__ll2double_rn(acc[3 + t]), -shift_t);
    }
    SiftKeypoint kp;
    const float scale_factor = ldexpf(1.f, cand.octave);  // pow(2.f, octave), :1044
    for (int a = 0; a < 3; a++) {
        kp.coor_layer[a] = c[a];
        kp.coor_img[a] = c[a] * scale_factor;
    }
    kp.octave = cand.octave;
    kp.layer = cand.layer;
    kp.scale = cand.scale;
    for (int t = 0; t < 9; t++) kp.rotation_matrix[t] = 0.f;
    const int verdict = sift_orient_finish(p, d, tensor, kp.rotation_matrix);
    if (verdict != 0)
        for (int t = 0; t < 9; t++) kp.rotation_matrix[t] = 0.f;
    status[m] = verdict;
    if (sums)
        for (int t = 0; t < 9; t++) sums[(size_t)m * 9 + t] = out[t];
    slots[m] = kp;
}

__global__ __launch_bounds__(256) void sift_orient_count_kernel(const int* __restrict__ status, size_t n, unsigned* __restrict__ block_counts) {
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long m = __ballot(i < n && status[i] == 0);
    if ((threadIdx.x & 63) == 0) atomicAdd(&total, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        block_counts[2 * (size_t)blockIdx.x] = total;
        block_counts[2 * (size_t)blockIdx.x + 1] = 0;
    }
}

__global__ __launch_bounds__(256) void sift_orient_fill_kernel(const int* __restrict__ status, const SiftKeypoint* __restrict__ slots, size_t n,
                                                               const unsigned* __restrict__ block_offsets, SiftKeypoint* __restrict__ out) {
    __shared__ unsigned wave_count[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool hit = i < n && status[i] == 0;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_count[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!hit) return;
    unsigned at = block_offsets[2 * (size_t)blockIdx.x];
    for (int w = 0; w < wave; w++) at += wave_count[w];
    at += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    out[at] = slots[i];
}

constexpr int kDescribeBlock = 256;
constexpr int kTileFloats = 25;  // e1, e2, t, q (3 each), q . e2, the three vertices, the unit vector to the centroid
// A tile is tried only when the ray lies within acos(0.75) = 41.4 degrees of its centroid.  No first hit is lost: a ray that
// cartisan2Barycentric accepts passes within 10 FLT_EPSILON of the triangle (k g = the barycentric point + the residual, and the
// point is at least 0.79 from the origin), and no point of a tile is further than 37.4 degrees (cos 0.7947) from its centroid.
constexpr float kTileCone = 0.75f;

// cartisan2Barycentric (:579-623) for one tile: true when the ray of g meets it
__device__ __forceinline__ bool sift_barycentric(const float* g, const float* T, float* bary) {
    const float *e1 = T, *e2 = T + 3, *t = T + 6, *q = T + 9, *v0 = T + 13, *v1 = T + 16, *v2 = T + 19;
    const float p[3] = {g[1] * e2[2] - g[2] * e2[1], g[2] * e2[0] - g[0] * e2[2], g[0] * e2[1] - g[1] * e2[0]};
    const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (fabsf(det) < FLT_EPSILON * 10.f) return false;
    const float det_inv = 1.f / det;
    bary[2] = det_inv * (g[0] * q[0] + g[1] * q[1] + g[2] * q[2]);
    bary[1] = det_inv * (p[0] * t[0] + p[1] * t[1] + p[2] * t[2]);
    bary[0] = 1.f - bary[1] - bary[2];
    const float k = det_inv * T[12];
    if (k < 0) return false;
    if (bary[0] < -FLT_EPSILON * 10.f || bary[1] < -FLT_EPSILON * 10.f || bary[2] < -FLT_EPSILON * 10.f) return false;
    float r[3];
    for (int a = 0; a < 3; a++) r[a] = k * g[a] - bary[0] * v0[a] - bary[1] * v1[a] - bary[2] * v2[a];
    return !(sift_norm(r[0], r[1], r[2]) > FLT_EPSILON * 10.f);
}

__global__ __launch_bounds__(kDescribeBlock) void sift_describe_kernel(const SiftKeypoint* __restrict__ list, unsigned n, SiftFeatureParams p,
                                                                       float* __restrict__ out) {
    __shared__ unsigned long long bins[kSiftDescriptorLength];
    __shared__ float desc[kSiftDescriptorLength];
    __shared__ float tile[20][kTileFloats];
    __shared__ float inv_norm;
    const unsigned m = blockIdx.x;
    if (m >= n) return;
    const int tid = threadIdx.x;
    for (int t = tid; t < kSiftDescriptorLength; t += kDescribeBlock) bins[t] = 0ull;
    if (tid < 20) {  // the per-tile vectors of :583-590 and q . e2 of :603, which do not depend on the gradient
        const float* V = kIcosaVertex[tid];
        float* T = tile[tid];
        for (int a = 0; a < 3; a++) {
            T[a] = V[3 + a] - V[a];
            T[3 + a] = V[6 + a] - V[a];
            T[6 + a] = -1.f * V[a];
            T[13 + a] = V[a];
            T[16 + a] = V[3 + a];
            T[19 + a] = V[6 + a];
        }
        T[9] = T[7] * T[2] - T[8] * T[1];
        T[10] = T[8] * T[0] - T[6] * T[2];
        T[11] = T[6] * T[1] - T[7] * T[0];
        T[12] = T[9] * T[3] + T[10] * T[4] + T[11] * T[5];
        const float cx = V[0] + V[3] + V[6], cy = V[1] + V[4] + V[7], cz = V[2] + V[5] + V[8], cn = sift_norm(cx, cy, cz);
        T[22] = cx / cn;
        T[23] = cy / cn;
        T[24] = cz / cn;
    }
    __syncthreads();
    const SiftKeypoint kp = list[m];
    const SiftFeatureLayer L = p.layers[kp.layer + kp.octave * (p.n_octave_layers + 3)];
    const float* R = kp.rotation_matrix;
    const int centre[3] = {(int)kp.coor_layer[0], (int)kp.coor_layer[1], (int)kp.coor_layer[2]};
    int lo[3], len[3];
    for (int a = 0; a < 3; a++)
        sift_window_axis(kp.coor_layer[a], L.describe_radius / L.unit[a], L.describe_radius / L.unit[a], L.dim[a], centre[a], L.describe_half[a], lo[a], len[a]);
    const unsigned total = (unsigned)len[0] * (unsigned)len[1] * (unsigned)len[2];
    const unsigned plane = (unsigned)len[0] * (unsigned)len[1];
    const size_t row = (size_t)L.dim[0], slab = (size_t)L.dim[0] * L.dim[1];
    const float cube_radius = L.cube_radius;
    const int shift = 39 - p.exponent;
    for (unsigned v = tid; v < total; v += kDescribeBlock) {
        const unsigned zi = v / plane, rem = v - zi * plane, yi = rem / (unsigned)len[0], xi = rem - yi * (unsigned)len[0];
        const int k = lo[0] + (int)xi, j = lo[1] + (int)yi, i = lo[2] + (int)zi;
        const int ax = abs(k - centre[0]), ay = abs(j - centre[1]), az = abs(i - centre[2]);
        if (ax > L.describe_half[0] || ay > L.describe_half[1] || az > L.describe_half[2]) continue;  // (beyond the table is beyond the sphere)
        const float w = L.describe[((size_t)az * (L.describe_half[1] + 1) + ay) * (L.describe_half[0] + 1) + ax];
        if (w < 0.f) continue;  // :1099
        const float px = ((float)k - kp.coor_layer[0]) * L.unit[0], py = ((float)j - kp.coor_layer[1]) * L.unit[1], pz = ((float)i - kp.coor_layer[2]) * L.unit[2];
        float sub[3];
        bool inside = true;
        for (int a = 0; a < 3; a++) {
            const float rotated = R[3 * a] * px + R[3 * a + 1] * py + R[3 * a + 2] * pz;
            sub[a] = 2.f * (rotated + cube_radius) / cube_radius;
            sub[a] -= 0.5f;
            inside = inside && !(sub[a] <= -0.5f || sub[a] >= 3.5f);
        }
        if (!inside) continue;  // :1122-1126
        const float* at = L.vol + ((size_t)i * slab + (size_t)j * row + (size_t)k);
        const float gx = w * ((0.5f * (at[1] - at[-1])) / L.unit[0]);
        const float gy = w * ((0.5f * (at[row] - at[-(ptrdiff_t)row])) / L.unit[1]);
        const float gz = w * ((0.5f * (at[slab] - at[-(ptrdiff_t)slab])) / L.unit[2]);
        float g[3];
        for (int a = 0; a < 3; a++) g[a] = R[3 * a] * gx + R[3 * a + 1] * gy + R[3 * a + 2] * gz;
        const float magnitude = sift_norm(g[0], g[1], g[2]);
        if (magnitude * magnitude < FLT_EPSILON * 10.f) continue;  // :1146
        int hit = -1;
        float bary[3];
        const float cone = kTileCone * magnitude;
        for (int t = 0; t < 20; t++) {
            if (g[0] * tile[t][22] + g[1] * tile[t][23] + g[2] * tile[t][24] < cone) continue;
            if (sift_barycentric(g, tile[t], bary)) {
                hit = t;
                break;
            }
        }
        if (hit < 0) continue;
        float dec[3];
        int base[3];
        for (int a = 0; a < 3; a++) {
            dec[a] = sub[a] - floorf(sub[a]);
            base[a] = (int)sub[a];  // truncation against floor: they differ on (-0.5, 0), as in :1174-1187
        }
        for (int dz = 0; dz < 2; dz++)
            for (int dy = 0; dy < 2; dy++)
                for (int dx = 0; dx < 2; dx++) {
                    const int local_x = base[0] + dx, local_y = base[1] + dy, local_z = base[2] + dz;
                    if (local_x < 0 || local_y < 0 || local_z < 0 || local_x >= 4 || local_y >= 4 || local_z >= 4) continue;
                    const int cube = local_x + local_y * 4 + local_z * 16;
                    const float interp = ((dx == 0) ? (1.f - dec[0]) : dec[0]) * ((dy == 0) ? (1.f - dec[1]) : dec[1]) * ((dz == 0) ? (1.f - dec[2]) : dec[2]);
                    for (int b = 0; b < 3; b++)
                        atomicAdd(&bins[cube * 12 + kIcosaIndex[hit][b]], (unsigned long long)sift_quantise(magnitude * interp * bary[b], shift));
                }
    }
    __syncthreads();
    for (int t = tid; t < kSiftDescriptorLength; t += kDescribeBlock) desc[t] = ldexpf(__ll2float_rn((long long)bins[t]), -shift);
    for (int pass = 0; pass < 2; pass++) {  // :1219-1247
        __syncthreads();
        if (tid == 0) {
            float sq_sum = 0;
            for (int t = 0; t < kSiftDescriptorLength; t++) sq_sum += desc[t] * desc[t];
            inv_norm = 1.f / (sqrtf(sq_sum) + FLT_EPSILON);
        }
        __syncthreads();
        for (int t = tid; t < kSiftDescriptorLength; t += kDescribeBlock) {
            float x = desc[t] * inv_norm;
            if (pass == 0) x = (x < p.truncate_threshold) ? x : p.truncate_threshold;
            desc[t] = x;
        }
    }
    for (int t = tid; t < kSiftDescriptorLength; t += kDescribeBlock) out[(size_t)m * kSiftDescriptorLength + t] = desc[t];
}

}  // namespace

hipError_t launch_sift_max_abs(const float* v, size_t count, unsigned* max_abs_bits, hipStream_t stream) {
    if (count < 1) return hipErrorInvalidValue;
    const size_t blocks = std::min<size_t>((count + 255) / 256, 4096);
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_max_abs_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, v, count, max_abs_bits);
    return hipGetLastError();
}

hipError_t launch_sift_check_candidates(const SiftCandidate* list, size_t n, const SiftFeatureParams& p, unsigned* flag, hipStream_t stream) {
    if (n < 1 || (n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_check_candidates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, list, n, p, flag);
    return hipGetLastError();
}

hipError_t launch_sift_check_keypoints(const SiftKeypoint* list, size_t n, const SiftFeatureParams& p, unsigned* flag, hipStream_t stream) {
    if (n < 1 || (n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_check_keypoints_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, list, n, p, flag);
    return hipGetLastError();
}

hipError_t launch_sift_orient(const SiftCandidate* list, size_t n, const SiftFeatureParams& p, int* status, float* sums, SiftKeypoint* slots,
                              hipStream_t stream) {
    if (n < 1 || n > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_orient_kernel, dim3((unsigned)n), dim3(64), 0, stream, list, (unsigned)n, p, status, sums, slots);
    return hipGetLastError();
}

hipError_t launch_sift_orient_count(const int* status, size_t n, unsigned* block_counts, hipStream_t stream) {
    if (n < 1 || sift_orient_blocks(n) > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_orient_count_kernel, dim3((unsigned)sift_orient_blocks(n)), dim3(256), 0, stream, status, n, block_counts);
    return hipGetLastError();
}

hipError_t launch_sift_orient_fill(const int* status, const SiftKeypoint* slots, size_t n, const unsigned* block_offsets, SiftKeypoint* out,
                                   hipStream_t stream) {
    if (n < 1 || sift_orient_blocks(n) > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_orient_fill_kernel, dim3((unsigned)sift_orient_blocks(n)), dim3(256), 0, stream, status, slots, n, block_offsets, out);
    return hipGetLastError();
}

hipError_t launch_sift_describe(const SiftKeypoint* list, size_t n, const SiftFeatureParams& p, float* out, hipStream_t stream) {
    if (n < 1 || n > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_describe_kernel, dim3((unsigned)n), dim3(kDescribeBlock), 0, stream, list, (unsigned)n, p, out);
    return hipGetLastError();
}

}  // namespace ochip

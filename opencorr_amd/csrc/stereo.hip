// stereo.hip -- Calibration::prepare / undistort and Stereovision::reconstruct on gfx950.
//
// Replaces Calibration::prepare(height, width) (src/oc_calibration.cpp:161-219: the map of undistorted image coordinates,
// a fixed-point iteration per pixel), Calibration::undistort (:221-264: bilinear look-up in that map) and
// Stereovision::reconstruct (src/oc_stereovision.cpp:70-133: least-squares triangulation of a point pair), plus the host
// loops of examples/test_3d_dic_epipolar_sift.cpp:303-317 that fill ref_coor / tar_coor / deformation of a POI2DS queue.
//
// Arithmetic.  Everything up to and including the 4 x 3 system is float32 in the reference's operand order, every
// operation rounded on its own (the library is built with -ffp-contract=off, IEEE divide): the map and the undistorted
// coordinates are bit-identical to a float32 restatement of the source.  The reference then solves the system with Eigen's
// column-pivoted Householder QR in float32, whose operation order is Eigen's own; here the system is solved by Householder
// QR in double and the solution rounded once to float32 ("Stereo").
//
// None of the kernels shares data between threads: one thread per pixel / point pair / POI.  The map kernel is bound by its
// dependent chain of divides (at most `iteration` rounds, 3 in practice), the point kernels by their scattered 4-texel reads.
#include "oc_device.h"
#include "oc_kernels.h"

namespace ochip {

namespace {

// Calibration::sensor_to_image, src/oc_calibration.cpp:126-133
__device__ __forceinline__ void sensor_to_image(const CameraParams& k, float sx, float sy, float& ix, float& iy) {
    iy = (sy - k.cy) / k.fy;
    ix = (sx - k.cx - k.fs * iy) / k.fx;
}

// Calibration::image_to_sensor, :117-124
__device__ __forceinline__ void image_to_sensor(const CameraParams& k, float ix, float iy, float& sx, float& sy) {
    sy = iy * k.fy + k.cy;
    sx = ix * k.fx + iy * k.fs + k.cx;
}

// Calibration::distort, :136-159
__device__ __forceinline__ void distort(const CameraParams& k, float x, float y, float& dx, float& dy) {
    const float xx = x * x;
    const float yy = y * y;
    const float xy = x * y;
    const float r2 = xx + yy;
    const float r4 = r2 * r2;
    const float r6 = r2 * r4;
    const float radial = (1.f + k.k1 * r2 + k.k2 * r4 + k.k3 * r6) / (1.f + k.k4 * r2 + k.k5 * r4 + k.k6 * r6);
    dy = y * radial;
    dx = x * radial;
    dy = dy + (k.p1 * (r2 + 2.f * yy) + 2.f * k.p2 * xy);
    dx = dx + (2.f * k.p1 * xy + k.p2 * (r2 + 2.f * xx));
}

// Calibration::prepare, :161-219
__global__ __launch_bounds__(256) void undistort_map_kernel(CameraParams k, int height, int width, float convergence,
                                                            int iteration, float* __restrict__ map_x,
                                                            float* __restrict__ map_y) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= width || r >= height) return;
    float x0, y0;
    sensor_to_image(k, (float)c, (float)r, x0, y0);
    float x = x0, y = y0;
    bool stop = false;
    int i = 0;
    while (i < iteration && !stop) {
        i++;
        float dx, dy, sx, sy;
        distort(k, x, y, dx, dy);
        image_to_sensor(k, dx, dy, sx, sy);
        float dev_y = (float)r - sy;
        float dev_x = (float)c - sx;
        if (isinf(dev_x) || isinf(dev_y)) {
            stop = true;
            y = y0;
            x = x0;
        }
        if (fabsf(dev_x) > convergence || fabsf(dev_y) > convergence) {
            dev_y = dev_y / k.fy;
            y = y + dev_y;
            x = x + (dev_x - dev_y * k.fs) / k.fx;
        } else {
            stop = true;
        }
    }
    const size_t at = (size_t)r * width + c;
    map_y[at] = y;
    map_x[at] = x;
}

// Calibration::undistort, :221-264.  NaN coordinates never reach this function.
__device__ __forceinline__ void undistort(const CameraView& v, float px, float py, float& ux, float& uy) {
    if (px < 0.f) px = 0.f;
    if (py < 0.f) py = 0.f;
    if (px > (float)(v.width - 2)) px = (float)v.width - 2.f;
    if (py > (float)(v.height - 2)) py = (float)v.height - 2.f;
    // the clamps leave 0 <= px <= width - 2; min / max only keep the reads inside the map whatever the arguments
    const int yi = min(max((int)floorf(py), 0), v.height - 2);
    const int xi = min(max((int)floorf(px), 0), v.width - 2);
    const float yd = py - (float)yi;
    const float xd = px - (float)xi;
    const size_t at = (size_t)yi * v.width + xi;
    const float w00 = (1.f - yd), w01 = (1.f - xd);
    float cy = v.map_y[at] * w00 * w01;
    cy = cy + v.map_y[at + v.width] * yd * w01;
    cy = cy + v.map_y[at + 1] * w00 * xd;
    cy = cy + v.map_y[at + v.width + 1] * yd * xd;
    float cx = v.map_x[at] * w00 * w01;
    cx = cx + v.map_x[at + v.width] * yd * w01;
    cx = cx + v.map_x[at + 1] * w00 * xd;
    cx = cx + v.map_x[at + v.width + 1] * yd * xd;
    image_to_sensor(v.cam, cx, cy, ux, uy);
}

__global__ __launch_bounds__(256) void undistort_points_kernel(CameraView v, const float* __restrict__ in, float* __restrict__ out,
                                                               int stride_f, unsigned count) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float px = in[(size_t)i * stride_f], py = in[(size_t)i * stride_f + 1];
    float ux = px + py, uy = ux;  // NaN in, NaN out (the reference's floor of a NaN is undefined)
    if (px == px && py == py) undistort(v, px, py, ux, uy);
    out[(size_t)i * stride_f] = ux;
    out[(size_t)i * stride_f + 1] = uy;
}

// Stereovision::reconstruct(Point2D&, Point2D&), src/oc_stereovision.cpp:70-124
__device__ __forceinline__ void triangulate(const CameraView& v1, const CameraView& v2, float p1x, float p1y, float p2x, float p2y,
                                            float (&world)[3]) {
    world[0] = world[1] = world[2] = 0.f;
    if (p1x != p1x || p1y != p1y || p2x != p2x || p2y != p2y) return;  // :72-76
    float x1, y1, x2, y2;
    undistort(v1, p1x, p1y, x1, y1);
    undistort(v2, p2x, p2y, x2, y2);
    const float* P1 = v1.proj;
    const float* P2 = v2.proj;
    // :88-112, in float
    double A[4][3], b[4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        A[0][j] = (double)(x1 * P1[8 + j] - P1[j]);
        A[1][j] = (double)(y1 * P1[8 + j] - P1[4 + j]);
        A[2][j] = (double)(x2 * P2[8 + j] - P2[j]);
        A[3][j] = (double)(y2 * P2[8 + j] - P2[4 + j]);
    }
    b[0] = (double)(P1[3] - x1 * P1[11]);
    b[1] = (double)(P1[7] - y1 * P1[11]);
    b[2] = (double)(P2[3] - x2 * P2[11]);
    b[3] = (double)(P2[7] - y2 * P2[11]);
    // Householder QR in double (no pivoting: the exact least-squares solution does not depend on it)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double n2 = 0.0;
#pragma unroll
        for (int i = k; i < 4; i++) n2 = n2 + A[i][k] * A[i][k];
        const double nrm = sqrt(n2);
        const double alpha = A[k][k] > 0.0 ? -nrm : nrm;
        double v[4];
#pragma unroll
        for (int i = k; i < 4; i++) v[i] = A[i][k];
        v[k] = v[k] - alpha;
        double vv = 0.0;
#pragma unroll
        for (int i = k; i < 4; i++) vv = vv + v[i] * v[i];
        if (vv > 0.0) {
#pragma unroll
            for (int j = k + 1; j < 3; j++) {
                double s = 0.0;
#pragma unroll
                for (int i = k; i < 4; i++) s = s + v[i] * A[i][j];
                s = 2.0 * s / vv;
#pragma unroll
                for (int i = k; i < 4; i++) A[i][j] = A[i][j] - s * v[i];
            }
            double s = 0.0;
#pragma unroll
            for (int i = k; i < 4; i++) s = s + v[i] * b[i];
            s = 2.0 * s / vv;
#pragma unroll
            for (int i = k; i < 4; i++) b[i] = b[i] - s * v[i];
        }
        A[k][k] = alpha;
    }
    const double z = b[2] / A[2][2];
    const double y = (b[1] - A[1][2] * z) / A[1][1];
    const double x = (b[0] - A[0][1] * y - A[0][2] * z) / A[0][0];
    world[0] = (float)x;
    world[1] = (float)y;
    world[2] = (float)z;
}

__global__ __launch_bounds__(256) void reconstruct_kernel(CameraView v1, CameraView v2, const float* __restrict__ p1, int s1,
                                                          const float* __restrict__ p2, int s2, float* __restrict__ out, int so,
                                                          unsigned count) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float w[3];
    triangulate(v1, v2, p1[(size_t)i * s1], p1[(size_t)i * s1 + 1], p2[(size_t)i * s2], p2[(size_t)i * s2 + 1], w);
    float* o = out + (size_t)i * so;
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
}

// examples/test_3d_dic_epipolar_sift.cpp:303-317 over the whole queue
__global__ __launch_bounds__(256) void reconstruct_pois_kernel(CameraView v1, CameraView v2, float* __restrict__ pois, int stride_f,
                                                               unsigned count) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float* p = pois + (size_t)i * stride_f;
    float ref[3], tar[3];
    triangulate(v1, v2, p[poi2ds::X], p[poi2ds::Y], p[poi2ds::R2_X], p[poi2ds::R2_Y], ref);
    triangulate(v1, v2, p[poi2ds::T1_X], p[poi2ds::T1_Y], p[poi2ds::T2_X], p[poi2ds::T2_Y], tar);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        p[poi2ds::REF + a] = ref[a];
        p[poi2ds::TAR + a] = tar[a];
        p[poi2ds::U + a] = tar[a] - ref[a];
    }
}

}  // namespace

hipError_t launch_undistort_map(const CameraParams& cam, int height, int width, float convergence, int iteration, float* map_x,
                                float* map_y, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(undistort_map_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, stream, cam, height, width,
                       convergence, iteration, map_x, map_y);
    return hipGetLastError();
}

hipError_t launch_undistort_points(const CameraView& view, const float* in, float* out, int stride_floats, size_t count,
                                   hipStream_t stream) {
    if (count == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, view, in, out,
                       stride_floats, (unsigned)count);
    return hipGetLastError();
}

hipError_t launch_reconstruct(const CameraView& view1, const CameraView& view2, const float* p1, int stride1_floats,
                              const float* p2, int stride2_floats, float* out, int stride_out_floats, size_t count,
                              hipStream_t stream) {
    if (count == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(reconstruct_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, view1, view2, p1,
                       stride1_floats, p2, stride2_floats, out, stride_out_floats, (unsigned)count);
    return hipGetLastError();
}

hipError_t launch_reconstruct_pois(const CameraView& view1, const CameraView& view2, float* pois, int stride_floats, size_t count,
                                   hipStream_t stream) {
    if (count == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(reconstruct_pois_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, view1, view2, pois,
                       stride_floats, (unsigned)count);
    return hipGetLastError();
}

}  // namespace ochip

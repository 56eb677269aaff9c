// sift2d.hip -- SIFT2D's detector: the 2x upscale, the separable Gaussian blur with the DoG subtraction in its last write, the
// nearest-neighbour half-size resample, the 26-neighbour extrema scan and the sub-pixel localisation with its contrast and edge
// rejections -- cv::SIFT as the reference's SIFT2D::compute() creates it (src/oc_sift.cpp:22-30, 60-93), restated in DESIGN.md
// section 4.13.  Images are [row][col] float32, columns contiguous.
//
// Contract:    per pixel and pass acc = w[0] * s[c], then for r = 1 ... R ascending acc = acc + w[r] * (s[lo(c - r)] + s[hi(c + r)]),
//              every operation rounding to float32 on its own (the file is built with -ffp-contract=off).  No re-association: one
//              thread owns one pixel's sum, so no tile shape changes a bit.  lo / hi are reflect-101 applied until the index is
//              inside (period 2 (n - 1)): the top octaves are narrower than the kernel.
// Shape:       bandwidth-bound.  Rows pass: a workgroup stages 256 pixels of one row plus R on either side in LDS.  Columns pass:
//              x stays on the 64 lanes (coalesced 256-B segments), a workgroup stages 64 + 2R lines and each of its 4 waves owns
//              every fourth output line -- LDS rows of 64 floats, so a wave's read of one row touches every bank once; it reads
//              the layer the blur started from once more and writes the DoG layer with the Gaussian one.  The weights travel as a
//              kernel argument (wave-uniform).  One launch per pass and layer: the layers of an octave depend on each other.
// Extrema:     count per workgroup, the exclusive scan of poi_split.hip, fill: the starts are in scan order (octave, layer, row,
//              column) whatever the launch shape.  Localisation: one thread per start, then the same count / scan / fill over the
//              located ones, so the list is in the order of the starts, identical from run to run.
#include <climits>

#include "oc_device.h"
#include "oc_kernels.h"
#include "host/sift2d_plan.h"

namespace ochip {

static_assert(kSift2dMaxRadius == kSiftMaxRadius && kSift2dMaxRadius == ochip_host::kSift2dMaxRadius, "SiftWeights holds the taps of both scale spaces");

namespace {

constexpr int kBlock = 256;
constexpr int kLines = 64;  // output lines of the columns pass per workgroup
constexpr int kBorder = ochip_host::kSift2dBorder;

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

template <class T>
__global__ __launch_bounds__(kBlock) void sift2d_upscale_kernel(const T* __restrict__ src, int cols, int rows, float* __restrict__ dst, size_t count,
                                                                unsigned* __restrict__ flag) {
    const size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= count) return;
    const int dcols = 2 * cols;
    const int y = (int)(idx / (size_t)dcols), x = (int)(idx - (size_t)y * dcols);
    const int kx = x >> 1, ky = y >> 1;
    // destination x samples the source at (x + 0.5) * 0.5 - 0.5: even x between kx - 1 (0.25) and kx (0.75), odd x between kx (0.75)
    // and kx + 1 (0.25), indices clamped to the edge
    const int x0 = (x & 1) ? kx : max(kx - 1, 0), x1 = (x & 1) ? min(kx + 1, cols - 1) : kx;
    const int y0 = (y & 1) ? ky : max(ky - 1, 0), y1 = (y & 1) ? min(ky + 1, rows - 1) : ky;
    const float wx0 = (x & 1) ? 0.75f : 0.25f, wx1 = (x & 1) ? 0.25f : 0.75f;
    const float wy0 = (y & 1) ? 0.75f : 0.25f, wy1 = (y & 1) ? 0.25f : 0.75f;
    const float s00 = (float)src[(size_t)y0 * cols + x0], s01 = (float)src[(size_t)y0 * cols + x1];
    const float s10 = (float)src[(size_t)y1 * cols + x0], s11 = (float)src[(size_t)y1 * cols + x1];
    const float a = wx0 * s00 + wx1 * s01;
    const float b = wx0 * s10 + wx1 * s11;
    dst[idx] = wy0 * a + wy1 * b;
    // four destination pixels share the source pixel (kx, ky): the even-even one looks at it
    if (((x | y) & 1) == 0 && !(fabsf((float)src[(size_t)ky * cols + kx]) <= 3.402823466e+38f)) atomicOr(flag, 1u);
}

// one workgroup: kBlock pixels of one row
__global__ __launch_bounds__(kBlock) void sift2d_blur_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int cols, unsigned xtiles,
                                                                  SiftWeights W, int R) {
    __shared__ float s[kBlock + 2 * kSift2dMaxRadius];
    const unsigned row = blockIdx.x / xtiles, tile = blockIdx.x - row * xtiles;
    const int x0 = (int)tile * kBlock;
    const float* srow = src + (size_t)row * cols;
    for (int p = threadIdx.x; p < kBlock + 2 * R; p += kBlock) s[p] = srow[reflect101(x0 - R + p, cols)];
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x >= cols) return;
    const int c = (int)threadIdx.x + R;
    float acc = W.w[0] * s[c];
    for (int r = 1; r <= R; r++) acc = acc + W.w[r] * (s[c - r] + s[c + r]);
    dst[(size_t)row * cols + x] = acc;
}

// one workgroup: 64 columns x kLines lines
template <bool DOG>
__global__ __launch_bounds__(kBlock) void sift2d_blur_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int cols, int rows,
                                                                  unsigned col_tiles, SiftWeights W, int R, const float* __restrict__ prev,
                                                                  float* __restrict__ dog) {
    __shared__ float s[kLines + 2 * kSift2dMaxRadius][64];
    const unsigned ct = blockIdx.x % col_tiles, lt = blockIdx.x / col_tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)ct * 64 + lane;
    const bool live = x < cols;
    const int j0 = (int)lt * kLines;
    const int lines = min(kLines, rows - j0);
    for (int p = wave; p < lines + 2 * R; p += kBlock / 64) s[p][lane] = live ? src[(size_t)reflect101(j0 - R + p, rows) * cols + x] : 0.f;
    __syncthreads();
    if (!live) return;
    for (int t = wave; t < lines; t += kBlock / 64) {
        const int c = t + R;
        float acc = W.w[0] * s[c][lane];
        for (int r = 1; r <= R; r++) acc = acc + W.w[r] * (s[c - r][lane] + s[c + r][lane]);
        const size_t at = (size_t)(j0 + t) * cols + x;
        dst[at] = acc;
        if (DOG) dog[at] = acc - prev[at];
    }
}

__global__ __launch_bounds__(kBlock) void sift2d_resample_kernel(const float* __restrict__ src, int scols, int srows, float* __restrict__ dst, int dcols,
                                                                 int drows, size_t count) {
    const size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= count) return;
    const int y = (int)(idx / (size_t)dcols), x = (int)(idx - (size_t)y * dcols);
    const int sx = min((int)floor(x * ((double)scols / dcols)), scols - 1);
    const int sy = min((int)floor(y * ((double)srows / drows)), srows - 1);
    dst[idx] = src[(size_t)sy * scols + sx];
}

__device__ __forceinline__ bool sift2d_is_candidate(const Sift2dExtremaLayer& L, unsigned idx, unsigned count, int& row, int& col) {
    if (idx >= count) return false;
    row = (int)(idx / (unsigned)L.cols);
    col = (int)(idx - (unsigned)row * (unsigned)L.cols);
    if (col < kBorder || col >= L.cols - kBorder || row < kBorder || row >= L.rows - kBorder) return false;
    const float v = L.here[idx];
    if (!(fabsf(v) > L.threshold)) return false;
    if (!(v > 0.f) && !(v < 0.f)) return false;
    bool ge = true, le = true;
    const float* layers[3] = {L.here, L.below, L.above};
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int dr = -1; dr <= 1; dr++)
#pragma unroll
            for (int dc = -1; dc <= 1; dc++) {
                if (k == 0 && dr == 0 && dc == 0) continue;
                const float q = layers[k][(size_t)((long long)idx + (long long)dr * L.cols + dc)];
                ge = ge && v >= q;
                le = le && v <= q;
            }
    return v > 0.f ? ge : le;
}

constexpr int kExtremaRounds = kSiftExtremaVoxels / kBlock;

__global__ __launch_bounds__(kBlock) void sift2d_extrema_count_kernel(Sift2dExtremaLayer L, unsigned count, unsigned* __restrict__ block_counts) {
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int round = 0; round < kExtremaRounds; round++) {
        const unsigned idx = blockIdx.x * (unsigned)kSiftExtremaVoxels + round * kBlock + threadIdx.x;
        int row, col;
        const unsigned long long m = __ballot(sift2d_is_candidate(L, idx, count, row, col));
        mine += (unsigned)__popcll(m);
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        block_counts[2 * (size_t)(L.first_block + blockIdx.x)] = total;
        block_counts[2 * (size_t)(L.first_block + blockIdx.x) + 1] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void sift2d_extrema_fill_kernel(Sift2dExtremaLayer L, unsigned count, const unsigned* __restrict__ block_offsets,
                                                                     Sift2dStart* __restrict__ out) {
    __shared__ unsigned wave_count[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned base = block_offsets[2 * (size_t)(L.first_block + blockIdx.x)];
    for (int round = 0; round < kExtremaRounds; round++) {
        const unsigned idx = blockIdx.x * (unsigned)kSiftExtremaVoxels + round * kBlock + threadIdx.x;
        int row = 0, col = 0;
        const bool hit = sift2d_is_candidate(L, idx, count, row, col);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_count[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned at = base, all = 0;
        for (int w = 0; w < kBlock / 64; w++) {
            if (w < wave) at += wave_count[w];
            all += wave_count[w];
        }
        if (hit) {
            at += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            out[at] = Sift2dStart{L.octave, L.layer, row, col};
        }
        base += all;
        __syncthreads();  // (wave_count is written again in the next round)
    }
}

// X of H X = b by elimination with partial pivoting (the first largest magnitude of a column wins); a zero pivot: X = 0
__device__ __forceinline__ void sift2d_solve3(float A[3][4], float X[3]) {
    X[0] = X[1] = X[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int p = k;
#pragma unroll
        for (int i = k + 1; i < 3; i++)
            if (fabsf(A[i][k]) > fabsf(A[p][k])) p = i;
        if (A[p][k] == 0.f) return;
#pragma unroll
        for (int i = k + 1; i < 3; i++)
            if (p == i)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float t = A[k][j];
                    A[k][j] = A[i][j];
                    A[i][j] = t;
                }
#pragma unroll
        for (int i = k + 1; i < 3; i++) {
            const float f = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k + 1; j < 4; j++) A[i][j] = A[i][j] - f * A[k][j];
        }
    }
    X[2] = A[2][3] / A[2][2];
    X[1] = (A[1][3] - A[1][2] * X[2]) / A[1][1];
    X[0] = ((A[0][3] - A[0][1] * X[1]) - A[0][2] * X[2]) / A[0][0];
}

__global__ __launch_bounds__(kBlock) void sift2d_localize_kernel(const Sift2dStart* __restrict__ starts, unsigned n_starts, Sift2dLocalizeParams P,
                                                                 int* __restrict__ status, Sift2dKeypoint* __restrict__ slots) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_starts) return;
    const Sift2dStart st = starts[i];
    const int o = st.octave, n = P.n_octave_layers, per = n + 2;
    int layer = st.layer, r = st.row, c = st.col;
    const Sift2dDogLayer first = P.dog[(size_t)o * per];
    const int cols = first.cols, rows = first.rows;
    const float img_scale = 1.f / 255, deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    float xc = 0.f, xr = 0.f, xi = 0.f, dD[3] = {0.f, 0.f, 0.f};
    int verdict = 0, step = 0;
#define AT(a, rr, cc) a[(size_t)(rr) * cols + (cc)]
    for (; step < ochip_host::kSift2dMaxSteps; step++) {
        // (layer in [1, n], r and c inside the 5-pixel border: every read below is inside the octave's layers)
        const float* img = P.dog[(size_t)o * per + layer].data;
        const float* prev = P.dog[(size_t)o * per + layer - 1].data;
        const float* next = P.dog[(size_t)o * per + layer + 1].data;
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
        sift2d_solve3(A, X);
        xc = -X[0], xr = -X[1], xi = -X[2];
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        const float big = (float)(INT_MAX / 3);
        if (!(fabsf(xi) <= big) || !(fabsf(xr) <= big) || !(fabsf(xc) <= big)) {  // (a NaN is rejected here too)
            verdict = 1;
            break;
        }
        c += (int)rintf(xc);
        r += (int)rintf(xr);
        layer += (int)rintf(xi);
        if (layer < 1 || layer > n || c < kBorder || c >= cols - kBorder || r < kBorder || r >= rows - kBorder) {
            verdict = 2;
            break;
        }
    }
    if (verdict == 0 && step >= ochip_host::kSift2dMaxSteps) verdict = 3;
    if (verdict != 0) {
        status[i] = verdict;
        return;
    }
    const float* img = P.dog[(size_t)o * per + layer].data;
    float dot = dD[0] * xc;
    dot = dot + dD[1] * xr;
    dot = dot + dD[2] * xi;
    const float contr = AT(img, r, c) * img_scale + 0.5f * dot;
    if (fabsf(contr) * n < P.contrast_threshold) {
        status[i] = 4;
        return;
    }
    const float v2 = AT(img, r, c) * 2;
    const float dxx = (AT(img, r, c + 1) + AT(img, r, c - 1) - v2) * second_scale;
    const float dyy = (AT(img, r + 1, c) + AT(img, r - 1, c) - v2) * second_scale;
    const float dxy = (AT(img, r + 1, c + 1) - AT(img, r + 1, c - 1) - AT(img, r - 1, c + 1) + AT(img, r - 1, c - 1)) * cross_scale;
#undef AT
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy, e = P.edge_threshold;
    if (det <= 0.f || tr * tr * e >= (e + 1) * (e + 1) * det) {
        status[i] = 5;
        return;
    }
    const float pw = (float)(1 << o);
    Sift2dKeypoint kp;
    kp.x = (c + xc) * pw * 0.5f;
    kp.y = (r + xr) * pw * 0.5f;
    kp.size = P.sigma * ochip_host::sift2d_pow2((layer + xi) / n) * pw * 2 * 0.5f;
    kp.response = fabsf(contr);
    kp.octave = o - 1, kp.layer = layer, kp.row = r, kp.col = c;
    kp.xc = xc, kp.xr = xr, kp.xi = xi;
    kp.packed_octave = ((o - 1) & 255) | (layer << 8) | ((int)rint(((double)xi + 0.5) * 255) << 16);
    slots[i] = kp;
    status[i] = 0;
}

__global__ __launch_bounds__(kBlock) void sift2d_fill_kernel(const int* __restrict__ status, const Sift2dKeypoint* __restrict__ slots, size_t n,
                                                             const unsigned* __restrict__ block_offsets, Sift2dKeypoint* __restrict__ out) {
    __shared__ unsigned wave_count[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
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

bool layer_ok(int cols, int rows) { return cols >= 1 && rows >= 1 && (size_t)cols * rows <= 0x7fffffffull; }

}  // namespace

hipError_t launch_sift2d_upscale(const void* src, bool src_u8, int cols, int rows, float* dst, unsigned* flag, hipStream_t stream) {
    if (cols < 1 || rows < 1 || 4ull * (size_t)cols * rows > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t count = 4 * (size_t)cols * rows;
    const dim3 grid((unsigned)((count + kBlock - 1) / kBlock));
    (void)hipGetLastError();
    if (src_u8) hipLaunchKernelGGL(sift2d_upscale_kernel<unsigned char>, grid, dim3(kBlock), 0, stream, static_cast<const unsigned char*>(src), cols, rows, dst, count, flag);
    else hipLaunchKernelGGL(sift2d_upscale_kernel<float>, grid, dim3(kBlock), 0, stream, static_cast<const float*>(src), cols, rows, dst, count, flag);
    return hipGetLastError();
}

hipError_t launch_sift2d_blur_rows(const float* src, float* dst, int cols, int rows, const SiftWeights& w, int radius, hipStream_t stream) {
    if (!layer_ok(cols, rows) || radius < 1 || radius > kSift2dMaxRadius) return hipErrorInvalidValue;
    const size_t xtiles = ((size_t)cols + kBlock - 1) / kBlock, blocks = (size_t)rows * xtiles;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift2d_blur_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, dst, cols, (unsigned)xtiles, w, radius);
    return hipGetLastError();
}

hipError_t launch_sift2d_blur_cols(const float* src, float* dst, int cols, int rows, const SiftWeights& w, int radius, const float* prev, float* dog,
                                   hipStream_t stream) {
    if (!layer_ok(cols, rows) || radius < 1 || radius > kSift2dMaxRadius || (dog != nullptr) != (prev != nullptr)) return hipErrorInvalidValue;
    const size_t col_tiles = ((size_t)cols + 63) / 64, line_tiles = ((size_t)rows + kLines - 1) / kLines, blocks = col_tiles * line_tiles;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (dog) hipLaunchKernelGGL(sift2d_blur_cols_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, dst, cols, rows, (unsigned)col_tiles, w, radius, prev, dog);
    else hipLaunchKernelGGL(sift2d_blur_cols_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, dst, cols, rows, (unsigned)col_tiles, w, radius, prev, dog);
    return hipGetLastError();
}

hipError_t launch_sift2d_resample(const float* src, int src_cols, int src_rows, float* dst, int dst_cols, int dst_rows, hipStream_t stream) {
    if (!layer_ok(src_cols, src_rows) || !layer_ok(dst_cols, dst_rows)) return hipErrorInvalidValue;
    const size_t count = (size_t)dst_cols * dst_rows;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift2d_resample_kernel, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, src, src_cols, src_rows, dst, dst_cols,
                       dst_rows, count);
    return hipGetLastError();
}

hipError_t launch_sift2d_extrema_count(const Sift2dExtremaLayer& layer, unsigned* block_counts, hipStream_t stream) {
    if (!layer_ok(layer.cols, layer.rows)) return hipErrorInvalidValue;
    const size_t count = (size_t)layer.cols * layer.rows;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift2d_extrema_count_kernel, dim3((unsigned)sift_extrema_blocks(count)), dim3(kBlock), 0, stream, layer, (unsigned)count, block_counts);
    return hipGetLastError();
}

hipError_t launch_sift2d_extrema_fill(const Sift2dExtremaLayer& layer, const unsigned* block_offsets, Sift2dStart* out, hipStream_t stream) {
    if (!layer_ok(layer.cols, layer.rows)) return hipErrorInvalidValue;
    const size_t count = (size_t)layer.cols * layer.rows;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift2d_extrema_fill_kernel, dim3((unsigned)sift_extrema_blocks(count)), dim3(kBlock), 0, stream, layer, (unsigned)count, block_offsets, out);
    return hipGetLastError();
}

hipError_t launch_sift2d_localize(const Sift2dStart* starts, size_t n, const Sift2dLocalizeParams& p, int* status, Sift2dKeypoint* slots, hipStream_t stream) {
    if (n < 1 || n > 0x7fffffffull || p.n_octave_layers < 1) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift2d_localize_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, starts, (unsigned)n, p, status, slots);
    return hipGetLastError();
}

hipError_t launch_sift2d_fill(const int* status, const Sift2dKeypoint* slots, size_t n, const unsigned* block_offsets, Sift2dKeypoint* out, hipStream_t stream) {
    if (n < 1 || sift_orient_blocks(n) > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift2d_fill_kernel, dim3((unsigned)sift_orient_blocks(n)), dim3(kBlock), 0, stream, status, slots, n, block_offsets, out);
    return hipGetLastError();
}

}  // namespace ochip

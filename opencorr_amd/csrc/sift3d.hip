// sift3d.hip -- SIFT3D's scale space: the separable Gaussian blur, the octave downsampling, the DoG layers with their maxima
// and the extrema search (SIFT3D::gaussianBlur, downSampling, createDogPyramid, detectExtrema; src/oc_sift.cpp:365-562,
// 756-847).  Volumes are [z][y][x] float32, x contiguous.
//
// Contract:    per voxel and pass acc = w[0] * s[c], then for r = 1 ... R ascending acc = acc + w[r] * (s[lo(c - r)] + s[hi(c + r)]),
//              every operation rounding to float32 on its own (the file is built with -ffp-contract=off), or
//              acc = fmaf(w[r], s_lo + s_hi, acc) under arith_fma = 1.  No re-association: one thread owns one voxel's sum.  The
//              reference's interior and border loops are this one formula.  lo / hi are mirrorLow / mirrorHigh (:1505-1517) as one
//              index map, clamped into the axis where the single reflection would leave it (R > n - 1: the reference is undefined).
//              Non-finite voxels are outside the contract; no index depends on a voxel's value.
// Shape:       bandwidth-bound: every pass reads and writes 4 B per voxel once, the taps come from LDS.  x pass: a workgroup
//              stages 256 voxels of one row plus R on either side.  y / z passes: one kernel over the volume as
//              [outer][n][inner]; x stays on the 64 lanes (coalesced 256 B segments), a workgroup stages 64 + 2R lines of the strided
//              axis and each of its 4 waves owns every fourth output line -- LDS rows of 64 floats, so a wave's read of one row
//              touches every bank once.  The weights travel as a kernel argument (wave-uniform, read through the scalar cache).
// DoG:         g[n + 1] - g[n] and the maximum of fabsf: a maximum is order-free, so wave shuffles, then one vector atomicMax
//              per workgroup on the bit pattern (non-negative floats order like their bits).
// Extrema:     count per workgroup, the exclusive scan of poi_split.hip, fill: the list is in scan order (octave, layer, z, y, x)
//              whatever the launch shape.
#include <algorithm>

#include "oc_device.h"
#include "oc_kernels.h"

namespace ochip {

namespace {

constexpr int kBlurBlock = 256;
constexpr int kBlurLines = 64;  // output lines of the strided axis per workgroup

__device__ __forceinline__ int sift_mirror(int i, int n) {
    if (i < 0) i = -i;
    else if (i > n - 1) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

template <bool FMA> __device__ __forceinline__ float sift_tap(float w, float lo, float hi, float acc) {
    const float pair = lo + hi;
    if (FMA) return __fmaf_rn(w, pair, acc);
    return acc + w * pair;
}

// one workgroup: kBlurBlock voxels of one row
template <bool FMA>
__global__ __launch_bounds__(kBlurBlock) void sift_blur_x_kernel(const float* __restrict__ src, float* __restrict__ dst, int nx, unsigned xtiles,
                                                                  SiftWeights W, int R) {
    __shared__ float s[kBlurBlock + 2 * kSiftMaxRadius];
    const unsigned row = blockIdx.x / xtiles, tile = blockIdx.x - row * xtiles;
    const int x0 = (int)tile * kBlurBlock;
    const float* srow = src + (size_t)row * nx;
    for (int p = threadIdx.x; p < kBlurBlock + 2 * R; p += kBlurBlock) s[p] = srow[sift_mirror(x0 - R + p, nx)];
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x >= nx) return;
    const int c = (int)threadIdx.x + R;
    float acc = W.w[0] * s[c];
    for (int r = 1; r <= R; r++) acc = sift_tap<FMA>(W.w[r], s[c - r], s[c + r], acc);
    dst[(size_t)row * nx + x] = acc;
}

// one workgroup: 64 positions of `inner` x kBlurLines lines of the blurred axis.  AXIS (1 = y, 2 = z) only names the instantiation,
// so that a kernel trace tells the two passes apart.
template <bool FMA, int AXIS>
__global__ __launch_bounds__(kBlurBlock) void sift_blur_strided_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, size_t inner,
                                                                        unsigned inner_tiles, unsigned line_tiles, SiftWeights W, int R) {
    __shared__ float s[kBlurLines + 2 * kSiftMaxRadius][64];
    unsigned b = blockIdx.x;
    const unsigned it = b % inner_tiles;
    b /= inner_tiles;
    const unsigned lt = b % line_tiles, outer = b / line_tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i = (size_t)it * 64 + lane;
    const bool live = i < inner;
    const size_t base = (size_t)outer * n * inner + (live ? i : 0);
    const int j0 = (int)lt * kBlurLines;
    const int lines = min(kBlurLines, n - j0);
    for (int p = wave; p < lines + 2 * R; p += kBlurBlock / 64)
        s[p][lane] = live ? src[base + (size_t)sift_mirror(j0 - R + p, n) * inner] : 0.f;
    __syncthreads();
    if (!live) return;
    for (int t = wave; t < lines; t += kBlurBlock / 64) {
        const int c = t + R;
        float acc = W.w[0] * s[c][lane];
        for (int r = 1; r <= R; r++) acc = sift_tap<FMA>(W.w[r], s[c - r][lane], s[c + r][lane], acc);
        dst[base + (size_t)(j0 + t) * inner] = acc;
    }
}

__global__ __launch_bounds__(256) void sift_downsample_kernel(const float* __restrict__ src, int sx, int sy, float* __restrict__ dst, int dx, int dy,
                                                              unsigned count) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= count) return;
    const unsigned k = idx % (unsigned)dx, rest = idx / (unsigned)dx;
    const unsigned j = rest % (unsigned)dy, i = rest / (unsigned)dy;
    dst[idx] = src[((size_t)(2 * i) * sy + 2 * j) * sx + 2 * k];
}

__global__ __launch_bounds__(256) void sift_dog_kernel(const float* __restrict__ g0, const float* __restrict__ g1, float* __restrict__ dog,
                                                       size_t count, unsigned* __restrict__ max_abs_bits) {
    __shared__ unsigned wave_max[4];
    float m = 0.f;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (size_t)gridDim.x * 256) {
        const float d = g1[idx] - g0[idx];
        dog[idx] = d;
        const float a = fabsf(d);
        m = m < a ? a : m;  // (:787; a NaN never becomes the maximum)
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off);
        m = m < o ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = __float_as_uint(m);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_abs_bits, max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3])));
}

// :803-830 for the voxel at linear index idx (< the layer's voxel count)
__device__ __forceinline__ bool sift_is_candidate(const SiftExtremaLayer& L, unsigned idx, unsigned count, int& x, int& y, int& z) {
    if (idx >= count) return false;
    const unsigned plane = (unsigned)L.nx * (unsigned)L.ny;
    z = (int)(idx / plane);
    const unsigned rem = idx - (unsigned)z * plane;
    y = (int)(rem / (unsigned)L.nx);
    x = (int)(rem - (unsigned)y * (unsigned)L.nx);
    if (x < 1 || x > L.nx - 2 || y < 1 || y > L.ny - 2 || z < 1 || z > L.nz - 2) return false;
    const float v = L.here[idx];
    if (!(fabsf(v) >= L.threshold)) return false;
    const float nb[8] = {L.here[idx - plane], L.here[idx + plane], L.here[idx - (unsigned)L.nx], L.here[idx + (unsigned)L.nx],
                         L.here[idx - 1],     L.here[idx + 1],     L.below[idx],                 L.above[idx]};
    bool greater = true, less = true;
    for (int q = 0; q < 8; q++) {
        greater = greater && v > nb[q];
        less = less && v < nb[q];
    }
    return greater || less;
}

constexpr int kExtremaBlock = 256;
constexpr int kExtremaRounds = kSiftExtremaVoxels / kExtremaBlock;

__global__ __launch_bounds__(kExtremaBlock) void sift_extrema_count_kernel(SiftExtremaLayer L, unsigned count, unsigned* __restrict__ block_counts) {
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int round = 0; round < kExtremaRounds; round++) {
        const unsigned idx = blockIdx.x * (unsigned)kSiftExtremaVoxels + round * kExtremaBlock + threadIdx.x;
        int x, y, z;
        const unsigned long long m = __ballot(sift_is_candidate(L, idx, count, x, y, z));
        mine += (unsigned)__popcll(m);
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        block_counts[2 * (size_t)(L.first_block + blockIdx.x)] = total;
        block_counts[2 * (size_t)(L.first_block + blockIdx.x) + 1] = 0;
    }
}

__global__ __launch_bounds__(kExtremaBlock) void sift_extrema_fill_kernel(SiftExtremaLayer L, unsigned count, const unsigned* __restrict__ block_offsets,
                                                                          SiftCandidate* __restrict__ out) {
    __shared__ unsigned wave_count[kExtremaBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned base = block_offsets[2 * (size_t)(L.first_block + blockIdx.x)];
    for (int round = 0; round < kExtremaRounds; round++) {
        const unsigned idx = blockIdx.x * (unsigned)kSiftExtremaVoxels + round * kExtremaBlock + threadIdx.x;
        int x = 0, y = 0, z = 0;
        const bool hit = sift_is_candidate(L, idx, count, x, y, z);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_count[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned at = base, all = 0;
        for (int w = 0; w < kExtremaBlock / 64; w++) {
            if (w < wave) at += wave_count[w];
            all += wave_count[w];
        }
        if (hit) {
            at += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            out[at] = SiftCandidate{x, y, z, L.octave, L.layer, L.scale};
        }
        base += all;
        __syncthreads();  // (wave_count is written again in the next round)
    }
}

}  // namespace

hipError_t launch_sift_blur_x(const float* src, float* dst, int nx, size_t rows, const SiftWeights& w, int radius, bool fma, hipStream_t stream) {
    if (nx < 1 || rows < 1 || radius < 1 || radius > kSiftMaxRadius) return hipErrorInvalidValue;
    const size_t xtiles = ((size_t)nx + kBlurBlock - 1) / kBlurBlock, blocks = rows * xtiles;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (fma) hipLaunchKernelGGL(sift_blur_x_kernel<true>, dim3((unsigned)blocks), dim3(kBlurBlock), 0, stream, src, dst, nx, (unsigned)xtiles, w, radius);
    else hipLaunchKernelGGL(sift_blur_x_kernel<false>, dim3((unsigned)blocks), dim3(kBlurBlock), 0, stream, src, dst, nx, (unsigned)xtiles, w, radius);
    return hipGetLastError();
}

hipError_t launch_sift_blur_strided(const float* src, float* dst, size_t outer, int n, size_t inner, const SiftWeights& w, int radius, bool fma,
                                    hipStream_t stream) {
    const bool z_pass = outer == 1;
    if (n < 1 || outer < 1 || inner < 1 || radius < 1 || radius > kSiftMaxRadius) return hipErrorInvalidValue;
    const size_t inner_tiles = (inner + 63) / 64, line_tiles = ((size_t)n + kBlurLines - 1) / kBlurLines, blocks = inner_tiles * line_tiles * outer;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    auto kernel = fma ? (z_pass ? sift_blur_strided_kernel<true, 2> : sift_blur_strided_kernel<true, 1>)
                      : (z_pass ? sift_blur_strided_kernel<false, 2> : sift_blur_strided_kernel<false, 1>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlurBlock), 0, stream, src, dst, n, inner, (unsigned)inner_tiles, (unsigned)line_tiles, w,
                       radius);
    return hipGetLastError();
}

hipError_t launch_sift_downsample(const float* src, int sx, int sy, float* dst, int dx, int dy, int dz, hipStream_t stream) {
    const size_t count = (size_t)dx * dy * dz;
    if (dx < 1 || dy < 1 || dz < 1 || count > 0x7fffffffull || 2 * (dx - 1) >= sx || 2 * (dy - 1) >= sy) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_downsample_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, src, sx, sy, dst, dx, dy, (unsigned)count);
    return hipGetLastError();
}

hipError_t launch_sift_dog(const float* g0, const float* g1, float* dog, size_t count, unsigned* max_abs_bits, hipStream_t stream) {
    if (count < 1) return hipErrorInvalidValue;
    const size_t blocks = std::min<size_t>((count + 255) / 256, 4096);
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_dog_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g0, g1, dog, count, max_abs_bits);
    return hipGetLastError();
}

hipError_t launch_sift_extrema_count(const SiftExtremaLayer& layer, unsigned* block_counts, hipStream_t stream) {
    const size_t count = (size_t)layer.nx * layer.ny * layer.nz;
    if (layer.nx < 1 || layer.ny < 1 || layer.nz < 1 || count > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_extrema_count_kernel, dim3((unsigned)sift_extrema_blocks(count)), dim3(kExtremaBlock), 0, stream, layer, (unsigned)count,
                       block_counts);
    return hipGetLastError();
}

hipError_t launch_sift_extrema_fill(const SiftExtremaLayer& layer, const unsigned* block_offsets, SiftCandidate* out, hipStream_t stream) {
    const size_t count = (size_t)layer.nx * layer.ny * layer.nz;
    if (layer.nx < 1 || layer.ny < 1 || layer.nz < 1 || count > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_extrema_fill_kernel, dim3((unsigned)sift_extrema_blocks(count)), dim3(kExtremaBlock), 0, stream, layer, (unsigned)count,
                       block_offsets, out);
    return hipGetLastError();
}

}  // namespace ochip

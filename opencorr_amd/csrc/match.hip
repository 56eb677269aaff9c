// match.hip -- brute-force descriptor matching: SIFT3D::bruteforceMatch, monodirectionalMatch and bidirectionalMatch of the
// reference (src/oc_sift.cpp:625-674, 1251-1418, 1420-1487) on the device.
//
// The arithmetic contract ("Descriptor matching"):
//   distance   acc = 0; for k = 0 ... dim - 1 in that order: d = a[k] - b[k]; acc = acc + d * d, every operation rounded to
//              float32 on its own (the file is built with -ffp-contract=off), or acc = fmaf(d, d, acc) under arith_fma = 1.  No
//              re-association over k, no |a|^2 + |b|^2 - 2 a.b, no matrix instructions: the order is the contract.
//   nearest    the reference scans j ascending with strict `<` against two FLT_MAX-initialised slots (:637-663).  That scan
//              returns the two smallest candidates under the lexicographic order (distance, j); a distance that is not
//              < FLT_MAX (NaN, inf, FLT_MAX) never enters a slot.  The lexicographic form has no scan order, so tiles, threads
//              and candidate parts can be folded in any grouping.
//   ratio      best < (ratio * ratio) * second in float32 (:666), second = FLT_MAX while fewer than two candidates exist.
//
// Launch shape of the distance kernel: a workgroup of 256 threads owns 64 queries and walks 64-candidate tiles; thread
// (ty, tx) of the 16 x 16 arrangement keeps a 4 x 4 register tile of accumulators (queries 4 ty ... 4 ty + 3, candidates
// 4 tx ... 4 tx + 3).  Both descriptor blocks pass through the LDS in k-chunks of 32, stored k-major ([k][row]) so that a thread's
// four queries / four candidates of one k are one 16-byte LDS read (the 16 tx lanes of a query group read 64 consecutive floats,
// the query read is a broadcast); two buffers per side = 32 KB, the next chunk travels global -> registers while the current one
// is consumed.  Per k and thread: 2 LDS reads, 16 subtractions, 16 multiplies, 16 additions (16 + 16 fused).
#include "oc_device.h"
#include "oc_kernels.h"

#include <cfloat>

namespace ochip {

namespace {

constexpr int kChunk = 32;
// Measurement builds only (tools/ablate_match.sh; the results are wrong on purpose): bit 0 = no staging after a tile's first chunk
// (no global loads, no LDS stores; the barriers stay), bit 1 = no top-2 fold (the distances are summed instead).  The library is built
// with 0.
#ifndef OC_MATCH_ABLATE
#define OC_MATCH_ABLATE 0
#endif
constexpr int kAblate = OC_MATCH_ABLATE;
constexpr int kPairBlock = 256;
constexpr unsigned long long kNoKey = ~0ull;

struct Top2 {
    float d0, d1;
    int j0, j1;
};

__device__ __forceinline__ void top2_init(Top2& t) {
    t.d0 = t.d1 = FLT_MAX;
    t.j0 = t.j1 = -1;
}

// (d, j) into the two smallest under the lexicographic order; the caller has checked d < FLT_MAX
__device__ __forceinline__ void top2_insert(Top2& t, float d, int j) {
    if (d < t.d0 || (d == t.d0 && j < t.j0)) {
        t.d1 = t.d0;
        t.j1 = t.j0;
        t.d0 = d;
        t.j0 = j;
    } else if (d < t.d1 || (d == t.d1 && j < t.j1)) {
        t.d1 = d;
        t.j1 = j;
    }
}

__device__ __forceinline__ void top2_offer(Top2& t, float d, int j) {
    if (j >= 0 && d < FLT_MAX) top2_insert(t, d, j);
}

__device__ __forceinline__ float4 load_chunk4(const float* row, bool ok, int k) {
    return ok ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void store_chunk4(float (*buf)[kMatchTile], int k, int row, const float4& v) {
    buf[k][row] = v.x;
    buf[k + 1][row] = v.y;
    buf[k + 2][row] = v.z;
    buf[k + 3][row] = v.w;
}

// DIM: compile-time descriptor length (0 = the run-time value dim_rt)
template <int DIM, bool FMA>
__global__ __launch_bounds__(256) void match_top2_kernel(const float* __restrict__ query, unsigned nq, const float* __restrict__ cand,
                                                         unsigned nc, int dim_rt, unsigned tiles_per_part, uint4* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[2][kChunk][kMatchTile];
    __shared__ __attribute__((aligned(16))) float Bs[2][kChunk][kMatchTile];
    const int dim = DIM ? DIM : dim_rt;
    const int nchunks = dim / kChunk;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const unsigned q_base = blockIdx.x * kMatchTile;
    const unsigned ctiles = (nc + kMatchTile - 1) / kMatchTile;
    const unsigned t_lo = blockIdx.y * tiles_per_part;
    const unsigned t_hi = min(t_lo + tiles_per_part, ctiles);
    // staging: thread -> row (tid & 63) and the float4 columns (tid >> 6) and (tid >> 6) + 4 of a chunk
    const int lrow = tid & 63, lcol = (tid >> 6) * 4;
    const bool qok = q_base + lrow < nq;
    const float* qrow = query + (size_t)(qok ? q_base + lrow : 0) * dim;

    Top2 top[4];
#pragma unroll
    for (int q = 0; q < 4; q++) top2_init(top[q]);

    for (unsigned t = t_lo; t < t_hi; t++) {
        const unsigned c_base = t * kMatchTile;
        const bool cok = c_base + lrow < nc;
        const float* crow = cand + (size_t)(cok ? c_base + lrow : 0) * dim;
        float acc[4][4];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[q][c] = 0.f;

        float4 a0 = load_chunk4(qrow, qok, lcol), a1 = load_chunk4(qrow, qok, lcol + 16);
        float4 b0 = load_chunk4(crow, cok, lcol), b1 = load_chunk4(crow, cok, lcol + 16);
        // (every thread has passed the barrier that ends the previous tile's last chunk: buffer 0 is free)
        store_chunk4(As[0], lcol, lrow, a0);
        store_chunk4(As[0], lcol + 16, lrow, a1);
        store_chunk4(Bs[0], lcol, lrow, b0);
        store_chunk4(Bs[0], lcol + 16, lrow, b1);
        __syncthreads();
        for (int ch = 0; ch < nchunks; ch++) {
            const int cur = ch & 1;
            const bool more = ch + 1 < nchunks && !(kAblate & 1);
            if (more) {
                const int k = (ch + 1) * kChunk + lcol;
                a0 = load_chunk4(qrow, qok, k);
                a1 = load_chunk4(qrow, qok, k + 16);
                b0 = load_chunk4(crow, cok, k);
                b1 = load_chunk4(crow, cok, k + 16);
            }
            // (unrolled by 8: a full unroll lets the compiler hoist all 64 LDS reads of a chunk -- 326 VGPRs, one wave per SIMD)
#pragma unroll 8
            for (int k = 0; k < kChunk; k++) {
                const float4 av = *reinterpret_cast<const float4*>(&As[cur][k][ty * 4]);
                const float4 bv = *reinterpret_cast<const float4*>(&Bs[cur][k][tx * 4]);
                const float a[4] = {av.x, av.y, av.z, av.w};
                const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const float d = a[q] - b[c];
                        if (FMA) acc[q][c] = __fmaf_rn(d, d, acc[q][c]);
                        else acc[q][c] = acc[q][c] + d * d;
                    }
            }
            if (more) {
                // the other buffer: its readers finished before the barrier that ended chunk ch - 1
                store_chunk4(As[cur ^ 1], lcol, lrow, a0);
                store_chunk4(As[cur ^ 1], lcol + 16, lrow, a1);
                store_chunk4(Bs[cur ^ 1], lcol, lrow, b0);
                store_chunk4(Bs[cur ^ 1], lcol + 16, lrow, b1);
            }
            __syncthreads();
        }
        // fold the tile (candidates past the end hold zeros and are skipped)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const unsigned j = c_base + tx * 4 + c;
            if (j < nc) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (kAblate & 2) top[q].d0 += acc[q][c];
                    else if (acc[q][c] < FLT_MAX) top2_insert(top[q], acc[q][c], (int)j);
                }
            }
        }
    }
    // the 16 threads of a query group are 16 consecutive lanes: butterfly under the same order
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const float pd0 = __shfl_xor(top[q].d0, off), pd1 = __shfl_xor(top[q].d1, off);
            const int pj0 = __shfl_xor(top[q].j0, off), pj1 = __shfl_xor(top[q].j1, off);
            top2_offer(top[q], pd0, pj0);
            top2_offer(top[q], pd1, pj1);
        }
        const unsigned qi = q_base + ty * 4 + q;
        if (tx == 0 && qi < nq)
            part[(size_t)blockIdx.y * nq + qi] = make_uint4(__float_as_uint(top[q].d0), (unsigned)top[q].j0, __float_as_uint(top[q].d1), (unsigned)top[q].j1);
    }
}

__global__ __launch_bounds__(kPairBlock) void match_finalize_kernel(const uint4* __restrict__ part, unsigned nq, int splits, float ratio_sq,
                                                                    int* __restrict__ matched_idx, float* __restrict__ best,
                                                                    float* __restrict__ second, unsigned* __restrict__ counter) {
    const unsigned i = blockIdx.x * kPairBlock + threadIdx.x;
    bool pass = false;
    if (i < nq) {
        Top2 t;
        top2_init(t);
        for (int s = 0; s < splits; s++) {
            const uint4 p = part[(size_t)s * nq + i];
            top2_offer(t, __uint_as_float(p.x), (int)p.y);
            top2_offer(t, __uint_as_float(p.z), (int)p.w);
        }
        pass = t.j0 >= 0 && t.d0 < ratio_sq * t.d1;  // src/oc_sift.cpp:666
        matched_idx[i] = pass ? t.j0 : -1;
        best[i] = t.d0;
        second[i] = t.d1;
    }
    const unsigned long long m = __ballot(pass);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned)__popcll(m));
}

__device__ __forceinline__ unsigned long long match_key(float d, unsigned i) {
    return ((unsigned long long)__float_as_uint(d) << 32) | i;  // d >= 0: the bit pattern orders like the value
}

// round 0: the smallest (distance, ref index) of every target slot; round 1: the smallest of the rest
__global__ __launch_bounds__(kPairBlock) void match_group_min_kernel(const int* __restrict__ r2t, const float* __restrict__ best, unsigned nr,
                                                                     unsigned nt, unsigned long long* __restrict__ keys, int round) {
    const unsigned i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= nr) return;
    const int j = r2t[i];
    if (j < 0 || (unsigned)j >= nt) return;
    const unsigned long long key = match_key(best[i], i);
    if (round == 0) atomicMin(&keys[j], key);
    else if (key != keys[j]) atomicMin(&keys[nt + j], key);
}

// the pair at output position p, if one survives there
template <int MODE>
__device__ __forceinline__ bool match_pair_at(unsigned p, const int* __restrict__ r2t, const int* __restrict__ t2r,
                                              const unsigned long long* __restrict__ keys, unsigned nr, unsigned nt, float ratio_sq, int& ref,
                                              int& tar) {
    if (MODE == 0) {
        // descending target index (the order the reference's two sorts leave, :1307, :1325); the group's smallest stays when
        // d0 < ratio^2 * d1 (:1361-1387), d1 = FLT_MAX for a group of one
        if (p >= nt) return false;
        const unsigned j = nt - 1 - p;
        const unsigned long long k0 = keys[j], k1 = keys[nt + j];
        if (k0 == kNoKey) return false;
        const float d0 = __uint_as_float((unsigned)(k0 >> 32));
        const float d1 = k1 == kNoKey ? FLT_MAX : __uint_as_float((unsigned)(k1 >> 32));
        ref = (int)(unsigned)(k0 & 0xffffffffull);
        tar = (int)j;
        return d0 < ratio_sq * d1;
    }
    // bidirectional (:1436-1445): ascending reference index
    if (p >= nr) return false;
    const int j = r2t[p];
    if (j < 0 || (unsigned)j >= nt) return false;
    ref = (int)p;
    tar = j;
    return t2r[j] == (int)p;
}

template <int MODE>
__global__ __launch_bounds__(kPairBlock) void match_pairs_count_kernel(const int* __restrict__ r2t, const int* __restrict__ t2r,
                                                                       const unsigned long long* __restrict__ keys, unsigned nr, unsigned nt,
                                                                       float ratio_sq, unsigned* __restrict__ block_counts) {
    __shared__ unsigned n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    int ref, tar;
    const bool keep = match_pair_at<MODE>(blockIdx.x * kPairBlock + threadIdx.x, r2t, t2r, keys, nr, nt, ratio_sq, ref, tar);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) atomicAdd(&n, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        block_counts[2 * blockIdx.x] = n;
        block_counts[2 * blockIdx.x + 1] = 0;
    }
}

template <int MODE>
__global__ __launch_bounds__(kPairBlock) void match_pairs_scatter_kernel(const int* __restrict__ r2t, const int* __restrict__ t2r,
                                                                         const unsigned long long* __restrict__ keys, unsigned nr, unsigned nt,
                                                                         float ratio_sq, const unsigned* __restrict__ block_offsets,
                                                                         int* __restrict__ ref_idx, int* __restrict__ tar_idx) {
    __shared__ unsigned wave_n[kPairBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ref = -1, tar = -1;
    const bool keep = match_pair_at<MODE>(blockIdx.x * kPairBlock + threadIdx.x, r2t, t2r, keys, nr, nt, ratio_sq, ref, tar);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned base = block_offsets[2 * blockIdx.x];
    for (int w = 0; w < wave; w++) base += wave_n[w];
    if (keep) {
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        const unsigned r = base + (unsigned)__popcll(m & below);
        ref_idx[r] = ref;
        tar_idx[r] = tar;
    }
}

unsigned pair_positions(size_t n_ref, size_t n_tar, int mode) { return (unsigned)(mode == 0 ? n_tar : n_ref); }

}  // namespace

bool match_dim_supported(int dim) { return dim >= 32 && dim <= 1024 && dim % kChunk == 0; }

hipError_t launch_match_top2(const float* query, size_t n_query, const float* cand, size_t n_cand, int dim, int splits, bool fma,
                             void* partials, hipStream_t stream) {
    if (n_query == 0) return hipSuccess;
    if (!match_dim_supported(dim) || splits < 1 || splits > kMatchMaxSplits || n_query > 0x7fffffffull || n_cand > 0x7fffffffull)
        return hipErrorInvalidValue;
    const unsigned nq = (unsigned)n_query, nc = (unsigned)n_cand;
    const unsigned ctiles = (nc + kMatchTile - 1) / kMatchTile;
    const unsigned per = (ctiles + splits - 1) / splits;  // (0 tiles: every part writes the empty record)
    const dim3 grid((nq + kMatchTile - 1) / kMatchTile, splits), block(256);
    uint4* part = static_cast<uint4*>(partials);
    (void)hipGetLastError();
#define OC_MATCH_LAUNCH(DIM)                                                                                                          \
    do {                                                                                                                              \
        if (fma) hipLaunchKernelGGL((match_top2_kernel<DIM, true>), grid, block, 0, stream, query, nq, cand, nc, dim, per, part);      \
        else hipLaunchKernelGGL((match_top2_kernel<DIM, false>), grid, block, 0, stream, query, nq, cand, nc, dim, per, part);         \
    } while (0)
    if (dim == 768) OC_MATCH_LAUNCH(768);
    else if (dim == 128) OC_MATCH_LAUNCH(128);
    else OC_MATCH_LAUNCH(0);
#undef OC_MATCH_LAUNCH
    return hipGetLastError();
}

hipError_t launch_match_finalize(const void* partials, size_t n_query, int splits, float ratio_sq, int* matched_idx, float* best,
                                 float* second, unsigned* counter, hipStream_t stream) {
    hipError_t err = hipMemsetAsync(counter, 0, sizeof(unsigned), stream);
    if (err != hipSuccess || n_query == 0) return err;
    if (n_query > 0x7fffffffull || splits < 1 || splits > kMatchMaxSplits) return hipErrorInvalidValue;
    const unsigned nq = (unsigned)n_query;
    (void)hipGetLastError();
    hipLaunchKernelGGL(match_finalize_kernel, dim3((nq + kPairBlock - 1) / kPairBlock), dim3(kPairBlock), 0, stream,
                       static_cast<const uint4*>(partials), nq, splits, ratio_sq, matched_idx, best, second, counter);
    return hipGetLastError();
}

hipError_t launch_match_many_to_one(const int* r2t, const float* best, size_t n_ref, size_t n_tar, unsigned long long* keys,
                                    hipStream_t stream) {
    if (n_tar == 0) return hipSuccess;
    if (n_ref > 0x7fffffffull || n_tar > 0x7fffffffull) return hipErrorInvalidValue;
    hipError_t err = hipMemsetAsync(keys, 0xff, 2 * n_tar * sizeof(unsigned long long), stream);
    if (err != hipSuccess || n_ref == 0) return err;
    const unsigned nr = (unsigned)n_ref, nt = (unsigned)n_tar;
    (void)hipGetLastError();
    for (int round = 0; round < 2; round++)
        hipLaunchKernelGGL(match_group_min_kernel, dim3((nr + kPairBlock - 1) / kPairBlock), dim3(kPairBlock), 0, stream, r2t, best, nr, nt,
                           keys, round);
    return hipGetLastError();
}

// per-block counts (2 per block) | totals[2]
size_t match_pairs_scratch_words(size_t n_ref, size_t n_tar, int mode) {
    const size_t n = mode == 0 ? n_tar : n_ref;
    return 2 * ((n + kPairBlock - 1) / kPairBlock) + 2;
}

hipError_t launch_match_pairs_count(int mode, const int* r2t, const int* t2r, const unsigned long long* keys, size_t n_ref, size_t n_tar,
                                    float ratio_sq, unsigned* scratch, hipStream_t stream) {
    if (n_ref > 0x7fffffffull || n_tar > 0x7fffffffull) return hipErrorInvalidValue;
    const unsigned n = pair_positions(n_ref, n_tar, mode);
    const unsigned nblocks = (n + kPairBlock - 1) / kPairBlock;
    unsigned* totals = scratch + 2 * (size_t)nblocks;
    if (n == 0 || n_ref == 0 || n_tar == 0) return hipMemsetAsync(totals, 0, 2 * sizeof(unsigned), stream);
    const unsigned nr = (unsigned)n_ref, nt = (unsigned)n_tar;
    (void)hipGetLastError();
    if (mode == 0)
        hipLaunchKernelGGL(match_pairs_count_kernel<0>, dim3(nblocks), dim3(kPairBlock), 0, stream, r2t, t2r, keys, nr, nt, ratio_sq, scratch);
    else
        hipLaunchKernelGGL(match_pairs_count_kernel<1>, dim3(nblocks), dim3(kPairBlock), 0, stream, r2t, t2r, keys, nr, nt, ratio_sq, scratch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    return launch_block_count_scan(scratch, nblocks, totals, stream);
}

hipError_t launch_match_pairs_scatter(int mode, const int* r2t, const int* t2r, const unsigned long long* keys, size_t n_ref,
                                      size_t n_tar, float ratio_sq, const unsigned* scratch, int* ref_idx, int* tar_idx,
                                      hipStream_t stream) {
    const unsigned n = pair_positions(n_ref, n_tar, mode);
    if (n == 0 || n_ref == 0 || n_tar == 0) return hipSuccess;
    const unsigned nblocks = (n + kPairBlock - 1) / kPairBlock;
    const unsigned nr = (unsigned)n_ref, nt = (unsigned)n_tar;
    (void)hipGetLastError();
    if (mode == 0)
        hipLaunchKernelGGL(match_pairs_scatter_kernel<0>, dim3(nblocks), dim3(kPairBlock), 0, stream, r2t, t2r, keys, nr, nt, ratio_sq, scratch,
                           ref_idx, tar_idx);
    else
        hipLaunchKernelGGL(match_pairs_scatter_kernel<1>, dim3(nblocks), dim3(kPairBlock), 0, stream, r2t, t2r, keys, nr, nt, ratio_sq, scratch,
                           ref_idx, tar_idx);
    return hipGetLastError();
}

}  // namespace ochip

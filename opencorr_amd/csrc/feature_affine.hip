// feature_affine.hip -- FeatureAffine2D/3D::compute(poi_queue) on gfx950: the RANSAC affine fit over the matched keypoints
// around every POI (src/oc_feature_affine.cpp:118-342 in 2D, :431-608 in 3D), seeded and deterministic.
//
// The neighbour search is Strain's: a uniform grid over the REFERENCE keypoints (pitch >= search radius, so the 3 x 3 (x 3)
// block around a POI's cell holds every neighbour), keypoints sorted by cell and by ascending index inside a cell, gathered
// into 32-byte records {ref xyz, tar x | tar yz, keypoint index, -}.
//
// compute: one wave owns one POI.  Its lanes stride over the records of the block's rows, the keypoints inside the radius are
// compacted (ballot + prefix count, so the list is in walk order whatever the timing) as POI-centred coordinates into the
// wave's own slice of LDS -- structure of arrays, 2 * DIM arrays of kFeatureAffineListLds floats -- and, past that many, into
// the wave's slice of a global scratch block.  Every trial then is
//   * the sample: a partial Fisher-Yates over the list positions with a counter-based generator (splitmix64 of the seed, the
//     POI's coordinates, the trial and the draw), tracked in registers, the same in every lane;
//   * the solve: lane e accumulates entry e of the normal equations in double over the sample's rows in order, the entries are
//     handed round, and every lane eliminates the (DIM + 1) x (DIM + 1) system with partial pivoting in double;
//   * the consensus: lanes stride over the list with the reference's float32 expressions; a lane adds the errors of its inliers
//     in ascending position and the 64 partials are combined by the xor butterfly of oc_device.h.
// Only the size and the trial number of the largest consensus set are kept; the set itself is formed again at the end (one
// more sweep), compacted in place to the front of the list, and fitted by the same routine in list order.
// Nothing here is atomic and nothing depends on which wave runs when: a POI's record is a function of its coordinates, the
// keypoints, the settings and the seed.
#include "oc_device.h"
#include "oc_kernels.h"

namespace ochip {

namespace {

constexpr int kFaWaves = 4;                             // waves of a workgroup, one POI each
constexpr int kFaLds = kFeatureAffineListLds;
constexpr int kFaLdsStride = kFaLds + 1;                // (+1: the 2 * DIM arrays start on different banks)
constexpr int kFaMax = kFeatureAffineListMax;
constexpr int kFaFeature3d = 21;                        // Result3D::feature (src/oc_poi.h:93-99): the float behind convergence

struct alignas(16) FaRec {
    float rx, ry, rz, tx;
    float ty, tz;
    unsigned idx, pad;
};

// cell of one coordinate: Strain's rule (strain.hip cell_axis)
__device__ __forceinline__ int fa_cell_axis(float c, float c0, float inv_pitch, int nc) {
    const float t = (c - c0) * inv_pitch;
    return t >= 0.f ? (t < (float)nc ? (int)t : nc - 1) : 0;
}

template <int DIM>
__device__ __forceinline__ void fa_cell_of(float x, float y, float z, const StrainGrid& g, int& cx, int& cy, int& cz) {
    cx = fa_cell_axis(x, g.x0, g.inv_pitch, g.ncx);
    cy = fa_cell_axis(y, g.y0, g.inv_pitch, g.ncy);
    cz = DIM == 3 ? fa_cell_axis(z, g.z0, g.inv_pitch, g.ncz) : 0;
}

// nanoflann L2_Simple, as Strain: sum over the dimensions of (query - point)^2, in order
template <int DIM>
__device__ __forceinline__ float fa_dist2(float px, float py, float pz, float x, float y, float z) {
    const float dx = px - x, dy = py - y;
    float d = dx * dx;
    d = d + dy * dy;
    if constexpr (DIM == 3) {
        const float dz = pz - z;
        d = d + dz * dz;
    }
    return d;
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// lanes below this one whose bit is set
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// orders the LDS / scratch traffic of the wave's lanes among themselves (a wave's slice is its own: no workgroup barrier)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a wave's candidate list: array c (0 ... DIM-1 ref - POI, DIM ... 2 DIM-1 tar - POI), position j
template <int DIM>
struct CandList {
    float* lds;
    float* ext;     // null when no POI of the launch has more than kFaLds candidates
    int ext_pitch;  // entries per array of the global slice: the launch's largest candidate count beyond kFaLds, rounded up
    __device__ __forceinline__ bool holds(int j) const { return j < kFaLds || (ext != nullptr && j - kFaLds < ext_pitch); }
    __device__ __forceinline__ float get(int c, int j) const {
        return j < kFaLds ? lds[c * kFaLdsStride + j] : ext[(size_t)c * ext_pitch + (j - kFaLds)];
    }
    __device__ __forceinline__ void put(int c, int j, float v) const {
        if (j < kFaLds) lds[c * kFaLdsStride + j] = v;
        else ext[(size_t)c * ext_pitch + (j - kFaLds)] = v;
    }
    __device__ __forceinline__ void put_local(int j, const float4& a, const float4& b, float px, float py, float pz) const {
        // src/oc_feature_affine.cpp:226-230 / :481-485
        put(0, j, a.x - px);
        put(1, j, a.y - py);
        if constexpr (DIM == 3) {
            put(2, j, a.z - pz);
            put(3, j, a.w - px);
            put(4, j, b.x - py);
            put(5, j, b.y - pz);
        } else {
            put(2, j, a.w - px);
            put(3, j, b.x - py);
        }
    }
};

// The radius walk: rows of the block in row-major order, one contiguous run of records per row, ascending keypoint index
// inside a cell.  STORE: the keypoints inside the radius go to the list in that order.  Returns their number.
template <int DIM, bool STORE>
__device__ __forceinline__ unsigned fa_radius_walk(const float4* __restrict__ rv, const unsigned* __restrict__ start, const StrainGrid& g,
                                                   float px, float py, float pz, float radius2, const CandList<DIM>& L, int lane) {
    int cx, cy, cz;
    fa_cell_of<DIM>(px, py, pz, g, cx, cy, cz);
    unsigned n = 0;
    for (int dz = (DIM == 3 ? -1 : 0); dz <= (DIM == 3 ? 1 : 0); dz++)
        for (int dy = -1; dy <= 1; dy++) {
            const int y = cy + dy, z = cz + dz;
            if (y < 0 || z < 0 || y >= g.ncy || z >= g.ncz) continue;
            const int xa = max(cx - 1, 0), xb = min(cx + 1, g.ncx - 1);
            const size_t rowc = ((size_t)z * g.ncy + y) * g.ncx;
            const unsigned s = start[rowc + xa], e = start[rowc + xb + 1];
            for (unsigned base = s; base < e; base += kWave) {
                const unsigned q = base + lane;
                bool in = false;
                float4 a = {0.f, 0.f, 0.f, 0.f};
                if (q < e) {
                    a = rv[2 * (size_t)q];
                    in = fa_dist2<DIM>(px, py, pz, a.x, a.y, a.z) < radius2;
                }
                const unsigned long long mask = __ballot(in);
                if constexpr (STORE) {
                    if (in) {
                        const unsigned pos = n + lanes_below(mask);
                        if (pos < (unsigned)kFaMax && L.holds((int)pos)) L.put_local((int)pos, a, rv[2 * (size_t)q + 1], px, py, pz);
                    }
                }
                n += (unsigned)__popcll(mask);
            }
        }
    return n;
}

// The K nearest keypoints by ascending (distance^2, keypoint index), ring by ring as Strain's KNN path; lane i ends with the
// record slot of the i-th nearest.  The sorted list lives across the lanes: a keypoint that precedes the K-th entry is
// inserted where the count of entries before it says, the lanes behind move up by one.
template <int DIM>
__device__ __forceinline__ int fa_knn(const float4* __restrict__ rv, const unsigned* __restrict__ start, const StrainGrid& g, float px,
                                      float py, float pz, int K, int lane, unsigned& my_q) {
    int cx, cy, cz;
    fa_cell_of<DIM>(px, py, pz, g, cx, cy, cz);
    float my_d = INFINITY;
    unsigned my_i = 0xffffffffu;
    my_q = 0;
    int have = 0;
    const float pitch = 1.f / g.inv_pitch;
    // the last ring that holds a cell of the grid; the shell of a ring is walked over its faces only and clipped to the grid,
    // so a POI far from every keypoint costs at most one visit of every cell (the K-th distance never ends its search early)
    const int reach = max(max(max(cx, g.ncx - 1 - cx), max(cy, g.ncy - 1 - cy)), max(cz, g.ncz - 1 - cz));
    for (int ring = 0; ring <= reach; ring++) {
        for (int dz = (DIM == 3 ? max(-ring, -cz) : 0); dz <= (DIM == 3 ? min(ring, g.ncz - 1 - cz) : 0); dz++)
            for (int dy = max(-ring, -cy); dy <= min(ring, g.ncy - 1 - cy); dy++) {
                // rows on a face of the shell take every x; the others its two ends
                const bool face = abs(dy) == ring || (DIM == 3 && abs(dz) == ring);
                const int lo = face ? max(-ring, -cx) : -ring, hi = face ? min(ring, g.ncx - 1 - cx) : ring;
                const int step = face || ring == 0 ? 1 : 2 * ring;
                for (int dx = lo; dx <= hi; dx += step) {
                    const int x = cx + dx, y = cy + dy, z = cz + dz;
                    if (x < 0 || x >= g.ncx) continue;
                    const size_t c = ((size_t)z * g.ncy + y) * g.ncx + x;
                    const unsigned s = start[c], e = start[c + 1];
                    for (unsigned base = s; base < e; base += kWave) {
                        const unsigned q = base + lane;
                        bool ok = false;
                        float d = 0.f;
                        unsigned idx = 0;
                        if (q < e) {
                            const float4 a = rv[2 * (size_t)q];
                            idx = __float_as_uint(rv[2 * (size_t)q + 1].z);
                            d = fa_dist2<DIM>(px, py, pz, a.x, a.y, a.z);
                            ok = d == d;  // NaN coordinates never enter
                        }
                        unsigned long long m = __ballot(ok);
                        while (m) {
                            const int src = __ffsll((long long)m) - 1;
                            m &= m - 1;
                            const float cd = __shfl(d, src);
                            const unsigned ci = __shfl(idx, src), cq = __shfl(q, src);
                            const bool before = lane < have && (my_d < cd || (my_d == cd && my_i < ci));
                            const int pos = __popcll(__ballot(before));
                            if (pos >= K) continue;
                            const float ud = __shfl_up(my_d, 1);
                            const unsigned ui = __shfl_up(my_i, 1), uq = __shfl_up(my_q, 1);
                            if (lane > pos && lane <= have && lane < K) {
                                my_d = ud;
                                my_i = ui;
                                my_q = uq;
                            }
                            if (lane == pos) {
                                my_d = cd;
                                my_i = ci;
                                my_q = cq;
                            }
                            if (have < K) have++;
                        }
                    }
                }
            }
        // everything in rings > `ring` is at least ring * pitch away (0.999: slack for the rounding of the cell assignment)
        if (have == K) {
            const float lim = (float)ring * pitch * 0.999f;
            if (__shfl(my_d, K - 1) < lim * lim) break;
        }
    }
    return have;
}

// The sample of trial t: s positions out of 0 ... n-1, a partial Fisher-Yates that starts from the identity every trial.
// The swaps are tracked as (position, value) pairs: position mpos[i] holds mval[i], every other position holds itself.
__device__ __forceinline__ void fa_sample(unsigned long long base, int t, int n, int s, int (&smp)[8]) {
    unsigned mpos[8];
    int mval[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        smp[j] = 0;
        mpos[j] = 0xffffffffu;
        mval[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j < s) {
            const unsigned long long h = splitmix64(base + (((unsigned long long)(unsigned)t << 8) | (unsigned long long)j));
            const unsigned k = (unsigned)j + (unsigned)(((h >> 32) * (unsigned long long)(unsigned)(n - j)) >> 32);
            int vj = j, vk = (int)k;
#pragma unroll
            for (int i = 0; i < j; i++) {
                if (mpos[i] == (unsigned)j) vj = mval[i];
                if (mpos[i] == k) vk = mval[i];
            }
            smp[j] = vk;
            bool found = false;
#pragma unroll
            for (int i = 0; i < j; i++)
                if (mpos[i] == k) {
                    mval[i] = vj;
                    found = true;
                }
            mpos[j] = found ? 0xffffffffu : k;
            mval[j] = vj;
        }
    }
}

// column c of the row [x y (z) 1 | x' y' (z')] of list position j
template <int DIM>
__device__ __forceinline__ double fa_row(const CandList<DIM>& L, int c, int j) {
    if (c == DIM) return 1.0;
    return (double)L.get(c < DIM ? c : c - 1, j);
}

// Least squares of [x y (z) 1] X = [x' y' (z')] over `rows` rows of the list -- the sample's positions in sample order
// (SAMPLE) or positions 0 ... rows-1 in order: normal equations in double, lane e owning entry e (ia, ib: the two columns it
// multiplies), Gaussian elimination with partial pivoting in double, X rounded to float once.  false: singular.
template <int DIM, bool SAMPLE>
__device__ __forceinline__ bool fa_fit(const CandList<DIM>& L, const int (&smp)[8], int rows, int ia, int ib, float (&X)[DIM + 1][DIM]) {
    constexpr int D = DIM + 1;
    double acc = 0.0;
    if constexpr (SAMPLE) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (i < rows) acc = acc + fa_row<DIM>(L, ia, smp[i]) * fa_row<DIM>(L, ib, smp[i]);
    } else {
        for (int j = 0; j < rows; j++) acc = acc + fa_row<DIM>(L, ia, j) * fa_row<DIM>(L, ib, j);
    }
    // every lane takes all entries: upper triangle of A^T A row-major, then A^T B row-major
    double A[D][D + DIM];
    int e = 0;
#pragma unroll
    for (int a = 0; a < D; a++)
#pragma unroll
        for (int b = a; b < D; b++) {
            const double v = __shfl(acc, e++);
            A[a][b] = v;
            A[b][a] = v;
        }
#pragma unroll
    for (int a = 0; a < D; a++)
#pragma unroll
        for (int r = 0; r < DIM; r++) A[a][D + r] = __shfl(acc, e++);
    double big = 0.0;
#pragma unroll
    for (int a = 0; a < D; a++)
#pragma unroll
        for (int b = 0; b < D; b++) big = fabs(A[a][b]) > big ? fabs(A[a][b]) : big;
    const double tiny = big * 0x1p-40;
    double rinv[D];
    bool singular = false;
#pragma unroll
    for (int k = 0; k < D; k++) {
        int p = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < D; i++)
            if (fabs(A[i][k]) > best) {
                best = fabs(A[i][k]);
                p = i;
            }
        if (!(best >= tiny)) singular = true;
#pragma unroll
        for (int i = k + 1; i < D; i++)
            if (p == i) {
#pragma unroll
                for (int j = 0; j < D + DIM; j++) {
                    const double t = A[k][j];
                    A[k][j] = A[i][j];
                    A[i][j] = t;
                }
            }
        rinv[k] = 1.0 / A[k][k];
#pragma unroll
        for (int i = k + 1; i < D; i++) {
            const double f = A[i][k] * rinv[k];
#pragma unroll
            for (int j = k + 1; j < D + DIM; j++) A[i][j] = A[i][j] - f * A[k][j];
        }
    }
    if (singular) return false;
#pragma unroll
    for (int r = 0; r < DIM; r++) {
        double x[D];
#pragma unroll
        for (int k = D - 1; k >= 0; k--) {
            double v = A[k][D + r];
#pragma unroll
            for (int j = k + 1; j < D; j++) v = v - A[k][j] * x[j];
            x[k] = v * rinv[k];
        }
#pragma unroll
        for (int k = 0; k < D; k++) X[k][r] = (float)x[k];
    }
    return true;
}

// estimation error of list position j under X (src/oc_feature_affine.cpp:262-275 / :519-537), c: the position's 2 DIM floats
template <int DIM>
__device__ __forceinline__ float fa_error(const float (&c)[2 * DIM], const float (&X)[DIM + 1][DIM]) {
    if constexpr (DIM == 2) {
        const float dx = (c[0] * X[0][0] + c[1] * X[1][0] + X[2][0]) - c[2];
        const float dy = (c[0] * X[0][1] + c[1] * X[1][1] + X[2][1]) - c[3];
        return sqrtf(dx * dx + dy * dy);
    } else {
        const float dx = (c[0] * X[0][0] + c[1] * X[1][0] + c[2] * X[2][0] + X[3][0]) - c[3];
        const float dy = (c[0] * X[0][1] + c[1] * X[1][1] + c[2] * X[2][1] + X[3][1]) - c[4];
        const float dz = (c[0] * X[0][2] + c[1] * X[1][2] + c[2] * X[2][2] + X[3][2]) - c[5];
        return sqrtf(dx * dx + dy * dy + dz * dz);
    }
}

// The consensus sweep.  Returns the number of inliers; `sum`: their errors added up (lane partials in ascending position, then
// the xor butterfly).  COMPACT: the inliers move to the front of the list, in order (a position is only ever written from
// the chunk that holds it or a later one, whose floats are in registers by then).
template <int DIM, bool COMPACT>
__device__ __forceinline__ int fa_consensus(const CandList<DIM>& L, int n, const float (&X)[DIM + 1][DIM], float threshold, int lane,
                                            float& sum) {
    float part = 0.f;
    int count = 0;
    for (int base = 0; base < n; base += kWave) {
        const int j = base + lane;
        float c[2 * DIM];
        bool in = false;
        float err = 0.f;
        if (j < n) {
#pragma unroll
            for (int k = 0; k < 2 * DIM; k++) c[k] = L.get(k, j);
            err = fa_error<DIM>(c, X);
            in = err < threshold;
        }
        const unsigned long long mask = __ballot(in);
        if constexpr (COMPACT) {
            wave_sync();
            if (in) {
                const int pos = count + lanes_below(mask);
#pragma unroll
                for (int k = 0; k < 2 * DIM; k++) L.put(k, pos, c[k]);
            }
            wave_sync();
        } else {
            if (in) part = part + err;
        }
        count += __popcll(mask);
    }
    sum = COMPACT ? 0.f : wave_allreduce_sum(part);
    return count;
}

template <int DIM>
__global__ __launch_bounds__(kFaWaves* kWave) void feature_affine_gather_kernel(const float* __restrict__ ref, const float* __restrict__ tar,
                                                                                unsigned count, const unsigned* __restrict__ order,
                                                                                FaRec* __restrict__ recs) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const unsigned i = order[k];
    const float* r = ref + (size_t)i * DIM;
    const float* t = tar + (size_t)i * DIM;
    FaRec o;
    o.rx = r[0];
    o.ry = r[1];
    o.rz = DIM == 3 ? r[DIM - 1] : 0.f;
    o.tx = t[0];
    o.ty = t[1];
    o.tz = DIM == 3 ? t[DIM - 1] : 0.f;
    o.idx = i;
    o.pad = 0;
    recs[k] = o;
}

template <int DIM>
__global__ __launch_bounds__(256) void feature_affine_pairs_kernel(const float* __restrict__ ref_kp, const float* __restrict__ tar_kp,
                                                                   const int* __restrict__ ref_idx, const int* __restrict__ tar_idx,
                                                                   unsigned n, float* __restrict__ out_ref, float* __restrict__ out_tar,
                                                                   unsigned* __restrict__ negative) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (ref_idx[k] < 0 || tar_idx[k] < 0) {  // (the matcher's -1 for "no match", or a stale list: nothing is read through it)
        atomicMin(negative, k);
        return;
    }
    const size_t r = (size_t)ref_idx[k], t = (size_t)tar_idx[k];
#pragma unroll
    for (int a = 0; a < DIM; a++) {
        out_ref[(size_t)k * DIM + a] = ref_kp[r * DIM + a];
        out_tar[(size_t)k * DIM + a] = tar_kp[t * DIM + a];
    }
}

// the verdict of a queue before anything is written: see launch_feature_affine_count
template <int DIM>
__global__ __launch_bounds__(kFaWaves* kWave) void feature_affine_count_kernel(const float* __restrict__ pois, int stride_f, unsigned count,
                                                                               StrainGrid g, FeatureAffineParams P,
                                                                               const unsigned* __restrict__ start,
                                                                               const FaRec* __restrict__ recs, unsigned* __restrict__ verdict) {
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned nwaves = gridDim.x * kFaWaves;
    const float4* rv = reinterpret_cast<const float4*>(recs);
    const CandList<DIM> none = {nullptr, nullptr, 0};
    for (unsigned p = blockIdx.x * kFaWaves + (threadIdx.x >> 6); p < count; p += nwaves) {
        const float* poi = pois + (size_t)p * stride_f;
        const float px = poi[0], py = poi[1], pz = DIM == 3 ? poi[2] : 0.f;
        if (!(px == px) || !(py == py) || !(pz == pz)) {
            if (lane == 0) atomicMin(verdict + 2, p);
            continue;
        }
        if (P.self_adaptive) continue;
        const unsigned n = fa_radius_walk<DIM, false>(rv, start, g, px, py, pz, P.radius2, none, lane);
        if (lane == 0) {
            atomicMax(verdict, n);
            if (n > (unsigned)kFaMax) atomicMin(verdict + 1, p);
        }
    }
}

template <int DIM>
__global__ __launch_bounds__(kFaWaves* kWave) void feature_affine_kernel(float* __restrict__ pois, int stride_f, unsigned count, StrainGrid g,
                                                                         FeatureAffineParams P, const unsigned* __restrict__ start,
                                                                         const FaRec* __restrict__ recs, float* __restrict__ scratch, int ext_pitch) {
    constexpr int D = DIM + 1, NS = D * (D + 1) / 2, NE = NS + D * DIM;
    extern __shared__ __attribute__((aligned(16))) float fa_lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const unsigned slot = blockIdx.x * kFaWaves + wave, nwaves = gridDim.x * kFaWaves;
    const float4* rv = reinterpret_cast<const float4*>(recs);
    CandList<DIM> L;
    L.lds = fa_lds + (size_t)wave * (2 * DIM) * kFaLdsStride;
    L.ext = scratch ? scratch + (size_t)slot * (2 * DIM) * ext_pitch : nullptr;
    L.ext_pitch = ext_pitch;
    // the entry of the normal equations this lane owns: columns ia, ib of [x y (z) 1 | x' y' (z')]
    int ia = DIM, ib = DIM;
    {
        int e = 0;
        for (int a = 0; a < D; a++)
            for (int b = a; b < D; b++, e++)
                if (e == lane) ia = a, ib = b;
        for (int a = 0; a < D; a++)
            for (int r = 0; r < DIM; r++, e++)
                if (e == lane) ia = a, ib = D + r;
        static_assert(NE <= kWave, "one lane per entry");
    }
    const int s = P.sample_number, nmin = P.neighbor_min;
    const float exit_mean = P.error_threshold / (float)nmin;  // :292 / :551
    for (unsigned p = slot; p < count; p += nwaves) {
        float* poi = pois + (size_t)p * stride_f;
        float px = poi[0], py = poi[1], pz = DIM == 3 ? poi[2] : 0.f;
        // the key of the generator: the coordinates the POI came with
        unsigned long long base = splitmix64(P.seed ^ ((unsigned long long)__float_as_uint(px) | ((unsigned long long)__float_as_uint(py) << 32)));
        if constexpr (DIM == 3) base = splitmix64(base ^ (unsigned long long)__float_as_uint(pz));
        int n = 0;
        wave_sync();  // the previous POI's reads of the list are over
        if (DIM == 2 && P.self_adaptive) {
            // :128-179: the subset_feature_min nearest keypoints, their bounding box, the POI and its subset radii follow
            unsigned my_q;
            n = fa_knn<DIM>(rv, start, g, px, py, pz, P.feature_min, lane, my_q);
            if (n < s) {
                if (lane == 0) poi[poi2d::ZNCC] = -1.f;
                continue;
            }
            float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            float x_min = P.width, x_max = -1.f, y_min = P.height, y_max = -1.f;
            if (lane < n) {
                a = rv[2 * (size_t)my_q];
                b = rv[2 * (size_t)my_q + 1];
                x_min = a.x < x_min ? a.x : x_min;
                x_max = a.x > x_max ? a.x : x_max;
                y_min = a.y < y_min ? a.y : y_min;
                y_max = a.y > y_max ? a.y : y_max;
            }
            for (int off = 32; off > 0; off >>= 1) {
                x_min = fminf(x_min, __shfl_xor(x_min, off));
                x_max = fmaxf(x_max, __shfl_xor(x_max, off));
                y_min = fminf(y_min, __shfl_xor(y_min, off));
                y_max = fmaxf(y_max, __shfl_xor(y_max, off));
            }
            int srx, sry;
            if (px >= x_min && px <= x_max && py >= y_min && py <= y_max) {
                srx = fabsf(x_max - px) > fabsf(px - x_min) ? (int)fabsf(x_max - px) : (int)fabsf(px - x_min);
                sry = fabsf(y_max - py) > fabsf(py - y_min) ? (int)fabsf(y_max - py) : (int)fabsf(py - y_min);
            } else {
                px = (float)(int)(0.5f * (x_max + x_min));
                py = (float)(int)(0.5f * (y_max + y_min));
                srx = (int)(0.5f * (x_max - x_min));
                sry = (int)(0.5f * (y_max - y_min));
            }
            srx = srx < P.radius_min ? P.radius_min : srx;
            sry = sry < P.radius_min ? P.radius_min : sry;
            if (lane == 0) {
                poi[poi2d::X] = px;
                poi[poi2d::Y] = py;
                poi[poi2d::SRX] = (float)srx;
                poi[poi2d::SRY] = (float)sry;
            }
            if (lane < n) L.put_local(lane, a, b, px, py, pz);
        } else {
            n = (int)fa_radius_walk<DIM, true>(rv, start, g, px, py, pz, P.radius2, L, lane);
            if (n < s) {
                if (lane == 0) poi[DIM == 2 ? poi2d::ZNCC : poi3d::ZNCC] = -1.f;  // :186-190 / :443-447
                continue;
            }
            if (n > kFaMax || !L.holds(n - 1)) continue;  // (the host refused such a queue before this launch)
            if (n < nmin) {
                // :204-221 / :461-478: the neighbor_number_min nearest instead
                unsigned my_q;
                wave_sync();
                n = fa_knn<DIM>(rv, start, g, px, py, pz, nmin, lane, my_q);
                if (lane < n) L.put_local(lane, rv[2 * (size_t)my_q], rv[2 * (size_t)my_q + 1], px, py, pz);
            }
        }
        wave_sync();
        // RANSAC (:232-292 / :487-551)
        int smp[8];
        float X[D][DIM];
        int trials = 0, best_count = 0, best_trial = 0;
        float mean;
        do {
            fa_sample(base, trials, n, s, smp);
            int cnt = 0;
            float sum = 0.f;
            if (fa_fit<DIM, true>(L, smp, s, ia, ib, X)) cnt = fa_consensus<DIM, false>(L, n, X, P.error_threshold, lane, sum);
            if (cnt > best_count) {
                best_count = cnt;
                best_trial = trials;
            }
            trials++;
            mean = sum / (float)cnt;  // an empty set: 0 / 0, which compares false
        } while (trials < P.trial_number && (best_count < nmin || mean > exit_mean));
        float* zncc = poi + (DIM == 2 ? poi2d::ZNCC : poi3d::ZNCC);
        bool ok = best_count >= D;  // :296 / :555
        if (ok) {
            // the largest set again, moved to the front of the list, and the fit over it
            fa_sample(base, best_trial, n, s, smp);
            ok = fa_fit<DIM, true>(L, smp, s, ia, ib, X);
            float unused;
            const int m = ok ? fa_consensus<DIM, true>(L, n, X, P.error_threshold, lane, unused) : 0;
            ok = ok && m == best_count && fa_fit<DIM, false>(L, smp, m, ia, ib, X);
        }
        if (!ok) {
            if (lane == 0) *zncc = -2.f;
            continue;
        }
        if (lane == 0) {
            if constexpr (DIM == 2) {  // :319-330
                poi[poi2d::U] = X[2][0];
                poi[poi2d::UX] = X[0][0] - 1.f;
                poi[poi2d::UY] = X[1][0];
                poi[poi2d::V] = X[2][1];
                poi[poi2d::VX] = X[0][1];
                poi[poi2d::VY] = X[1][1] - 1.f;
                poi[poi2d::ITER] = (float)trials;
                poi[poi2d::FEATURE] = (float)best_count;
            } else {  // :579-596
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    poi[poi3d::P + 4 * r] = X[3][r];
#pragma unroll
                    for (int a = 0; a < 3; a++) poi[poi3d::P + 4 * r + 1 + a] = a == r ? X[a][r] - 1.f : X[a][r];
                }
                poi[poi3d::ITER] = (float)trials;
                poi[kFaFeature3d] = (float)best_count;
            }
            *zncc = 0.f;
        }
    }
}

template <int DIM>
constexpr size_t fa_lds_bytes() {
    return (size_t)kFaWaves * 2 * DIM * kFaLdsStride * sizeof(float);
}

unsigned fa_blocks(size_t count, bool slices) {
    const size_t want = (count + kFaWaves - 1) / kFaWaves;
    const size_t cap = slices ? (size_t)kFeatureAffineMaxSlots / kFaWaves : 16384;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace

hipError_t launch_feature_affine_gather(int ndim, const float* ref, const float* tar, size_t count, const unsigned* order, void* recs,
                                        hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((count + 255) / 256);
    (void)hipGetLastError();
    if (ndim == 2)
        hipLaunchKernelGGL(feature_affine_gather_kernel<2>, dim3(blocks), dim3(256), 0, stream, ref, tar, (unsigned)count, order,
                           static_cast<FaRec*>(recs));
    else
        hipLaunchKernelGGL(feature_affine_gather_kernel<3>, dim3(blocks), dim3(256), 0, stream, ref, tar, (unsigned)count, order,
                           static_cast<FaRec*>(recs));
    return hipGetLastError();
}

hipError_t launch_feature_affine_pairs(int ndim, const float* ref_kp, const float* tar_kp, const int* ref_idx, const int* tar_idx,
                                       size_t n_pairs, float* out_ref, float* out_tar, unsigned* negative, hipStream_t stream) {
    static const unsigned none = 0xffffffffu;
    hipError_t err = hipMemcpyAsync(negative, &none, sizeof(none), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess || n_pairs == 0) return err;
    const unsigned blocks = (unsigned)((n_pairs + 255) / 256);
    (void)hipGetLastError();
    if (ndim == 2)
        hipLaunchKernelGGL(feature_affine_pairs_kernel<2>, dim3(blocks), dim3(256), 0, stream, ref_kp, tar_kp, ref_idx, tar_idx,
                           (unsigned)n_pairs, out_ref, out_tar, negative);
    else
        hipLaunchKernelGGL(feature_affine_pairs_kernel<3>, dim3(blocks), dim3(256), 0, stream, ref_kp, tar_kp, ref_idx, tar_idx,
                           (unsigned)n_pairs, out_ref, out_tar, negative);
    return hipGetLastError();
}

hipError_t launch_feature_affine_count(int ndim, const float* pois, int stride_f, size_t count, const StrainGrid& g,
                                       const FeatureAffineParams& P, const unsigned* start, const void* recs, unsigned* verdict,
                                       hipStream_t stream) {
    static const unsigned init[3] = {0u, 0xffffffffu, 0xffffffffu};  // (static: the asynchronous copy may read it after this returns)
    hipError_t err = hipMemcpyAsync(verdict, init, sizeof(init), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess || count == 0) return err;
    const unsigned blocks = fa_blocks(count, false);
    (void)hipGetLastError();
    if (ndim == 2)
        hipLaunchKernelGGL(feature_affine_count_kernel<2>, dim3(blocks), dim3(kFaWaves * kWave), 0, stream, pois, stride_f, (unsigned)count,
                           g, P, start, static_cast<const FaRec*>(recs), verdict);
    else
        hipLaunchKernelGGL(feature_affine_count_kernel<3>, dim3(blocks), dim3(kFaWaves * kWave), 0, stream, pois, stride_f, (unsigned)count,
                           g, P, start, static_cast<const FaRec*>(recs), verdict);
    return hipGetLastError();
}

// entries per array of a wave's global slice: what the launch's largest list has beyond the LDS part, in whole waves
static int fa_ext_pitch(unsigned max_candidates) {
    if (max_candidates <= (unsigned)kFaLds) return 0;
    const unsigned most = max_candidates < (unsigned)kFaMax ? max_candidates : (unsigned)kFaMax;
    return (int)((most - kFaLds + kWave - 1) / kWave * kWave);
}

size_t feature_affine_scratch_bytes(int ndim, size_t count, unsigned max_candidates) {
    const int pitch = fa_ext_pitch(max_candidates);
    if (pitch == 0) return 0;
    return (size_t)fa_blocks(count, true) * kFaWaves * 2 * ndim * pitch * sizeof(float);
}

template <int DIM>
static hipError_t compute_t(float* pois, int stride_f, size_t count, const StrainGrid& g, const FeatureAffineParams& P,
                            const unsigned* start, const void* recs, int ext_pitch, float* scratch, hipStream_t stream) {
    const bool slices = ext_pitch > 0;
    auto kern = feature_affine_kernel<DIM>;
    const size_t lds = fa_lds_bytes<DIM>();  // above the 64 KB a kernel gets unasked
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    const unsigned blocks = fa_blocks(count, slices);
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kFaWaves * kWave), lds, stream, pois, stride_f, (unsigned)count, g, P, start,
                       static_cast<const FaRec*>(recs), slices ? scratch : nullptr, ext_pitch);
    return hipGetLastError();
}

hipError_t launch_feature_affine_compute(int ndim, float* pois, int stride_f, size_t count, const StrainGrid& g,
                                         const FeatureAffineParams& P, const unsigned* start, const void* recs,
                                         unsigned max_candidates, float* scratch, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const int ext_pitch = fa_ext_pitch(max_candidates);
    if (ext_pitch > 0 && !scratch) return hipErrorInvalidValue;
    return ndim == 2 ? compute_t<2>(pois, stride_f, count, g, P, start, recs, ext_pitch, scratch, stream)
                     : compute_t<3>(pois, stride_f, count, g, P, start, recs, ext_pitch, scratch, stream);
}

}  // namespace ochip

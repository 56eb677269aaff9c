// icgn3d_onepass.hip -- ICGN3D1 under the ONE-PASS arithmetic contract (oc_hip_set_tuning "arith_onepass3d", opt-in) on gfx950.
//
// The default kernel (icgn3d.hip) writes every warped sample of an iteration to a per-workgroup global scratch slot, reads the slot
// back for the norm, and reads it a third time -- with the reference voxel and the three gradients -- for the error image, ZNSSD and
// numerator: three block reductions and two streaming passes around the tap sweep.  Here an iteration is the tap sweep alone, with
// 3 + 12 running sums and NO scratch slot: a sample is interpolated, consumed and forgotten, and ONE block reduction follows.
//
// Algebra (carried to 12 DoF).  Set-up per POI as under the fused contract (mean r-, r~ = r - r-,
// R2 = sum r~^2, |R| = sqrt(R2), steepest-descent rows SD_j, H, H^-1) plus R0 = sum r~, A_j = sum SD_j, B_j = sum SD_j r~.  R2's
// sweep becomes two half sweeps for them (14 + 12 running sums; each reads r and the three gradients once more than the fused
// contract's set-up does).  Two scalars travel from iteration to iteration: a shift c (first: r-) and a scale g (first: 1).  The sweep
// forms, per sample,
//     e' = fma(g, t - c, -r~)       E0 += e'   E2 = fma(e', e', E2)   Er = fma(e', r~, Er)   E_j = fma(SD_j, e', E_j)
// and after the reduction of the 15 sums
//     S1 = (E0 + R0) / g            S2 = ((E2 + 2 Er) + R2) / (g g)        m = S1 / N        |T| = sqrt(S2 - S1 m)
//     f = |R| / |T|                 a = (f - g) / g    alpha = 1 + a       q = f m
//     ZNSSD = (alpha^2 E2 + a^2 R2 + N q^2 + 2 alpha a Er - 2 alpha q E0 - 2 a q R0) / R2
//     b_j = (alpha E_j + a B_j) - q A_j            then  c <- c + m,  g <- f
// Everything behind b (dp = H^-1 b, the 4 x 4 warp update, the norm, the exits, which fields are written) is icgn3d.hip's,
// expression for expression.
// NOT bit-identical to the other two contracts.  Pinned bit for bit on tests/cpp/icgn3d_onepass_twin.cpp, which fixes the rounding
// order of the scalar expressions (onepass_scalars below is its scalars()) and the association of the sums: sample s is owned by
// thread s % 512, a thread adds its samples in increasing s, then block_allreduce (icgn3d_device.h).
//
// Mapping, walk, passes, coefficient boxes, row-pitch instantiations, global-tap fallback and launch shape are icgn3d.hip's.  In
// the sweep a sample additionally loads r, g_x, g_y, g_z at its own reference voxel (x-contiguous across the lanes, issued ahead of
// the 64 taps so that the tap evaluation covers their latency).
#define OC_FMA 1   // the fused `mad` of oc_device.h: every per-sample multiply-add is one v_fma_f32
#include "icgn3d_device.h"

namespace ochip {
namespace onepass3d {

constexpr int kSums = 15;  // E_0 .. E_11, E0, E2, Er

// what follows the reduction of an iteration's sums; every operation rounds on its own (the library is built with
// -ffp-contract=off), in the order of the CPU restatement
struct OnepassScalars {
    float m, f, znssd, alpha, a, q;
};
__device__ __forceinline__ OnepassScalars onepass_scalars(float E0, float E2, float Er, float R0, float R2, float ref_norm, float fN,
                                                          float g) {
    OnepassScalars r;
    const float S1 = (E0 + R0) / g;
    const float S2 = ((E2 + 2.f * Er) + R2) / (g * g);
    r.m = S1 / fN;
    const float tar_norm = sqrtf(S2 - S1 * r.m);
    r.f = ref_norm / tar_norm;
    r.a = (r.f - g) / g;
    r.alpha = 1.f + r.a;
    r.q = r.f * r.m;
    float z = (r.alpha * r.alpha) * E2;
    z = z + (r.a * r.a) * R2;
    z = z + (fN * r.q) * r.q;
    z = z + ((2.f * r.alpha) * r.a) * Er;
    z = z - ((2.f * r.alpha) * r.q) * E0;
    z = z - ((2.f * r.a) * r.q) * R0;
    r.znssd = z / R2;
    return r;
}

// Hessian rows [R0, R1): sums of fma(sd[r], sd[c]), c <= r, over all samples, block-reduced and filed into the symmetric matrix A
// (LDS).  The fused build of icgn3d.hip's hessian_rows, restated here because that file keeps its code: packed pairs over adjacent
// columns, four samples' gradients in flight.
template <int R0, int R1>
__device__ __forceinline__ void hessian_rows(const Icgn3dParams& P, int tid, int wave, int lane, int SX, int SY, int N, int rx, int ry,
                                             int rz, int cx, int cy, int cz, int DX, int DY, float* red, float* __restrict__ A) {
    constexpr int NE = (R1 * (R1 + 1) - R0 * (R0 + 1)) / 2;
    f2 hp[12][6];
    float hd[12];
#pragma unroll
    for (int r = 0; r < 12; r++) {
        hd[r] = 0.f;
#pragma unroll
        for (int q = 0; q < 6; q++) hp[r][q] = mk2(0.f, 0.f);
    }
    Walk3 w(tid, SX, SY, 0, DX, DY);
    const size_t gbase = ((size_t)(cz - rz) * DY + (cy - ry)) * DX + (cx - rx);
    const float* __restrict__ pgx = P.gx + gbase;
    const float* __restrict__ pgy = P.gy + gbase;
    const float* __restrict__ pgz = P.gz + gbase;
    struct G3 {
        float x, y, z;
    };
    const int cnt = N > tid ? (N - tid + kBlock3d - 1) / kBlock3d : 0;
    sweep_batched<4>(
        w, rx, ry, rz, cnt, [&](const WalkPoint& q, int) { return G3{pgx[q.off], pgy[q.off], pgz[q.off]}; },
        [&](const WalkPoint& q, const G3& g, int) {
            const float g_x = g.x, g_y = g.y, g_z = g.z;
            const f2 m01 = mk2(1.f, q.x), m23 = mk2(q.y, q.z);  // g * 1.f is exact
            const f2 sdp[6] = {g_x * m01, g_x * m23, g_y * m01, g_y * m23, g_z * m01, g_z * m23};
#pragma unroll
            for (int r = R0; r < R1; r++) {
                const float sr = (r & 1) ? sdp[r / 2].y : sdp[r / 2].x;
#pragma unroll
                for (int q2 = 0; q2 < (r + 1) / 2; q2++) hp[r][q2] = mad(sr, sdp[q2], hp[r][q2]);
                if ((r & 1) == 0) hd[r] = mad(sr, sr, hd[r]);
            }
        });
    float h[NE];
    {
        int t = 0;
#pragma unroll
        for (int r = R0; r < R1; r++)
#pragma unroll
            for (int c = 0; c <= r; c++, t++)
                h[t] = (c == r && (r & 1) == 0) ? hd[r] : ((c & 1) ? hp[r][c / 2].y : hp[r][c / 2].x);
    }
    constexpr int NCH = (NE + kSums - 1) / kSums;
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        float part[kSums];
#pragma unroll
        for (int q = 0; q < kSums; q++) part[q] = (ch * kSums + q < NE) ? h[(ch * kSums + q) % NE] : 0.f;
        block_allreduce<kSums>(part, red, wave, lane);
#pragma unroll
        for (int q = 0; q < kSums; q++)
            if (ch * kSums + q < NE) h[(ch * kSums + q) % NE] = part[q];
    }
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int r = R0; r < R1; r++)
#pragma unroll
            for (int c = 0; c <= r; c++, t++) {
                A[r * 12 + c] = h[t];
                A[c * 12 + r] = h[t];
            }
    }
}

// PX: row pitch of the staged coefficient box in LDS (0 = the box's own width, decided per pass)
template <int PX>
__global__ __launch_bounds__(kBlock3d, 4) void icgn3d_onepass_kernel(Icgn3dParams P, float* __restrict__ pois, int stride_f,
                                                                  unsigned long long count) {
    __shared__ __attribute__((aligned(16))) float lds[kSums * kWaves3d + 12 * kWave + kWinCap + 6 * kBoxSlots + 24];
    float* red = lds;                               // kSums * 8 floats
    float* lds_hinv = lds + kSums * kWaves3d;       // 12 x 64 floats: column j of H^-1 in lane j
    float* win = lds_hinv + 12 * kWave;             // staged coefficient box of the current pass
    int* boxes = reinterpret_cast<int*>(win + kWinCap);  // origin + extent of the box of each pass (kBoxSlots x 6)
    float* lds_ab = win + kWinCap + 6 * kBoxSlots;  // A_j (12), B_j (12) of the current POI
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    const int rx = P.rx, ry = P.ry, rz = P.rz, DX = P.dx, DY = P.dy, DZ = P.dz;
    const int SX = 2 * rx + 1, SY = 2 * ry + 1, SZ = 2 * rz + 1;
    const int N = SX * SY * SZ;
    const float fN = (float)N;
    const int plane = SX * SY;

    // the XCD-interleaved walk of icgn3d.hip
    const unsigned long long xcd_chunk = (count + 7) / 8, xcd_lo = (blockIdx.x & 7u) * xcd_chunk;
    const unsigned long long xcd_hi = min(count, xcd_lo + xcd_chunk);
    for (unsigned long long idx = xcd_lo + (blockIdx.x >> 3); idx < xcd_hi; idx += gridDim.x >> 3) {
        float* poi = pois + (P.perm ? (unsigned long long)P.perm[idx] : idx) * (unsigned long long)stride_f;
        const float px = uni3(poi[poi3d::X]), py = uni3(poi[poi3d::Y]), pz = uni3(poi[poi3d::Z]);
        float init[12];
#pragma unroll
        for (int i = 0; i < 12; i++) init[i] = uni3(poi[poi3d::P + i]);
        const float zncc_in = uni3(poi[poi3d::ZNCC]);
        __syncthreads();  // everyone has read the record before anyone may overwrite it

        // guard, src/oc_icgn.cpp:1279-1286
        // (the geometric part written negated: a NaN coordinate fails every comparison, so it is rejected like a subvolume that
        // leaves the image, before any address is formed from it)
        if (!((px - rx) >= 0 && (py - ry) >= 0 && (pz - rz) >= 0 && (px + rx) <= (DX - 1) && (py + ry) <= (DY - 1) &&
              (pz + rz) <= (DZ - 1)) || fabsf(init[0]) >= DX || fabsf(init[4]) >= DY || fabsf(init[8]) >= DZ ||
            zncc_in < 0 || isnan(init[0]) || isnan(init[4]) || isnan(init[8])) {
            if (tid == 0) poi[poi3d::ZNCC] = zncc_in >= 0 ? -3.f : zncc_in;
            continue;
        }

        // ---- reference subvolume (src/oc_subset.cpp:89-135): per-element truncation, one box unless an addition rounds across an
        // integer (checked per POI, as icgn3d.hip does)
        const float sxf = px - rx, syf = py - ry, szf = pz - rz;
        bool ref_box = true;
        for (int q = tid; q < SX + SY + SZ; q += kBlock3d) {
            const int ax = q < SX ? 0 : (q < SX + SY ? 1 : 2);
            const int e = ax == 0 ? q : (ax == 1 ? q - SX : q - SX - SY);
            const float st = ax == 0 ? sxf : (ax == 1 ? syf : szf);
            ref_box = ref_box && ((int)(st + e) == (int)st + e);
        }
        ref_box = __syncthreads_and(ref_box ? 1 : 0) != 0;
        const float* __restrict__ pref = P.ref + (((size_t)(int)szf * DY + (int)syf) * DX + (int)sxf);
        const int cx = (int)px, cy = (int)py, cz = (int)pz;
        const size_t gbase = ((size_t)(cz - rz) * DY + (cy - ry)) * DX + (cx - rx);
        const float* __restrict__ pgx = P.gx + gbase;
        const float* __restrict__ pgy = P.gy + gbase;
        const float* __restrict__ pgz = P.gz + gbase;
        const int cnt = N > tid ? (N - tid + kBlock3d - 1) / kBlock3d : 0;  // samples this thread owns
        auto ref_fast = [&](const WalkPoint& q, int) { return pref[q.off]; };
        auto ref_slow = [&](const WalkPoint& q, int) {
            return P.ref[((size_t)(int)(szf + ((int)q.z + rz)) * DY + (int)(syf + ((int)q.y + ry))) * DX + (int)(sxf + ((int)q.x + rx))];
        };
        float ref_mean, ref_norm, R0, R2;
        struct S4 {
            float r, x, y, z;
        };
        // sweep 1: the mean.  Sweep 2, as two half sweeps beside a batch of four samples (like the Hessian's): R2, R0, A_0..5, B_0..5
        // (14 running sums), then A_6..11, B_6..11 (12); each half reads r and the three gradients
        auto ref_stats = [&](auto&& ref_of) {
            float acc[1] = {0.f};
            Walk3 w(tid, SX, SY, 0, DX, DY);
            sweep_batched<8>(w, rx, ry, rz, cnt, ref_of, [&](const WalkPoint&, float v, int) { acc[0] += v; });
            block_allreduce<1>(acc, red, wave, lane);
            ref_mean = acc[0] / fN;
            float aux[14];
#pragma unroll
            for (int i = 0; i < 14; i++) aux[i] = 0.f;
            Walk3 w2(tid, SX, SY, 0, DX, DY);
            sweep_batched<4>(
                w2, rx, ry, rz, cnt,
                [&](const WalkPoint& q, int sidx) { return S4{ref_of(q, sidx), pgx[q.off], pgy[q.off], pgz[q.off]}; },
                [&](const WalkPoint& q, const S4& v, int) {
                    const float d = v.r - ref_mean;
                    aux[12] = mad(d, d, aux[12]);
                    aux[13] += d;
                    const float sd[6] = {v.x, v.x * q.x, v.x * q.y, v.x * q.z, v.y, v.y * q.x};
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        aux[j] += sd[j];
                        aux[6 + j] = mad(sd[j], d, aux[6 + j]);
                    }
                });
            block_allreduce<14>(aux, red, wave, lane);
            R2 = aux[12];
            R0 = aux[13];
            ref_norm = sqrtf(R2);
            if (tid == 0) {
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    lds_ab[j] = aux[j];
                    lds_ab[12 + j] = aux[6 + j];
                }
            }
            float aux2[12];
#pragma unroll
            for (int i = 0; i < 12; i++) aux2[i] = 0.f;
            Walk3 w3(tid, SX, SY, 0, DX, DY);
            sweep_batched<4>(
                w3, rx, ry, rz, cnt,
                [&](const WalkPoint& q, int sidx) { return S4{ref_of(q, sidx), pgx[q.off], pgy[q.off], pgz[q.off]}; },
                [&](const WalkPoint& q, const S4& v, int) {
                    const float d = v.r - ref_mean;
                    const float sd[6] = {v.y * q.y, v.y * q.z, v.z, v.z * q.x, v.z * q.y, v.z * q.z};
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        aux2[j] += sd[j];
                        aux2[6 + j] = mad(sd[j], d, aux2[6 + j]);
                    }
                });
            block_allreduce<12>(aux2, red, wave, lane);
            if (tid == 0) {
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    lds_ab[6 + j] = aux2[j];
                    lds_ab[18 + j] = aux2[6 + j];
                }
            }
        };
        if (ref_box) ref_stats(ref_fast);
        else ref_stats(ref_slow);
        R0 = uni3(R0);
        R2 = uni3(R2);
        ref_mean = uni3(ref_mean);
        ref_norm = uni3(ref_norm);

        // ---- SD image + Hessian (src/oc_icgn.cpp:1299-1337) and its inverse (:1339): two sweeps (rows 0-7, rows 8-11), the idle
        // coefficient window hosts the matrix, one wave inverts
        {
            float* A = win;
            hessian_rows<0, 8>(P, tid, wave, lane, SX, SY, N, rx, ry, rz, cx, cy, cz, DX, DY, red, A);
            hessian_rows<8, 12>(P, tid, wave, lane, SX, SY, N, rx, ry, rz, cx, cy, cz, DX, DY, red, A);
            if (wave == 0) lu_inverse12_lds(A, reinterpret_cast<int*>(win + 144), lds_hinv, lane);
            // visible to every wave after the barriers of the first sweep below
        }

        // ---- IC-GN loop (src/oc_icgn.cpp:1344-1447)
        float Wm[16];
        set_warp_3d1(Wm, init);
        int iter = 0;
        float dp_norm = 0.f, znssd = 0.f;
        float cshift = ref_mean, gscale = 1.f;
        bool failed = false;
#pragma nounroll
        do {
            iter++;
            bool out_of_range = false;
            float sum[kSums];
#pragma unroll
            for (int i = 0; i < kSums; i++) sum[i] = 0.f;
            {
                // Deformation3D1::warp (src/oc_deformation.cpp:518-530) + subvolume centre, as every sample evaluates it
                auto warp_x = [&](float xl, float yl, float zl) { return px + (mad(Wm[2], zl, mad(Wm[1], yl, Wm[0] * xl)) + Wm[3] * 1.f); };
                auto warp_y = [&](float xl, float yl, float zl) { return py + (mad(Wm[6], zl, mad(Wm[5], yl, Wm[4] * xl)) + Wm[7] * 1.f); };
                auto warp_z = [&](float xl, float yl, float zl) { return pz + (mad(Wm[10], zl, mad(Wm[9], yl, Wm[8] * xl)) + Wm[11] * 1.f); };
                // coefficient boxes of all passes of this sweep, one pass per thread (icgn3d.hip): a pass = M * 512 consecutive
                // samples, thread tid owns s = tid + 512 * (M * pass + m), m < M
                const int M = P.samples_per_pass;
                const int pass_len = M * kBlock3d;
                const int npass = (N + pass_len - 1) / pass_len;
                for (int round0 = 0; round0 < npass; round0 += kBoxSlots) {
                    __syncthreads();  // the previous round's boxes are no longer needed
                    for (int pass = round0 + tid; pass < min(npass, round0 + kBoxSlots); pass += kBlock3d) {
                        const int s0 = pass * pass_len, s1 = min(s0 + pass_len - 1, N - 1);
                        const int i0 = s0 / plane, i1 = s1 / plane;
                        const int ra = (s0 - i0 * plane) / SX, rb = (s1 - i1 * plane) / SX;
                        const int j0 = i0 == i1 ? ra : 0, j1 = i0 == i1 ? rb : SY - 1;
                        const bool one_row = i0 == i1 && j0 == j1;
                        const int k0 = one_row ? s0 - i0 * plane - ra * SX : 0, k1 = one_row ? s1 - i1 * plane - rb * SX : SX - 1;
                        // the image of the index box under the warp: every coordinate is monotone in each index (also in floating
                        // point, fused or not), so the 8 corners bound what any sample of the pass computes
                        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
                        for (int c = 0; c < 8; c++) {
                            const float xl = (float)(((c & 1) ? k1 : k0) - rx), yl = (float)(((c & 2) ? j1 : j0) - ry),
                                        zl = (float)(((c & 4) ? i1 : i0) - rz);
                            const float q[3] = {warp_x(xl, yl, zl), warp_y(xl, yl, zl), warp_z(xl, yl, zl)};
#pragma unroll
                            for (int a = 0; a < 3; a++) {
                                lo[a] = fminf(lo[a], q[a]);
                                hi[a] = fmaxf(hi[a], q[a]);
                            }
                        }
                        // taps of an in-range sample lie in [floor - 1, floor + 2]; in-range means [1, D - 2)
                        const int D[3] = {DX, DY, DZ};
                        int o[3], n[3];
                        bool usable = true;
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            usable = usable && lo[a] == lo[a] && hi[a] == hi[a] && fabsf(lo[a]) < 1.0e9f && fabsf(hi[a]) < 1.0e9f;
                            const int fl = (int)floorf(fmaxf(lo[a], 1.f)) - 1, fh = (int)floorf(fminf(hi[a], (float)(D[a] - 3))) + 2;
                            o[a] = max(fl, 0);
                            n[a] = min(fh, D[a] - 1) - o[a] + 1;
                        }
                        // n[0] = 0 marks "do not stage": nothing of the pass is in range, or the box does not fit -> global taps
                        const bool stage = usable && n[0] >= 4 && n[1] >= 4 && n[2] >= 4 && (PX == 0 || n[0] <= PX) &&
                                           (long long)(PX ? PX : n[0]) * n[1] * n[2] <= kWinCap;
                        int* slot = boxes + (pass - round0) * 6;
                        slot[0] = o[0]; slot[1] = o[1]; slot[2] = o[2];
                        slot[3] = stage ? n[0] : 0; slot[4] = n[1]; slot[5] = n[2];
                    }
                    __syncthreads();
                    Walk3 w(tid, SX, SY, round0 * M, DX, DY);
                    for (int pass = round0; pass < min(npass, round0 + kBoxSlots); pass++) {
                        const int* slot = boxes + (pass - round0) * 6;
                        int o[3], n[3];
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            o[a] = __builtin_amdgcn_readfirstlane(slot[a]);
                            n[a] = __builtin_amdgcn_readfirstlane(slot[3 + a]);
                        }
                        const bool staged = n[0] > 0;
                        const int nx = n[0];                 // floats fetched per row
                        const int pitch = PX ? PX : n[0];    // floats between rows in LDS
                        const int nxy = pitch * n[1];
                        if (staged) {
                            __syncthreads();  // the previous pass has finished reading the box
                            const int rows = n[1] * n[2];
                            int zr = wave / n[1], yr = wave - zr * n[1];
                            const int dzr = kWaves3d / n[1], dyr = kWaves3d - dzr * n[1];
                            if (nx <= kWave) {
                                // a row fits one wave-wide load: kStageRows rows in flight before the first LDS write
                                constexpr int kStageRows = 16;
                                for (int row0 = wave; row0 < rows; row0 += kStageRows * kWaves3d) {
                                    float v[kStageRows];
#pragma unroll
                                    for (int u = 0; u < kStageRows; u++) {
                                        const int row = row0 + u * kWaves3d;
                                        v[u] = 0.f;
                                        if (row < rows && lane < nx)
                                            v[u] = P.coef[((size_t)(o[2] + zr) * DY + (o[1] + yr)) * DX + o[0] + lane];
                                        yr += dyr;
                                        zr += dzr;
                                        if (yr >= n[1]) {
                                            yr -= n[1];
                                            zr++;
                                        }
                                    }
#pragma unroll
                                    for (int u = 0; u < kStageRows; u++) {
                                        const int row = row0 + u * kWaves3d;
                                        if (row < rows && lane < nx) win[row * pitch + lane] = v[u];
                                    }
                                }
                            } else {
                                for (int row = wave; row < rows; row += kWaves3d) {
                                    const float* __restrict__ src = P.coef + ((size_t)(o[2] + zr) * DY + (o[1] + yr)) * DX + o[0];
                                    for (int x = lane; x < nx; x += kWave) win[row * pitch + x] = src[x];
                                    yr += dyr;
                                    zr += dzr;
                                    if (yr >= n[1]) {
                                        yr -= n[1];
                                        zr++;
                                    }
                                }
                            }
                            __syncthreads();
                        }
                        for (int m = 0; m < M; m++, w.next()) {
                            if (w.s < N) {
                                // the sample's own reference voxel and gradients first: the 64 taps cover their latency
                                const float rv = ref_box ? pref[w.off]
                                                         : P.ref[((size_t)(int)(szf + (float)w.i) * DY + (int)(syf + (float)w.j)) * DX +
                                                                 (int)(sxf + (float)w.k)];
                                const float g_x = pgx[w.off], g_y = pgy[w.off], g_z = pgz[w.off];
                                const float xl = (float)(w.k - rx), yl = (float)(w.j - ry), zl = (float)(w.i - rz);
                                const float x = warp_x(xl, yl, zl), y = warp_y(xl, yl, zl), z = warp_z(xl, yl, zl);
                                const float v = staged ? bspline3d_eval_lds<PX>(win, o[0], o[1], o[2], pitch, nxy, DZ, DY, DX, x, y, z)
                                                       : bspline3d_eval(P.coef, DZ, DY, DX, x, y, z);
                                out_of_range = out_of_range || (v < 0.f);
                                const float rt = rv - ref_mean;
                                const float e = mad(gscale, v - cshift, -rt);
                                sum[12] += e;
                                sum[13] = mad(e, e, sum[13]);
                                sum[14] = mad(e, rt, sum[14]);
                                sum[0] = mad(g_x, e, sum[0]); sum[1] = mad(g_x * xl, e, sum[1]); sum[2] = mad(g_x * yl, e, sum[2]); sum[3] = mad(g_x * zl, e, sum[3]);
                                sum[4] = mad(g_y, e, sum[4]); sum[5] = mad(g_y * xl, e, sum[5]); sum[6] = mad(g_y * yl, e, sum[6]); sum[7] = mad(g_y * zl, e, sum[7]);
                                sum[8] = mad(g_z, e, sum[8]); sum[9] = mad(g_z * xl, e, sum[9]); sum[10] = mad(g_z * yl, e, sum[10]); sum[11] = mad(g_z * zl, e, sum[11]);
                            }
                        }
                    }
                }
            }
            // src/oc_icgn.cpp:1396-1400
            if (__syncthreads_or(out_of_range ? 1 : 0)) {
                failed = true;
                break;
            }
            block_allreduce<kSums>(sum, red, wave, lane);
            const OnepassScalars sc = onepass_scalars(sum[12], sum[13], sum[14], R0, R2, ref_norm, fN, gscale);
            znssd = sc.znssd;
            cshift = uni3(cshift + sc.m);
            gscale = uni3(sc.f);
            // b_j in lane j, then dp = H^-1 b (src/oc_icgn.cpp:1435-1443)
            float ej = 0.f;
#pragma unroll
            for (int j = 0; j < 12; j++) ej = lane == j ? sum[j] : ej;
            const int lj = lane < 12 ? lane : 0;
            const float numj = (sc.alpha * ej + sc.a * lds_ab[12 + lj]) - sc.q * lds_ab[lj];
            float dp[12];
#pragma unroll
            for (int i = 0; i < 12; i++) {
                const float prod = lds_hinv[i * kWave + lane] * numj;
                float v = 0.f;
#pragma unroll
                for (int j = 0; j < 12; j++) v += wave_bcast(prod, j);
                dp[i] = v;
            }
            float dW[16], dWi[16], Wn[16];
            set_warp_3d1(dW, dp);
            inverse4(dW, dWi);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float v = Wm[i * 4 + 0] * dWi[0 * 4 + j];
#pragma unroll
                    for (int k = 1; k < 4; k++) v = v + Wm[i * 4 + k] * dWi[k * 4 + j];
                    Wn[i * 4 + j] = v;
                }
#pragma unroll
            for (int i = 0; i < 16; i++) Wm[i] = uni3(Wn[i]);
            // src/oc_icgn.cpp:1445
            dp_norm = uni3(sqrtf(dp[0] * dp[0] + dp[4] * dp[4] + dp[8] * dp[8]));
        } while (iter < P.stop && dp_norm >= P.conv);

        if (failed) {
            if (tid == 0) poi[poi3d::ZNCC] = -3.f;
            continue;
        }
        // ---- outputs (src/oc_icgn.cpp:1449-1489)
        if (tid == 0) {
            const float cur[12] = {Wm[3], Wm[0] - 1.f, Wm[1], Wm[2], Wm[7],  Wm[4],
                                   Wm[5] - 1.f, Wm[6], Wm[11], Wm[8], Wm[9], Wm[10] - 1.f};
            float zncc = 0.5f * (2 - znssd);
            const float fiter = (float)iter;
            if (dp_norm >= P.conv && fiter >= P.stop) zncc = -4.f;
            float o0 = cur[0], o4 = cur[4], o8 = cur[8];
            if (isnan(zncc) || isnan(o0) || isnan(o4) || isnan(o8)) {
                o0 = init[0]; o4 = init[4]; o8 = init[8];
                zncc = -5.f;
            }
#pragma unroll
            for (int i = 0; i < 12; i++) poi[poi3d::P + i] = cur[i];
            poi[poi3d::U] = o0;
            poi[poi3d::V] = o4;
            poi[poi3d::W] = o8;
            poi[poi3d::U0] = init[0];
            poi[poi3d::V0] = init[4];
            poi[poi3d::W0] = init[8];
            poi[poi3d::ZNCC] = zncc;
            poi[poi3d::ITER] = fiter;
            poi[poi3d::CONV] = dp_norm;
            poi[poi3d::SRX] = (float)rx;
            poi[poi3d::SRY] = (float)ry;
            poi[poi3d::SRZ] = (float)rz;
        }
    }
}

}  // namespace onepass3d

// The launch shape is launch_icgn3d1's (icgn3d.hip): 512 persistent workgroups in whole XCD rounds, the row pitch by radius, as
// many samples per thread and pass as keep the nominal coefficient box inside the LDS window.  No scratch: p.scratch is not read.
hipError_t launch_icgn3d1_onepass(const Icgn3dParams& p, float* pois, int stride_f, size_t count, hipStream_t stream) {
    using namespace onepass3d;
    if (count == 0) return hipSuccess;
    int blocks = 0;
    (void)icgn3d1_scratch_floats(p.rx, p.ry, p.rz, &blocks);  // (the workgroup count only)
    unsigned grid = (unsigned)(count < (size_t)blocks ? count : (size_t)blocks);
    grid = (grid + 7) / 8 * 8;
    Icgn3dParams q = p;
    q.scratch = nullptr;
    q.samples_per_pass = 1;
    const int want = 2 * p.rx + 1 + 5;
    const int px = want <= 40 ? 40 : want <= 48 ? 48 : want <= 64 ? 64 : 0;
    const int tries[] = {16, 12, 10, 8, 6, 4, 3, 2, 1};
    for (int m : tries) {
        const long long sx = 2 * p.rx + 1, sy = 2 * p.ry + 1, sz = 2 * p.rz + 1, len = (long long)m * kBlock3d;
        const long long planes = (len + sx * sy - 1) / (sx * sy) + 1;
        const long long nz = (planes < sz ? planes : sz) + 3 + 1;
        const long long rows = planes > 1 ? sy : (len + sx - 1) / sx + 1;
        const long long ny = (rows < sy ? rows : sy) + 3 + 2, nx = px ? px : sx + 3 + 2;
        if (nx * ny * nz <= kWinCap) {
            q.samples_per_pass = m;
            break;
        }
    }
    (void)hipGetLastError();  // drop stale errors of earlier, unrelated calls
    switch (px) {
        case 40: hipLaunchKernelGGL(icgn3d_onepass_kernel<40>, dim3(grid), dim3(kBlock3d), 0, stream, q, pois, stride_f, (unsigned long long)count); break;
        case 48: hipLaunchKernelGGL(icgn3d_onepass_kernel<48>, dim3(grid), dim3(kBlock3d), 0, stream, q, pois, stride_f, (unsigned long long)count); break;
        case 64: hipLaunchKernelGGL(icgn3d_onepass_kernel<64>, dim3(grid), dim3(kBlock3d), 0, stream, q, pois, stride_f, (unsigned long long)count); break;
        default: hipLaunchKernelGGL(icgn3d_onepass_kernel<0>, dim3(grid), dim3(kBlock3d), 0, stream, q, pois, stride_f, (unsigned long long)count); break;
    }
    return hipGetLastError();
}

}  // namespace ochip

// icgn2d_onepass.hip -- ICGN2D1 / ICGN2D2 under the ONE-PASS arithmetic contract (oc_hip_set_tuning "arith_onepass", opt-in).
//
// The default kernel (icgn2d.hip) passes over the warped target subset three times per iteration: the interpolation sweep parks
// every sample in LDS, a second pass forms mean and norm, a third the error image, ZNSSD and numerator.  Here an iteration is ONE
// sweep with 3 + DOF running sums and NO target array: a sample is interpolated, consumed and forgotten.
//
// Algebra.  Set-up per POI as under the fused contract (mean r-, r~ = r - r-, R2 = sum r~^2, |R| = sqrt(R2),
// steepest-descent rows SD_j, H, H^-1) plus three constants from the same pass: R0 = sum r~, A_j = sum SD_j, B_j = sum SD_j r~.
// Two scalars travel from iteration to iteration: a shift c (first: r-) and a scale g (first: 1).  The sweep forms, per sample,
//     e' = fma(g, t - c, -r~)       E0 += e'   E2 = fma(e', e', E2)   Er = fma(e', r~, Er)   E_j = fma(SD_j, e', E_j)
// and after ONE reduction of the 3 + DOF sums
//     S1 = (E0 + R0) / g            S2 = ((E2 + 2 Er) + R2) / (g g)        m = S1 / N        |T| = sqrt(S2 - S1 m)
//     f = |R| / |T|                 a = (f - g) / g    alpha = 1 + a       q = f m
//     ZNSSD = (alpha^2 E2 + a^2 R2 + N q^2 + 2 alpha a Er - 2 alpha q E0 - 2 a q R0) / R2
//     b_j = (alpha E_j + a B_j) - q A_j            then  c <- c + m,  g <- f
// -- the exact error image is e = alpha e' + a r~ - q; with c and g one iteration old, a and q are small and e' IS the residual
// to rounding, which is why this form keeps the accuracy of the two-pass arithmetic where the closed form 2 - 2 sum t~ r~ / (|R| |T|)
// loses it to cancellation.  Everything behind b (dp = H^-1 b, warp update, convergence norm, exits, outputs) is icgn2d.hip's,
// expression for expression.
// NOT bit-identical to the other two contracts.  Pinned bit for bit on tests/cpp/icgn2d_onepass_twin.cpp, which fixes the rounding
// order of the scalar expressions (onepass_scalars below is its scalars()) and the association of the sums: sample s is owned by
// lane s % 64, a lane's passes run in order, then the xor butterfly of oc_device.h.
//
// Shape: ONE wave per POI, eight waves (eight consecutive POIs of the visiting order) per workgroup, as the big-queue default.  LDS
// holds the workgroup's coordinate table only (local coordinates and byte offset per (lane, pass): 12 B per sample, 13.5 KB at
// r = 16) and 2 KB for the cooperative 6 x 6 inverse -- occupancy is set by registers, not by LDS.  r~, g_x, g_y are re-read from
// the images in the sweep (coalesced, L1 / L2 hits) next to the sample's four 16-byte table gathers; G = 2 samples in flight.
// Wave-uniform state (warp, c, g, the set-up constants) lives in SGPRs.  Barriers: the table fill, the two of the cooperative
// inverse (6 DoF), and the lockstep barrier of the sweep -- same three invariants as icgn2d.hip: one POI per wave and no POI loop,
// every data-carrying barrier strictly before a wave's first sweep barrier (early leavers through leave()), nothing behind the loop
// waits.  One radius per launch: centre offsets and self-adaptive radii are refused by the caller (capi.hip).
#define OC_FMA 1   // the fused `mad` of oc_device.h: every per-sample multiply-add is one v_fma_f32
#include <atomic>
#include <type_traits>

#include "dic2d_device.h"
#include "host/icgn2d_plan.h"  // the LDS budget and the one-pass table's footprint, which run_icgn2d's limit is computed from
#include "oc_kernels.h"

namespace ochip {
namespace onepass {

struct OnepassLaunch {
    int stride_f;              // floats between POI records
    int nt;                    // ceil(N / 64)
    int xcd_chunk;             // > 0: workgroup b serves POI group (b % 8) * xcd_chunk + b / 8
    unsigned long long count;  // POIs
};

constexpr int kWpb = 8;                            // waves (POIs) per workgroup
constexpr int kLdsBudget = ochip_host::kIcgn2dLdsBudget;

struct GradRef {
    float gx, gy, ref;
};

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

template <int DOF>
__global__ __launch_bounds__(64 * kWpb, DOF == 6 ? 6 : 4) void icgn2d_onepass_kernel(Icgn2dParams P, float* __restrict__ pois,
                                                                                    OnepassLaunch L) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NH = DOF * (DOF + 1) / 2;
    constexpr int NAUX = 2 + 2 * DOF;            // R2, R0, A_j, B_j
    constexpr int G = 1;                         // samples whose gathers are issued back to back
    constexpr bool COOP = DOF == 6;              // ONE wave inverts the workgroup's eight 6 x 6 Hessians (coop_inverse6_x8)
    constexpr int SWEEP_SYNC = DOF == 6 ? 2 : 3; // pass groups between two lockstep barriers of the sweep (icgn2d.hip)
    __shared__ float coop_area[COOP ? kWpb * 64 : 1];
    const int NT = L.nt;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // every wave passes COOP's two barriers exactly once: on the ordinary path, or here when it abandons its POI before
    auto leave = [&]() {
        if constexpr (COOP) {
            if (lane < 24) coop_area[wave * 64 + lane] = 0.f;
            __syncthreads();
            if (wave == 0) coop_inverse6_x8(coop_area, lane);
            __syncthreads();
        }
    };
    // the workgroup's table: [NT * 64] float pairs (x_local, y_local), then [NT * 64] byte offsets from the subset origin
    f2* __restrict__ tab_xy = reinterpret_cast<f2*>(lds);
    unsigned* __restrict__ tab_off = reinterpret_cast<unsigned*>(lds + 2 * NT * kWave);
    {
        const int Wt = 2 * P.rx + 1;
        const unsigned w4t = (unsigned)P.width * 4u;
        for (int s = threadIdx.x; s < NT * kWave; s += kWave * kWpb) {
            const int r = s / Wt, c = s - r * Wt;
            tab_xy[s] = mk2((float)(c - P.rx), (float)(r - P.ry));
            tab_off[s] = (unsigned)r * w4t + ((unsigned)c << 2);
        }
        __syncthreads();
    }
    unsigned long long grp = blockIdx.x;
    if (L.xcd_chunk > 0) grp = (unsigned long long)(blockIdx.x & 7u) * L.xcd_chunk + (blockIdx.x >> 3);
    const unsigned long long slot = grp * kWpb + wave;
    if (slot >= L.count) {
        leave();
        return;
    }
    const unsigned long long idx = P.perm ? (unsigned long long)__builtin_amdgcn_readfirstlane((int)P.perm[slot]) : slot;
    float* poi = pois + idx * (unsigned long long)L.stride_f;
    const float rec = lane < poi2d::FLOATS ? poi[lane] : 0.f;
    const float px = wave_bcast(rec, poi2d::X), py = wave_bcast(rec, poi2d::Y);
    const float u_in = wave_bcast(rec, poi2d::U), ux_in = wave_bcast(rec, poi2d::UX), uy_in = wave_bcast(rec, poi2d::UY);
    const float v_in = wave_bcast(rec, poi2d::V), vx_in = wave_bcast(rec, poi2d::VX), vy_in = wave_bcast(rec, poi2d::VY);
    const float zncc_in = wave_bcast(rec, poi2d::ZNCC);
    const int height = P.height, width = P.width;
    const int rx = P.rx, ry = P.ry;

    // guard, src/oc_icgn.cpp:160-167 (2D2: 705-712)
    // (the geometric part negated, as in icgn2d.hip: a NaN coordinate is rejected like a subset that leaves the image)
    if (!(py - ry >= 0 && px - rx >= 0 && py + ry <= height - 1 && px + rx <= width - 1) || fabsf(u_in) >= width || fabsf(v_in) >= height ||
        zncc_in < 0 || isnan(u_in) || isnan(v_in)) {
        if (lane == 0) poi[poi2d::ZNCC] = zncc_in >= 0 ? -3.f : zncc_in;
        leave();
        return;
    }
    const int W = 2 * rx + 1, N = W * (2 * ry + 1);
    const float fN = (float)N;
    const int NF = N / kWave;  // passes in which every lane owns a sample; pass NF (if any) is partial
    const bool tail_valid = (NF * kWave + lane) < N;
    // subset origin as a wave-uniform byte offset (images are <= 2^28 bytes)
    const unsigned goff = (unsigned)__builtin_amdgcn_readfirstlane((((int)py - ry) * width + ((int)px - rx)) * 4);
    const unsigned roff = (unsigned)__builtin_amdgcn_readfirstlane(((int)(py - ry) * width + (int)(px - rx)) * 4);
    const __amdgpu_buffer_rsrc_t r_gx = make_rsrc(P.gx), r_gy = make_rsrc(P.gy), r_ref = make_rsrc(P.ref);
    const LutPlanes4 r_lut(P.lut, height, width);
    auto tab_at = [&](int t) { return tab_xy[t * kWave + lane]; };
    auto off_at = [&](int t) { return tab_off[t * kWave + lane]; };

    // ---- set-up: reference mean (src/oc_subset.cpp:39-53) ...
    float ref_mean;
    {
        float acc = 0.f;
        passes_batched<6>(
            NF, NT, tail_valid, [&](int t, bool valid) { return valid ? buf_f32(r_ref, off_at(t), roff) : 0.f; },
            [&](int, bool valid, float v) { acc = valid ? acc + v : acc; });
        ref_mean = uni(wave_allreduce_sum(acc) / fN);
    }
    // ... then R2, R0, A_j, B_j and the Hessian (src/oc_icgn.cpp:179-207; 2D2: 716-756): one pass at 6 DoF, two at 12 (the 78
    // running sums of the 12-DoF Hessian leave no registers for the other 26)
    float aux[NAUX], h[NH];
#pragma unroll
    for (int i = 0; i < NAUX; i++) aux[i] = 0.f;
#pragma unroll
    for (int i = 0; i < NH; i++) h[i] = 0.f;
    auto fetch = [&](int t, bool valid) {
        GradRef v;
        const unsigned off = off_at(t);
        v.gx = valid ? buf_f32(r_gx, off, goff) : 0.f;
        v.gy = valid ? buf_f32(r_gy, off, goff) : 0.f;
        v.ref = valid ? buf_f32(r_ref, off, roff) : 0.f;
        return v;
    };
    // A lane without a sample in the partial pass contributes EXACT zeros instead of being masked out: its gradients are loaded
    // as 0 and its r~ is forced to 0, so every product is +-0 and every running sum keeps its bits (a sum that starts at +0 never
    // holds -0) -- no select per sum, and no second copy of the sums alive across it.
    auto setup_sample = [&](int t, bool valid, const GradRef& v, auto with_aux, auto with_hess) {
        const f2 xy = tab_at(t);
        float sd[DOF];
        sd_row<DOF>(v.gx, v.gy, xy.x, xy.y, sd);
        if constexpr (decltype(with_aux)::value) {
            const float d = valid ? v.ref - ref_mean : 0.f;
            aux[0] = mad(d, d, aux[0]);
            aux[1] = aux[1] + d;
#pragma unroll
            for (int j = 0; j < DOF; j++) {
                aux[2 + j] = aux[2 + j] + sd[j];
                aux[2 + DOF + j] = mad(sd[j], d, aux[2 + DOF + j]);
            }
        }
        if constexpr (decltype(with_hess)::value) {
            int k = 0;
#pragma unroll
            for (int i = 0; i < DOF; i++)
#pragma unroll
                for (int j = 0; j <= i; j++, k++) h[k] = mad(sd[i], sd[j], h[k]);
        }
    };
    if constexpr (DOF == 6) {
        passes_prefetched(NF, NT, tail_valid, fetch,
                          [&](int t, bool valid, const GradRef& v) { setup_sample(t, valid, v, std::true_type{}, std::true_type{}); });
    } else {
        passes_prefetched(NF, NT, tail_valid, fetch,
                          [&](int t, bool valid, const GradRef& v) { setup_sample(t, valid, v, std::true_type{}, std::false_type{}); });
        auto fetch_grad = [&](int t, bool valid) {
            GradRef v;
            const unsigned off = off_at(t);
            v.gx = valid ? buf_f32(r_gx, off, goff) : 0.f;
            v.gy = valid ? buf_f32(r_gy, off, goff) : 0.f;
            v.ref = 0.f;
            return v;
        };
        passes_prefetched(NF, NT, tail_valid, fetch_grad,
                          [&](int t, bool valid, const GradRef& v) { setup_sample(t, valid, v, std::false_type{}, std::true_type{}); });
    }
    wave_allreduce_sum_multi<NAUX>(aux, lane);
    const float R2 = uni(aux[0]), R0 = uni(aux[1]);
    const float ref_norm = uni(sqrtf(R2));
    // A_j and B_j stay where lane j can use them (one register each instead of 2 DOF wave-uniform values)
    float a_mine = 0.f, b_mine = 0.f;
#pragma unroll
    for (int j = 0; j < DOF; j++) {
        a_mine = lane == j ? aux[2 + j] : a_mine;
        b_mine = lane == j ? aux[2 + DOF + j] : b_mine;
    }
    // H^-1 (src/oc_icgn.cpp:210 / :759); lane i < DOF ends with ROW i of it
    float hinv_row[COOP ? 1 : DOF];
    if constexpr (COOP) {
        wave_reduce_sum_multi_to_lds<NH>(h, lane, coop_area + wave * 64);
        __syncthreads();
        if (wave == 0) coop_inverse6_x8(coop_area, lane);
        __syncthreads();
        // (H^-1 stays in the workgroup's LDS area, row-major at coop_area[64 wave + 24 ...]: nobody writes there any more, and an
        // iteration reads its row back -- six registers less across the sweep)
    } else {
        float col[DOF], hinv_col[DOF];
#pragma unroll
        for (int i = 0; i < DOF; i++) col[i] = 0.f;
        wave_allreduce_sum_multi<NH>(h, lane);
        int k = 0;
#pragma unroll
        for (int i = 0; i < DOF; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                const float v = h[k++];
                if (lane == j) col[i] = v;  // H(i,j)
                if (lane == i) col[j] = v;  // H(j,i)
            }
        lu_inverse_lanes<DOF>(col, hinv_col, lane);
#pragma unroll
        for (int j = 0; j < DOF; j++) hinv_row[j] = 0.f;
#pragma unroll
        for (int i = 0; i < DOF; i++)
#pragma unroll
            for (int j = 0; j < DOF; j++) {
                const float v = wave_bcast(hinv_col[i], j);  // H^-1(i, j)
                hinv_row[j] = lane == i ? v : hinv_row[j];
            }
    }

    // ---- IC-GN loop (src/oc_icgn.cpp:216-307; 2D2: 762-858)
    float Wm[9];      // 2D1: 3 x 3 warp, wave-uniform
    float Wcol[6];    // 2D2: 6 x 6 warp, column j in lane j
    float row3[6], row4[6];
    if constexpr (DOF == 6) {
        set_warp_2d1(Wm, u_in, ux_in, uy_in, v_in, vx_in, vy_in);
    } else {
        const float q[12] = {u_in, ux_in, uy_in, 0.f, 0.f, 0.f, v_in, vx_in, vy_in, 0.f, 0.f, 0.f};
        float w36[36];
        set_warp_2d2(w36, q);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            float c = 0.f;
#pragma unroll
            for (int j = 0; j < 6; j++) c = lane == j ? w36[i * 6 + j] : c;
            Wcol[i] = c;
        }
    }
    int iter = 0;
    float dp_norm = 0.f, znssd = 0.f;
    float cur[12];
#pragma unroll
    for (int i = 0; i < 12; i++) cur[i] = 0.f;
    float cshift = ref_mean, gscale = 1.f;
#pragma nounroll
    do {
        iter++;
        if constexpr (DOF == 12) {
#pragma unroll
            for (int k = 0; k < 6; k++) {
                row3[k] = wave_bcast(Wcol[3], k);
                row4[k] = wave_bcast(Wcol[4], k);
            }
        }
        bool negative = false;
        // The range rule of BicubicBspline::compute (src/oc_cubic_bspline.cpp:137-142) for the AFFINE warp, decided before the
        // sweep from the subset's four corner samples (icgn2d.hip: every float operation of the warp is monotone in x and in y);
        // a sample outside is a -1.f in the target subset, i.e. the POI is abandoned with zncc = -3 and nothing else written.
        if constexpr (DOF == 6) {
            const float cxl = (float)((lane & 1) ? rx : -rx), cyl = (float)((lane & 2) ? ry : -ry);
            const float cax = px + (mad(Wm[1], cyl, Wm[0] * cxl) + Wm[2]), cay = py + (mad(Wm[4], cyl, Wm[3] * cxl) + Wm[5]);
            const int cxi = floor_to_int(cax), cyi = floor_to_int(cay);
            const bool cout = (unsigned)(cxi - 1) > (unsigned)(width - 4) || (unsigned)(cyi - 1) > (unsigned)(height - 4);
            if (wave_any(cout)) {
                if (lane == 0) poi[poi2d::ZNCC] = -3.f;
                return;
            }
        }
        float e0 = 0.f, e2 = 0.f, er = 0.f;
        float ej[DOF];
#pragma unroll
        for (int j = 0; j < DOF; j++) ej[j] = 0.f;
        {
            // warp the next G samples of this lane, issue their table gathers and the three image reads; CHECKED = false: every
            // lane owns a sample in all G passes
            auto issue = [&](LutFetch(&f)[G], GradRef(&v)[G], f2(&xy)[G], bool(&valid)[G], int t0, auto checked) {
                constexpr bool CHECKED = decltype(checked)::value;
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const int t = CHECKED ? min(t0 + g, NT - 1) : t0 + g;  // (a pass past the end reads the last one: unused)
                    valid[g] = CHECKED ? ((t0 + g) * kWave + lane) < N : true;
                    xy[g] = tab_at(t);
                    const float xl = xy[g].x, yl = xy[g].y;
                    float wx, wy;
                    if constexpr (DOF == 6) {
                        // Deformation2D1::warp, src/oc_deformation.cpp:94-105
                        wx = mad(Wm[1], yl, Wm[0] * xl) + Wm[2];
                        wy = mad(Wm[4], yl, Wm[3] * xl) + Wm[5];
                    } else {
                        // Deformation2D2::warp, src/oc_deformation.cpp:268-282: rows 3, 4 of W * [x^2 xy y^2 x y 1]
                        const float pv[6] = {xl * xl, xl * yl, yl * yl, xl, yl, 1.f};
                        wx = row3[0] * pv[0];
                        wy = row4[0] * pv[0];
#pragma unroll
                        for (int k = 1; k < 6; k++) {
                            wx = mad(row3[k], pv[k], wx);
                            wy = mad(row4[k], pv[k], wy);
                        }
                    }
                    float ax = px + wx, ay = py + wy;
                    if constexpr (CHECKED) {  // a lane past the end of the subset fetches a harmless in-range point
                        ax = valid[g] ? ax : 1.f;
                        ay = valid[g] ? ay : 1.f;
                    }
                    if constexpr (DOF == 6) {
                        // inside the interpolatable range (the corner test above)
                        const int xi = floor_to_int(ax), yi = floor_to_int(ay);
                        f[g].dx = __builtin_amdgcn_fractf(ax);
                        f[g].dy = __builtin_amdgcn_fractf(ay);
                        r_lut.load(f[g], (__umul24((unsigned)yi, (unsigned)width) + (unsigned)xi) << 4);
                    } else {
                        bool out = false;
                        lut_fetch<false>(f[g], r_lut, height, width, ax, ay, out);
                        negative = negative || out;
                    }
                    const unsigned off = off_at(t);
                    v[g].gx = valid[g] ? buf_f32(r_gx, off, goff) : 0.f;
                    v[g].gy = valid[g] ? buf_f32(r_gy, off, goff) : 0.f;
                    v[g].ref = valid[g] ? buf_f32(r_ref, off, roff) : 0.f;
                }
            };
            auto consume = [&](const LutFetch(&f)[G], const GradRef(&v)[G], const f2(&xy)[G], const bool(&valid)[G], auto checked) {
                constexpr bool CHECKED = decltype(checked)::value;
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const float tv = lut_value(f[g]);
                    const float rsv = v[g].ref - ref_mean;
                    const bool ok = CHECKED ? valid[g] : true;
                    // (a lane without a sample: e' = 0 and zero gradients, i.e. exact zeros into every sum -- see the set-up)
                    const float e = ok ? mad(gscale, tv - cshift, -rsv) : 0.f;
                    float sd[DOF];
                    sd_row<DOF>(v[g].gx, v[g].gy, xy[g].x, xy[g].y, sd);
                    negative = negative || (ok && tv < 0.f);
#pragma unroll
                    for (int j = 0; j < DOF; j++) ej[j] = mad(sd[j], e, ej[j]);
                    e0 = e0 + e;
                    e2 = mad(e, e, e2);
                    er = mad(e, rsv, er);
                }
            };
            const int full_groups = NF / G;
            int t0 = 0;
#pragma nounroll
            for (int q = 0; q < full_groups; q++, t0 += G) {
                if (q % SWEEP_SYNC == 0) __builtin_amdgcn_s_barrier();  // lockstep: scheduling only, no data crosses it
                LutFetch f[G];
                GradRef v[G];
                f2 xy[G];
                bool valid[G];
                issue(f, v, xy, valid, t0, std::false_type{});
                consume(f, v, xy, valid, std::false_type{});
            }
#pragma nounroll
            for (; t0 < NT; t0 += G) {
                LutFetch f[G];
                GradRef v[G];
                f2 xy[G];
                bool valid[G];
                issue(f, v, xy, valid, t0, std::true_type{});
                consume(f, v, xy, valid, std::true_type{});
            }
        }
        // src/oc_icgn.cpp:251-255
        if (wave_any(negative)) {
            if (lane == 0) poi[poi2d::ZNCC] = -3.f;
            return;
        }
        float red[DOF + 3];
#pragma unroll
        for (int j = 0; j < DOF; j++) red[j] = ej[j];
        red[DOF] = e0;
        red[DOF + 1] = e2;
        red[DOF + 2] = er;
        wave_allreduce_sum_multi<DOF + 3>(red, lane);
        const OnepassScalars sc = onepass_scalars(red[DOF], red[DOF + 1], red[DOF + 2], R0, R2, ref_norm, fN, gscale);
        znssd = uni(sc.znssd);
        // b_j = (alpha E_j + a B_j) - q A_j, formed in lane j and handed round
        float num[DOF];
        {
            float e_mine = 0.f;
#pragma unroll
            for (int j = 0; j < DOF; j++) e_mine = lane == j ? red[j] : e_mine;
            const float n_mine = (sc.alpha * e_mine + sc.a * b_mine) - sc.q * a_mine;
#pragma unroll
            for (int j = 0; j < DOF; j++) num[j] = wave_bcast(n_mine, j);
        }
        cshift = uni(cshift + sc.m);
        gscale = uni(sc.f);
        // dp = H^-1 * b (src/oc_icgn.cpp:279-286): lane i forms row i, ascending j like the reference loop
        float dp[DOF];
        {
            float mine = 0.f;
            if constexpr (COOP) {
                const float* __restrict__ row = coop_area + wave * 64 + 24 + min(lane, DOF - 1) * DOF;
#pragma unroll
                for (int j = 0; j < DOF; j++) mine += (lane < DOF ? row[j] : 0.f) * num[j];
            } else {
#pragma unroll
                for (int j = 0; j < DOF; j++) mine += hinv_row[j % (COOP ? 1 : DOF)] * num[j];
            }
#pragma unroll
            for (int i = 0; i < DOF; i++) dp[i] = wave_bcast(mine, i);
        }
        // W <- W * (dW)^-1 ; p <- W (src/oc_icgn.cpp:287-293 / 828-834)
        const int rx2 = rx * rx, ry2 = ry * ry;
        if constexpr (DOF == 6) {
            float dW[9], dWi[9], Wn[9];
            set_warp_2d1(dW, dp[0], dp[1], dp[2], dp[3], dp[4], dp[5]);
            inverse3(dW, dWi);
            mat_mul<3>(Wm, dWi, Wn);
#pragma unroll
            for (int i = 0; i < 9; i++) Wm[i] = uni(Wn[i]);
            // src/oc_deformation.cpp:107-115
            cur[0] = Wm[2]; cur[1] = Wm[0] - 1.f; cur[2] = Wm[1];
            cur[6] = Wm[5]; cur[7] = Wm[3]; cur[8] = Wm[4] - 1.f;
            // convergence norm (src/oc_icgn.cpp:296-306)
            const float d = dp[0] * dp[0] + dp[1] * dp[1] * rx2 + dp[2] * dp[2] * ry2 + dp[3] * dp[3] + dp[4] * dp[4] * rx2 +
                            dp[5] * dp[5] * ry2;
            dp_norm = uni(sqrtf(d));
        } else {
            float dW[36];
            set_warp_2d2(dW, dp);
            // (dW)^-1 by the lane-distributed LU (Eigen PartialPivLU for 6 x 6, src/oc_icgn.cpp:831)
            float dcol[6], dinv[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                float c = 0.f;
#pragma unroll
                for (int j = 0; j < 6; j++) c = lane == j ? dW[i * 6 + j] : c;
                dcol[i] = c;
            }
            lu_inverse_lanes<6>(dcol, dinv, lane);
            // lane j: column j of W * dW^-1, inner index ascending
            float ncol[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                float v = wave_bcast(Wcol[i], 0) * dinv[0];
#pragma unroll
                for (int k = 1; k < 6; k++) v = v + wave_bcast(Wcol[i], k) * dinv[k];
                ncol[i] = v;
            }
#pragma unroll
            for (int i = 0; i < 6; i++) Wcol[i] = ncol[i];
            // Deformation2D2::setDeformation(), src/oc_deformation.cpp:284-299
            const float r30 = wave_bcast(Wcol[3], 0), r31 = wave_bcast(Wcol[3], 1), r32 = wave_bcast(Wcol[3], 2);
            const float r33 = wave_bcast(Wcol[3], 3), r34 = wave_bcast(Wcol[3], 4), r35 = wave_bcast(Wcol[3], 5);
            const float r40 = wave_bcast(Wcol[4], 0), r41 = wave_bcast(Wcol[4], 1), r42 = wave_bcast(Wcol[4], 2);
            const float r43 = wave_bcast(Wcol[4], 3), r44 = wave_bcast(Wcol[4], 4), r45 = wave_bcast(Wcol[4], 5);
            cur[0] = r35; cur[1] = r33 - 1.f; cur[2] = r34; cur[3] = r30 * 2.f; cur[4] = r31; cur[5] = r32 * 2.f;
            cur[6] = r45; cur[7] = r43; cur[8] = r44 - 1.f; cur[9] = r40 * 2.f; cur[10] = r41; cur[11] = r42 * 2.f;
            const int rxy2 = rx2 * ry2;
            constexpr int D = DOF;  // keeps the dp[] indices in range when this branch is discarded
            // src/oc_icgn.cpp:837-857 (integer-truncated weights are reference behaviour)
            const int rx4 = (int)(rx2 * rx2 * 0.25f), ry4 = (int)(ry2 * ry2 * 0.25f);
            const float d = dp[0] * dp[0] + dp[1] * dp[1] * rx2 + dp[2] * dp[2] * ry2 + dp[3 % D] * dp[3 % D] * rx4 +
                            dp[5 % D] * dp[5 % D] * ry4 + dp[4 % D] * dp[4 % D] * rxy2 + dp[6 % D] * dp[6 % D] +
                            dp[7 % D] * dp[7 % D] * rx2 + dp[8 % D] * dp[8 % D] * ry2 + dp[9 % D] * dp[9 % D] * rx4 +
                            dp[11 % D] * dp[11 % D] * ry4 + dp[10 % D] * dp[10 % D] * rxy2;
            dp_norm = uni(sqrtf(d));
        }
    } while (iter < P.stop && dp_norm >= P.conv);

    // ---- outputs (src/oc_icgn.cpp:310-340; 2D2: 860-897)
    if (lane == 0) {
        float zncc = 0.5f * (2 - znssd);
        const float fiter = (float)iter;
        if (dp_norm >= P.conv && fiter >= P.stop) zncc = -4.f;
        float out_u = cur[0], out_v = cur[6];
        if (isnan(zncc) || isnan(out_u) || isnan(out_v)) {
            out_u = u_in;
            out_v = v_in;
            zncc = -5.f;
        }
        poi[poi2d::U] = out_u;
        poi[poi2d::UX] = cur[1];
        poi[poi2d::UY] = cur[2];
        poi[poi2d::V] = out_v;
        poi[poi2d::VX] = cur[7];
        poi[poi2d::VY] = cur[8];
        if constexpr (DOF == 12) {
            poi[poi2d::UXX] = cur[3];
            poi[poi2d::UXY] = cur[4];
            poi[poi2d::UYY] = cur[5];
            poi[poi2d::VXX] = cur[9];
            poi[poi2d::VXY] = cur[10];
            poi[poi2d::VYY] = cur[11];
        }
        poi[poi2d::U0] = u_in;
        poi[poi2d::V0] = v_in;
        poi[poi2d::ZNCC] = zncc;
        poi[poi2d::ITER] = fiter;
        poi[poi2d::CONV] = dp_norm;
        poi[poi2d::SRX] = (float)rx;
        poi[poi2d::SRY] = (float)ry;
    }
}

template <int DOF>
static hipError_t launch_dof(const Icgn2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (p.offsets || p.self_adaptive) return hipErrorNotSupported;  // one radius per launch, integer local coordinates
    const long long N = (2LL * p.rx + 1) * (2LL * p.ry + 1);
    const int nt = (int)((N + 63) / 64);
    const size_t lds = ochip_host::icgn2d_onepass_lds_bytes((size_t)nt);
    if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
    auto kern = icgn2d_onepass_kernel<DOF>;
    // the dynamic-LDS limit is a per-device property of the loaded function: raised once on every device this process launches on
    static std::atomic<unsigned long long> attr_devices{0};
    int dev = 0;
    hipError_t derr = hipGetDevice(&dev);
    if (derr != hipSuccess) return derr;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_devices.load(std::memory_order_acquire) & bit)) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
        if (err != hipSuccess) return err;
        attr_devices.fetch_or(bit, std::memory_order_release);
    }
    const size_t groups = (count + kWpb - 1) / kWpb;
    OnepassLaunch L;
    L.stride_f = stride_f;
    L.nt = nt;
    L.count = count;
    L.xcd_chunk = xcd ? (int)((groups + 7) / 8) : 0;
    const size_t grid = xcd ? (size_t)L.xcd_chunk * 8 : groups;
    (void)hipGetLastError();  // drop stale errors of earlier, unrelated calls
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * kWpb), lds, stream, p, pois, L);
    return hipGetLastError();
}

}  // namespace onepass

hipError_t launch_icgn2d1_onepass(const Icgn2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    return onepass::launch_dof<6>(p, pois, stride_f, count, xcd, stream);
}

hipError_t launch_icgn2d2_onepass(const Icgn2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    return onepass::launch_dof<12>(p, pois, stride_f, count, xcd, stream);
}

}  // namespace ochip

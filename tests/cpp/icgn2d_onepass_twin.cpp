// icgn2d_onepass_twin.cpp -- CPU restatement of the one-pass arithmetic contract of ICGN2D1 / ICGN2D2
// (oc_hip_set_tuning "arith_onepass", opencorr_amd/csrc/icgn2d_onepass.hip).
//
// Test infrastructure: the kernel must equal this file in EVERY bit.  Built by tests/onepass_twin.py with
// g++ -O2 -ffp-contract=off -fopenmp: the compiler contracts nothing, every fused site is an explicit std::fmaf, every
// other operation rounds on its own.  Arrays are those of oracle.Prepared2D (the bicubic table interleaved, 16 floats per
// pixel), records are POI2D (25 floats).
//
// Summation: sample s = r * W + c is owned by lane s % 64, a lane adds its samples in increasing s, the 64 partial sums are
// combined by the xor butterfly with ascending offsets 1, 2, ... 32 (the association of every kernel of the library).
//
// Set-up per POI (what the fused contract computes): mean, r~ = r - mean, R2 = sum fma(r~, r~), |R| = sqrt(R2), the
// steepest-descent rows SD_j, H = sum fma(SD_i, SD_j), H^-1 by LU with partial pivoting; new: R0 = sum r~, A_j = sum SD_j,
// B_j = sum fma(SD_j, r~).
// Iteration: ONE sweep.  With the carried shift c (first: the reference mean) and scale g (first: 1) a sample contributes
// e' = fma(g, t - c, -r~) to  E0 += e',  E2 = fma(e', e', E2),  Er = fma(e', r~, Er),  E_j = fma(SD_j, e', E_j);  the
// scalar expressions behind the reduction are written out in scalars() below, each operation rounded on its own.
#include <cmath>
#include <cstddef>
#include <vector>

namespace {

constexpr int kLanes = 64;

template <int K>
struct Acc {
    std::vector<float> part;   // [K][64]
    Acc() : part((size_t)K * kLanes, 0.f) {}
    inline void add(int s, int k, float v) { part[(size_t)k * kLanes + (s & (kLanes - 1))] += v; }
    inline void mac(int s, int k, float x, float y) {
        float& slot = part[(size_t)k * kLanes + (s & (kLanes - 1))];
        slot = std::fmaf(x, y, slot);
    }
    inline void finish() {
        float tmp[kLanes];
        for (int k = 0; k < K; k++) {
            float* p = &part[(size_t)k * kLanes];
            for (int off = 1; off < kLanes; off <<= 1) {
                for (int l = 0; l < kLanes; l++) tmp[l] = p[l] + p[l ^ off];
                for (int l = 0; l < kLanes; l++) p[l] = tmp[l];
            }
        }
    }
    inline float get(int k) const { return part[(size_t)k * kLanes]; }
};

// inverse of an n x n row-major matrix: LU with partial (row) pivoting, solve against the identity
void lu_inverse(const float* A, float* Ainv, int n) {
    float lu[12 * 12];
    int perm[12];
    for (int i = 0; i < n * n; i++) lu[i] = A[i];
    for (int i = 0; i < n; i++) perm[i] = i;
    for (int k = 0; k < n; k++) {
        int piv = k;
        float best = std::fabs(lu[k * n + k]);
        for (int r = k + 1; r < n; r++) {
            const float v = std::fabs(lu[r * n + k]);
            if (v > best) { best = v; piv = r; }
        }
        if (piv != k) {
            for (int c = 0; c < n; c++) { const float t = lu[k * n + c]; lu[k * n + c] = lu[piv * n + c]; lu[piv * n + c] = t; }
            const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
        }
        const float d = lu[k * n + k];
        for (int r = k + 1; r < n; r++) {
            const float f = lu[r * n + k] / d;
            lu[r * n + k] = f;
            for (int c = k + 1; c < n; c++) lu[r * n + c] = lu[r * n + c] - f * lu[k * n + c];
        }
    }
    for (int col = 0; col < n; col++) {
        float y[12];
        for (int i = 0; i < n; i++) {
            float v = (perm[i] == col) ? 1.f : 0.f;
            for (int j = 0; j < i; j++) v = v - lu[i * n + j] * y[j];
            y[i] = v;
        }
        for (int i = n - 1; i >= 0; i--) {
            float v = y[i];
            for (int j = i + 1; j < n; j++) v = v - lu[i * n + j] * y[j];
            y[i] = v / lu[i * n + i];
        }
        for (int i = 0; i < n; i++) Ainv[i * n + col] = y[i];
    }
}

void mat_mul(const float* a, const float* b, float* c, int n) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            float v = a[i * n + 0] * b[0 * n + j];
            for (int k = 1; k < n; k++) v = v + a[i * n + k] * b[k * n + j];
            c[i * n + j] = v;
        }
}

inline float cof3(const float* m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
void inverse3(const float* m, float* r) {
    const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
    const float det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
    const float invdet = 1.f / det;
    r[0] = c0 * invdet; r[1] = c1 * invdet; r[2] = c2 * invdet;
    r[3] = cof3(m, 0, 1) * invdet; r[4] = cof3(m, 1, 1) * invdet; r[5] = cof3(m, 2, 1) * invdet;
    r[6] = cof3(m, 0, 2) * invdet; r[7] = cof3(m, 1, 2) * invdet; r[8] = cof3(m, 2, 2) * invdet;
}

// bicubic value with every "+ product" fused; -1 outside the interpolatable range
inline float bspline(const float* lut, int height, int width, float x, float y) {
    if (x < 1 || y < 1 || x >= width - 2 || y >= height - 2 || std::isnan(x) || std::isnan(y)) return -1.f;
    const int xi = (int)std::floor(x), yi = (int)std::floor(y);
    const float dx = x - xi, dy = y - yi;
    const float dx2 = dx * dx, dy2 = dy * dy;
    const float dx3 = dx2 * dx, dy3 = dy2 * dy;
    const float* c = lut + ((size_t)yi * width + xi) * 16;
    float v = c[0];
    v = std::fmaf(c[1], dx, v);
    v = std::fmaf(c[2], dx2, v);
    v = std::fmaf(c[3], dx3, v);
    v = std::fmaf(c[4], dy, v);
    v = std::fmaf(c[5] * dy, dx, v);
    v = std::fmaf(c[6] * dy, dx2, v);
    v = std::fmaf(c[7] * dy, dx3, v);
    v = std::fmaf(c[8], dy2, v);
    v = std::fmaf(c[9] * dy2, dx, v);
    v = std::fmaf(c[10] * dy2, dx2, v);
    v = std::fmaf(c[11] * dy2, dx3, v);
    v = std::fmaf(c[12], dy3, v);
    v = std::fmaf(c[13] * dy3, dx, v);
    v = std::fmaf(c[14] * dy3, dx2, v);
    v = std::fmaf(c[15] * dy3, dx3, v);
    return v;
}

template <int DOF>
inline void sd_row(float g_x, float g_y, float xl, float yl, float* sd) {
    if (DOF == 6) {
        sd[0] = g_x; sd[1] = g_x * xl; sd[2] = g_x * yl;
        sd[3] = g_y; sd[4] = g_y * xl; sd[5] = g_y * yl;
    } else {
        const float xx = (xl * xl) * 0.5f, xy = xl * yl, yy = (yl * yl) * 0.5f;
        sd[0] = g_x; sd[1] = g_x * xl; sd[2] = g_x * yl; sd[3] = g_x * xx; sd[4] = g_x * xy; sd[5] = g_x * yy;
        sd[6 % DOF] = g_y; sd[7 % DOF] = g_y * xl; sd[8 % DOF] = g_y * yl; sd[9 % DOF] = g_y * xx; sd[10 % DOF] = g_y * xy;
        sd[11 % DOF] = g_y * yy;
    }
}

inline void set_warp_2d1(float* w, float u, float ux, float uy, float v, float vx, float vy) {
    w[0] = 1.f + ux; w[1] = uy; w[2] = u;
    w[3] = vx; w[4] = 1.f + vy; w[5] = v;
    w[6] = 0.f; w[7] = 0.f; w[8] = 1.f;
}

inline void set_warp_2d2(float* w, const float* q) {
    const float u = q[0], ux = q[1], uy = q[2], uxx = q[3], uxy = q[4], uyy = q[5];
    const float v = q[6], vx = q[7], vy = q[8], vxx = q[9], vxy = q[10], vyy = q[11];
    w[0] = 1.f + 2.f * ux + ux * ux + u * uxx;
    w[1] = 2.f * u * uxy + 2.f * (1.f + ux) * uy;
    w[2] = uy * uy + u * uyy;
    w[3] = 2.f * u * (1 + ux);
    w[4] = 2.f * u * uy;
    w[5] = u * u;
    w[6] = 0.5f * (v * uxx + 2.f * (1.f + ux) * vx + u * vxx);
    w[7] = 1.f + uy * vx + ux * vy + v * uxy + u * vxy + vy + ux;
    w[8] = 0.5f * (v * uyy + 2.f * uy * (1.f + vy) + u * vyy);
    w[9] = v + v * ux + u * vx;
    w[10] = u + v * uy + u * vy;
    w[11] = u * v;
    w[12] = vx * vx + v * vxx;
    w[13] = 2.f * v * vxy + 2.f * vx * (1.f + vy);
    w[14] = 1.f + 2.f * vy + vy * vy + v * vyy;
    w[15] = 2.f * v * vx;
    w[16] = 2.f * v * (1.f + vy);
    w[17] = v * v;
    w[18] = 0.5f * uxx; w[19] = uxy; w[20] = 0.5f * uyy; w[21] = 1.f + ux; w[22] = uy; w[23] = u;
    w[24] = 0.5f * vxx; w[25] = vxy; w[26] = 0.5f * vyy; w[27] = vx; w[28] = 1.f + vy; w[29] = v;
    w[30] = 0.f; w[31] = 0.f; w[32] = 0.f; w[33] = 0.f; w[34] = 0.f; w[35] = 1.f;
}

// What follows the reduction of an iteration's sums: every operation rounds on its own, in exactly this order.
struct Scalars {
    float m, f, znssd, alpha, a, q;
};
inline Scalars scalars(float E0, float E2, float Er, float R0, float R2, float ref_norm, float fN, float g) {
    Scalars r;
    const float S1 = (E0 + R0) / g;
    const float S2 = ((E2 + 2.f * Er) + R2) / (g * g);
    r.m = S1 / fN;
    const float tar_norm = std::sqrt(S2 - S1 * r.m);
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
void onepass_poi(const float* ref, const float* gxi, const float* gyi, const float* lut, int height, int width, int rx, int ry,
                 float conv, float stop, float* poi, std::vector<float>& scratch) {
    const float px = poi[0], py = poi[1];
    float* p = poi + 2;
    float* res = poi + 14;
    float* srad = poi + 23;
    const float u_in = p[0], v_in = p[6];
    // (the geometric part negated, as the kernel has it: a NaN coordinate is rejected like a subset that leaves the image)
    if (!(py - ry >= 0 && px - rx >= 0 && py + ry <= height - 1 && px + rx <= width - 1) || std::fabs(u_in) >= width ||
        std::fabs(v_in) >= height || res[2] < 0 || std::isnan(u_in) || std::isnan(v_in)) {
        res[2] = res[2] >= 0 ? -3.f : res[2];
        return;
    }
    const int W = 2 * rx + 1, H = 2 * ry + 1, N = W * H;
    const float fN = (float)N;
    scratch.resize((size_t)N * 3);
    float* rs = scratch.data();
    float* sgx = rs + N;
    float* sgy = sgx + N;
    const int x0 = (int)(px - rx), y0 = (int)(py - ry);

    // ---- set-up
    float ref_mean, ref_norm, R0, R2;
    {
        Acc<1> a;
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const int s = r * W + c;
                rs[s] = ref[(size_t)(y0 + r) * width + (x0 + c)];
                a.add(s, 0, rs[s]);
            }
        a.finish();
        ref_mean = a.get(0) / fN;
    }
    constexpr int NH = DOF * (DOF + 1) / 2;
    float hess[DOF * DOF], hinv[DOF * DOF], A[DOF], B[DOF];
    {
        Acc<2 + 2 * DOF> aux;   // R2, R0, A_j, B_j
        Acc<NH> ah;
        const int gx0 = (int)px, gy0 = (int)py;
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const int s = r * W + c;
                const int xl = c - rx, yl = r - ry;
                const float d = rs[s] - ref_mean;
                rs[s] = d;
                const float g_x = gxi[(size_t)(gy0 + yl) * width + (gx0 + xl)];
                const float g_y = gyi[(size_t)(gy0 + yl) * width + (gx0 + xl)];
                sgx[s] = g_x;
                sgy[s] = g_y;
                float sd[DOF];
                sd_row<DOF>(g_x, g_y, (float)xl, (float)yl, sd);
                aux.mac(s, 0, d, d);
                aux.add(s, 1, d);
                for (int j = 0; j < DOF; j++) {
                    aux.add(s, 2 + j, sd[j]);
                    aux.mac(s, 2 + DOF + j, sd[j], d);
                }
                int t = 0;
                for (int i = 0; i < DOF; i++)
                    for (int j = 0; j <= i; j++) ah.mac(s, t++, sd[i], sd[j]);
            }
        aux.finish();
        ah.finish();
        R2 = aux.get(0);
        R0 = aux.get(1);
        ref_norm = std::sqrt(R2);
        for (int j = 0; j < DOF; j++) {
            A[j] = aux.get(2 + j);
            B[j] = aux.get(2 + DOF + j);
        }
        int t = 0;
        for (int i = 0; i < DOF; i++)
            for (int j = 0; j <= i; j++) {
                hess[i * DOF + j] = ah.get(t);
                hess[j * DOF + i] = ah.get(t);
                t++;
            }
    }
    lu_inverse(hess, hinv, DOF);

    const float u0 = p[0], ux0 = p[1], uy0 = p[2], v0 = p[6], vx0 = p[7], vy0 = p[8];
    constexpr int WN = (DOF == 6) ? 3 : 6;
    float Wm[WN * WN];
    if (DOF == 6) {
        set_warp_2d1(Wm, u0, ux0, uy0, v0, vx0, vy0);
    } else {
        const float q[12] = {u0, ux0, uy0, 0.f, 0.f, 0.f, v0, vx0, vy0, 0.f, 0.f, 0.f};
        set_warp_2d2(Wm, q);
    }

    int iter = 0;
    float dp_norm = 0.f, znssd = 0.f;
    float cur[12] = {0.f};
    float cshift = ref_mean, gscale = 1.f;
    do {
        iter++;
        bool negative = false;
        Acc<DOF + 3> ae;   // E_j, E0, E2, Er
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const int s = r * W + c;
                const float xl = (float)(c - rx), yl = (float)(r - ry);
                float wx, wy;
                if (DOF == 6) {
                    wx = std::fmaf(Wm[1], yl, Wm[0] * xl) + Wm[2];
                    wy = std::fmaf(Wm[4], yl, Wm[3] * xl) + Wm[5];
                } else {
                    const float pv[6] = {xl * xl, xl * yl, yl * yl, xl, yl, 1.f};
                    const float* r3 = Wm + 3 * WN;
                    const float* r4 = Wm + 4 * WN;
                    wx = r3[0] * pv[0];
                    wy = r4[0] * pv[0];
                    for (int k = 1; k < 6; k++) {
                        wx = std::fmaf(r3[k], pv[k], wx);
                        wy = std::fmaf(r4[k], pv[k], wy);
                    }
                }
                const float t = bspline(lut, height, width, px + wx, py + wy);
                if (t < 0.f) negative = true;
                const float e = std::fmaf(gscale, t - cshift, -rs[s]);
                float sd[DOF];
                sd_row<DOF>(sgx[s], sgy[s], xl, yl, sd);
                for (int j = 0; j < DOF; j++) ae.mac(s, j, sd[j], e);
                ae.add(s, DOF, e);
                ae.mac(s, DOF + 1, e, e);
                ae.mac(s, DOF + 2, e, rs[s]);
            }
        if (negative) {
            res[2] = -3.f;
            return;
        }
        ae.finish();
        const float E0 = ae.get(DOF), E2 = ae.get(DOF + 1), Er = ae.get(DOF + 2);
        const Scalars sc = scalars(E0, E2, Er, R0, R2, ref_norm, fN, gscale);
        znssd = sc.znssd;
        float num[DOF];
        for (int j = 0; j < DOF; j++) num[j] = (sc.alpha * ae.get(j) + sc.a * B[j]) - sc.q * A[j];
        cshift = cshift + sc.m;
        gscale = sc.f;

        float dp[DOF];
        for (int i = 0; i < DOF; i++) {
            float v = 0.f;
            for (int j = 0; j < DOF; j++) v += hinv[i * DOF + j] * num[j];
            dp[i] = v;
        }
        float dW[WN * WN], dWi[WN * WN], Wn[WN * WN];
        if (DOF == 6) {
            set_warp_2d1(dW, dp[0], dp[1], dp[2], dp[3], dp[4], dp[5]);
            inverse3(dW, dWi);
        } else {
            float q12[12];
            for (int i = 0; i < 12; i++) q12[i] = dp[i % DOF];
            set_warp_2d2(dW, q12);
            lu_inverse(dW, dWi, WN);
        }
        mat_mul(Wm, dWi, Wn, WN);
        for (int i = 0; i < WN * WN; i++) Wm[i] = Wn[i];
        const int rx2 = rx * rx, ry2 = ry * ry;
        if (DOF == 6) {
            cur[0] = Wm[2]; cur[1] = Wm[0] - 1.f; cur[2] = Wm[1];
            cur[6] = Wm[5]; cur[7] = Wm[3]; cur[8] = Wm[4] - 1.f;
            const float d = dp[0] * dp[0] + dp[1] * dp[1] * rx2 + dp[2] * dp[2] * ry2 + dp[3] * dp[3] + dp[4] * dp[4] * rx2 +
                            dp[5] * dp[5] * ry2;
            dp_norm = std::sqrt(d);
        } else {
            const float* r3 = Wm + 3 * WN;
            const float* r4 = Wm + 4 * WN;
            cur[0] = r3[5]; cur[1] = r3[3] - 1.f; cur[2] = r3[4]; cur[3] = r3[0] * 2.f; cur[4] = r3[1]; cur[5] = r3[2] * 2.f;
            cur[6] = r4[5]; cur[7] = r4[3]; cur[8] = r4[4] - 1.f; cur[9] = r4[0] * 2.f; cur[10] = r4[1]; cur[11] = r4[2] * 2.f;
            const int rxy2 = rx2 * ry2;
            const int rx4 = (int)(rx2 * rx2 * 0.25f), ry4 = (int)(ry2 * ry2 * 0.25f);
            constexpr int D = DOF;
            const float* q = dp;
            const float d = q[0] * q[0] + q[1] * q[1] * rx2 + q[2] * q[2] * ry2 + q[3 % D] * q[3 % D] * rx4 + q[5 % D] * q[5 % D] * ry4 +
                            q[4 % D] * q[4 % D] * rxy2 + q[6 % D] * q[6 % D] + q[7 % D] * q[7 % D] * rx2 + q[8 % D] * q[8 % D] * ry2 +
                            q[9 % D] * q[9 % D] * rx4 + q[11 % D] * q[11 % D] * ry4 + q[10 % D] * q[10 % D] * rxy2;
            dp_norm = std::sqrt(d);
        }
    } while (iter < stop && dp_norm >= conv);

    if (DOF == 6) {
        p[0] = cur[0]; p[1] = cur[1]; p[2] = cur[2];
        p[6] = cur[6]; p[7] = cur[7]; p[8] = cur[8];
    } else {
        for (int i = 0; i < 12; i++) p[i] = cur[i];
    }
    res[0] = u0;
    res[1] = v0;
    res[2] = 0.5f * (2 - znssd);
    res[3] = (float)iter;
    res[4] = dp_norm;
    srad[0] = (float)rx;
    srad[1] = (float)ry;
    if (res[4] >= conv && res[3] >= stop) res[2] = -4.f;
    if (std::isnan(res[2]) || std::isnan(p[0]) || std::isnan(p[6])) {
        p[0] = res[0];
        p[6] = res[1];
        res[2] = -5.f;
    }
}

}  // namespace

extern "C" void oc_twin_icgn2d_onepass(int dof, const float* ref, const float* gx, const float* gy, const float* lut, int height,
                                       int width, int rx, int ry, float conv, float stop, float* pois, long n, int stride_floats) {
#pragma omp parallel
    {
        std::vector<float> scratch;
#pragma omp for schedule(dynamic, 16)
        for (long i = 0; i < n; i++) {
            float* poi = pois + (size_t)i * stride_floats;
            if (dof == 6) onepass_poi<6>(ref, gx, gy, lut, height, width, rx, ry, conv, stop, poi, scratch);
            else onepass_poi<12>(ref, gx, gy, lut, height, width, rx, ry, conv, stop, poi, scratch);
        }
    }
}

// sift3d_jacobi.h -- the eigen-decomposition of SIFT3D::assignOrientation's structure tensor (src/oc_sift.cpp:948-950 calls
// Eigen::EigenSolver<Matrix3f>): a cyclic Jacobi iteration on the symmetric 3 x 3 in double.  ONE text for the kernel
// (sift3d_features.hip) and the CPU twin (tests/cpp/sift3d_features_twin.cpp): both compile this header with -ffp-contract=off, and
// IEEE double +, -, *, / and sqrt give the same bits on either side.  No transcendental call.
//
//   sweep:   the pairs (p, q) = (0, 1), (0, 2), (1, 2) in that order
//   skip:    a pair with |a_pq| <= 2^-62 (|a_pp| + |a_qq|) is set to 0 and left alone
//   rotate:  theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (sgn(0) = +1), c = 1 / sqrt(t^2 + 1),
//            s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, the third row / column and the columns p, q of V rotated by (c, s)
//   stop:    after a sweep that skipped all three pairs, or after kSiftJacobiSweeps sweeps
// value[i] = a_ii, vector[i] = column i of V (V starts as the identity), in the order of the diagonal: the caller sorts.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define OC_SIFT_HD __host__ __device__
#else
#define OC_SIFT_HD
#endif

namespace ochip_sift {

constexpr int kSiftJacobiSweeps = 16;

// a: xx xy xz yy yz zz
OC_SIFT_HD inline void sift3d_jacobi(const double* a, double* value, double (*vector)[3]) {
    double m[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < kSiftJacobiSweeps; sweep++) {
        int rotated = 0;
        for (int pair = 0; pair < 3; pair++) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = m[p][q];
            if (fabs(apq) <= 0x1p-62 * (fabs(m[p][p]) + fabs(m[q][q]))) {
                m[p][q] = m[q][p] = 0.0;
                continue;
            }
            rotated++;
            const double theta = (m[q][q] - m[p][p]) / (2.0 * apq);
            const double root = fabs(theta) + sqrt(theta * theta + 1.0);
            const double t = theta < 0.0 ? -1.0 / root : 1.0 / root;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            m[p][p] = m[p][p] - t * apq;
            m[q][q] = m[q][q] + t * apq;
            m[p][q] = m[q][p] = 0.0;
            const double arp = m[r][p], arq = m[r][q];
            m[r][p] = m[p][r] = c * arp - s * arq;
            m[r][q] = m[q][r] = s * arp + c * arq;
            for (int k = 0; k < 3; k++) {
                const double vkp = v[k][p], vkq = v[k][q];
                v[k][p] = c * vkp - s * vkq;
                v[k][q] = s * vkp + c * vkq;
            }
        }
        if (rotated == 0) break;
    }
    for (int i = 0; i < 3; i++) {
        value[i] = m[i][i];
        for (int k = 0; k < 3; k++) vector[i][k] = v[k][i];
    }
}

}  // namespace ochip_sift

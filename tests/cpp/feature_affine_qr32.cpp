// feature_affine_qr32.cpp -- the final fit of FeatureAffine in the reference's arithmetic: float32 Householder QR with column
// pivoting, `ref_neighbors.colPivHouseholderQr().solve(tar_neighbors)` of src/oc_feature_affine.cpp:303-316 / :561-576, through
// the stand-in of oracle/ref_stubs/Eigen.  tests/test_feature_affine_twin_cpu.py measures the distance between this and the
// float64 model: four times its largest value is the bar the twin's deformations are held to.
#include <Eigen>

extern "C" void oc_fa_qr32(int ndim, const float* ref_rows, const float* tar_rows, int m, float* X) {
    const int D = ndim + 1;
    Eigen::MatrixXf a(m, D);
    for (int i = 0; i < m; i++) {
        for (int c = 0; c < ndim; c++) a(i, c) = ref_rows[i * ndim + c];
        a(i, ndim) = 1.f;
    }
    const auto qr = a.colPivHouseholderQr();
    for (int r = 0; r < D; r++) {  // the reference solves for D columns, the last being the ones
        Eigen::VectorXf b(m);
        for (int i = 0; i < m; i++) b(i) = r < ndim ? tar_rows[i * ndim + r] : 1.f;
        const Eigen::VectorXf x = qr.solve(b);
        if (r < ndim)
            for (int k = 0; k < D; k++) X[k * ndim + r] = x(k);
    }
}

// fft_hermitian_host_check.hip -- the real-output inverse transform of opencorr_amd/csrc/fft_device.h (ifft32_hermitian, the last
// pass of the 32 x 32 FFTCC2D kernel), executed on the HOST against a double-precision DFT (test infrastructure;
// tests/test_fft_hermitian_host.py builds and runs it, no GPU needed).  Random Hermitian lines X[32 - k] = conj X[k] with real
// X[0], X[16]; the routine sees X[0 .. 16] only.  Prints one line per seed
//     32  max|err| / max|x|
// and exits non-zero if any relative error exceeds 2e-6 * log2(32), the bar of fft_host_check.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../opencorr_amd/csrc/fft_device.h"

using namespace ochip::fftdev;

static double check_one(unsigned seed) {
    constexpr int N = 32;
    c2 X[N / 2 + 1], z[N / 2];
    double re[N], im[N];
    srand(seed);
    for (int k = 0; k <= N / 2; k++) {
        const float a = (float)((rand() / (double)RAND_MAX) * 2.0 - 1.0), b = (float)((rand() / (double)RAND_MAX) * 2.0 - 1.0);
        X[k] = mkc(a, (k == 0 || k == N / 2) ? 0.f : b);
        re[k] = (double)X[k].x;
        im[k] = (double)X[k].y;
        re[(N - k) % N] = re[k];
        im[(N - k) % N] = k == 0 ? 0.0 : -im[k];
    }
    ifft32_hermitian(X, z);
    double worst = 0.0, scale = 0.0;
    for (int n = 0; n < N; n++) {
        double xr = 0.0;
        for (int k = 0; k < N; k++) {
            const double a = 2.0 * M_PI * (double)(k * n % N) / N;
            xr += re[k] * cos(a) - im[k] * sin(a);
        }
        const c2 zz = z[fft_pos(N / 2, n >> 1)];
        const double got = (n & 1) ? (double)zz.y : (double)zz.x;
        worst = fmax(worst, fabs(got - xr));
        scale = fmax(scale, fabs(xr));
    }
    return worst / scale;
}

int main() {
    int failures = 0;
    const double bar = 2e-6 * log2(32.0);
    for (unsigned seed = 1; seed <= 16; seed++) {
        const double e = check_one(3000u + seed);
        const bool ok = e <= bar;
        printf("32 %.3e %s\n", e, ok ? "ok" : "FAIL");
        if (!ok) failures++;
    }
    return failures ? 1 : 0;
}

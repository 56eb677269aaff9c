// fftcc2d_fusedp.hip -- the single-kernel FFTCC2D (fftcc2d_fusedn_impl.h) for the square window sides with a prime factor
// above 5 (OC_FFTCC2D_PRIME_SIDES, host/fftcc_plan.h: factors 7, 11, 13 and 17, 19, 23, 29, 31), the thirteen radii that fell onto
// the five-kernel rocFFT pipeline until round 3 (3 - 8 x slower per POI, costing more than the ICGN refinement behind it).  The prime factors are transformed by fft_device.h dft_prime -- the
// symmetric (p_j, m_j) form of a P-point DFT, (P-1)^2 / 2 real-by-complex multiply-adds, all in registers; checked for
// every size on the host against a double-precision DFT (tests/test_fft_device_host.py) and on the GPU against the oracle
// and the rocFFT pipeline (tests/test_gpu_parity_2d.py::test_fftcc2d_every_fused_shape).
#include "fftcc2d_fusedn_impl.h"
#include "host/fftcc_plan.h"

namespace ochip {

using fusedn::launch_n;

hipError_t launch_fftcc2d_fusedp(const Fftcc2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (ochip_host::fftcc2d_kernel(p.rx, p.ry, 1) != ochip_host::Fftcc2dKernel::Prime) return hipErrorInvalidValue;
    switch (2 * p.rx) {
#define OC_PRIME_CASE(NN) \
    case NN: return launch_n<NN, NN>(p, pois, stride_f, count, xcd, stream);
        OC_FFTCC2D_PRIME_SIDES(OC_PRIME_CASE)
#undef OC_PRIME_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ochip

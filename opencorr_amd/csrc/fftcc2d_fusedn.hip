// fftcc2d_fusedn.hip -- single-kernel FFTCC2D for square windows whose side N = 2 * radius is not 32: every even side
// from 8 to 64, i.e. every radius from 4 to 32 (N = 32 has its own kernel in fftcc2d_fused.hip).  The 5-smooth sides are
// instantiated here (OC_FFTCC2D_SMOOTH_SIDES, host/fftcc_plan.h: the list, and the rule that sends a window here), the sides with a
// prime factor of 7 ... 31 (round 4: fft_device.h dft_prime) in fftcc2d_fusedp.hip, rectangular windows (rx != ry) in
// fftcc2d_fusedr.hip -- all from the same template (fftcc2d_fusedn_impl.h).
//
// Same plan as the 32 x 32 kernel (fftcc2d_fused32x2_kernel): the whole FFTCC2D::compute(POI2D*) (src/oc_fftcc.cpp:177-275)
// on chip -- z = ref + i*tar, ONE complex NR x NC FFT, R(k) = (Z(k) + conj Z(-k))/2, T(k) = (Z(k) - conj Z(-k))/(2i),
// C = conj(R) T, inverse FFT (unnormalised like FFTW's c2r), arg-max with the first-max rule.
// A lane owns a whole column, then a whole line: lane l gathers column l of the transform's array into its registers and
// transforms it there with an N-point mixed-radix FFT (fft_device.h: factors 2, 3, 4, 5, twiddles from a generated
// table); an NR x (NC + 1) tile of floats in LDS (odd pitch: lines and columns both conflict-free; real parts travel
// first, imaginary parts second) carries the data between the passes.  Windows whose longer side fits 32 lanes share a
// wave in pairs.  The rocFFT pipeline this replaces spends more time on these windows than the ICGN refinement that
// follows it (config C, r = 20: 4.9 ms of FFTCC against 4.2 ms of ICGN2D2 for 99 856 POIs).
#include "fftcc2d_fusedn_impl.h"
#include "host/fftcc_plan.h"

namespace ochip {

using fusedn::launch_n;

hipError_t launch_fftcc2d_fusedn(const Fftcc2dParams& p, float* pois, int stride_f, size_t count, bool xcd,
                                 hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (ochip_host::fftcc2d_kernel(p.rx, p.ry, 2) != ochip_host::Fftcc2dKernel::Smooth) return hipErrorInvalidValue;  // (2: 32 x 32 is ours too)
    switch (2 * p.rx) {
#define OC_SMOOTH_CASE(NN) \
    case NN: return launch_n<NN, NN>(p, pois, stride_f, count, xcd, stream);
        OC_FFTCC2D_SMOOTH_SIDES(OC_SMOOTH_CASE)
#undef OC_SMOOTH_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ochip

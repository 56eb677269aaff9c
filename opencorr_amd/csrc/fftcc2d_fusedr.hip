// fftcc2d_fusedr.hip -- the single-kernel FFTCC2D (fftcc2d_fusedn_impl.h) for RECTANGULAR windows, rx != ry, with both
// sides out of OC_FFTCC2D_PAIR_SIDES (host/fftcc_plan.h: seven sides, 42 instances of the register-FFT kernel).
// Other rectangular shapes take the run-time-sides kernel (fftcc2d_rect.hip) or the rocFFT pipeline (fftcc2d.hip).  What is transformed is the reference's own re-cut of
// the window buffer (FFTW planned with (width, height) over data filled [row * width + col], src/oc_fftcc.cpp:40-42,
// 204-221): 2 * rx lines of 2 * ry elements -- see the kernel.
#include "fftcc2d_fusedn_impl.h"
#include "host/fftcc_plan.h"

namespace ochip {

using fusedn::launch_n;

namespace {

// one line of the pair table: NR = 2rx is fixed, NC = 2ry runs over the list; the diagonal (the square kernels of
// fftcc2d_fusedn.hip / fftcc2d_fused.hip) is not instantiated here
template <int NR, int NC>
hipError_t launch_pair(const Fftcc2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    if constexpr (NR != NC) return launch_n<NR, NC>(p, pois, stride_f, count, xcd, stream);
    else return hipErrorInvalidValue;
}

template <int NR>
hipError_t launch_pair_line(const Fftcc2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    switch (2 * p.ry) {
#define OC_PAIR_CASE(NC) \
    case NC: return launch_pair<NR, NC>(p, pois, stride_f, count, xcd, stream);
        OC_FFTCC2D_PAIR_SIDES(OC_PAIR_CASE)
#undef OC_PAIR_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_fftcc2d_fusedr(const Fftcc2dParams& p, float* pois, int stride_f, size_t count, bool xcd, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (ochip_host::fftcc2d_kernel(p.rx, p.ry, 1) != ochip_host::Fftcc2dKernel::Pair) return hipErrorInvalidValue;
    switch (2 * p.rx) {
#define OC_PAIR_LINE(NR) \
    case NR: return launch_pair_line<NR>(p, pois, stride_f, count, xcd, stream);
        OC_FFTCC2D_PAIR_SIDES(OC_PAIR_LINE)
#undef OC_PAIR_LINE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ochip

// fftcc3d_planes.hip -- the plane-wise single-kernel FFTCC3D (fftcc3d_planes_impl.h) for cubic windows of side 28 ... 64
// except 32: the dispatcher and the instances up to side 46 (OC_FFTCC3D_PLANES_SIDES, host/fftcc_plan.h); sides 48 ... 64
// (OC_FFTCC3D_PLANESB_SIDES, among them the 60^3 windows of the reference's DVC example) are instantiated in fftcc3d_planesb.hip.
#include "fftcc3d_planes_impl.h"
#include "host/fftcc_plan.h"

namespace ochip {

using planes::launch_planes;

hipError_t launch_fftcc3d_planes_b(const Fftcc3dParams& p, float* pois, int stride_f, size_t count, void* scratch, int blocks,
                                   hipStream_t stream);  // fftcc3d_planesb.hip

hipError_t launch_fftcc3d_planes(const Fftcc3dParams& p, float* pois, int stride_f, size_t count, void* scratch, int blocks,
                                 hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (ochip_host::fftcc3d_kernel(p.rx, p.ry, p.rz, 1, false) != ochip_host::Fftcc3dKernel::Planes || !scratch || blocks < 8 || (blocks & 7))
        return hipErrorInvalidValue;
    switch (2 * p.rx) {
#define OC_PLANES_CASE(NN) \
    case NN: return launch_planes<NN>(p, pois, stride_f, count, scratch, blocks, stream);
        OC_FFTCC3D_PLANES_SIDES(OC_PLANES_CASE)
#undef OC_PLANES_CASE
        default: return launch_fftcc3d_planes_b(p, pois, stride_f, count, scratch, blocks, stream);
    }
}

}  // namespace ochip

// fftcc_plan.h -- which kernel serves an FFTCC window, without the engine: the lists of window sides the single-kernel templates
// are instantiated for, the limits of the kernels that take their sides at run time, and the rule that maps the radii and the
// "fftcc2d_fused" / "fftcc3d_fused" tuning value to one kernel -- or to the rocFFT pipeline.  run_fftcc2d / run_fftcc3d (capi.hip)
// switch on the answer, the dispatchers generate their switches from the lists and the launchers refuse what the plan gives to
// another kernel.  Standard headers only (tests/cpp/fftcc_plan_check.cpp runs the rules on a CPU; tests/fftcc_plan_model.py
// restates them as ranges and arithmetic).
#pragma once
#include <cstddef>

// Window sides (2 * radius) with an instantiation of a kernel template, once.
// fftcc2d_fusedn.hip, square N x N windows: the 5-smooth sides (32 serves "fftcc2d_fused" = 2 only: fftcc2d_fused.hip has 32 x 32)
#define OC_FFTCC2D_SMOOTH_SIDES(X) X(8) X(10) X(12) X(16) X(18) X(20) X(24) X(30) X(32) X(36) X(40) X(48) X(50) X(54) X(60) X(64)
// fftcc2d_fusedp.hip, square windows: the sides with a prime factor of 7 ... 31 (fft_device.h dft_prime)
#define OC_FFTCC2D_PRIME_SIDES(X) X(14) X(22) X(26) X(28) X(34) X(38) X(42) X(44) X(46) X(52) X(56) X(58) X(62)
// fftcc2d_fusedr.hip, rectangular windows: every ordered pair of two DIFFERENT sides out of these (42 kernels)
#define OC_FFTCC2D_PAIR_SIDES(X) X(16) X(20) X(24) X(32) X(40) X(48) X(64)
// fftcc3d_fusedn.hip, cubic windows whose complex volume stays in LDS
#define OC_FFTCC3D_CUBE_SIDES(X) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26)
// fftcc3d_planes.hip and fftcc3d_planesb.hip (two translation units for the build's sake), cubic windows through a scratch volume
#define OC_FFTCC3D_PLANES_SIDES(X) X(28) X(30) X(34) X(36) X(38) X(40) X(42) X(44) X(46)
#define OC_FFTCC3D_PLANESB_SIDES(X) X(48) X(50) X(52) X(54) X(56) X(58) X(60) X(62) X(64)

namespace ochip_host {

#define OC_FFTCC_SIDE_IS(N) || side == N
constexpr bool fftcc2d_smooth_side(int side) { return false OC_FFTCC2D_SMOOTH_SIDES(OC_FFTCC_SIDE_IS); }
constexpr bool fftcc2d_prime_side(int side) { return false OC_FFTCC2D_PRIME_SIDES(OC_FFTCC_SIDE_IS); }
constexpr bool fftcc2d_pair_side(int side) { return false OC_FFTCC2D_PAIR_SIDES(OC_FFTCC_SIDE_IS); }
constexpr bool fftcc3d_cube_side(int side) { return false OC_FFTCC3D_CUBE_SIDES(OC_FFTCC_SIDE_IS); }
constexpr bool fftcc3d_planes_a_side(int side) { return false OC_FFTCC3D_PLANES_SIDES(OC_FFTCC_SIDE_IS); }
constexpr bool fftcc3d_planes_b_side(int side) { return false OC_FFTCC3D_PLANESB_SIDES(OC_FFTCC_SIDE_IS); }
#undef OC_FFTCC_SIDE_IS

constexpr int kFftccWave = 64;
constexpr size_t kFftccMaxLaunch = 1u << 30;     // windows per launch of a one-workgroup-per-window kernel (grid.x < 2^31): longer queues take several
constexpr int kFftcc2dFusedSide = 32, kFftcc3dFusedSide = 32;   // fftcc2d_fused.hip: 32 x 32; fftcc3d_fused.hip (A/B build: and fftcc3d_fused_r5.hip): 32^3
constexpr int kFftcc2dRectMinRadius = 4, kFftcc2dRectMaxRadius = 32;   // fftcc2d_rect.hip: both radii, run-time sides
constexpr int kFftcc3dBoxMinRadius = 4, kFftcc3dBoxMaxSide = 32;   // fftcc3d_box.hip: every radius from 4 to kFftcc3dBoxMaxSide / 2
constexpr int kFftcc3dBoxMaxWaves = kFftcc3dBoxMaxSide * kFftcc3dBoxMaxSide / kFftccWave;
constexpr size_t kFftcc3dBoxLdsLimit = 160 * 1024;
constexpr int kFftcc3dPlanesBlocks = 256;        // persistent workgroups of the plane-wise kernel unless "fftcc3d_planes_blocks" says otherwise
constexpr size_t kFftcc2dRocfftChunk = 32768;    // POIs per batch of the rocFFT pipeline
constexpr size_t kFftcc3dRocfftChunk = 1024;

// fftcc2d_rect.hip has three instantiations, because a kernel's register allocation is that of its longest line: the longer
// side of the window at most 32, 48 or 64
constexpr int fftcc2d_rect_maxn(int rx, int ry) {
    const int side = 2 * (rx > ry ? rx : ry);
    return side <= 32 ? 32 : side <= 48 ? 48 : 64;
}
// dynamic LDS of the box kernel: the complex volume [2rx][2ry][2rz + 1], six index tables and the reduction slots of its waves
constexpr size_t fftcc3d_box_lds_bytes(int rx, int ry, int rz) {
    const size_t nx = 2 * (size_t)rx, ny = 2 * (size_t)ry, nz = 2 * (size_t)rz;
    return nx * ny * (nz + 1) * 2 * sizeof(float) + 6 * kFftcc3dBoxMaxSide * sizeof(int) + 2 * kFftcc3dBoxMaxWaves * sizeof(float) +
           kFftcc3dBoxMaxWaves * sizeof(int);
}
constexpr bool fftcc3d_box_radius(int r) { return r >= kFftcc3dBoxMinRadius && 2 * r <= kFftcc3dBoxMaxSide; }
// the plane-wise kernel: persistent workgroups in multiples of 8 (one share per XCD), no more than the queue can occupy ...
constexpr int fftcc3d_planes_blocks(int tuned, size_t count) {
    const size_t blocks = ((size_t)(tuned > 0 ? tuned : kFftcc3dPlanesBlocks) + 7) / 8 * 8, queue = (count + 7) / 8 * 8;
    return (int)(blocks > queue ? queue : blocks);
}
// ... each with a private complex N^3 scratch volume
constexpr size_t fftcc3d_planes_scratch_bytes(int radius, int blocks) {
    const size_t n = (size_t)(2 * radius);
    return n * n * n * 8u * (size_t)blocks;
}
// the rocFFT pipeline, per POI: floats of one window and complex bins of its half spectrum (rz = 0: FFTCC2D).  The reference
// plans FFTW with n0 = 2rx slowest and the last dimension fastest (capi.hip ensure_fft), so the halved dimension is 2ry in 2D
// and 2rz in 3D.
constexpr size_t fftcc_rocfft_window_floats(int rx, int ry, int rz) { return (size_t)(2 * rx) * (size_t)(2 * ry) * (size_t)(rz ? 2 * rz : 1); }
constexpr size_t fftcc_rocfft_bins(int rx, int ry, int rz) {
    return rz ? (size_t)(2 * rx) * (size_t)(2 * ry) * (size_t)(rz + 1) : (size_t)(2 * rx) * (size_t)(ry + 1);
}

// ---- the decision ----------------------------------------------------------------------------------------------------------
// fused_key = "fftcc2d_fused": 0 = the rocFFT pipeline for every window; 2 = the generic N x N kernel also for 32 x 32 (an A/B
// switch); 3, 4, 5 = bodies of the 32 x 32 kernel (launch_fftcc2d_fused picks them), here like 1 and every other value.
enum class Fftcc2dKernel { Fused32, Smooth, Prime, Pair, Rect, RocFft };
constexpr Fftcc2dKernel fftcc2d_kernel(int rx, int ry, int fused_key) {
    if (fused_key == 0) return Fftcc2dKernel::RocFft;
    if (rx == ry) {
        if (2 * rx == kFftcc2dFusedSide && fused_key != 2) return Fftcc2dKernel::Fused32;
        return fftcc2d_smooth_side(2 * rx) ? Fftcc2dKernel::Smooth : fftcc2d_prime_side(2 * rx) ? Fftcc2dKernel::Prime : Fftcc2dKernel::RocFft;
    }
    if (rx < kFftcc2dRectMinRadius || rx > kFftcc2dRectMaxRadius || ry < kFftcc2dRectMinRadius || ry > kFftcc2dRectMaxRadius)
        return Fftcc2dKernel::RocFft;
    return fftcc2d_pair_side(2 * rx) && fftcc2d_pair_side(2 * ry) ? Fftcc2dKernel::Pair : Fftcc2dKernel::Rect;
}

// fused_key = "fftcc3d_fused": 0 = the rocFFT pipeline; 2 = the round-5 decomposition of the 32^3 kernel where the library has it
// (ab_build: -DOC_BUILD_AB=1), else like 1 and every other value.
enum class Fftcc3dKernel { Fused32, Fused32R5, Cube, Planes, Box, RocFft };
constexpr Fftcc3dKernel fftcc3d_kernel(int rx, int ry, int rz, int fused_key, bool ab_build) {
    if (fused_key == 0) return Fftcc3dKernel::RocFft;
    if (rx == ry && ry == rz) {
        if (2 * rx == kFftcc3dFusedSide) return ab_build && fused_key == 2 ? Fftcc3dKernel::Fused32R5 : Fftcc3dKernel::Fused32;
        if (fftcc3d_cube_side(2 * rx)) return Fftcc3dKernel::Cube;
        return fftcc3d_planes_a_side(2 * rx) || fftcc3d_planes_b_side(2 * rx) ? Fftcc3dKernel::Planes : Fftcc3dKernel::RocFft;
    }
    if (!fftcc3d_box_radius(rx) || !fftcc3d_box_radius(ry) || !fftcc3d_box_radius(rz)) return Fftcc3dKernel::RocFft;
    return fftcc3d_box_lds_bytes(rx, ry, rz) <= kFftcc3dBoxLdsLimit ? Fftcc3dKernel::Box : Fftcc3dKernel::RocFft;
}

// ---- the lists partition what they claim ---------------------------------------------------------------------------------------
// every side from 0 to 129 is in exactly one of the two lists when it is even, inside [lo, hi] and not `hole`, and in none otherwise
constexpr bool fftcc_no_side(int) { return false; }
constexpr bool fftcc_lists_cover(bool (*a)(int), bool (*b)(int), int lo, int hi, int hole) {
    for (int side = 0; side < 130; side++)
        if (a(side) + b(side) != (side % 2 == 0 && side >= lo && side <= hi && side != hole)) return false;
    return true;
}
static_assert(fftcc_lists_cover(fftcc2d_smooth_side, fftcc2d_prime_side, 8, 64, -1), "every even side from 8 to 64 has exactly one generic square 2D kernel");
static_assert(fftcc2d_smooth_side(kFftcc2dFusedSide), "\"fftcc2d_fused\" = 2 needs the generic kernel at 32 x 32");
static_assert(fftcc_lists_cover(fftcc3d_cube_side, fftcc_no_side, 8, 26, -1), "fftcc3d_fusedn.hip: cubes of side 8 ... 26");
static_assert(fftcc_lists_cover(fftcc3d_planes_a_side, fftcc_no_side, 28, 46, kFftcc3dFusedSide) && fftcc_lists_cover(fftcc3d_planes_b_side, fftcc_no_side, 48, 64, -1),
              "the plane-wise kernel: cubes of side 28 ... 64 except 32; launch_fftcc3d_planes hands sides from 48 up to fftcc3d_planesb.hip");

}  // namespace ochip_host

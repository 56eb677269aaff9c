// fftcc_plan_check.cpp -- runs opencorr_amd/csrc/host/fftcc_plan.h on a CPU (tests/test_fftcc_plan_cpu.py).
//
// stdin, one request per line, stdout, one plan per line:
//   2 rx ry fused_key              ->  <kernel> <MAXN class of the rect kernel> <window floats> <spectrum bins>     (the last two: the
//   3 rx ry rz fused_key ab_build  ->  <kernel> <LDS bytes of the box kernel> <window floats> <spectrum bins>        rocFFT pipeline's)
//   p tuned_blocks count radius    ->  <workgroups of the plane-wise kernel> <bytes of their scratch volumes>
// With the argument "constants": the chunk limits of the rocFFT pipeline (2D, 3D), the launch split, the fused sides (2D, 3D).
#include <cstdio>
#include <cstring>

#include "../../opencorr_amd/csrc/host/fftcc_plan.h"

using namespace ochip_host;

static const char* name(Fftcc2dKernel k) {
    switch (k) {
        case Fftcc2dKernel::Fused32: return "fused32";
        case Fftcc2dKernel::Smooth: return "smooth";
        case Fftcc2dKernel::Prime: return "prime";
        case Fftcc2dKernel::Pair: return "pair";
        case Fftcc2dKernel::Rect: return "rect";
        case Fftcc2dKernel::RocFft: return "rocfft";
    }
    return "?";
}

static const char* name(Fftcc3dKernel k) {
    switch (k) {
        case Fftcc3dKernel::Fused32: return "fused32";
        case Fftcc3dKernel::Fused32R5: return "fused32_r5";
        case Fftcc3dKernel::Cube: return "cube";
        case Fftcc3dKernel::Planes: return "planes";
        case Fftcc3dKernel::Box: return "box";
        case Fftcc3dKernel::RocFft: return "rocfft";
    }
    return "?";
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "constants")) {
        std::printf("%zu %zu %zu %d %d\n", kFftcc2dRocfftChunk, kFftcc3dRocfftChunk, kFftccMaxLaunch, kFftcc2dFusedSide, kFftcc3dFusedSide);
        return 0;
    }
    char kind[2];
    while (std::scanf("%1s", kind) == 1) {
        int rx, ry, rz, key, ab, tuned, radius;
        unsigned long long count;
        if (kind[0] == '2' && std::scanf("%d %d %d", &rx, &ry, &key) == 3) {
            std::printf("%s %d %zu %zu\n", name(fftcc2d_kernel(rx, ry, key)), fftcc2d_rect_maxn(rx, ry), fftcc_rocfft_window_floats(rx, ry, 0),
                        fftcc_rocfft_bins(rx, ry, 0));
        } else if (kind[0] == '3' && std::scanf("%d %d %d %d %d", &rx, &ry, &rz, &key, &ab) == 5) {
            std::printf("%s %zu %zu %zu\n", name(fftcc3d_kernel(rx, ry, rz, key, ab != 0)), fftcc3d_box_lds_bytes(rx, ry, rz),
                        fftcc_rocfft_window_floats(rx, ry, rz), fftcc_rocfft_bins(rx, ry, rz));
        } else if (kind[0] == 'p' && std::scanf("%d %llu %d", &tuned, &count, &radius) == 3) {
            const int blocks = fftcc3d_planes_blocks(tuned, (size_t)count);
            std::printf("%d %zu\n", blocks, fftcc3d_planes_scratch_bytes(radius, blocks));
        } else {
            std::fprintf(stderr, "malformed request line of kind '%s'\n", kind);
            return 2;
        }
    }
    return 0;
}

// sift2d_compat_main.cpp -- a caller of opencorr::SIFT2DScaleSpace written the way SIFT2D::compute runs its detector
// (src/oc_sift.cpp:60-93): an Image2D in, the reference's Sift2dConfig, the located keypoints out.
// tests/test_sift2d_compat_compile.py compiles and links it; without arguments it exits with 2 before touching the GPU.
//   argv: <raw float32 image file, row-major> width height
//   ->    "octaves <n> keypoints <n>", then one "kp <x bits> <y bits> <size bits> <response bits> octave layer row col <packed>" each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "opencorr_compat/opencorr.h"

using namespace opencorr;

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <raw float32 image> width height\n", argv[0]);
        return 2;
    }
    const int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
    try {
        std::vector<float> pixels((size_t)width * height);
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f || std::fread(pixels.data(), sizeof(float), pixels.size(), f) != pixels.size()) {
            std::fprintf(stderr, "cannot read %zu floats from %s\n", pixels.size(), argv[1]);
            return 2;
        }
        std::fclose(f);
        Image2D img(width, height);
        img.fromRowMajor(pixels.data());

        SIFT2DScaleSpace sift;
        Sift2dConfig sift_config = sift.getSiftConfig();
        sift_config.n_features = 0;
        sift_config.n_octave_layers = 3;
        sift_config.contrast_threshold = 0.04f;
        sift_config.edge_threshold = 10.f;
        sift_config.sigma = 1.6f;
        sift.setSiftConfig(sift_config);
        sift.compute(&img);
        std::vector<Keypoint2D> kp_queue;
        sift.detect(kp_queue);

        std::printf("octaves %d keypoints %zu\n", sift.getOctaveNumber(), kp_queue.size());
        for (const Keypoint2D& kp : kp_queue)
            std::printf("kp %08x %08x %08x %08x %d %d %d %d %d\n", bits(kp.pt.x), bits(kp.pt.y), bits(kp.size), bits(kp.response), kp.octave, kp.layer, kp.row,
                        kp.col, kp.packed_octave);
        return 0;
    } catch (std::string& message) {
        std::fprintf(stderr, "%s\n", message.c_str());
        return 3;
    }
}

// sift3d_compat_main.cpp -- a caller of opencorr::SIFT3DScaleSpace written the way SIFT3D::compute runs its front half
// (src/oc_sift.cpp:237-250): an Image3D in, createGaussianPyramid + createDogPyramid, detectExtrema into a keypoint queue, the
// pyramids handed on as Layer3D records.  tests/test_sift3d_compat_compile.py compiles and links it; without arguments it exits
// with 2 before touching the GPU.
//   argv: <raw float32 volume file> dim_x dim_y dim_z
//   ->    "octaves <n> gauss <n> dog <n>", "maxabs <bits> ..." (DoG layers), one "kp x y z octave layer <scale bits>" per candidate,
//         "sum <pyramid> <layer> <sum of the voxels' bit patterns>" per layer
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
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <raw float32 volume> dim_x dim_y dim_z\n", argv[0]);
        return 2;
    }
    const int dim_x = std::atoi(argv[2]), dim_y = std::atoi(argv[3]), dim_z = std::atoi(argv[4]);
    try {
        Image3D vol_img(dim_x, dim_y, dim_z);
        std::FILE* f = std::fopen(argv[1], "rb");
        const size_t count = (size_t)dim_x * dim_y * dim_z;
        if (!f || std::fread(&vol_img.vol_mat[0][0][0], sizeof(float), count, f) != count) {
            std::fprintf(stderr, "cannot read %zu floats from %s\n", count, argv[1]);
            return 2;
        }
        std::fclose(f);

        SIFT3DScaleSpace sift;
        Sift3dConfig sift_config = sift.getSiftConfig();
        sift_config.n_octave_layers = 3;
        sift.setSiftConfig(sift_config);
        sift.setPhysicalUnit(1.f, 1.f, 1.f);
        sift.compute(&vol_img);
        std::vector<Layer3D> gaussian_pyramid, dog_pyramid;
        std::vector<Keypoint3D> kp_queue;
        sift.detectExtrema(kp_queue);
        sift.downloadPyramid(0, gaussian_pyramid);
        sift.downloadPyramid(1, dog_pyramid);

        std::printf("octaves %d gauss %zu dog %zu\nmaxabs", sift.getSiftConfig().n_octave, gaussian_pyramid.size(), dog_pyramid.size());
        for (const Layer3D& layer : dog_pyramid) std::printf(" %08x", bits(layer.max_abs));
        std::printf("\n");
        for (const Keypoint3D& kp : kp_queue)
            std::printf("kp %d %d %d %d %d %08x\n", (int)kp.coor_layer.x, (int)kp.coor_layer.y, (int)kp.coor_layer.z, kp.octave, kp.layer, bits(kp.scale));
        for (int pyramid = 0; pyramid < 2; pyramid++) {
            const std::vector<Layer3D>& layers = pyramid == 0 ? gaussian_pyramid : dog_pyramid;
            for (size_t n = 0; n < layers.size(); n++) {
                unsigned long long sum = 0;
                for (int i = 0; i < layers[n].dim_xyz[2]; i++)
                    for (int j = 0; j < layers[n].dim_xyz[1]; j++)
                        for (int k = 0; k < layers[n].dim_xyz[0]; k++) sum += bits(layers[n].vol_mat[i][j][k]);
                std::printf("sum %d %zu %llu\n", pyramid, n, sum);
            }
        }
        return 0;
    } catch (std::string& message) {
        std::fprintf(stderr, "%s\n", message.c_str());
        return 3;
    }
}

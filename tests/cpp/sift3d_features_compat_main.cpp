// sift3d_features_compat_main.cpp -- a caller of opencorr::SIFT3D written the way the reference's DVC example uses the class
// (examples/test_dvc_sift_icgn1.cpp:82-104: new SIFT3D, setImages, prepare, compute, ref_matched_kp / tar_matched_kp streamed out),
// followed by the stage-by-stage form on opencorr::SIFT3DScaleSpace (detectExtrema, assignOrientation, constructDescriptor).
// tests/test_sift3d_features_compat_compile.py compiles and links it; without arguments it exits with 2 before touching the GPU.
//   argv: <raw float32 ref volume> <raw float32 tar volume> dim_x dim_y dim_z
//   ->    "pairs <n>", one "pair x,y,z x,y,z" per match, "keypoints <n>", one "kp x y z octave layer <sum of the descriptor's bits>" each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "opencorr_compat/opencorr.h"

using namespace opencorr;
using std::cout;
using std::endl;

static bool read_volume(const char* path, Image3D& img) {
    std::FILE* f = std::fopen(path, "rb");
    const size_t count = (size_t)img.dim_x * img.dim_y * img.dim_z;
    const bool ok = f && std::fread(&img.vol_mat[0][0][0], sizeof(float), count, f) == count;
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <raw float32 ref volume> <raw float32 tar volume> dim_x dim_y dim_z\n", argv[0]);
        return 2;
    }
    const int dim_x = std::atoi(argv[3]), dim_y = std::atoi(argv[4]), dim_z = std::atoi(argv[5]);
    try {
        Image3D ref_img(dim_x, dim_y, dim_z), tar_img(dim_x, dim_y, dim_z);
        if (!read_volume(argv[1], ref_img) || !read_volume(argv[2], tar_img)) {
            std::fprintf(stderr, "cannot read the volumes\n");
            return 2;
        }
        const char* delimiter = " ";

        //SIFT extraction and matching
        SIFT3D* sift = new SIFT3D();
        sift->setImages(ref_img, tar_img);
        sift->prepare();
        sift->compute();

        int kp_amount = (int)sift->ref_matched_kp.size();
        cout << "pairs " << kp_amount << endl;
        for (int i = 0; i < kp_amount; i++) {
            cout << "pair " << sift->ref_matched_kp[i] << delimiter << sift->tar_matched_kp[i] << endl;
        }
        Sift3dConfig sift_config = sift->getSiftConfig();
        const float matching_ratio = sift->getMatchingRatio(), unit_x = sift->getPhysicalUnit(0);
        sift->setSiftConfig(sift_config);
        sift->setMatchingRatio(matching_ratio);
        sift->setPhysicalUnit(unit_x, sift->getPhysicalUnit(1), sift->getPhysicalUnit(2));
        sift->clear();
        delete sift;

        // the stages one by one, with host queues in between as SIFT3D::compute has them (src/oc_sift.cpp:246-255)
        SIFT3DScaleSpace stages;
        std::vector<Keypoint3D> ref_kp;
        stages.compute(&ref_img);
        stages.detectExtrema(ref_kp);
        stages.assignOrientation(ref_kp);
        int ref_amount = (int)ref_kp.size();
        std::vector<float> block((size_t)ref_amount * 768);
        std::vector<float*> ref_descriptor((size_t)ref_amount);
        for (int i = 0; i < ref_amount; i++) ref_descriptor[(size_t)i] = block.data() + (size_t)i * 768;
        stages.constructDescriptor(ref_kp, ref_descriptor.data());
        cout << "keypoints " << ref_amount << endl;
        for (int i = 0; i < ref_amount; i++) {
            unsigned long long sum = 0;
            for (int t = 0; t < 768; t++) {
                unsigned u;
                std::memcpy(&u, &ref_descriptor[(size_t)i][t], sizeof u);
                sum += u;
            }
            const Keypoint3D& kp = ref_kp[(size_t)i];
            cout << "kp " << (int)kp.coor_img.x << " " << (int)kp.coor_img.y << " " << (int)kp.coor_img.z << " " << kp.octave << " " << kp.layer << " " << sum << endl;
        }
        return 0;
    } catch (std::string& message) {
        std::fprintf(stderr, "%s\n", message.c_str());
        return 3;
    }
}

// feature_affine_compat_main.cpp -- a caller of opencorr::FeatureAffine2D / FeatureAffine3D written the way the reference's
// examples use them (examples/test_dvc_sift_icgn1.cpp:113-117, examples/test_2d_dic_self_adaptive_subset.cpp): keypoint pairs in,
// prepare, compute(poi_queue), compute(POI*).  tests/test_feature_affine_compat_compile.py compiles and links it; without
// arguments it exits with 2 before touching the GPU.
//   argv: <ndim> <raw float32 file: count, then ref pairs, then tar pairs> <seed>
//   ->    one line "poi <i> <bits of every float of the record>" per POI of a fixed 3 x 3 (x 3) queue, the last POI computed
//         through compute(POI*), then (2D) the same queue in self-adaptive mode
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "opencorr_compat/opencorr.h"

using namespace opencorr;

template <class Poi>
static void print_queue(const char* tag, const std::vector<Poi>& queue) {
    for (size_t i = 0; i < queue.size(); i++) {
        std::printf("%s %zu", tag, i);
        unsigned words[sizeof(Poi) / 4];
        std::memcpy(words, &queue[i], sizeof(Poi));
        for (unsigned w : words) std::printf(" %08x", w);
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <ndim> <keypoint file> <seed>\n", argv[0]);
        return 2;
    }
    const int ndim = std::atoi(argv[1]);
    const unsigned long long seed = std::strtoull(argv[3], nullptr, 10);
    try {
        std::FILE* f = std::fopen(argv[2], "rb");
        float count_f = 0.f;
        if (!f || std::fread(&count_f, sizeof(float), 1, f) != 1) return 2;
        const size_t count = (size_t)count_f;
        std::vector<float> ref(count * ndim), tar(count * ndim);
        if (std::fread(ref.data(), sizeof(float), ref.size(), f) != ref.size() || std::fread(tar.data(), sizeof(float), tar.size(), f) != tar.size()) return 2;
        std::fclose(f);
        if (ndim == 3) {
            std::vector<Point3D> ref_kp, tar_kp;
            for (size_t i = 0; i < count; i++) {
                ref_kp.push_back(Point3D(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]));
                tar_kp.push_back(Point3D(tar[3 * i], tar[3 * i + 1], tar[3 * i + 2]));
            }
            std::vector<POI3D> queue;
            for (int z = 0; z < 3; z++)
                for (int y = 0; y < 3; y++)
                    for (int x = 0; x < 3; x++) queue.push_back(POI3D(15 + 15 * x, 15 + 15 * y, 15 + 15 * z));
            FeatureAffine3D* feature_affine = new FeatureAffine3D(8, 8, 8, 4);
            feature_affine->setSeed(seed);
            RansacConfig config = feature_affine->getRansacConfig();
            config.trial_number = 24;
            feature_affine->setRansacConfig(config);
            feature_affine->setSearch(feature_affine->getSearchRadius(), feature_affine->getNeighborMin());
            feature_affine->setKeypointPair(ref_kp, tar_kp);
            feature_affine->prepare();
            POI3D last = queue.back();
            feature_affine->compute(queue);
            feature_affine->compute(&last);
            queue.back() = last;
            print_queue("poi", queue);
            delete feature_affine;
        } else {
            std::vector<Point2D> ref_kp, tar_kp;
            for (size_t i = 0; i < count; i++) {
                ref_kp.push_back(Point2D(ref[2 * i], ref[2 * i + 1]));
                tar_kp.push_back(Point2D(tar[2 * i], tar[2 * i + 1]));
            }
            std::vector<POI2D> queue;
            for (int y = 0; y < 3; y++)
                for (int x = 0; x < 3; x++) queue.push_back(POI2D(40 + 60 * x, 40 + 60 * y));
            std::vector<POI2D> adaptive_queue(queue);
            FeatureAffine2D* feature_affine = new FeatureAffine2D(16, 16, 4);
            feature_affine->setSeed(seed);
            feature_affine->setKeypointPair(ref_kp, tar_kp);
            feature_affine->prepare();
            POI2D last = queue.back();
            feature_affine->compute(queue);
            feature_affine->compute(&last);
            queue.back() = last;
            print_queue("poi", queue);
            Image2D ref_img(200, 200), tar_img(200, 200);
            feature_affine->setImages(ref_img, tar_img);
            feature_affine->setSelfAdaptive(true);
            feature_affine->setSubsetAdjustment(14, 10);
            feature_affine->compute(adaptive_queue);
            print_queue("adaptive", adaptive_queue);
            delete feature_affine;
        }
    } catch (const std::string& what) {
        std::fprintf(stderr, "error: %s\n", what.c_str());
        return 1;
    }
    return 0;
}

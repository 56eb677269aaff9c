// match_compat_main.cpp -- a caller of opencorr::DescriptorMatcher3D written the way SIFT3D::compute calls its matching stage
// (src/oc_sift.cpp:282-288): descriptors as float** rows, keypoint coordinates in, matched coordinate queues out -- the
// arguments FeatureAffine3D::setKeypointPair takes.  tests/test_match_compat_compile.py compiles and links it; without an
// argument it exits with 2 before touching the GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "opencorr_compat/opencorr.h"

using namespace opencorr;

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <keypoints>\n", argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[1]), dim = 768;
    try {
        std::vector<std::vector<float>> rows1(n, std::vector<float>(dim, 0.f)), rows2(n, std::vector<float>(dim, 0.f));
        std::vector<float*> descriptor1(n), descriptor2(n);
        std::vector<Point3D> kp1, kp2;
        for (int i = 0; i < n; i++) {
            rows1[i][i % dim] = 1.f;
            rows2[n - 1 - i][i % dim] = 0.875f;
            descriptor1[i] = rows1[i].data();
            descriptor2[i] = rows2[i].data();
            kp1.push_back(Point3D(i, 2 * i, 3 * i));
            kp2.push_back(Point3D(n - 1 - i, 0, 0));
        }
        DescriptorMatcher3D matcher(dim);
        matcher.setMatchingRatio(0.85f);
        matcher.setDescriptors(0, descriptor1.data(), n);
        matcher.setDescriptors(1, rows2[0].data(), 1);  // (the contiguous-block overload)
        matcher.setDescriptors(1, descriptor2.data(), n);
        std::vector<int> matched_idx(n);
        const int matched = matcher.bruteforceMatch(0, matched_idx.data());
        std::vector<Point3D> ref_matched_kp, tar_matched_kp, ref_bi, tar_bi;
        matcher.monodirectionalMatch(kp1, kp2, ref_matched_kp, tar_matched_kp);
        matcher.bidirectionalMatch(kp1, kp2, ref_bi, tar_bi);
        std::printf("%d %zu %zu\n", matched, ref_matched_kp.size(), ref_bi.size());
        for (size_t i = 0; i < ref_matched_kp.size(); i++)
            if (ref_matched_kp[i].x != tar_matched_kp[i].x) return 1;
        return matched == n && (int)ref_matched_kp.size() == n && (int)tar_bi.size() == n ? 0 : 1;
    } catch (std::string& message) {
        std::fprintf(stderr, "%s\n", message.c_str());
        return 3;
    }
}

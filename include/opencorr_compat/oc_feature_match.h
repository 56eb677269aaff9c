// oc_feature_match.h -- the matching stage of the reference's SIFT3D over the HIP C-ABI: bruteforceMatch, monodirectionalMatch
// and bidirectionalMatch (src/oc_sift.cpp:625-674, 1251-1418, 1420-1487) for descriptors computed anywhere.
//
//   DescriptorMatcher3D   setDescriptors(side, rows, count) takes the reference's float** rows (gathered into one block) or a
//                         contiguous block; bruteforceMatch(direction, matched_idx) returns the match count like the reference's;
//                         monodirectionalMatch / bidirectionalMatch take the keypoint coordinates of both sides and fill
//                         matched_kp1 / matched_kp2 -- exactly what FeatureAffine3D::setKeypointPair takes.
//
// Differences a caller can observe ("Descriptor matching"): every entry of matched_idx is written (-1 where the
// ratio test fails); the last many-to-one group is closed by the end of the list, not by the element behind it; all matches are
// processed when every reference keypoint passed the ratio test.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "../opencorr_hip.h"
#include "oc_engines.h"
#include "oc_types.h"

namespace opencorr {

class DescriptorMatcher3D {
public:
    // descriptor_length: 768 for the reference's SIFT3D (a multiple of 32 in [32, 1024]); matching_ratio: SIFT3D's default 0.85
    // (src/oc_sift.cpp:154)
    explicit DescriptorMatcher3D(int descriptor_length = 768, float matching_ratio = 0.85f) : dim_(descriptor_length), ratio_(matching_ratio) {
        hipdetail::check(oc_hip_matcher_create(dim_, ratio_, hipdetail::default_device(), &engine_));
        const char* fma = std::getenv("OC_HIP_ARITH_FMA");
        if (fma && std::atoi(fma) != 0) hipdetail::check(oc_hip_set_tuning(engine_, "arith_fma", 1));
    }
    ~DescriptorMatcher3D() { (void)oc_hip_destroy(engine_); }
    DescriptorMatcher3D(const DescriptorMatcher3D&) = delete;
    DescriptorMatcher3D& operator=(const DescriptorMatcher3D&) = delete;

    float getMatchingRatio() const { return ratio_; }
    void setMatchingRatio(float matching_ratio) {  // src/oc_sift.cpp:204-207
        hipdetail::check(oc_hip_matcher_set_ratio(engine_, matching_ratio));
        ratio_ = matching_ratio;
    }

    // side 0 = reference keypoints, 1 = target keypoints; rows[i] = the descriptor of keypoint i (the reference's float**)
    void setDescriptors(int side, const float* const* rows, int count) {
        std::vector<float> block((size_t)(count > 0 ? count : 0) * dim_);
        for (int i = 0; i < count; i++) std::memcpy(block.data() + (size_t)i * dim_, rows[i], sizeof(float) * dim_);
        setDescriptors(side, block.data(), count);
    }
    // the same as one contiguous block [count][descriptor_length]
    void setDescriptors(int side, const float* block, int count) {
        if (side != 0 && side != 1) throw std::string("DescriptorMatcher3D: side must be 0 (reference) or 1 (target)");
        if (count < 0) throw std::string("DescriptorMatcher3D: negative keypoint count");
        hipdetail::check(oc_hip_matcher_set_descriptors(engine_, side, block, (size_t)count, OC_HIP_HOST));
        count_[side] = count;
    }

    // a block that is already on the device (16-byte aligned; oc_hip_sift3d_describe writes such blocks): used in place, so it
    // must stay valid until the side is set again
    void setDeviceDescriptors(int side, const float* device_block, int count) {
        if (side != 0 && side != 1) throw std::string("DescriptorMatcher3D: side must be 0 (reference) or 1 (target)");
        if (count < 0) throw std::string("DescriptorMatcher3D: negative keypoint count");
        hipdetail::check(oc_hip_matcher_set_descriptors(engine_, side, device_block, (size_t)count, OC_HIP_DEVICE));
        count_[side] = count;
    }

    // SIFT3D::bruteforceMatch (:625-674); direction 0: reference -> target (matched_idx has one entry per reference keypoint),
    // 1: target -> reference.  Returns the number of matches.
    int bruteforceMatch(int direction, int* matched_idx) {
        size_t n = 0;
        hipdetail::check(oc_hip_matcher_nearest(engine_, direction, matched_idx, nullptr, nullptr, &n, OC_HIP_HOST));
        return (int)n;
    }

    // SIFT3D::monodirectionalMatch (:1251-1418); kp1 / kp2: the image coordinates of the keypoints whose descriptors were set as
    // side 0 / side 1 (Keypoint3D::coor_img)
    void monodirectionalMatch(const std::vector<Point3D>& kp1, const std::vector<Point3D>& kp2, std::vector<Point3D>& matched_kp1,
                              std::vector<Point3D>& matched_kp2) {
        match(0, kp1, kp2, matched_kp1, matched_kp2);
    }
    // SIFT3D::bidirectionalMatch (:1420-1487)
    void bidirectionalMatch(const std::vector<Point3D>& kp1, const std::vector<Point3D>& kp2, std::vector<Point3D>& matched_kp1,
                            std::vector<Point3D>& matched_kp2) {
        match(1, kp1, kp2, matched_kp1, matched_kp2);
    }

    oc_hip_engine* handle() const { return engine_; }

private:
    void match(int mode, const std::vector<Point3D>& kp1, const std::vector<Point3D>& kp2, std::vector<Point3D>& matched_kp1,
               std::vector<Point3D>& matched_kp2) {
        if ((int)kp1.size() != count_[0] || (int)kp2.size() != count_[1])
            throw std::string("DescriptorMatcher3D: keypoint queues and descriptor blocks differ in length");
        const size_t cap = (size_t)(count_[0] < count_[1] ? count_[0] : count_[1]);
        std::vector<int> ref(cap), tar(cap);
        size_t n = 0;
        hipdetail::check(oc_hip_matcher_match(engine_, mode, ref.data(), tar.data(), cap, &n, OC_HIP_HOST));
        for (size_t i = 0; i < n; i++) {
            matched_kp1.push_back(kp1[ref[i]]);
            matched_kp2.push_back(kp2[tar[i]]);
        }
    }

    oc_hip_engine* engine_ = nullptr;
    int dim_;
    float ratio_;
    int count_[2] = {0, 0};
};

}  // namespace opencorr

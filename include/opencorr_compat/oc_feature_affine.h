// oc_feature_affine.h -- FeatureAffine2D / FeatureAffine3D of the reference (src/oc_feature_affine.h:26-106) over the GPU engine
// of include/opencorr_hip.h ("FeatureAffine2D / FeatureAffine3D"): the keypoint-guided RANSAC affine initial guess.
//
// Same class names, constructor and method signatures and call order as the reference:
//     FeatureAffine3D* fa = new FeatureAffine3D(rx, ry, rz, thread_number);
//     fa->setKeypointPair(sift->ref_matched_kp, sift->tar_matched_kp);
//     fa->prepare();
//     fa->compute(poi_queue);
// plus setSeed: the reference seeds its generator from std::random_device and differs from run to run; this engine draws its
// samples from a counter-based generator keyed by the seed (0 unless set) and the POI's coordinates, so a run can be repeated.
// FeatureAffine2D in self-adaptive mode (setSelfAdaptive(true), setSubsetAdjustment) reads the size of the reference image
// (src/oc_feature_affine.cpp:130-133): setImages comes first, as in examples/test_2d_dic_self_adaptive_subset.cpp.
// thread_number is kept for the signature; the images themselves are never uploaded.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "../opencorr_hip.h"
#include "oc_engines.h"
#include "oc_types.h"

namespace opencorr {

// parameters in RANSAC (src/oc_feature_affine.h:26-31; the reference's spelling)
struct RansacConfig {
    int trial_number;       // maximum number of trials in RANSAC
    int sample_mumber;      // number of samples in every trial
    float error_threshold;  // error threshold in RANSAC
};

static_assert(sizeof(Point2D) == 8 && sizeof(Point3D) == 12, "keypoint vectors travel as packed floats");

class FeatureAffine2D : public DIC {
public:
    std::vector<Point2D> ref_kp;  // matched keypoints in ref image
    std::vector<Point2D> tar_kp;  // matched keypoints in tar image

    FeatureAffine2D(int radius_x, int radius_y, int thread_number_) {
        subset_radius_x = radius_x;
        subset_radius_y = radius_y;
        thread_number = thread_number_;
        hipdetail::check(oc_hip_feature_affine_create(2, radius_x, radius_y, 0, device_, &engine_));
        neighbor_search_radius = std::sqrt((float)(radius_x * radius_x + radius_y * radius_y));
    }

    RansacConfig getRansacConfig() const { return ransac_config; }
    float getSearchRadius() const { return neighbor_search_radius; }
    int getNeighborMin() const { return neighbor_number_min; }

    void setSearch(float neighbor_search_radius_, int neighbor_number_min_) {
        hipdetail::check(oc_hip_feature_affine_set_search(engine_, neighbor_search_radius_, neighbor_number_min_));
        neighbor_search_radius = neighbor_search_radius_;
        neighbor_number_min = neighbor_number_min_;
    }
    void setRansacConfig(RansacConfig config) {
        hipdetail::check(oc_hip_feature_affine_set_ransac(engine_, config.trial_number, config.sample_mumber, config.error_threshold));
        ransac_config = config;
    }
    void setSubsetAdjustment(int feature_min, int radius_min) {
        subset_feature_min = feature_min;
        subset_radius_min = radius_min;
    }
    void setSeed(unsigned long long seed) { hipdetail::check(oc_hip_feature_affine_set_seed(engine_, seed)); }

    void setKeypointPair(std::vector<Point2D>& ref_kp_, std::vector<Point2D>& tar_kp_) {
        if (ref_kp_.size() != tar_kp_.size()) throw std::string("FeatureAffine2D::setKeypointPair: the two lists differ in length");
        ref_kp = ref_kp_;
        tar_kp = tar_kp_;
    }
    void prepare() override {
        hipdetail::check(oc_hip_feature_affine_set_keypoints(engine_, reinterpret_cast<const float*>(ref_kp.data()),
                                                             reinterpret_cast<const float*>(tar_kp.data()), ref_kp.size(), OC_HIP_HOST));
        hipdetail::check(oc_hip_feature_affine_prepare(engine_));
    }
    // a queue of one (a POI's record does not depend on the queue it travels in); loops belong to compute(poi_queue)
    void compute(POI2D* poi) override { run(poi, 1); }
    void compute(std::vector<POI2D>& poi_queue) override { run(poi_queue.data(), poi_queue.size()); }

protected:
    float neighbor_search_radius;
    int neighbor_number_min = 7;
    RansacConfig ransac_config = {20, 3, 1.5f};
    int subset_feature_min = 14;
    int subset_radius_min = 10;

private:
    void run(POI2D* pois, size_t n) {
        if (self_adaptive && !ref_img) throw std::string("FeatureAffine2D: self-adaptive subsets need setImages()");
        hipdetail::check(oc_hip_feature_affine_set_self_adaptive(engine_, self_adaptive ? 1 : 0, subset_feature_min, subset_radius_min,
                                                                 self_adaptive ? ref_img->width : 0, self_adaptive ? ref_img->height : 0));
        hipdetail::check(oc_hip_feature_affine_compute(engine_, pois, n, sizeof(POI2D), OC_HIP_HOST));
    }
};

class FeatureAffine3D : public DVC {
public:
    std::vector<Point3D> ref_kp;  // matched keypoints in ref image
    std::vector<Point3D> tar_kp;  // matched keypoints in tar image

    FeatureAffine3D(int radius_x, int radius_y, int radius_z, int thread_number_) {
        subset_radius_x = radius_x;
        subset_radius_y = radius_y;
        subset_radius_z = radius_z;
        thread_number = thread_number_;
        hipdetail::check(oc_hip_feature_affine_create(3, radius_x, radius_y, radius_z, device_, &engine_));
        neighbor_search_radius = std::sqrt((float)(radius_x * radius_x + radius_y * radius_y + radius_z * radius_z));
    }

    RansacConfig getRansacConfig() const { return ransac_config; }
    float getSearchRadius() const { return neighbor_search_radius; }
    int getNeighborMin() const { return neighbor_number_min; }

    void setSearch(float neighbor_search_radius_, int neighbor_number_min_) {
        hipdetail::check(oc_hip_feature_affine_set_search(engine_, neighbor_search_radius_, neighbor_number_min_));
        neighbor_search_radius = neighbor_search_radius_;
        neighbor_number_min = neighbor_number_min_;
    }
    void setRansacConfig(RansacConfig config) {
        hipdetail::check(oc_hip_feature_affine_set_ransac(engine_, config.trial_number, config.sample_mumber, config.error_threshold));
        ransac_config = config;
    }
    void setSeed(unsigned long long seed) { hipdetail::check(oc_hip_feature_affine_set_seed(engine_, seed)); }

    void setKeypointPair(std::vector<Point3D>& ref_kp_, std::vector<Point3D>& tar_kp_) {
        if (ref_kp_.size() != tar_kp_.size()) throw std::string("FeatureAffine3D::setKeypointPair: the two lists differ in length");
        ref_kp = ref_kp_;
        tar_kp = tar_kp_;
    }
    void prepare() override {
        hipdetail::check(oc_hip_feature_affine_set_keypoints(engine_, reinterpret_cast<const float*>(ref_kp.data()),
                                                             reinterpret_cast<const float*>(tar_kp.data()), ref_kp.size(), OC_HIP_HOST));
        hipdetail::check(oc_hip_feature_affine_prepare(engine_));
    }
    void compute(POI3D* poi) override { hipdetail::check(oc_hip_feature_affine_compute(engine_, poi, 1, sizeof(POI3D), OC_HIP_HOST)); }
    void compute(std::vector<POI3D>& poi_queue) override {
        hipdetail::check(oc_hip_feature_affine_compute(engine_, poi_queue.data(), poi_queue.size(), sizeof(POI3D), OC_HIP_HOST));
    }

protected:
    float neighbor_search_radius;
    int neighbor_number_min = 16;
    RansacConfig ransac_config = {32, 4, 3.2f};
};

}  // namespace opencorr

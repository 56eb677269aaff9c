// oc_feature_detect.h -- the front half of the reference's SIFT3D::compute over the HIP C-ABI: createGaussianPyramid,
// createDogPyramid and detectExtrema (src/oc_sift.cpp:676-754, 756-793, 795-847).
//
//   SIFT3DScaleSpace   setSiftConfig / setPhysicalUnit like SIFT3D's; compute(Image3D*) builds both pyramids on the device;
//                      detectExtrema(kp_queue) appends the candidates exactly as :832-839 fills them (coor_layer, layer, octave,
//                      scale; coor_img and rotation_matrix are the later stages'); downloadPyramid(pyramid, layers) hands the
//                      layers to a CPU assignOrientation / constructDescriptor as Layer3D records with vol_mat[z][y][x].
//
// One difference a caller can observe ("SIFT3D scale space"): where a blur radius exceeds dim - 1 on an axis the
// reference's mirrored index leaves the array; here it is clamped into the axis.  Orientation, descriptors, SIFT2D and
// FeatureAffine are not part of this header.
#pragma once

#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../opencorr_hip.h"
#include "oc_engines.h"
#include "oc_types.h"

namespace opencorr {

// src/oc_sift.h:71-83
struct Sift3dConfig {
    int n_octave_layers;
    int n_octave;  // written by compute() (:683-684)
    int min_dimension;
    float alpha;
    float beta;
    float gamma;
    float sigma_source;
    float sigma_base;
    float gradient_threshold;
    float truncate_threshold;
};

// src/oc_sift.h:85-94; vol_mat points into memory the SIFT3DScaleSpace that filled the record owns
struct Layer3D {
    float*** vol_mat;
    int dim_xyz[3];
    float unit_xyz[3];
    int octave;
    float max_abs;
    float scale;
    float sigma;
};

// src/oc_sift.h:96-103
struct Keypoint3D {
    Point3D coor_layer;
    Point3D coor_img;
    int octave, layer;
    float scale;
    float rotation_matrix[9];
};

class SIFT3DScaleSpace {
public:
    SIFT3DScaleSpace() {
        // SIFT3D::SIFT3D(), src/oc_sift.cpp:142-159
        sift_config.n_octave_layers = 3;
        sift_config.n_octave = 0;
        sift_config.min_dimension = 8;
        sift_config.alpha = 0.1f;
        sift_config.beta = 0.9f;
        sift_config.gamma = 0.4f;
        sift_config.sigma_source = 1.15f;
        sift_config.sigma_base = 1.6f;
        sift_config.gradient_threshold = 0.0000000001f;
        sift_config.truncate_threshold = 0.2f * 128 / 768;
        hipdetail::check(oc_hip_sift3d_create(hipdetail::default_device(), &engine_));
        const char* fma = std::getenv("OC_HIP_ARITH_FMA");
        if (fma && std::atoi(fma) != 0) hipdetail::check(oc_hip_set_tuning(engine_, "arith_fma", 1));
    }
    ~SIFT3DScaleSpace() { (void)oc_hip_destroy(engine_); }
    SIFT3DScaleSpace(const SIFT3DScaleSpace&) = delete;
    SIFT3DScaleSpace& operator=(const SIFT3DScaleSpace&) = delete;

    Sift3dConfig getSiftConfig() const { return sift_config; }
    void setSiftConfig(Sift3dConfig config) { sift_config = config; }  // src/oc_sift.cpp:192-195
    float getPhysicalUnit(int dim) const { return dim >= 0 && dim < 3 ? physical_unit[dim] : 0.f; }
    void setPhysicalUnit(float unit_x, float unit_y, float unit_z) {  // :197-202
        physical_unit[0] = unit_x;
        physical_unit[1] = unit_y;
        physical_unit[2] = unit_z;
    }

    // createGaussianPyramid + createDogPyramid (:676-793) of vol_img; the pyramids stay on the device
    void compute(Image3D* vol_img) {
        hipdetail::check(oc_hip_sift3d_set_config(engine_, sift_config.n_octave_layers, sift_config.min_dimension, sift_config.alpha,
                                                  sift_config.sigma_source, sift_config.sigma_base));
        hipdetail::check(oc_hip_sift3d_set_physical_unit(engine_, physical_unit[0], physical_unit[1], physical_unit[2]));
        hipdetail::check(oc_hip_sift3d_set_volume(engine_, &vol_img->vol_mat[0][0][0], vol_img->dim_x, vol_img->dim_y, vol_img->dim_z, OC_HIP_HOST));
        hipdetail::check(oc_hip_sift3d_build(engine_));
        int n_layers = 0;
        hipdetail::check(oc_hip_sift3d_layer_count(engine_, 0, &n_layers, &sift_config.n_octave));
    }

    // detectExtrema (:795-847): appends to kp_queue like the reference's push_back
    void detectExtrema(std::vector<Keypoint3D>& kp_queue) {
        size_t n = 0;
        const int rc = oc_hip_sift3d_detect(engine_, nullptr, 0, &n, OC_HIP_HOST);
        if (rc != OC_HIP_OK && n == 0) hipdetail::check(rc);
        std::vector<oc_hip_sift3d_candidate> list(n);
        if (n > 0) hipdetail::check(oc_hip_sift3d_detect(engine_, list.data(), n, &n, OC_HIP_HOST));
        for (size_t i = 0; i < n; i++) {
            Keypoint3D keypoint_candidate{};
            keypoint_candidate.coor_layer.x = (float)list[i].x;  // :833-839
            keypoint_candidate.coor_layer.y = (float)list[i].y;
            keypoint_candidate.coor_layer.z = (float)list[i].z;
            keypoint_candidate.layer = list[i].layer;
            keypoint_candidate.octave = list[i].octave;
            keypoint_candidate.scale = list[i].scale;
            kp_queue.push_back(keypoint_candidate);
        }
    }

    // pyramid 0 = Gaussian, 1 = DoG.  The records replace the contents of `layers`; their vol_mat stay valid until the next
    // download of the same pyramid or the end of this object.
    void downloadPyramid(int pyramid, std::vector<Layer3D>& layers) {
        if (pyramid != 0 && pyramid != 1) throw std::string("SIFT3DScaleSpace: pyramid must be 0 (Gaussian) or 1 (DoG)");
        int n_layers = 0, n_octave = 0;
        hipdetail::check(oc_hip_sift3d_layer_count(engine_, pyramid, &n_layers, &n_octave));
        std::vector<std::unique_ptr<Volume>>& store = store_[pyramid];
        store.clear();
        layers.clear();
        for (int i = 0; i < n_layers; i++) {
            Layer3D layer{};
            hipdetail::check(oc_hip_sift3d_layer_info(engine_, pyramid, i, layer.dim_xyz, layer.unit_xyz, &layer.octave, &layer.scale, &layer.sigma,
                                                      &layer.max_abs));
            store.emplace_back(new Volume(layer.dim_xyz[0], layer.dim_xyz[1], layer.dim_xyz[2]));
            hipdetail::check(oc_hip_sift3d_get_layer(engine_, pyramid, i, store.back()->data.data(), OC_HIP_HOST));
            layer.vol_mat = store.back()->slabs.data();
            layers.push_back(layer);
        }
    }

    oc_hip_engine* handle() const { return engine_; }

private:
    // one contiguous block with the reference's float*** view on it (new3D, src/oc_array.h)
    struct Volume {
        std::vector<float> data;
        std::vector<float*> rows;
        std::vector<float**> slabs;
        Volume(int dx, int dy, int dz) : data((size_t)dx * dy * dz), rows((size_t)dy * dz), slabs((size_t)dz) {
            for (size_t r = 0; r < rows.size(); r++) rows[r] = data.data() + r * (size_t)dx;
            for (size_t z = 0; z < slabs.size(); z++) slabs[z] = rows.data() + z * (size_t)dy;
        }
    };

    oc_hip_engine* engine_ = nullptr;
    Sift3dConfig sift_config;
    float physical_unit[3] = {1.f, 1.f, 1.f};
    std::vector<std::unique_ptr<Volume>> store_[2];
};

}  // namespace opencorr

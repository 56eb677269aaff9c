// oc_feature_detect.h -- the reference's SIFT3D over the HIP C-ABI: createGaussianPyramid, createDogPyramid, detectExtrema,
// assignOrientation and constructDescriptor (src/oc_sift.cpp:676-754, 756-793, 795-847, 849-1049, 1051-1249) and, with the
// matcher of oc_feature_match.h, the whole of SIFT3D::compute (:234-293).
//
//   SIFT3DScaleSpace   setSiftConfig / setPhysicalUnit like SIFT3D's; compute(Image3D*) builds both pyramids on the device;
//                      detectExtrema(kp_queue) appends the candidates exactly as :832-839 fills them (coor_layer, layer, octave,
//                      scale); assignOrientation(kp_queue) replaces the queue by the accepted keypoints with coor_img and
//                      rotation_matrix; constructDescriptor(kp_queue, descriptor) fills the reference's float** rows;
//                      downloadPyramid(pyramid, layers) hands the layers out as Layer3D records with vol_mat[z][y][x].
//   SIFT3D             the public interface of src/oc_sift.h:135-180 that a caller of compute() uses: setImages, prepare, compute,
//                      clear, the config / unit / ratio setters and getters, ref_matched_kp, tar_matched_kp.  Keypoints and
//                      descriptors never leave the device between the stages.
//
// Differences a caller can observe ("SIFT3D scale space" and "SIFT3D orientation and descriptors"): where a blur
// radius exceeds dim - 1 on an axis the reference's mirrored index leaves the array, here it is clamped into the axis; sums over
// a keypoint's window are exact instead of sequential float32; the eigen-decomposition is a Jacobi iteration in double.
//
//   SIFT2DScaleSpace   the detector of SIFT2D::compute (src/oc_sift.cpp:60-93): setSiftConfig with the reference's Sift2dConfig;
//                      compute(Image2D*) builds the Gaussian and DoG pyramids of cv::SIFT::detect on the device;
//                      detect(kp_queue) appends the located keypoints (position, size, response, octave, layer) in the scan order
//                      of the extrema they started from.  Orientation, descriptors, duplicate removal, n_features trimming and
//                      SIFT2D::compute itself are not part of this header yet ("SIFT2D detector"); FeatureAffine
//                      lives in oc_feature_affine.h.
#pragma once

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../opencorr_hip.h"
#include "oc_engines.h"
#include "oc_feature_match.h"
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

    // assignOrientation (:849-1049): kp_queue becomes the accepted keypoints, in the queue's order, with coor_img and
    // rotation_matrix set (:1020-1028, :1044-1045).  The queue must hold records of this pyramid (detectExtrema's).
    void assignOrientation(std::vector<Keypoint3D>& kp_queue) {
        feature_config();
        std::vector<oc_hip_sift3d_candidate> list(kp_queue.size());
        for (size_t i = 0; i < kp_queue.size(); i++) {
            const Keypoint3D& kp = kp_queue[i];
            if (kp.coor_layer.x != (float)(int)kp.coor_layer.x || kp.coor_layer.y != (float)(int)kp.coor_layer.y || kp.coor_layer.z != (float)(int)kp.coor_layer.z)
                throw std::string("SIFT3DScaleSpace: keypoint coordinates must be whole voxels");
            list[i] = oc_hip_sift3d_candidate{(int)kp.coor_layer.x, (int)kp.coor_layer.y, (int)kp.coor_layer.z, kp.octave, kp.layer, kp.scale};
        }
        std::vector<oc_hip_sift3d_keypoint> out(list.size());
        size_t n = 0;
        hipdetail::check(oc_hip_sift3d_orient(engine_, list.data(), list.size(), OC_HIP_HOST, out.data(), out.size(), &n, nullptr, nullptr, OC_HIP_HOST));
        kp_queue.clear();
        for (size_t i = 0; i < n; i++) kp_queue.push_back(from_record(out[i]));
    }

    // constructDescriptor (:1051-1249): descriptor[m][0 ... 767] for every keypoint of kp_queue (rows the caller allocated, new2D)
    void constructDescriptor(std::vector<Keypoint3D>& kp_queue, float** descriptor) {
        feature_config();
        std::vector<oc_hip_sift3d_keypoint> list(kp_queue.size());
        for (size_t i = 0; i < kp_queue.size(); i++) list[i] = to_record(kp_queue[i]);
        std::vector<float> block(list.size() * 768);
        hipdetail::check(oc_hip_sift3d_describe(engine_, list.data(), list.size(), OC_HIP_HOST, block.data(), OC_HIP_HOST));
        for (size_t i = 0; i < list.size(); i++) std::memcpy(descriptor[i], block.data() + i * 768, 768 * sizeof(float));
    }

    // The two stages for every candidate of the pyramid, without a host list in between: the accepted keypoints (appended to
    // kp_queue) and their descriptors as a device block [n][768] (null for n = 0) that lives until the next call or the end of this object.
    const float* extractOnDevice(std::vector<Keypoint3D>& kp_queue) {
        feature_config();
        size_t n_candidates = 0, n = 0;
        hipdetail::check(oc_hip_sift3d_candidate_count(engine_, &n_candidates));
        std::vector<oc_hip_sift3d_keypoint> out(n_candidates);
        hipdetail::check(oc_hip_sift3d_orient(engine_, nullptr, 0, OC_HIP_HOST, out.data(), out.size(), &n, nullptr, nullptr, OC_HIP_HOST));
        for (size_t i = 0; i < n; i++) kp_queue.push_back(from_record(out[i]));
        hipdetail::check(oc_hip_sift3d_describe(engine_, nullptr, n, OC_HIP_HOST, nullptr, OC_HIP_DEVICE));  // (the block stays in the engine)
        const float* block = nullptr;
        size_t count = 0;
        if (n > 0) hipdetail::check(oc_hip_get_field(engine_, "descriptors", &block, &count));
        return block;
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
    void feature_config() {
        hipdetail::check(oc_hip_sift3d_set_feature_config(engine_, sift_config.beta, sift_config.gamma, sift_config.gradient_threshold,
                                                          sift_config.truncate_threshold));
    }
    static Keypoint3D from_record(const oc_hip_sift3d_keypoint& r) {
        Keypoint3D kp{};
        kp.coor_layer = Point3D(r.coor_layer[0], r.coor_layer[1], r.coor_layer[2]);
        kp.coor_img = Point3D(r.coor_img[0], r.coor_img[1], r.coor_img[2]);
        kp.octave = r.octave;
        kp.layer = r.layer;
        kp.scale = r.scale;
        std::memcpy(kp.rotation_matrix, r.rotation_matrix, sizeof kp.rotation_matrix);
        return kp;
    }
    static oc_hip_sift3d_keypoint to_record(const Keypoint3D& kp) {
        oc_hip_sift3d_keypoint r{};
        r.coor_layer[0] = kp.coor_layer.x, r.coor_layer[1] = kp.coor_layer.y, r.coor_layer[2] = kp.coor_layer.z;
        r.coor_img[0] = kp.coor_img.x, r.coor_img[1] = kp.coor_img.y, r.coor_img[2] = kp.coor_img.z;
        r.octave = kp.octave;
        r.layer = kp.layer;
        r.scale = kp.scale;
        std::memcpy(r.rotation_matrix, kp.rotation_matrix, sizeof r.rotation_matrix);
        return r;
    }

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

// SIFT3D of the reference (src/oc_sift.h:135-180), for callers of compute(): two extractions and the matcher, descriptors handed
// over as device blocks.  compute() ends with monodirectionalMatch like :285; setBidirectional(true) selects :288 instead.
class SIFT3D {
public:
    std::vector<Point3D> ref_matched_kp;  // matched keypoints in ref image
    std::vector<Point3D> tar_matched_kp;  // matched keypoints in tar image

    SIFT3D() : matcher_(768, 0.85f) {}
    SIFT3D(const SIFT3D&) = delete;
    SIFT3D& operator=(const SIFT3D&) = delete;

    void setImages(Image3D& ref_img, Image3D& tar_img) {  // Feature3D::setImages
        this->ref_img = &ref_img;
        this->tar_img = &tar_img;
    }
    Sift3dConfig getSiftConfig() const { return extractor_[0].getSiftConfig(); }
    float getPhysicalUnit(int dim) const { return extractor_[0].getPhysicalUnit(dim); }
    float getMatchingRatio() const { return matcher_.getMatchingRatio(); }
    void setSiftConfig(Sift3dConfig sift_config) {
        for (SIFT3DScaleSpace& s : extractor_) s.setSiftConfig(sift_config);
    }
    void setPhysicalUnit(float unit_x, float unit_y, float unit_z) {
        for (SIFT3DScaleSpace& s : extractor_) s.setPhysicalUnit(unit_x, unit_y, unit_z);
    }
    void setMatchingRatio(float matching_ratio) { matcher_.setMatchingRatio(matching_ratio); }
    void setBidirectional(bool on) { bidirectional_ = on; }

    void prepare() {}  // (:209-232 fills the icosahedron: a constant of the descriptor kernel here)

    void compute() {  // :234-293
        if (!ref_img || !tar_img) throw std::string("SIFT3D: no images (setImages)");
        std::vector<Keypoint3D> kp[2];
        Image3D* img[2] = {ref_img, tar_img};
        for (int side = 0; side < 2; side++) {
            extractor_[side].compute(img[side]);
            const float* block = extractor_[side].extractOnDevice(kp[side]);
            matcher_.setDeviceDescriptors(side, block, (int)kp[side].size());
        }
        clear();
        std::vector<Point3D> coor[2];
        for (int side = 0; side < 2; side++)
            for (const Keypoint3D& k : kp[side]) coor[side].push_back(k.coor_img);
        if (bidirectional_) matcher_.bidirectionalMatch(coor[0], coor[1], ref_matched_kp, tar_matched_kp);
        else matcher_.monodirectionalMatch(coor[0], coor[1], ref_matched_kp, tar_matched_kp);
    }

    void clear() {  // :295-299
        std::vector<Point3D>().swap(ref_matched_kp);
        std::vector<Point3D>().swap(tar_matched_kp);
    }

protected:
    Image3D* ref_img = nullptr;
    Image3D* tar_img = nullptr;

private:
    SIFT3DScaleSpace extractor_[2];  // one per image: each keeps its descriptor block alive until the match is done
    DescriptorMatcher3D matcher_;
    bool bidirectional_ = false;
};

// src/oc_sift.h:30-37
struct Sift2dConfig {
    int n_features;
    int n_octave_layers;
    float contrast_threshold;
    float edge_threshold;
    float sigma;
};

// one located keypoint of cv::SIFT::detect before orientation: the members of cv::KeyPoint that are final at that point, and the
// cell and offsets the next stages read
struct Keypoint2D {
    Point2D pt;
    float size, response;
    int octave, layer;   // octave as cv::SIFT counts it (-1 = the doubled base)
    int row, col;
    float offset_col, offset_row, offset_layer;
    int packed_octave;   // cv::KeyPoint::octave
};

class SIFT2DScaleSpace {
public:
    SIFT2DScaleSpace() {
        // SIFT2D::SIFT2D(), src/oc_sift.cpp:22-30
        sift_config.n_features = 0;
        sift_config.n_octave_layers = 3;
        sift_config.contrast_threshold = 0.04f;
        sift_config.edge_threshold = 10.f;
        sift_config.sigma = 1.6f;
        hipdetail::check(oc_hip_sift2d_create(hipdetail::default_device(), &engine_));
    }
    ~SIFT2DScaleSpace() { (void)oc_hip_destroy(engine_); }
    SIFT2DScaleSpace(const SIFT2DScaleSpace&) = delete;
    SIFT2DScaleSpace& operator=(const SIFT2DScaleSpace&) = delete;

    Sift2dConfig getSiftConfig() const { return sift_config; }
    void setSiftConfig(Sift2dConfig config) { sift_config = config; }  // src/oc_sift.cpp:44-47

    // the pyramids of cv::SIFT::detect (:86) of img; they stay on the device
    void compute(Image2D* img) {
        hipdetail::check(oc_hip_sift2d_set_config(engine_, sift_config.n_features, sift_config.n_octave_layers, sift_config.contrast_threshold,
                                                  sift_config.edge_threshold, sift_config.sigma));
        std::vector<float> rows((size_t)img->width * img->height);
        for (int r = 0; r < img->height; r++)
            for (int c = 0; c < img->width; c++) rows[(size_t)r * img->width + c] = img->eg_mat(r, c);
        hipdetail::check(oc_hip_sift2d_set_image(engine_, rows.data(), 1, img->width, img->height, OC_HIP_HOST));
        hipdetail::check(oc_hip_sift2d_build(engine_));
    }

    int getOctaveNumber() const {
        int n_layers = 0, n_octave = 0;
        hipdetail::check(oc_hip_sift2d_layer_count(engine_, 0, &n_layers, &n_octave));
        return n_octave;
    }

    // the located keypoints (:86), appended to kp_queue
    void detect(std::vector<Keypoint2D>& kp_queue) {
        size_t n = 0;
        hipdetail::check(oc_hip_sift2d_keypoint_count(engine_, &n));
        std::vector<oc_hip_sift2d_keypoint> list(n);
        if (n > 0) hipdetail::check(oc_hip_sift2d_detect(engine_, list.data(), n, &n, OC_HIP_HOST));
        for (size_t i = 0; i < n; i++) {
            Keypoint2D kp{};
            kp.pt.x = list[i].x;
            kp.pt.y = list[i].y;
            kp.size = list[i].size;
            kp.response = list[i].response;
            kp.octave = list[i].octave;
            kp.layer = list[i].layer;
            kp.row = list[i].row;
            kp.col = list[i].col;
            kp.offset_col = list[i].xc;
            kp.offset_row = list[i].xr;
            kp.offset_layer = list[i].xi;
            kp.packed_octave = list[i].packed_octave;
            kp_queue.push_back(kp);
        }
    }

    oc_hip_engine* engine() const { return engine_; }

private:
    Sift2dConfig sift_config;
    oc_hip_engine* engine_ = nullptr;
};

}  // namespace opencorr

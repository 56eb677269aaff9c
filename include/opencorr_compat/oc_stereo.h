// oc_stereo.h -- the stereo-DIC classes of the reference over the HIP C-ABI: CameraIntrinsics / CameraExtrinsics / Calibration
// (src/oc_calibration.h:25-97), Stereovision (src/oc_stereovision.h) and EpipolarSearch (src/oc_epipolar_search.h), with the
// reference's names, public members and call order, so that examples/test_3d_reconstruction_epipolar.cpp and
// examples/test_3d_dic_strain.cpp compile unmodified.
//
//   Calibration   the four matrices are host arithmetic inside the library (oc_hip_calibration_create / _get); prepare(height,
//                 width) builds the undistortion map on the device (one thread per pixel), undistort() looks points up in it.
//                 The reference's Eigen members become small fixed types with operator()(r, c).  Copies of a Calibration
//                 (EpipolarSearch keeps two) share the prepared map.
//   Stereovision  prepare() = both cameras' matrices + the fundamental matrix; reconstruct(view1, view2, points3d) is one
//                 launch over the queue.  Extension: reconstruct(std::vector<POI2DS>&) fills ref_coor, tar_coor and deformation
//                 of every record in one launch (the host loops of examples/test_3d_dic_epipolar_sift.cpp:303-317).
//   EpipolarSearch  compute(poi_queue) builds the trial positions of ALL POIs on the host (oc_epipolar.h, the reference's
//                 expressions) and refines them as ONE ICGN2D1 batch with the selection on the device
//                 (ICGN2D1::computeBestOf) instead of the reference's per-POI loop (src/oc_epipolar_search.cpp:133-204).
#pragma once

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../opencorr_hip.h"
#include "oc_engines.h"
#include "oc_epipolar.h"
#include "oc_types.h"

namespace opencorr {

union CameraIntrinsics {
    struct {
        float fx, fy, fs;
        float cx, cy;
        float k1, k2, k3, k4, k5, k6;
        float p1, p2;
    };
    float cam_i[13];
};

union CameraExtrinsics {
    struct {
        float tx, ty, tz;
        float rx, ry, rz;
    };
    float cam_e[6];
};

// Row-major R x C floats with the (r, c) / (i) access of the Eigen types they stand for
template <int R, int C>
struct CameraMatrix {
    float m[R * C] = {};
    float& operator()(int r, int c) { return m[r * C + c]; }
    float operator()(int r, int c) const { return m[r * C + c]; }
    float& operator()(int i) { return m[i]; }
    float operator()(int i) const { return m[i]; }
    int rows() const { return R; }
    int cols() const { return C; }
    float* data() { return m; }
    const float* data() const { return m; }
    void setIdentity() {
        for (int r = 0; r < R; r++)
            for (int c = 0; c < C; c++) m[r * C + c] = r == c ? 1.f : 0.f;
    }
};
using CameraMatrix3f = CameraMatrix<3, 3>;
using CameraVector3f = CameraMatrix<3, 1>;
using CameraMatrix34f = CameraMatrix<3, 4>;

class Calibration {
public:
    CameraIntrinsics intrinsics;
    CameraExtrinsics extrinsics;

    CameraMatrix3f intrinsic_matrix;
    CameraMatrix3f rotation_matrix;
    CameraVector3f translation_vector;
    CameraMatrix34f projection_matrix;

    float convergence = 0.001f;  // src/oc_calibration.cpp:21-25
    int iteration = 40;

    Calibration() {
        std::memset(&intrinsics, 0, sizeof(intrinsics));
        std::memset(&extrinsics, 0, sizeof(extrinsics));
    }
    Calibration(CameraIntrinsics& intrinsics_, CameraExtrinsics& extrinsics_) { updateCalibration(intrinsics_, extrinsics_); }

    // src/oc_calibration.cpp:36-93.  The reference's four update functions are one host computation here: each of them
    // refreshes all four matrices from the present intrinsics / extrinsics ("Null intrinsics matrix" is thrown as there).
    void updateMatrices() {
        oc_hip_engine* h = nullptr;
        hipdetail::check(oc_hip_calibration_create(intrinsics.cam_i, extrinsics.cam_e, hipdetail::default_device(), &h));
        std::shared_ptr<oc_hip_engine> guard(h, oc_hip_destroy);
        hipdetail::check(oc_hip_calibration_get(h, OC_HIP_CAL_INTRINSIC, intrinsic_matrix.data()));
        hipdetail::check(oc_hip_calibration_get(h, OC_HIP_CAL_ROTATION, rotation_matrix.data()));
        hipdetail::check(oc_hip_calibration_get(h, OC_HIP_CAL_TRANSLATION, translation_vector.data()));
        hipdetail::check(oc_hip_calibration_get(h, OC_HIP_CAL_PROJECTION, projection_matrix.data()));
    }
    void updateIntrinsicMatrix() { updateMatrices(); }
    void updateRotationMatrix() { updateMatrices(); }
    void updateTranslationVector() { updateMatrices(); }
    void updateProjectionMatrix() { updateMatrices(); }
    void updateCalibration(CameraIntrinsics& intrinsics_, CameraExtrinsics& extrinsics_) {
        intrinsics = intrinsics_;
        extrinsics = extrinsics_;
        updateMatrices();
    }
    void clear() {
        for (float& v : intrinsics.cam_i) v = 0.f;
        for (float& v : extrinsics.cam_e) v = 0.f;
    }

    float getConvergence() const { return convergence; }
    int getIteration() const { return iteration; }
    void setUndistortion(float convergence_, int iteration_) {
        convergence = convergence_;
        iteration = iteration_;
    }

    // src/oc_calibration.cpp:117-159 (host float arithmetic, the source's expressions)
    Point2D image_to_sensor(Point2D& point) {
        float sensor_y = point.y * intrinsics.fy + intrinsics.cy;
        float sensor_x = point.x * intrinsics.fx + point.y * intrinsics.fs + intrinsics.cx;
        return Point2D(sensor_x, sensor_y);
    }
    Point2D sensor_to_image(Point2D& point) {
        float image_y = (point.y - intrinsics.cy) / intrinsics.fy;
        float image_x = (point.x - intrinsics.cx - intrinsics.fs * image_y) / intrinsics.fx;
        return Point2D(image_x, image_y);
    }
    Point2D distort(Point2D& point) {
        float xx = point.x * point.x, yy = point.y * point.y, xy = point.x * point.y;
        float r2 = xx + yy, r4 = r2 * r2, r6 = r2 * r4;
        float radial = (1 + intrinsics.k1 * r2 + intrinsics.k2 * r4 + intrinsics.k3 * r6) / (1 + intrinsics.k4 * r2 + intrinsics.k5 * r4 + intrinsics.k6 * r6);
        float dy = point.y * radial, dx = point.x * radial;
        dy += intrinsics.p1 * (r2 + 2 * yy) + 2 * intrinsics.p2 * xy;
        dx += 2 * intrinsics.p1 * xy + intrinsics.p2 * (r2 + 2 * xx);
        return Point2D(dx, dy);
    }

    // src/oc_calibration.cpp:161-219: the map stays on the device (oc_hip_calibration_maps copies it out)
    void prepare(int height, int width) {
        oc_hip_engine* h = nullptr;
        hipdetail::check(oc_hip_calibration_create(intrinsics.cam_i, extrinsics.cam_e, hipdetail::default_device(), &h));
        engine_.reset(h, oc_hip_destroy);
        std::memcpy(made_with_, intrinsics.cam_i, sizeof(intrinsics.cam_i));
        std::memcpy(made_with_ + 13, extrinsics.cam_e, sizeof(extrinsics.cam_e));
        hipdetail::check(oc_hip_calibration_set_undistortion(h, convergence, iteration));
        hipdetail::check(oc_hip_calibration_prepare(h, height, width));
        height_ = height;
        width_ = width;
    }

    // src/oc_calibration.cpp:221-264; like the reference the argument is clamped to the map in place
    Point2D undistort(Point2D& point) {
        if (point.x < 0) point.x = 0;
        if (point.y < 0) point.y = 0;
        if (point.x > width_ - 2) point.x = (float)width_ - 2.f;
        if (point.y > height_ - 2) point.y = (float)height_ - 2.f;
        Point2D out;
        hipdetail::check(oc_hip_calibration_undistort(handle(), &point, &out, 1, sizeof(Point2D), OC_HIP_HOST));
        return out;
    }

    // The prepared handle.  Parameters edited after prepare() make the map stale: the reference would go on using it, here
    // prepare() has to be called again.
    oc_hip_engine* handle() {
        if (!engine_) throw std::string("Calibration: prepare(height, width) has not been called");
        if (std::memcmp(made_with_, intrinsics.cam_i, sizeof(intrinsics.cam_i)) != 0 ||
            std::memcmp(made_with_ + 13, extrinsics.cam_e, sizeof(extrinsics.cam_e)) != 0)
            throw std::string("Calibration: intrinsics / extrinsics changed since prepare(height, width); call it again");
        return engine_.get();
    }

private:
    std::shared_ptr<oc_hip_engine> engine_;
    float made_with_[19] = {};
    int height_ = 0, width_ = 0;
};

namespace stereodetail {
// updateFundementalMatrix of Stereovision and EpipolarSearch (src/oc_stereovision.cpp:36-54, src/oc_epipolar_search.cpp:103-121:
// the same four lines): computed by the library from the cameras' parameters alone, no map and no device needed
inline void fundamental(const float* cam1_i, const float* cam1_e, const float* cam2_i, const float* cam2_e, float* out9) {
    oc_hip_engine *h1 = nullptr, *h2 = nullptr, *hs = nullptr;
    hipdetail::check(oc_hip_calibration_create(cam1_i, cam1_e, hipdetail::default_device(), &h1));
    std::shared_ptr<oc_hip_engine> g1(h1, oc_hip_destroy);
    hipdetail::check(oc_hip_calibration_create(cam2_i, cam2_e, hipdetail::default_device(), &h2));
    std::shared_ptr<oc_hip_engine> g2(h2, oc_hip_destroy);
    hipdetail::check(oc_hip_stereo_create(h1, h2, &hs));
    std::shared_ptr<oc_hip_engine> gs(hs, oc_hip_destroy);
    hipdetail::check(oc_hip_stereo_fundamental(hs, out9));
}
}  // namespace stereodetail

class Stereovision {
protected:
    Calibration* view1_cam = nullptr;
    Calibration* view2_cam = nullptr;
    int thread_number;

public:
    CameraMatrix3f fundamental_matrix;

    Stereovision(Calibration* view1_cam_, Calibration* view2_cam_, int thread_number_)
        : view1_cam(view1_cam_), view2_cam(view2_cam_), thread_number(thread_number_) {}
    Stereovision(const Stereovision&) = delete;
    Stereovision& operator=(const Stereovision&) = delete;

    void updateCameras(Calibration* view1_cam_, Calibration* view2_cam_) {
        view1_cam = view1_cam_;
        view2_cam = view2_cam_;
        engine_.reset();
    }
    // src/oc_stereovision.cpp:36-54
    void updateFundementalMatrix() {
        stereodetail::fundamental(view1_cam->intrinsics.cam_i, view1_cam->extrinsics.cam_e, view2_cam->intrinsics.cam_i,
                                  view2_cam->extrinsics.cam_e, fundamental_matrix.data());
    }
    // src/oc_stereovision.cpp:56-68
    void prepare() {
        view1_cam->updateMatrices();
        view2_cam->updateMatrices();
        updateFundementalMatrix();
    }

    // src/oc_stereovision.cpp:70-124 (one point pair: a launch of its own -- use the queue form)
    Point3D reconstruct(Point2D& view1_2d_point, Point2D& view2_2d_point) {
        Point3D out;
        hipdetail::check(oc_hip_stereo_reconstruct(handle(), &view1_2d_point, sizeof(Point2D), &view2_2d_point, sizeof(Point2D), &out,
                                                   sizeof(Point3D), 1, OC_HIP_HOST));
        return out;
    }
    // src/oc_stereovision.cpp:126-133
    void reconstruct(std::vector<Point2D>& view1_2d_point_queue, std::vector<Point2D>& view2_2d_point_queue,
                     std::vector<Point3D>& space_3d_point_queue) {
        if (view2_2d_point_queue.size() < view1_2d_point_queue.size() || space_3d_point_queue.size() < view1_2d_point_queue.size())
            throw std::string("Stereovision::reconstruct: the queues are shorter than view1_2d_point_queue");
        static_assert(sizeof(Point2D) == 8 && sizeof(Point3D) == 12, "Point2D / Point3D must be packed floats");
        hipdetail::check(oc_hip_stereo_reconstruct(handle(), view1_2d_point_queue.data(), sizeof(Point2D), view2_2d_point_queue.data(),
                                                   sizeof(Point2D), space_3d_point_queue.data(), sizeof(Point3D),
                                                   view1_2d_point_queue.size(), OC_HIP_HOST));
    }
    // ref_coor, tar_coor and deformation = tar_coor - ref_coor of every record (examples/test_3d_dic_epipolar_sift.cpp:303-317)
    void reconstruct(std::vector<POI2DS>& poi_queue) {
        hipdetail::check(oc_hip_stereo_reconstruct_pois(handle(), poi_queue.data(), poi_queue.size(), sizeof(POI2DS), OC_HIP_HOST));
    }

    oc_hip_engine* handle() {
        // the cameras' handles are the ones their last prepare(height, width) made
        oc_hip_engine* h1 = view1_cam->handle();
        oc_hip_engine* h2 = view2_cam->handle();
        if (!engine_ || h1 != cam_handles_[0] || h2 != cam_handles_[1]) {
            oc_hip_engine* h = nullptr;
            hipdetail::check(oc_hip_stereo_create(h1, h2, &h));
            engine_.reset(h, oc_hip_destroy);
            cam_handles_[0] = h1;
            cam_handles_[1] = h2;
        }
        return engine_.get();
    }

private:
    std::shared_ptr<oc_hip_engine> engine_;
    oc_hip_engine* cam_handles_[2] = {nullptr, nullptr};
};

class EpipolarSearch : public DIC {
protected:
    int search_radius = 0;
    int search_step = 1;
    Calibration view1_cam;
    Calibration view2_cam;
    CameraMatrix3f fundamental_matrix;
    Point2D parallax;
    float parallax_x[3] = {0.f, 0.f, 0.f}, parallax_y[3] = {0.f, 0.f, 0.f};

public:
    std::unique_ptr<ICGN2D1> icgn1;

    EpipolarSearch(Calibration& view1_cam_, Calibration& view2_cam_, int thread_number_) : view1_cam(view1_cam_), view2_cam(view2_cam_) {
        thread_number = thread_number_;
    }

    int getSearchRadius() const { return search_radius; }
    int getSearchStep() const { return search_step; }
    void setSearch(int search_radius_, int search_step_) {
        if (search_radius_ < search_step_) throw std::string("Search radius is less than search step");
        if (search_step_ < 1) throw std::string("Search step must be at least 1");  // (the reference's loop would not end)
        search_radius = search_radius_;
        search_step = search_step_;
    }
    void createICGN(int subset_radius_x_, int subset_radius_y_, float conv_criterion, float stop_condition) {
        icgn1 = std::make_unique<ICGN2D1>(subset_radius_x_, subset_radius_y_, conv_criterion, stop_condition, thread_number);
    }
    void prepareICGN() {
        if (!icgn1) throw std::string("EpipolarSearch: createICGN() has not been called");
        if (!ref_img || !tar_img) throw std::string("setImages() has not been called");
        icgn1->setImages(*ref_img, *tar_img);
        icgn1->prepare();
    }
    void destoryICGN() { icgn1.reset(); }

    void setParallax(Point2D parallax_) {
        parallax = parallax_;
        parallax_x[0] = parallax_x[1] = 0.f;
        parallax_x[2] = parallax_.x;
        parallax_y[0] = parallax_y[1] = 0.f;
        parallax_y[2] = parallax_.y;
    }
    void setParallax(float coefficient_x[3], float coefficient_y[3]) {
        for (int i = 0; i < 3; i++) {
            parallax_x[i] = coefficient_x[i];
            parallax_y[i] = coefficient_y[i];
        }
    }

    void updateCameras(Calibration& view1_cam_, Calibration& view2_cam_) {
        view1_cam = view1_cam_;
        view2_cam = view2_cam_;
    }
    // src/oc_epipolar_search.cpp:103-121
    void updateFundementalMatrix() {
        stereodetail::fundamental(view1_cam.intrinsics.cam_i, view1_cam.extrinsics.cam_e, view2_cam.intrinsics.cam_i,
                                  view2_cam.extrinsics.cam_e, fundamental_matrix.data());
    }

    // src/oc_epipolar_search.cpp:123-131
    void prepare() override {
        view1_cam.updateMatrices();
        view2_cam.updateMatrices();
        updateFundementalMatrix();
        prepareICGN();
    }
    // src/oc_epipolar_search.cpp:133-195
    void compute(POI2D* poi) override {
        std::vector<POI2D> one(1, *poi);
        compute(one);
        poi->deformation = one[0].deformation;
        poi->result = one[0].result;
    }
    // src/oc_epipolar_search.cpp:197-205: all POIs' trials as one batch
    void compute(std::vector<POI2D>& poi_queue) override {
        if (!icgn1) throw std::string("EpipolarSearch: createICGN() has not been called");
        if (!ref_img) throw std::string("setImages() has not been called");
        const EpipolarSearchSetting s = setting();
        std::vector<POI2D> candidates;
        std::vector<unsigned> segment_starts;
        epipolarCandidates(poi_queue, s, candidates, segment_starts);
        icgn1->computeBestOf(candidates, segment_starts, poi_queue);
    }
    // what compute() hands to epipolarCandidates
    EpipolarSearchSetting setting() const {
        EpipolarSearchSetting s;
        for (int i = 0; i < 9; i++) s.fundamental_matrix[i] = fundamental_matrix.m[i];
        for (int i = 0; i < 3; i++) {
            s.parallax_x[i] = parallax_x[i];
            s.parallax_y[i] = parallax_y[i];
        }
        s.search_radius = search_radius;
        s.search_step = search_step;
        s.subset_radius_x = icgn1 ? icgn1->subset_radius_x : 0;
        s.subset_radius_y = icgn1 ? icgn1->subset_radius_y : 0;
        s.image_width = ref_img ? ref_img->width : 0;
        s.image_height = ref_img ? ref_img->height : 0;
        return s;
    }
};

}  // namespace opencorr

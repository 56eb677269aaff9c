// oc_kernels.h -- host-side launch interface of the gfx950 kernels (internal).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

// OC_BUILD_AB = 1: the A/B build of the library (opencorr_amd/build.py --ab -> lib/ab/libopencorr_hip_ab.so) also contains the
// measured losers kept as comparison partners -- icgn2d variants 0 and 6, the ICGN3D1 row mapping (icgn3d_rows.hip) -- and
// honours the experiment environment knobs (OC_ICGN3D_BLOCKS, OC_ICGN2D_LDS_PAD).  The library that ships is built without it.
#ifndef OC_BUILD_AB
#define OC_BUILD_AB 0
#endif

namespace ochip {

// ---- prepare2d.hip ---------------------------------------------------------
hipError_t launch_grad2d(const float* img, int height, int width, float* gx, float* gy, hipStream_t stream);
// value_plane (optional, height * width floats): the table's interpolant at each pixel's own integer position -- lut_value() of
// the pixel's 16 coefficients at dx = dy = 0 -- for the integer-translation sweep of icgn2d.hip (Icgn2dParams::lut_val)
hipError_t launch_bspline2d_lut(const float* img, int height, int width, float* lut, hipStream_t stream, float* value_plane = nullptr);
hipError_t launch_colmajor_to_rowmajor(const float* src, int height, int width, float* dst, hipStream_t stream);

// ---- icgn2d.hip ------------------------------------------------------------
struct Icgn2dParams {
    const float* ref;  // reference image, row-major
    const float* gx;   // reference gradients
    const float* gy;
    const float* lut;  // target bicubic coefficient LUT, 16 floats per pixel
    int height, width;
    int rx, ry;        // subset radius (self_adaptive: the largest radii of the batch)
    float conv, stop;
    const float* offsets;  // per-POI centre offsets (x, y), or nullptr: compute(poi_queue, center_offset_queue)
    const unsigned* perm;  // visiting order of the queue (poi_order.hip), or nullptr: queue order
    int self_adaptive;     // DIC::setSelfAdaptive: every POI carries its own subset radius
    // IC-LM only (launch_iclm2d*): DampingParameter of src/oc_iclm.h:33-38 with ln(lambda) taken on the host
    double lm_log_lambda;
    float lm_alpha, lm_beta;
    int arith_fma;  // 1: the build whose per-sample multiply-adds are fused (oc_device.h OC_FMA; oracle OC_ORDER_LANES_FMA)
    float* setup;   // variant 8 (split launch shape): icgn2d_setup_record_floats(dof) floats per POI -- mean, norm, H^-1 -- written by
                    // the set-up kernel and read by the iteration kernel; nullptr otherwise
    // Set-up cache of the big-queue table variants (4, 5, 10, 11; icgn2d.hip): nullptr = off.  Otherwise icgn2d_setup_record_floats(dof)
    // floats per POI that outlive the call.  The launch FILLS them (and computes as ever) when cache_force_fill is set or
    // *cache_word == cache_epoch -- the stamp launch_poi2d_xy_check leaves when the queue's coordinates are not the ones the
    // records were built for -- and otherwise starts from them.
    float* cache_recs;
    const unsigned* cache_word;
    unsigned cache_epoch;
    int cache_force_fill;
    // Value plane of the target table (launch_bspline2d_lut), or nullptr: the interpolation sweep of a wave whose warp is an integer
    // translation reads a sample's value from it instead of gathering the 16 coefficients (icgn2d.hip, kIntSweep); nullptr = every
    // sweep is the full one ("icgn2d_int_first" = 0)
    const float* lut_val;
};
// writes max over the queue of (int)subset_radius.x / .y to out2[0], out2[1]
hipError_t launch_poi2d_max_radius(const float* pois, int stride_floats, size_t count, int* out2, hipStream_t stream);
// The ICGN2D kernels exist in several bit-identical variants (gather depth, LDS footprint,
// software pipelining, waves per workgroup; icgn2d.hip).  `variant` indexes that table,
// `xcd` turns on the XCD-contiguous mapping of workgroups to the POI queue.
// Returns hipErrorInvalidValue if the subset does not fit the variant's LDS budget.
// phase (variant 8 only): 0 = set-up kernel then iteration kernel on `stream`, 1 = the set-up kernel alone, 2 = the iteration
// kernel alone (the caller orders it behind the set-up of the same POIs)
hipError_t launch_icgn2d1(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, int variant, bool xcd,
                          hipStream_t stream, int phase = 0);
// ICLM2D1 / ICLM2D2 (src/oc_iclm.cpp): the same kernel with the Levenberg-Marquardt step
hipError_t launch_iclm2d1(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
hipError_t launch_iclm2d2(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
hipError_t launch_icgn2d2(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, int variant, bool xcd,
                          hipStream_t stream, int phase = 0);
int icgn2d_setup_record_floats(int dof);
// the two builds of icgn2d.hip (oc_device.h: OC_FMA = 0 / 1) behind the four launchers above
#define OC_DECLARE_ICGN2D_LAUNCHERS                                                                                          \
    hipError_t launch_icgn2d1(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, int variant, bool xcd,   \
                              hipStream_t stream, int phase);                                                               \
    hipError_t launch_icgn2d2(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, int variant, bool xcd,   \
                              hipStream_t stream, int phase);                                                               \
    hipError_t launch_iclm2d1(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream); \
    hipError_t launch_iclm2d2(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
namespace sep {
OC_DECLARE_ICGN2D_LAUNCHERS
}
namespace fma {
OC_DECLARE_ICGN2D_LAUNCHERS
}
#undef OC_DECLARE_ICGN2D_LAUNCHERS
// icgn2d_band.hip (round 6): the same solvers with the workgroup's band of the bicubic table staged in LDS and the warped subset in
// registers; hipErrorInvalidValue when the subset has more passes than the kernel holds in registers or radii are per POI
hipError_t launch_icgn2d1_band(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
hipError_t launch_icgn2d2_band(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
bool icgn2d_band_supported(int dof, int rx, int ry);  // an instantiation for this subset's pass count exists
namespace sep {
hipError_t launch_icgn2d1_band(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
hipError_t launch_icgn2d2_band(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
}
namespace fma {
hipError_t launch_icgn2d1_band(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
hipError_t launch_icgn2d2_band(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
}
// icgn2d_onepass.hip: ICGN2D1 / ICGN2D2 under the one-pass arithmetic contract (oc_hip_set_tuning "arith_onepass"): one sweep per
// iteration, no target array; one radius per launch and no centre offsets (hipErrorNotSupported), hipErrorInvalidValue when the
// workgroup's coordinate table does not fit LDS.  p.arith_fma does not matter: the kernel is built with the fused multiply-add.
hipError_t launch_icgn2d1_onepass(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
hipError_t launch_icgn2d2_onepass(const Icgn2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
// (which variant ids exist, what each holds in LDS and which one a call launches: host/icgn2d_plan.h)

// ---- poi_order.hip ---------------------------------------------------------
// locality schedule: perm[k] = index of the k-th POI to visit (tile by tile, queue order inside a tile); tiles =
// scratch of poi2d_tile_count(height, width, tile_px) unsigned ints, slots = scratch of `count` unsigned ints
size_t poi2d_tile_count(int height, int width, int tile_px);
hipError_t launch_poi2d_tile_order(const float* pois, int stride_floats, size_t count, int height, int width, int tile_px,
                                   unsigned* tiles, unsigned* slots, unsigned* perm, hipStream_t stream, unsigned* xy_copy = nullptr,
                                   unsigned* xy_word = nullptr, unsigned xy_epoch = 0);
// Coordinate check of the ICGN2D set-up cache: xy_copy holds the (x, y) bit patterns the records were built for (2 words per
// POI).  Every POI whose coordinates differ gets its pair rewritten and stamps *word with `epoch` (plain stores of one
// value).  launch_poi2d_tile_order does the same inside its histogram pass when xy_copy is given: no extra kernel.
hipError_t launch_poi2d_xy_check(const float* pois, int stride_floats, size_t count, unsigned* xy_copy, unsigned* word, unsigned epoch,
                                 hipStream_t stream);
// the same for POI3D queues (cubic tiles of tile_vox voxels): the ICGN3D1 kernels visit the queue block by block
size_t poi3d_tile_count(int depth, int height, int width, int tile_vox);
hipError_t launch_poi3d_tile_order(const float* pois, int stride_floats, size_t count, int depth, int height, int width, int tile_vox,
                                   unsigned* tiles, unsigned* slots, unsigned* perm, hipStream_t stream);

// ---- strain.hip -------------------------------------------------------------
// Strain::prepare / Strain::compute (src/oc_strain.cpp): uniform grid over the queue's coordinates
struct StrainGrid {
    float x0, y0, z0, inv_pitch;
    int ncx, ncy, ncz;
};
struct StrainParams {
    float radius2;         // subregion_radius * subregion_radius, in float
    float zncc_threshold;  // Strain::setZnccThreshold, default 0.9
    int neighbor_min;      // neighbor_number_min
    int approximation;     // 1 = Cauchy, 2 = Green
};
int strain_knn_max();  // largest neighbor_number_min the KNN path holds
hipError_t launch_strain_bbox(int ndim, const float* pois, int stride_floats, size_t count, unsigned* box6, hipStream_t stream);
StrainGrid strain_make_grid(int ndim, const unsigned* box6_host, float radius);
size_t strain_cell_count(const StrainGrid& g);
hipError_t launch_strain_sort(int ndim, const float* pois, int stride_floats, size_t count, const StrainGrid& g,
                              unsigned* counts, unsigned* start, unsigned* cursor, unsigned* slots, unsigned* order,
                              hipStream_t stream);
hipError_t launch_strain_gather(int ndim, const float* pois, int stride_floats, size_t count, const unsigned* order, void* recs,
                                hipStream_t stream);
// RegionFit2D/3D::compute (src/oc_region_fit.cpp): plane through the reliable cloud (recs) for every POI of `pois`
hipError_t launch_region_fit_compute(int ndim, float* pois, int stride_floats, size_t count, const StrainGrid& g,
                                     const StrainParams& P, const unsigned* start, const void* recs, unsigned* fallback,
                                     hipStream_t stream);
hipError_t launch_strain_compute(int ndim, float* pois, int stride_floats, size_t count, const StrainGrid& g,
                                 const StrainParams& P, const unsigned* start, const unsigned* order, void* recs,
                                 unsigned* fallback, hipStream_t stream);

// Strain::compute(std::vector<POI2DS>&) (src/oc_strain.cpp:250-370): the neighbour search is the 2D one over (x, y) --
// launch_strain_bbox / launch_strain_sort with ndim 2 on the 28-float records -- the fit has four columns over ref_coor.
// recs: count * 48 bytes
hipError_t launch_strain2ds_compute(float* pois, int stride_floats, size_t count, const StrainGrid& g, const StrainParams& P,
                                    const unsigned* start, const unsigned* order, void* recs, unsigned* fallback,
                                    hipStream_t stream);

// ---- feature_affine.hip -------------------------------------------------------
// FeatureAffine2D/3D::compute (src/oc_feature_affine.cpp): the seeded RANSAC affine fit over the matched keypoints around a POI.
// The grid over the reference keypoints is Strain's (launch_strain_bbox / strain_make_grid / launch_strain_sort on the packed
// keypoint array, stride ndim floats).  The contract: DESIGN.md section 4.12.
struct FeatureAffineParams {
    float radius2;           // neighbor_search_radius squared, rounded to float
    float error_threshold;   // RansacConfig::error_threshold
    int neighbor_min;        // neighbor_number_min
    int sample_number;       // RansacConfig::sample_mumber, ndim + 1 ... 8
    int trial_number;        // RansacConfig::trial_number, 1 ... 1024
    int self_adaptive;       // 2D only (src/oc_feature_affine.cpp:128-179)
    int feature_min;         // subset_feature_min
    int radius_min;          // subset_radius_min
    float width, height;     // of the reference image (:130-133)
    unsigned long long seed;
};
constexpr int kFeatureAffineListLds = 1024;   // candidates of a POI kept in LDS; the rest lives in a global slice
constexpr int kFeatureAffineListMax = 16384;  // largest candidate count of a POI
constexpr int kFeatureAffineMaxSlots = 1024;  // waves of a launch that needs global slices (a slice: 2 ndim arrays of the launch's largest list beyond the LDS part)
// {ref xyz, tar xyz, keypoint index} in cell order.  recs: count * 32 bytes
hipError_t launch_feature_affine_gather(int ndim, const float* ref, const float* tar, size_t count, const unsigned* order, void* recs,
                                        hipStream_t stream);
// out_ref / out_tar[k] = ref_kp[ref_idx[k]] / tar_kp[tar_idx[k]], packed ndim floats per point.  *negative (device) = the first
// pair with a negative index (0xffffffff: none); such a pair reads nothing
hipError_t launch_feature_affine_pairs(int ndim, const float* ref_kp, const float* tar_kp, const int* ref_idx, const int* tar_idx,
                                       size_t n_pairs, float* out_ref, float* out_tar, unsigned* negative, hipStream_t stream);
// Candidate count of every POI (what the radius walk of compute finds; 0 in self-adaptive mode, whose list is the KNN's).
// verdict[0] = the largest count, verdict[1] = smallest index of a POI with more than kFeatureAffineListMax candidates,
// verdict[2] = smallest index of a POI with a NaN coordinate (0xffffffff: none).  Writes nothing else.
hipError_t launch_feature_affine_count(int ndim, const float* pois, int stride_floats, size_t count, const StrainGrid& g,
                                       const FeatureAffineParams& P, const unsigned* start, const void* recs, unsigned* verdict,
                                       hipStream_t stream);
// bytes of the global slices a launch over `count` POIs needs when the largest candidate count is `max_candidates`
size_t feature_affine_scratch_bytes(int ndim, size_t count, unsigned max_candidates);
hipError_t launch_feature_affine_compute(int ndim, float* pois, int stride_floats, size_t count, const StrainGrid& g,
                                         const FeatureAffineParams& P, const unsigned* start, const void* recs,
                                         unsigned max_candidates, float* scratch, hipStream_t stream);

// float offsets inside a POI2DS, the stereo record (src/oc_poi.h:53-60, 73-90, 140-183): x, y | u, v, w | r1r2, r1t1, r1t2 zncc,
// r2, t1, t2 | ref_coor | tar_coor | six strains | subset_radius
namespace poi2ds {
constexpr int X = 0, Y = 1, U = 2, V = 3, W = 4, R1R2_ZNCC = 5, R1T1_ZNCC = 6, R1T2_ZNCC = 7, R2_X = 8, R2_Y = 9, T1_X = 10,
              T1_Y = 11, T2_X = 12, T2_Y = 13, REF = 14, TAR = 17, EXX = 20, SRX = 26, SRY = 27;
constexpr int FLOATS = 28;
}  // namespace poi2ds

// ---- stereo.hip -------------------------------------------------------------
// Calibration::prepare / undistort (src/oc_calibration.cpp:161-264), Stereovision::reconstruct (src/oc_stereovision.cpp:70-133)
struct CameraParams {
    float fx, fy, fs, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2;  // CameraIntrinsics::cam_i order, src/oc_calibration.h:25-35
};
struct CameraView {
    CameraParams cam;
    const float* map_x;  // height * width, row-major
    const float* map_y;
    int height, width;
    float proj[12];  // projection matrix, row-major 3 x 4
};
hipError_t launch_undistort_map(const CameraParams& cam, int height, int width, float convergence, int iteration, float* map_x,
                                float* map_y, hipStream_t stream);
hipError_t launch_undistort_points(const CameraView& view, const float* in, float* out, int stride_floats, size_t count,
                                   hipStream_t stream);
hipError_t launch_reconstruct(const CameraView& view1, const CameraView& view2, const float* p1, int stride1_floats,
                              const float* p2, int stride2_floats, float* out, int stride_out_floats, size_t count,
                              hipStream_t stream);
// every POI2DS record: ref_coor <- (x, y) / (r2), tar_coor <- (t1) / (t2), deformation <- tar_coor - ref_coor
hipError_t launch_reconstruct_pois(const CameraView& view1, const CameraView& view2, float* pois, int stride_floats, size_t count,
                                   hipStream_t stream);

// best candidate (highest ZNCC) of every segment of a candidate queue -> deformation + result of the segment's POI
hipError_t launch_poi2d_best_of_segments(const float* cand, int cand_stride_floats, const unsigned* seg_start, size_t nseg,
                                         float* pois, int stride_floats, hipStream_t stream);

// ---- nr2d.hip --------------------------------------------------------------
struct Nr2dParams {
    const float* ref;     // reference image, row-major
    const float* lut;     // bicubic LUT of the target image
    const float* lut_gx;  // bicubic LUT of d/dx target
    const float* lut_gy;  // bicubic LUT of d/dy target
    int height, width;
    int rx, ry;
    float conv, stop;
    const unsigned* perm;  // visiting order of the queue (poi_order.hip), or nullptr: queue order
};
hipError_t launch_nr2d1(const Nr2dParams& p, float* pois, int stride_floats, size_t count, hipStream_t stream);
int nr2d1_max_samples();

// ---- prepare3d.hip ---------------------------------------------------------
hipError_t launch_grad3d(const float* vol, int dz, int dy, int dx, float* gx, float* gy, float* gz, hipStream_t stream);
// coef <- prefilter_z(prefilter_y(prefilter_x(vol))); tmp is a scratch volume of the same size
hipError_t launch_bspline3d_prefilter(const float* vol, int dz, int dy, int dx, float* coef, float* tmp,
                                      hipStream_t stream);

// ---- icgn3d.hip ------------------------------------------------------------
struct Icgn3dParams {
    const float* ref;
    const float* gx;
    const float* gy;
    const float* gz;
    const float* coef;  // tricubic B-spline coefficient volume of the target
    int dz, dy, dx;
    int rx, ry, rz;
    float conv, stop;
    float* scratch;  // per-workgroup slots for the warped subvolume
    int samples_per_pass;  // samples (row mapping: steps of 16 rows) per thread between two coefficient-box stagings (set by the launchers)
    int tail_steps_per_pass;  // row mapping: steps of 512 tail samples per tail pass (set by launch_icgn3d1_rows)
    const unsigned* perm;     // locality schedule (poi_order.hip launch_poi3d_tile_order): the k-th solve takes POI perm[k]; nullptr = queue order
    int arith_fma;            // 1: the build whose per-sample multiply-adds are fused (icgn3d.hip only; the row mapping has no such build)
};
// floats of global scratch the kernel needs for this radius (0 when the subvolume fits LDS);
// *blocks receives the number of persistent workgroups in scratch mode (0 in LDS mode)
size_t icgn3d1_scratch_floats(int rx, int ry, int rz, int* blocks);
hipError_t launch_icgn3d1(const Icgn3dParams& p, float* pois, int stride_floats, size_t count, hipStream_t stream);
namespace sep {
hipError_t launch_icgn3d1(const Icgn3dParams& p, float* pois, int stride_floats, size_t count, hipStream_t stream);
}
namespace fma {
hipError_t launch_icgn3d1(const Icgn3dParams& p, float* pois, int stride_floats, size_t count, hipStream_t stream);
}
// icgn3d_onepass.hip: ICGN3D1 under the one-pass arithmetic contract (oc_hip_set_tuning "arith_onepass3d"): the tap sweep forms
// 15 running sums and stores no sample, one block reduction per iteration.  Mapping and launch shape of launch_icgn3d1; p.scratch is
// not read and p.arith_fma does not matter: the kernel is built with the fused multiply-add.
hipError_t launch_icgn3d1_onepass(const Icgn3dParams& p, float* pois, int stride_floats, size_t count, hipStream_t stream);
// icgn3d_rows.hip (A/B builds only, OC_BUILD_AB; NOT the default -- the default is icgn3d.hip, oracle order OC_ORDER_LANES): the
// same solver with one half-wave per subvolume row (oracle order OC_ORDER_ROWS), measured 12 - 25 % slower; its scratch
// slots are a little larger (whole steps): icgn3d1_rows_slot_floats floats per workgroup, 512 workgroups
size_t icgn3d1_rows_slot_floats(int rx, int ry, int rz);
hipError_t launch_icgn3d1_rows(const Icgn3dParams& p, float* pois, int stride_floats, size_t count, int blocks, hipStream_t stream);

// ---- fftcc2d.hip -----------------------------------------------------------
struct Fftcc2dParams {
    const float* ref;
    const float* tar;
    int height, width;
    int rx, ry;
};
// gathers zero-mean windows of POIs [first, first+count) into ref_win/tar_win (count x (2ry*2rx)),
// writes norms[2*i], norms[2*i+1] = sum of squares, flags[i] = 1 if the bounds guard fired
hipError_t launch_fftcc2d_gather(const Fftcc2dParams& p, const float* pois, int stride_floats, size_t count,
                                 float* ref_win, float* tar_win, float* norms, int* flags, hipStream_t stream);
// zf = conj(rf) * tf over `bins` complex values
hipError_t launch_fftcc_conjmul(const float2* rf, const float2* tf, float2* zf, size_t bins, hipStream_t stream);
// arg-max of each (2ry*2rx) surface with the first-max rule, writes u,v,u0,v0,zncc into the POIs
hipError_t launch_fftcc2d_argmax(const Fftcc2dParams& p, const float* surf, const float* norms, const int* flags,
                                 float* pois, int stride_floats, size_t count, hipStream_t stream);

// The single-kernel paths of FFTCC2D: the whole FFTCC2D::compute on chip, no rocFFT, no scratch.  Which window each of them
// serves -- the lists of instantiated sides and the rule -- is host/fftcc_plan.h (fftcc2d_kernel); every launcher refuses a
// window the plan gives to another one with hipErrorInvalidValue.
// ---- fftcc2d_fusedn.hip / fftcc2d_fusedp.hip / fftcc2d_fusedr.hip -------------
// one template (fftcc2d_fusedn_impl.h), one line per lane: square windows with 5-smooth sides (Fftcc2dKernel::Smooth), square
// windows whose side has a prime factor of 7 ... 31 (Prime), rectangular windows with both sides out of a short list (Pair)
hipError_t launch_fftcc2d_fusedn(const Fftcc2dParams& p, float* pois, int stride_floats, size_t count, bool xcd,
                                 hipStream_t stream);
hipError_t launch_fftcc2d_fusedp(const Fftcc2dParams& p, float* pois, int stride_floats, size_t count, bool xcd,
                                 hipStream_t stream);
hipError_t launch_fftcc2d_fusedr(const Fftcc2dParams& p, float* pois, int stride_floats, size_t count, bool xcd,
                                 hipStream_t stream);

// ---- fftcc2d_rect.hip ------------------------------------------------------
// every OTHER rectangular window inside the plan's radius range (Rect): ONE kernel in three instantiations (fftcc2d_rect_maxn),
// the two sides are run-time values (each axis pass switches to the line transform of its length)
hipError_t launch_fftcc2d_rect(const Fftcc2dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);

// ---- fftcc2d_fused.hip -----------------------------------------------------
// 32 x 32 windows (Fused32)
// body: 3 / 4 / 5 = the A/B partners of the gfx950 instruction-count work (fftcc2d_fused.hip), anything else = the default
hipError_t launch_fftcc2d_fused(const Fftcc2dParams& p, float* pois, int stride_floats, size_t count, bool xcd,
                                hipStream_t stream, int body = 1);

// ---- fftcc3d.hip -----------------------------------------------------------
struct Fftcc3dParams {
    const float* ref;
    const float* tar;
    int dz, dy, dx;
    int rx, ry, rz;
    // locality schedule of the single-kernel paths (poi_order.hip launch_poi3d_tile_order): the k-th window of the launch
    // belongs to POI perm[k]; nullptr = queue order.  Round 5: the POIs in flight behind one L2 form a compact block of the
    // volume instead of a 1 x 1 x 32 row of the queue, so that their overlapping windows are fetched from HBM once.
    const unsigned* perm = nullptr;
};
hipError_t launch_fftcc3d_gather(const Fftcc3dParams& p, const float* pois, int stride_floats, size_t count,
                                 float* ref_win, float* tar_win, float* norms, hipStream_t stream);
hipError_t launch_fftcc3d_argmax(const Fftcc3dParams& p, const float* surf, const float* norms, float* pois,
                                 int stride_floats, size_t count, hipStream_t stream);

// The single-kernel paths of FFTCC3D, all of FFTCC3D::compute(POI3D*) in one kernel; host/fftcc_plan.h (fftcc3d_kernel) says which
// window each serves, and every launcher refuses the others' with hipErrorInvalidValue.
// ---- fftcc3d_fused.hip -----------------------------------------------------
// 32 x 32 x 32 windows (Fused32)
hipError_t launch_fftcc3d_fused(const Fftcc3dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);
#if OC_BUILD_AB
// fftcc3d_fused_r5.hip (A/B build, Fused32R5): the decomposition of rounds 1 - 5.  needs_clamped: fftcc3d_fused_flag_bytes(count) bytes of device
// scratch (its first launch flags the POIs whose windows are clamped at a volume border and raises one "any" word behind the flags,
// its second one computes those -- and returns at once when the word is 0)
size_t fftcc3d_fused_flag_bytes(size_t count);
hipError_t launch_fftcc3d_fused_r5(const Fftcc3dParams& p, float* pois, int stride_floats, size_t count, bool xcd,
                                   unsigned char* needs_clamped, hipStream_t stream);
#endif

// ---- fftcc3d_fusedn.hip ----------------------------------------------------
// small cubic windows (Cube): the complex volume stays in LDS between the axis passes
hipError_t launch_fftcc3d_fusedn(const Fftcc3dParams& p, float* pois, int stride_floats, size_t count, bool xcd,
                                 hipStream_t stream);

// ---- fftcc3d_box.hip ---------------------------------------------------------
// NON-cubic windows whose complex volume fits the LDS (Box; fftcc3d_box_lds_bytes): ONE kernel, the three sides are run-time
// values (each axis pass switches to the line transform of its length)
hipError_t launch_fftcc3d_box(const Fftcc3dParams& p, float* pois, int stride_floats, size_t count, bool xcd, hipStream_t stream);

// ---- fftcc3d_planes.hip / fftcc3d_planesb.hip -------------------------------
// large cubic windows (Planes): one persistent 512-thread workgroup per scratch slot, the complex volume passes through a private
// N^3 scratch volume between the in-LDS plane transforms and the z pass.  blocks: fftcc3d_planes_blocks, scratch:
// fftcc3d_planes_scratch_bytes
hipError_t launch_fftcc3d_planes(const Fftcc3dParams& p, float* pois, int stride_floats, size_t count, void* scratch, int blocks,
                                 hipStream_t stream);

// ---- poi_split.hip ----------------------------------------------------------
// order-preserving partition of a POI queue by result quality (oc_hip_split_reliable / oc_hip_merge_recovered)
struct PoiSplitParams {
    int mode;        // 0: reliable | unreliable | neither (first selection), 1: recovered | still unreliable (after a round)
    int rec_floats;  // 25 (POI2D) or 31 (POI3D)
    int zncc_at, conv_at;
    float zncc_low, zncc_high, conv;
};
// flag[0] <- 1 when any of the n device-resident indices is >= limit, else 0
hipError_t launch_poi_index_range(const unsigned* index, size_t n, size_t limit, unsigned* flag, hipStream_t stream);
// unsigned words of device scratch: per-block counts, then the two totals and the bad-index flag (the last three words)
size_t poi_split_scratch_words(size_t count);
// main_queue / main_count: class-0 records are also written back to main_queue[index_in[i]] -- never past main_count
// records (the flag word is raised instead)
hipError_t launch_poi_split(const float* pois, int stride_floats, size_t count, const PoiSplitParams& p, const unsigned* index_in,
                            float* out0, size_t out0_offset, unsigned* index_out0, float* out1, unsigned* index_out,
                            float* main_queue, size_t main_count, unsigned* scratch, hipStream_t stream);
// the partitions' exclusive scan on its own: block_counts[2 * b + k] -> exclusive prefix over b, in place; totals[k] = the sums
hipError_t launch_block_count_scan(unsigned* block_counts, size_t nblocks, unsigned* totals, hipStream_t stream);

// ---- match.hip --------------------------------------------------------------
// brute-force descriptor matching (SIFT3D::bruteforceMatch / monodirectionalMatch / bidirectionalMatch, src/oc_sift.cpp:625-674,
// 1251-1418, 1420-1487): squared distances as sequential float32 sums over k, the two nearest candidates of every query under
// (distance, index), the ratio test, and the two pair selections.  A partial is { bits(d0), j0, bits(d1), j1 }.
constexpr int kMatchTile = 64;       // queries per workgroup and candidates per tile
constexpr int kMatchMaxSplits = 64;
bool match_dim_supported(int dim);   // a multiple of 32 in [32, 1024]
// the candidate range cut into `splits` parts (gridDim.y); partials: splits * n_query records of 16 bytes
hipError_t launch_match_top2(const float* query, size_t n_query, const float* cand, size_t n_cand, int dim, int splits, bool fma,
                             void* partials, hipStream_t stream);
// merges the parts, applies best < ratio_sq * second, writes every entry of matched_idx (-1 = no match), best, second and adds
// the number of matches to *counter
hipError_t launch_match_finalize(const void* partials, size_t n_query, int splits, float ratio_sq, int* matched_idx, float* best,
                                 float* second, unsigned* counter, hipStream_t stream);
// mode 0 (monodirectional): keys = 2 * n_tar 64-bit slots; the two rounds of atomicMin over the accepted reference keypoints
hipError_t launch_match_many_to_one(const int* r2t, const float* best, size_t n_ref, size_t n_tar, unsigned long long* keys,
                                    hipStream_t stream);
// the surviving pairs in output order (mode 0: descending target index, mode 1: ascending reference index).  Words of scratch:
size_t match_pairs_scratch_words(size_t n_ref, size_t n_tar, int mode);
// count: per-block counts + scan, scratch's last-but-one two words are the totals (total pairs = the first of them)
hipError_t launch_match_pairs_count(int mode, const int* r2t, const int* t2r, const unsigned long long* keys, size_t n_ref, size_t n_tar,
                                    float ratio_sq, unsigned* scratch, hipStream_t stream);
hipError_t launch_match_pairs_scatter(int mode, const int* r2t, const int* t2r, const unsigned long long* keys, size_t n_ref,
                                      size_t n_tar, float ratio_sq, const unsigned* scratch, int* ref_idx, int* tar_idx,
                                      hipStream_t stream);

// ---- sift3d.hip -------------------------------------------------------------
// SIFT3D's scale space (SIFT3D::gaussianBlur, downSampling, createDogPyramid, detectExtrema; src/oc_sift.cpp:365-562, 756-847).
// Volumes are [z][y][x] float32, x contiguous.  Per blurred voxel: acc = w[0] * s[c], then r = 1 ... radius ascending
// acc = acc + w[r] * (s[lo(c - r)] + s[hi(c + r)]) (fma: fmaf(w[r], s_lo + s_hi, acc)), the mirrored index clamped into the axis.
constexpr int kSiftMaxRadius = 32;
struct SiftWeights {
    float w[kSiftMaxRadius + 1];
};
// the x pass: `rows` rows of nx floats
hipError_t launch_sift_blur_x(const float* src, float* dst, int nx, size_t rows, const SiftWeights& w, int radius, bool fma, hipStream_t stream);
// the y and z passes: the volume as [outer][n][inner], blurred along n (y: outer = nz, inner = nx; z: outer = 1, inner = ny * nx)
hipError_t launch_sift_blur_strided(const float* src, float* dst, size_t outer, int n, size_t inner, const SiftWeights& w, int radius,
                                    bool fma, hipStream_t stream);
// dst[i][j][k] = src[2i][2j][2k]; src rows of sx floats, planes of sy rows
hipError_t launch_sift_downsample(const float* src, int sx, int sy, float* dst, int dx, int dy, int dz, hipStream_t stream);
// dog = g1 - g0 over `count` voxels; *max_abs_bits (set to 0 before) becomes the bit pattern of max fabsf(dog)
hipError_t launch_sift_dog(const float* g0, const float* g1, float* dog, size_t count, unsigned* max_abs_bits, hipStream_t stream);
// One DoG layer of the extrema search: a voxel with 1 <= index <= dim - 2 on every axis is a candidate when
// fabsf(v) >= threshold and v is strictly greater, or strictly less, than its 6 face neighbours and the same voxel of the DoG
// layers below and above.  A workgroup owns kSiftExtremaVoxels consecutive voxels; first_block: its workgroups' place among
// those of all searched layers, in list order.
constexpr int kSiftExtremaVoxels = 2048;
struct SiftExtremaLayer {
    const float *below, *here, *above;
    int nx, ny, nz, octave, layer;
    float scale, threshold;
    unsigned first_block;
};
struct SiftCandidate {
    int x, y, z, octave, layer;
    float scale;
};
inline size_t sift_extrema_blocks(size_t voxels) { return (voxels + kSiftExtremaVoxels - 1) / kSiftExtremaVoxels; }
// block_counts[2 * (first_block + b)] = candidates of workgroup b (the odd words 0): what launch_block_count_scan takes
hipError_t launch_sift_extrema_count(const SiftExtremaLayer& layer, unsigned* block_counts, hipStream_t stream);
// after the scan: the candidates at out[block_offsets[2 * block] + rank in scan order]
hipError_t launch_sift_extrema_fill(const SiftExtremaLayer& layer, const unsigned* block_offsets, SiftCandidate* out, hipStream_t stream);

// ---- sift3d_features.hip ----------------------------------------------------
// SIFT3D's orientation and descriptor stages (SIFT3D::assignOrientation, constructDescriptor; src/oc_sift.cpp:849-1049, 1051-1249).
// Per-voxel terms are the reference's float32 expressions; the Gaussian weights come from the tables of
// host/sift3d_feature_plan.h; sums over voxels are 64-bit integers on the grid that header defines.
struct SiftFeatureLayer {   // one Gaussian layer; orient / describe: its weight tables ([|dz|][|dy|][|dx|], half-extents *_half)
    const float* vol;
    const float* orient;
    const float* describe;
    int dim[3], orient_half[3], describe_half[3];
    float unit[3];
    float scale, orient_radius, describe_radius, cube_radius;   // window_radius (:860), sphere_radius (:1062), cube_radius (:1063)
};
struct SiftFeatureParams {
    const SiftFeatureLayer* layers;   // device, n_octave * (n_octave_layers + 3)
    int n_octave, n_octave_layers;
    int exponent;                     // E of the grid
    float beta, gamma, gradient_threshold, truncate_threshold;
};
struct SiftKeypoint {   // oc_hip_sift3d_keypoint
    float coor_layer[3], coor_img[3];
    int octave, layer;
    float scale;
    float rotation_matrix[9];
};
constexpr int kSiftDescriptorLength = 768;
// *max_abs_bits (set to 0 before) becomes the bit pattern of max fabsf(v); a NaN or an infinity gives a pattern >= 0x7f800000
hipError_t launch_sift_max_abs(const float* v, size_t count, unsigned* max_abs_bits, hipStream_t stream);
// *flag (set to 0 before) is raised when a record names no layer a keypoint can lie in, a scale that is not that layer's, or a
// coordinate outside it (keypoints: also a non-integer or non-finite coordinate, a rotation entry that is not finite or beyond +-2)
hipError_t launch_sift_check_candidates(const SiftCandidate* list, size_t n, const SiftFeatureParams& p, unsigned* flag, hipStream_t stream);
hipError_t launch_sift_check_keypoints(const SiftKeypoint* list, size_t n, const SiftFeatureParams& p, unsigned* flag, hipStream_t stream);
// assignOrientation for n validated candidates: status[i] (0 accepted, 1 gradient threshold, 2 eigenvalues, 3 angle), sums[9 i ...]
// (d_x d_y d_z, tensor xx xy xz yy yz zz) and the keypoint record of candidate i at slots[i] (the rotation matrix only when accepted)
hipError_t launch_sift_orient(const SiftCandidate* list, size_t n, const SiftFeatureParams& p, int* status, float* sums, SiftKeypoint* slots,
                              hipStream_t stream);
// the accepted slots in candidate order: count -> launch_block_count_scan -> fill (block_counts: 2 words per 256 candidates)
inline size_t sift_orient_blocks(size_t n) { return (n + 255) / 256; }
hipError_t launch_sift_orient_count(const int* status, size_t n, unsigned* block_counts, hipStream_t stream);
hipError_t launch_sift_orient_fill(const int* status, const SiftKeypoint* slots, size_t n, const unsigned* block_offsets, SiftKeypoint* out,
                                   hipStream_t stream);
// constructDescriptor for n validated keypoints: out[768 i ...]
hipError_t launch_sift_describe(const SiftKeypoint* list, size_t n, const SiftFeatureParams& p, float* out, hipStream_t stream);

// ---- sift2d.hip -------------------------------------------------------------
// SIFT2D's detector: cv::SIFT as SIFT2D::compute() creates it (src/oc_sift.cpp:22-30, 60-93), the contract of DESIGN.md section
// 4.13.  Images are [row][col] float32.  Per blurred pixel and pass: acc = w[0] * s[c], then r = 1 ... radius ascending
// acc = acc + w[r] * (s[lo] + s[hi]), every operation rounding on its own, lo / hi by reflect-101 repeated until inside.
constexpr int kSift2dMaxRadius = 32;
// dst (2 cols x 2 rows) = the bilinear 2x upscale of src (uint8 when src_u8, else float32); *flag (set to 0 before) is raised by a
// non-finite source pixel
hipError_t launch_sift2d_upscale(const void* src, bool src_u8, int cols, int rows, float* dst, unsigned* flag, hipStream_t stream);
// rows pass: dst = src blurred along x
hipError_t launch_sift2d_blur_rows(const float* src, float* dst, int cols, int rows, const SiftWeights& w, int radius, hipStream_t stream);
// columns pass: dst = src blurred along y; with dog: dog = dst - prev at every pixel (prev: the Gaussian layer the blur started from)
hipError_t launch_sift2d_blur_cols(const float* src, float* dst, int cols, int rows, const SiftWeights& w, int radius, const float* prev, float* dog,
                                   hipStream_t stream);
// nearest-neighbour resample: dst[y][x] = src[min(floor(y * (double)src_rows / dst_rows), src_rows - 1)][the same in x]
hipError_t launch_sift2d_resample(const float* src, int src_cols, int src_rows, float* dst, int dst_cols, int dst_rows, hipStream_t stream);
// One DoG layer of the extrema scan: rows and columns in [5, size - 5); a pixel is a candidate when fabsf(v) > threshold and
// v > 0 and v >= all 26 neighbours, or v < 0 and v <= all 26.  A workgroup owns kSiftExtremaVoxels consecutive pixels;
// first_block: its workgroups' place among those of all scanned layers, in list order.
struct Sift2dExtremaLayer {
    const float *below, *here, *above;
    int cols, rows, octave, layer;   // octave counts from 0 at the doubled base
    float threshold;
    unsigned first_block;
};
struct Sift2dStart {
    int octave, layer, row, col;
};
hipError_t launch_sift2d_extrema_count(const Sift2dExtremaLayer& layer, unsigned* block_counts, hipStream_t stream);
hipError_t launch_sift2d_extrema_fill(const Sift2dExtremaLayer& layer, const unsigned* block_offsets, Sift2dStart* out, hipStream_t stream);
struct Sift2dDogLayer {   // device table, n_octave * (n_octave_layers + 2)
    const float* data;
    int cols, rows;
};
struct Sift2dKeypoint {   // oc_hip_sift2d_keypoint
    float x, y, size, response;
    int octave, layer, row, col;
    float xc, xr, xi;
    int packed_octave;
};
struct Sift2dLocalizeParams {
    const Sift2dDogLayer* dog;
    int n_octave, n_octave_layers;
    float contrast_threshold, edge_threshold, sigma;
};
// one thread per start: status[i] = 0 and slots[i] = the record when start i is located, status[i] != 0 when it is rejected
hipError_t launch_sift2d_localize(const Sift2dStart* starts, size_t n, const Sift2dLocalizeParams& p, int* status, Sift2dKeypoint* slots, hipStream_t stream);
// the located slots in start order: launch_sift_orient_count -> launch_block_count_scan -> this
hipError_t launch_sift2d_fill(const int* status, const Sift2dKeypoint* slots, size_t n, const unsigned* block_offsets, Sift2dKeypoint* out, hipStream_t stream);

}  // namespace ochip

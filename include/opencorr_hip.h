/*
 * opencorr_hip.h -- C-ABI of the MI355X-native FFTCC -> ICGN engines.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point replaces one piece of OpenCorr's host interface for the
 * hot path (citations are file:line in the OpenCorr tree).  The OpenCorr-shaped
 * C++ classes in include/opencorr_compat/ (FFTCC2D, ICGN2D1, ...) are thin
 * shims over these functions; INTEGRATION.md shows the binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - All functions return an oc_hip_status (0 = OK).  On failure
 *     oc_hip_last_error() returns a thread-local description; the C++ shim turns
 *     it into `throw std::string`, the reference's only exception type
 *     (src/oc_fftcc.cpp:145, src/oc_icgn.cpp:65, src/oc_image.cpp:43).
 *   - Per-POI failures stay in-band exactly like the reference: result.zncc is
 *     set to -3 / -4 / -5 (src/oc_dic.h:28-34) and nothing else is written.
 *     One deviation: a POI whose own coordinate (x, y or z) is NaN is rejected
 *     at the entry guard like a POI whose subset leaves the image -- -3 from
 *     ICGN2D1/2D2, ICLM2D1/2D2 and ICGN3D1 (an incoming negative or NaN zncc is
 *     kept), NR2D1's guard branch (-1, then its -4 / -5 rules), and FFTCC2D
 *     leaves the record untouched.  The reference's guard is a chain of `<` and
 *     `>` that a NaN passes, and it then indexes the images with (int)NaN, which
 *     is undefined.  +-inf and out-of-image coordinates are rejected by the guard
 *     as the reference writes it.  FFTCC3D has no guard in the reference and none
 *     here: every index is clamped per element.
 *   - POIs are passed as the reference's own AoS records, updated in place:
 *     POI2D = 25 floats / 100 B (src/oc_poi.h:102-136), POI3D = 31 floats / 124 B
 *     (src/oc_poi.h:187-222).  `stride_bytes` lets a caller embed them in a
 *     larger struct (must be a multiple of 4).
 *   - An engine lives on the device named at creation.  Every entry point makes that
 *     device current for its own duration and hands the calling thread's current
 *     device back on return.
 *   - `memory` says where a buffer lives: OC_HIP_HOST buffers are copied by the
 *     engine (pageable or pinned), OC_HIP_DEVICE buffers are used in place on the
 *     engine's device and stream (no copy).  On a stream the caller chose with
 *     oc_hip_set_stream such a call is asynchronous and stream-ordered (chain the
 *     engines of a pipeline on one stream); on the engine's own private stream it
 *     completes before it returns.  Producer ordering of OC_HIP_DEVICE inputs (queues,
 *     offsets, images used in place): on a caller-chosen stream they are read in that
 *     stream's order; on the private stream the engine first waits for everything the
 *     caller has enqueued on HIP's legacy default stream at the time of the call.  Data
 *     still being written on any OTHER stream must be complete (or that stream be named
 *     with oc_hip_set_stream) before the call.
 *   - Images are snapshotted at set_images time (like the CUDA module of the
 *     reference, examples/test_2d_dic_gpu_icgn.cpp:99-136): later edits of the
 *     host image need another set_images + prepare.
 *   - The engines never fall back to a CPU path.  If the HIP runtime, rocFFT or
 *     the device is unavailable the call fails with OC_HIP_ERR_HIP / _ROCFFT.
 */
#ifndef OPENCORR_HIP_H_
#define OPENCORR_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum oc_hip_status {
    OC_HIP_OK = 0,
    OC_HIP_ERR_INVALID = 1, /* bad argument or call order (e.g. compute before prepare) */
    OC_HIP_ERR_HIP = 2,     /* HIP runtime error (no device, launch failure, ...) */
    OC_HIP_ERR_ROCFFT = 3,  /* rocFFT plan / execute failure */
    OC_HIP_ERR_NOMEM = 4,   /* device allocation failed */
    OC_HIP_ERR_UNSUPPORTED = 5 /* subset too large for the on-chip working set */
} oc_hip_status;

typedef enum oc_hip_memory { OC_HIP_HOST = 0, OC_HIP_DEVICE = 1 } oc_hip_memory;

/* Image2D::eg_mat is an Eigen::MatrixXf, i.e. column-major (src/oc_image.h:37);
 * Img2D of the CUDA module is row-major (gpu_lib/opencorr_gpu.h:31-35). */
typedef enum oc_hip_layout { OC_HIP_ROW_MAJOR = 0, OC_HIP_COL_MAJOR = 1 } oc_hip_layout;

typedef enum oc_hip_kind {
    OC_HIP_FFTCC2D = 1,
    OC_HIP_ICGN2D1 = 2,
    OC_HIP_ICGN2D2 = 3,
    OC_HIP_FFTCC3D = 4,
    OC_HIP_ICGN3D1 = 5,
    OC_HIP_NR2D1 = 6,
    OC_HIP_ICLM2D1 = 7,
    OC_HIP_ICLM2D2 = 8,
    OC_HIP_STRAIN = 9,
    OC_HIP_REGION_FIT = 10,
    OC_HIP_CALIBRATION = 11,
    OC_HIP_STEREOVISION = 12,
    OC_HIP_MATCHER = 13,
    OC_HIP_SIFT3D = 14,
    OC_HIP_FEATURE_AFFINE = 15,
    OC_HIP_SIFT2D = 16
} oc_hip_kind;

#define OC_HIP_POI2D_BYTES 100
#define OC_HIP_POI3D_BYTES 124
/* POI2DS, the stereo record: 28 floats (src/oc_poi.h:53-60, 73-90, 140-183): x, y | u, v, w | r1r2_zncc, r1t1_zncc,
 * r1t2_zncc, r2_x, r2_y, t1_x, t1_y, t2_x, t2_y | ref_coor x, y, z | tar_coor x, y, z | exx, eyy, ezz, exy, eyz, ezx |
 * subset_radius x, y */
#define OC_HIP_POI2DS_BYTES 112
/* value of `ndim` that selects POI2DS records in oc_hip_strain_prepare / oc_hip_strain_compute (2 = POI2D, 3 = POI3D) */
#define OC_HIP_POI2DS 22

/* `what` of oc_hip_calibration_get */
typedef enum oc_hip_calibration_matrix {
    OC_HIP_CAL_INTRINSIC = 0,   /* 3 x 3 */
    OC_HIP_CAL_ROTATION = 1,    /* 3 x 3 */
    OC_HIP_CAL_TRANSLATION = 2, /* 3 */
    OC_HIP_CAL_PROJECTION = 3   /* 3 x 4 */
} oc_hip_calibration_matrix;

typedef struct oc_hip_engine oc_hip_engine; /* opaque */

/* thread-local text of the last failure on the calling thread */
const char* oc_hip_last_error(void);
/* number of visible HIP devices (0 + OC_HIP_ERR_HIP when the runtime is unusable) */
int oc_hip_device_count(int* count);
/* library / ABI version, bumped on any signature change */
int oc_hip_abi_version(void);

/* ---- construction: one per reference class ------------------------------ */
/* FFTCC2D(int subset_radius_x, int subset_radius_y, int thread_number)  src/oc_fftcc.cpp:151-163 */
int oc_hip_fftcc2d_create(int radius_x, int radius_y, int device, oc_hip_engine** out);
/* ICGN2D1(int rx, int ry, float conv_criterion, float stop_condition, int thread_number)  src/oc_icgn.cpp:71-88 */
int oc_hip_icgn2d1_create(int radius_x, int radius_y, float conv_criterion, float stop_condition, int device,
                          oc_hip_engine** out);
/* ICGN2D2(int rx, int ry, float conv, float stop, int thread_number)  src/oc_icgn.cpp:612-629 */
int oc_hip_icgn2d2_create(int radius_x, int radius_y, float conv_criterion, float stop_condition, int device,
                          oc_hip_engine** out);
/* NR2D1(int rx, int ry, float conv_criterion, float stop_condition, int thread_number)  src/oc_nr.cpp:75-91
 * (forward-additive Newton-Raphson).  prepare() = NR2D1::prepare (:119-158): target gradients and
 * three bicubic tables; compute() = NR2D1::compute(poi_queue) (:324-332).  Per-POI codes: -1 (guard), -4, -5. */
int oc_hip_nr2d1_create(int radius_x, int radius_y, float conv_criterion, float stop_condition, int device,
                        oc_hip_engine** out);
/* ICLM2D1 / ICLM2D2(int rx, int ry, float conv_criterion, float stop_condition, int thread_number)
 * src/oc_iclm.cpp:70-87, 422-439 (inverse-compositional Levenberg-Marquardt).  prepare() as for
 * ICGN2D*; compute() = ICLM2D1::compute(poi_queue) (:360-368) / ICLM2D2::compute(poi_queue) (:733-741); both honour
 * oc_hip_set_self_adaptive.  Per-POI codes: -3 (guard), -4, -5; unlike ICGN there is no abort when the warped subset
 * leaves the image (out-of-range samples take the interpolator's -1.f, src/oc_iclm.cpp:230-243). */
int oc_hip_iclm2d1_create(int radius_x, int radius_y, float conv_criterion, float stop_condition, int device,
                          oc_hip_engine** out);
int oc_hip_iclm2d2_create(int radius_x, int radius_y, float conv_criterion, float stop_condition, int device,
                          oc_hip_engine** out);
/* ICLM2D1::setDamping / ICLM2D2::setDamping(float lambda, float alpha, float beta)  src/oc_iclm.cpp:114-119, 466-471;
 * defaults 100, 0.1, 10 (struct DampingParameter, src/oc_iclm.h:33-38).  lambda must be > 0. */
int oc_hip_set_damping(oc_hip_engine* engine, float lambda, float alpha, float beta);
/* Strain(float subregion_radius, int neighbor_number_min, int thread_number)  src/oc_strain.cpp:31-46
 * (first consumer of the device-resident displacement field).  The handle supports set_stream,
 * synchronize, profile_* and destroy like the other engines; it holds no images. */
int oc_hip_strain_create(float subregion_radius, int neighbor_number_min, int device, oc_hip_engine** out);
/* setSubregionRadius / setNeighborMin / setZnccThreshold / setApproximation  src/oc_strain.cpp:72-95
 * (defaults of the constructor: threshold 0.9, approximation 1 = Cauchy; 2 = Green).  A new radius needs a new
 * oc_hip_strain_prepare. */
int oc_hip_strain_set(oc_hip_engine* engine, float subregion_radius, int neighbor_number_min, float zncc_threshold,
                      int approximation);
/* Strain::prepare(std::vector<POI2D>&) / (std::vector<POI3D>&)  src/oc_strain.cpp:96-107, 136-147: builds the
 * neighbour search over the queue's coordinates (the reference: one kd-tree per thread; here a cell-sorted order on
 * the device).  ndim 2 = POI2D records, 3 = POI3D records, OC_HIP_POI2DS = POI2DS records (Strain::prepare(std::vector<POI2DS>&)
 * :111-133: the search runs over the image coordinates x, y); layout and `memory` as for oc_hip_compute. */
int oc_hip_strain_prepare(oc_hip_engine* engine, const void* pois, size_t count, size_t stride_bytes, int ndim, int memory);
/* Strain::compute(std::vector<POI2D>&) src/oc_strain.cpp:236-247 / (std::vector<POI3D>&) :476-488.  Writes
 * strain.exx, eyy, exy (POI2D floats 20..22) or exx, eyy, ezz, exy, eyz, ezx (POI3D floats 22..27) of every POI with
 * ZNCC >= threshold that finds at least neighbor_number_min accepted neighbours; everything else is left untouched.
 * OC_HIP_POI2DS: Strain::compute(std::vector<POI2DS>&) :357-370 (-> :250-355): a POI takes part, as itself and as a
 * neighbour, when r1r2_zncc, r1t1_zncc and r1t2_zncc all reach the threshold; the fit runs over ref_coor differences with
 * u, v, w as right-hand sides and writes the six strains (floats 20..25).
 * The queue must be the one prepare() saw (same length and coordinates). */
int oc_hip_strain_compute(oc_hip_engine* engine, void* pois, size_t count, size_t stride_bytes, int ndim, int memory);
/* RegionFit2D / RegionFit3D(float neighbor_search_radius, int neighbor_number_min, int thread_number)
 * src/oc_region_fit.cpp:32-46, 189-203: re-initialises POIs from the plane fitted through the
 * reliable POIs around them, before they are handed to ICGN again. */
int oc_hip_region_fit_create(float neighbor_search_radius, int neighbor_number_min, int device, oc_hip_engine** out);
/* setSearchRadius / setNeighborMin  src/oc_region_fit.cpp:65-73, 222-230.  A new radius needs a new prepare. */
int oc_hip_region_fit_set(oc_hip_engine* engine, float neighbor_search_radius, int neighbor_number_min);
/* setNeighbor(reliable_pois) + prepare()  src/oc_region_fit.cpp:75-92, 232-249: neighbour search over the reliable
 * POIs' coordinates.  Their displacements are snapshotted here (the reference keeps a pointer and reads them during
 * compute; editing the reliable queue between prepare and compute needs a new prepare). */
int oc_hip_region_fit_prepare(oc_hip_engine* engine, const void* reliable_pois, size_t count, size_t stride_bytes, int ndim,
                              int memory);
/* RegionFit2D::compute(std::vector<POI2D>&) src/oc_region_fit.cpp:166-174 (-> :94-164) / RegionFit3D :334-342
 * (-> :251-332): every POI that finds at least neighbor_number_min reliable POIs (inside the radius, else the K
 * nearest) gets deformation.{u,ux,uy,v,vx,vy} (POI3D: all twelve) from the fitted plane and result.zncc = 0; other
 * POIs and all other fields are left untouched. */
int oc_hip_region_fit_compute(oc_hip_engine* engine, void* pois, size_t count, size_t stride_bytes, int ndim, int memory);
/* Candidate batching for callers like EpipolarSearch::compute(POI2D*) (src/oc_epipolar_search.cpp:133-195): the
 * reference refines a few trial positions per POI with icgn1->compute(&candidate) one at a time and keeps the one
 * with the highest ZNCC (:181-190).  Here the trials of all POIs are ONE queue for oc_hip_compute, and this call
 * does the selection: candidates segment_starts[s] .. segment_starts[s+1]-1 belong to POI s (n_segments + 1 offsets,
 * uint32, same memory space as the queues); the winner's deformation and result vectors are copied into POI s
 * (poi->deformation = best.deformation; poi->result = best.result), nothing else is touched; highest ZNCC wins, the
 * earliest candidate among equals, NaN never; an empty segment leaves its POI as it was.  POI2D records; any 2D
 * engine handle supplies the device and stream. */
int oc_hip_select_best(oc_hip_engine* engine, const void* candidates, size_t n_candidates, size_t candidate_stride_bytes,
                       const unsigned* segment_starts, size_t n_segments, void* pois, size_t stride_bytes, int memory);
/* ---- stereo DIC: Calibration, Stereovision --------------------------------------------------------------------
 * Handles of these two kinds are created by host arithmetic alone (no device is touched until prepare / maps / undistort /
 * reconstruct), support set_stream, reset_stream, synchronize, get_kind and destroy like the others, and hold no images.
 *
 * Calibration(CameraIntrinsics&, CameraExtrinsics&)  src/oc_calibration.cpp:27-32 -> updateCalibration :87-93 ->
 * updateMatrices :79-85.  intrinsics = cam_i (fx, fy, fs, cx, cy, k1 ... k6, p1, p2), extrinsics = cam_e (tx, ty, tz, rx, ry,
 * rz), src/oc_calibration.h:25-45.  The four matrices are float32 host code: updateIntrinsicMatrix :36-48 (an intrinsic
 * matrix equal to the identity -- "Null intrinsics matrix", :44-47 -- fails with OC_HIP_ERR_INVALID), updateRotationMatrix
 * :50-60 (Eigen's AngleAxisf::toRotationMatrix for angle |r| about r / |r|; the zero vector gives the exact identity,
 * handled explicitly), updateTranslationVector :62-67, updateProjectionMatrix :69-77 (K * [R | t], inner index ascending). */
int oc_hip_calibration_create(const float intrinsics[13], const float extrinsics[6], int device, oc_hip_engine** out);
/* Calibration::setUndistortion(float convergence, int iteration)  src/oc_calibration.cpp:111-115; defaults 0.001, 40 (:21-25) */
int oc_hip_calibration_set_undistortion(oc_hip_engine* engine, float convergence, int iteration);
/* Calibration::prepare(int height, int width)  src/oc_calibration.cpp:161-219: the map of undistorted image coordinates
 * of every pixel, one thread per pixel, kept on the device.  Completes before it returns.  height, width >= 2. */
int oc_hip_calibration_prepare(oc_hip_engine* engine, int height, int width);
/* intrinsic_matrix (9), rotation_matrix (9), translation_vector (3), projection_matrix (12) of
 * src/oc_calibration.h:53-56, row-major; `what` is an oc_hip_calibration_matrix */
int oc_hip_calibration_get(const oc_hip_engine* engine, int what, float* out);
/* map_x / map_y of src/oc_calibration.h:62-63 after prepare, height * width floats each, row-major, copied to the caller's
 * buffers (`memory` says where they live; either pointer may be null) */
int oc_hip_calibration_maps(oc_hip_engine* engine, float* map_x, float* map_y, int memory);
/* Calibration::undistort(Point2D&)  src/oc_calibration.cpp:221-264 for `count` points: (x, y) pairs `stride_bytes` apart in
 * `in` -> undistorted sensor coordinates at the same positions of `out` (which may be `in`).  The input is not clamped
 * in place (the reference clamps its argument); a NaN coordinate gives a NaN pair. */
int oc_hip_calibration_undistort(oc_hip_engine* engine, const void* in, void* out, size_t count, size_t stride_bytes, int memory);
/* Stereovision(Calibration* view1_cam, Calibration* view2_cam, int thread_number)  src/oc_stereovision.cpp:21-26 +
 * prepare() :56-68.  Both cameras must outlive the handle (the reference keeps the pointers too) and name the same
 * device, which becomes the handle's. */
int oc_hip_stereo_create(oc_hip_engine* view1_cam, oc_hip_engine* view2_cam, oc_hip_engine** out);
/* Stereovision::updateFundementalMatrix()  src/oc_stereovision.cpp:36-54, row-major 3 x 3, recomputed from the cameras'
 * present matrices at every call: the 3 x 3 inverses as cofactors over the determinant, the products with ascending inner
 * index, left to right */
int oc_hip_stereo_fundamental(oc_hip_engine* engine, float out[9]);
/* Stereovision::reconstruct(std::vector<Point2D>&, std::vector<Point2D>&, std::vector<Point3D>&)
 * src/oc_stereovision.cpp:126-133 (-> :70-124): (x, y) pairs of view 1 and view 2, (x, y, z) out, each queue with its own
 * stride in bytes.  A NaN among the four inputs gives (0, 0, 0).  The 4 x 3 system is built in float32 as written and solved
 * in double, rounded once (the reference: Eigen's float32 colPivHouseholderQr).  Both cameras must be prepared. */
int oc_hip_stereo_reconstruct(oc_hip_engine* engine, const void* view1_points, size_t stride1_bytes, const void* view2_points,
                              size_t stride2_bytes, void* points3d, size_t stride_out_bytes, size_t count, int memory);
/* The host loops of examples/test_3d_dic_epipolar_sift.cpp:303-317 as one launch over a POI2DS queue: ref_coor =
 * reconstruct((x, y), (r2_x, r2_y)), tar_coor = reconstruct((t1_x, t1_y), (t2_x, t2_y)), deformation = tar_coor - ref_coor;
 * nothing else of a record is written. */
int oc_hip_stereo_reconstruct_pois(oc_hip_engine* engine, void* pois2ds, size_t count, size_t stride_bytes, int memory);

/* The two selections of the RegionFit -> re-ICGN loop (examples/test_3d_reconstruction_sift_icgn2_regfit.cpp:214-260), as
 * order-preserving partitions ON THE DEVICE, so that a queue resident in HBM never travels to the host between ICGN,
 * RegionFit and the next ICGN pass.  Any engine handle supplies the device and the stream; ndim = 2 (POI2D) / 3 (POI3D);
 * all queues share `stride_bytes`; the counts come back to the host (the call completes before it returns).
 *
 * oc_hip_split_reliable: for every POI of `pois` in queue order (:216-229)
 *     result.zncc < zncc_threshold_low || result.convergence > conv_criterion  -> appended to `unreliable`, its queue index to
 *                                                                                 `unreliable_index`
 *     else result.zncc >= zncc_threshold_high                                  -> appended to `reliable` (from record
 *                                                                                 `reliable_offset` on)
 *   (the example's own float comparisons: a NaN makes all of them false, the POI goes to neither set).  The caller's
 *   buffers hold up to `count` records (reliable: reliable_offset + count). */
int oc_hip_split_reliable(oc_hip_engine* engine, const void* pois, size_t count, size_t stride_bytes, int ndim,
                          float zncc_threshold_low, float zncc_threshold_high, float conv_criterion, void* reliable,
                          size_t reliable_offset, void* unreliable, unsigned* unreliable_index, size_t* n_reliable,
                          size_t* n_unreliable, int memory);
/* oc_hip_merge_recovered: after RegionFit + ICGN over `unreliable` (:236-256): every POI with result.zncc >=
 * zncc_threshold_high && result.convergence <= conv_criterion is written back to pois[unreliable_index[j]] and appended to
 * `reliable` (from record `reliable_offset` on); the others are moved to the front of `unreliable` / `unreliable_index`
 * in their old order.  (The example erases inside its loop and thereby skips the POI after every success for one round;
 * here every POI is looked at in every round.)  `count` = records in `pois`: an unreliable_index entry >= count is never
 * written through -- the call fails with OC_HIP_ERR_INVALID (HOST: before anything is touched; DEVICE: the offending
 * records are not written back, `unreliable` / `unreliable_index` are left as they were).  On both paths only the
 * record's own bytes are written: with stride_bytes > the record size the caller's bytes between records are kept. */
int oc_hip_merge_recovered(oc_hip_engine* engine, void* pois, size_t count, size_t stride_bytes, int ndim, void* unreliable,
                           unsigned* unreliable_index, size_t n_unreliable, float zncc_threshold_high, float conv_criterion,
                           void* reliable, size_t reliable_offset, size_t* n_recovered, size_t* n_remaining, int memory);
/* FFTCC3D(int rx, int ry, int rz, int thread_number)  src/oc_fftcc.cpp:300-313 */
int oc_hip_fftcc3d_create(int radius_x, int radius_y, int radius_z, int device, oc_hip_engine** out);
/* ICGN3D1(int rx, int ry, int rz, float conv, float stop, int thread_number)  src/oc_icgn.cpp:1197-1213 */
int oc_hip_icgn3d1_create(int radius_x, int radius_y, int radius_z, float conv_criterion, float stop_condition,
                          int device, oc_hip_engine** out);
/* ~FFTCC2D / ~ICGN2D1 ...  src/oc_fftcc.cpp:165-173, src/oc_icgn.cpp:90-101 */
int oc_hip_destroy(oc_hip_engine* engine);

/* ---- configuration ------------------------------------------------------- */
/* DIC::setImages(Image2D&, Image2D&)  src/oc_dic.cpp:22-26 (pointer stored there; snapshotted here) */
int oc_hip_set_images2d(oc_hip_engine* engine, const float* ref, const float* tar, int height, int width,
                        int layout, int memory);
/* DVC::setImages(Image3D&, Image3D&)  src/oc_dic.cpp:45-49; data = &vol_mat[0][0][0] (z,y,x contiguous) */
int oc_hip_set_images3d(oc_hip_engine* engine, const float* ref, const float* tar, int dim_x, int dim_y, int dim_z,
                        int memory);
/* Reuse the device-resident images of another engine on the same device (an
 * FFTCC and an ICGN engine working on one image pair upload it once).  The
 * donor must outlive the borrower or call set_images again. */
int oc_hip_share_images(oc_hip_engine* engine, oc_hip_engine* donor);
/* DIC::setSubset / DVC::setSubset  src/oc_dic.cpp:28-32,51-56 (radius_z ignored by 2D engines) */
int oc_hip_set_subset(oc_hip_engine* engine, int radius_x, int radius_y, int radius_z);
/* ICGN2D1::setIteration(float, float)  src/oc_icgn.cpp:103-107 (also 2D2 :644-648, 3D1 :1228-1232) */
int oc_hip_set_iteration(oc_hip_engine* engine, float conv_criterion, float stop_condition);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the engine's own stream.  The handle is used as given: NULL is HIP's default
 * (null) stream, which is what torch.cuda.current_stream().cuda_stream returns
 * for torch's default stream.  The new stream is ordered behind the work already
 * enqueued on the stream in use so far (prepare()'s kernels, say) ON THE DEVICE --
 * an event, no host-side wait -- so switching never blocks and never races.  The
 * outgoing stream may already have been destroyed by its owner (destroy, then
 * set_stream(other) is a valid sequence): a dead stream has nothing left to order
 * behind, the new one is installed regardless.  Fails only if the NEW handle is
 * unusable. */
int oc_hip_set_stream(oc_hip_engine* engine, void* hip_stream);
/* Go back to the engine's own (non-blocking) stream; ordered like set_stream, always succeeds. */
int oc_hip_reset_stream(oc_hip_engine* engine);

/* ---- device groups: one engine, several GPUs of the node -------------------------------
 * The loop being replaced is the reference's per-POI loop, src/oc_icgn.cpp:343-351 (`#pragma omp parallel for` over
 * poi_queue): every POI is independent, so member g of the group takes the contiguous block
 * [g * ceil(n / G), (g + 1) * ceil(n / G)) of the queue.  device_ids[0] is where the engine itself lives (it moves
 * there if necessary: images must then be set again); for each further id a full engine of the same kind and
 * settings is created on that device.  From then on every call on the handle fans out: setters, set_images (host
 * images are uploaded by every member, device images are copied peer to peer), prepare (every member builds its own
 * gradients / tables: cheaper than moving 64 B per pixel over xGMI) and compute:
 *   - OC_HIP_HOST queues: every member moves and solves its own block from its own host thread; results land in the
 *     caller's vector, no exchange is needed.
 *   - OC_HIP_DEVICE queues (resident on device_ids[0]): members pull their block over xGMI (hipMemcpyPeerAsync),
 *     solve it and push the records back; stream-ordered like a single-device call.  With the tuning key
 *     "group_allgather" = 1 every member additionally ends up with the COMPLETE result queue in its own mirror
 *     (oc_hip_group_queue) -- one ncclAllGather (RCCL) of equal, padded blocks when the members sit on distinct
 *     devices -- for consumers that run on every GPU (Strain / RegionFit per device).
 * Results are bit-identical for every group size (a POI's arithmetic does not depend on the block it travels in).
 * A device may be named more than once (two members on one GPU): only useful to exercise the sharding on a one-GPU
 * machine.  n_devices = 1 dissolves a group.  Strain / RegionFit engines stay on one device. */
int oc_hip_set_devices(oc_hip_engine* engine, const int* device_ids, int n_devices);
/* members of the group (1 for a plain engine); device_ids may be NULL */
int oc_hip_get_devices(const oc_hip_engine* engine, int* device_ids, int capacity, int* n_devices);
/* after a DEVICE-queue compute with "group_allgather" = 1: member `member`'s copy of the whole queue on ITS device --
 * G blocks of block_bytes (ceil(n / G) records; the last block padded), valid once the engine's stream has been
 * synchronised */
int oc_hip_group_queue(const oc_hip_engine* engine, int member, const void** device_ptr, size_t* block_bytes);

/* Knobs.  Every key but "arith_fma", "arith_onepass" and "arith_onepass3d" selects among kernels that compute BIT-IDENTICAL results; unknown keys and values
 * outside a key's range fail with OC_HIP_ERR_INVALID; values this build does not contain, and non-zero values on an engine kind
 * the key does not belong to, with OC_HIP_ERR_UNSUPPORTED.  The default of every key, its range, the engine kinds that may set
 * it and the values only the A/B build of the library accepts are stated ONCE, as a table: opencorr_amd/csrc/host/engine_tuning.h
 * (the initialisers of EngineTuning, the rows of kTuningKeys).  What the keys do:
 *   "arith_fma"       ICGN2D1 / ICGN2D2 / ICLM2D1 / ICLM2D2 / ICGN3D1 only (and the descriptor matcher and the SIFT3D scale space, see there).  0: every
 *                     multiply and add of the solver rounds on its own -- the reference built for baseline x86-64; GPU ==
 *                     oracle OC_ORDER_LANES bit for bit.  1: every PER-SAMPLE multiply-add is one fused multiply-add -- what a
 *                     compiler with FMA hardware makes of the reference's source expressions (src/oc_cubic_bspline.cpp:159-177,
 *                     390-401; src/oc_icgn.cpp:198-205, 266-276, 1314-1445; the reference's build files fix no contraction
 *                     mode); GPU == oracle OC_ORDER_LANES_FMA bit for bit.  Results of the two modes differ by rounding only:
 *                     against the reference's separately rounded loop order both keep identical failure flags, >= 99.5 %
 *                     identical iteration counts, |d u, v, w| <= 1e-4 and |d ZNCC| <= 1e-5 (all BASELINE configs:
 *                     tests/test_gpu_fullsize.py).  Kernel time on one MI355X: ICGN2D1 -3 ... -9 %, ICGN2D2 -13 ... -17 %,
 *                     ICGN3D1 -5 ... -7 %.  The once-per-POI dense algebra is never fused
 *   "arith_onepass"   ICGN2D1 / ICGN2D2 only.  0:
 *                     the contract "arith_fma" selects.  1: the ONE-PASS arithmetic contract (icgn2d_onepass.hip) -- an iteration is
 *                     one sweep over the warped subset with 3 + DOF running sums of e' = g (t - c) - r~ (c, g: mean and scale of the
 *                     previous iteration) and no target array; mean, norm, ZNSSD and the numerator are recovered from the sums
 *                     (DESIGN.md section 3).  The set-up and every per-sample multiply-add are the fused contract's; under 1 the
 *                     value of "arith_fma" does not matter.  NOT bit-identical to the other two contracts: GPU ==
 *                     tests/cpp/icgn2d_onepass_twin.cpp (its CPU restatement) bit for bit, and against the reference's separately
 *                     rounded loop order the same bars as "arith_fma" -- identical failure codes, >= 99.5 % identical iteration
 *                     counts, |d u, v| <= 1e-4 (whole queues of configs B and C: >= 99.99 % of the POIs, none beyond 2e-4) and
 *                     |d ZNCC| <= 1e-5; the golden OHT table and the float64 model of ICGN2D2 within their committed bars
 *                     (tests/test_gpu_arith_onepass.py, tests/test_gpu_fullsize_onepass.py).  Host and device queues, device
 *                     groups, oc_hip_compute_chain and oc_hip_compute_one work as under the other contracts.  NOT supported under
 *                     1: centre offsets (oc_hip_compute_with_offsets, oc_hip_compute_one_with_offset) and self-adaptive radii --
 *                     both fail with OC_HIP_ERR_UNSUPPORTED, they never run another contract -- and the set-up cache, which is
 *                     simply not used (oc_hip_icgn2d_setup_cache_last reports "none").  Measured compute() time on one MI355X
 *                     against "arith_fma" = 1 computing its set-up (tools/onepass_ab.py, profiles/r7a_onepass_ab_config_*.json):
 *                     SLOWER -- ICGN2D1 on config B 3.39 against 3.16 ms (x 1.07), ICGN2D2 on config C 3.66 against 3.17 ms
 *                     (x 1.15); against "arith_fma" = 1 as it ships, i.e. served by the set-up cache on repeated calls over one
 *                     reference, x 1.18 and x 1.41.  The contract is an option kept for its arithmetic, not a faster path
 *   "arith_onepass3d" ICGN3D1 only (which in turn refuses "arith_onepass" = 1 and names this key).  0: the contract "arith_fma" selects.  1: the ONE-PASS
 *                     arithmetic contract carried to DVC (icgn3d_onepass.hip) -- the tap sweep of an iteration forms, per sample,
 *                     e' = g (t - c) - r~ and adds it to 3 + 12 running sums; no warped sample is stored, no scratch is reserved,
 *                     and mean, norm, ZNSSD and the numerator are recovered from the sums after ONE block reduction (DESIGN.md
 *                     section 3).  The set-up and every per-sample multiply-add are the fused contract's; under 1 the value of
 *                     "arith_fma" does not matter.  NOT bit-identical to the other two contracts: GPU ==
 *                     tests/cpp/icgn3d_onepass_twin.cpp (its CPU restatement, 512-lane association) bit for bit, and against the
 *                     reference's separately rounded loop order the same bars as "arith_fma" -- identical failure codes,
 *                     >= 99.5 % identical iteration counts, |d u, v, w| <= 1e-4 and |d ZNCC| <= 1e-5; the float64 model of the
 *                     3D iteration within its committed bars (tests/test_onepass3d_twin_cpu.py,
 *                     tests/test_gpu_arith_onepass3d.py).  Host and device queues, device groups, oc_hip_compute_chain,
 *                     oc_hip_compute_one and "icgn3d_tile_vox" work as under the other contracts; the A/B build's
 *                     "icgn3d_mapping" = 1 together with this key fails with OC_HIP_ERR_UNSUPPORTED.  NOT RUN ON AN MI355X YET:
 *                     neither the kernel's bits nor its time have been measured (tools/onepass3d_ab.py)
 *   "icgn2d_variant"  launch shape of the ICGN2D kernel (gather depth, LDS footprint, per-workgroup coordinate table, waves per
 *                     workgroup); -1 lets the engine choose: 5 / 4 (6 / 12 DoF: coordinate table, lockstep sweeps,
 *                     8-wave workgroups) for queues >= 32768 POIs of subsets up to 35 x 34 / 41 x 41, 2 / 3 (no table) below,
 *                     7 (target array only) for self-adaptive subsets from 27 passes up (2 / 3 below), 1 (single-wave
 *                     workgroups) for what fits nothing else.  10 / 11 (6 / 12 DoF): the lockstep sweeps in 4-WAVE workgroups, six /
 *                     four per CU, on a coordinate table of 6 instead of 12 bytes per sample (byte offset, 8-bit column and
 *                     row); both use the set-up cache.  They apply to launches with one radius pair (no self-adaptive radii, no
 *                     IC-LM), subsets of at most 256 x 256 whose six / four workgroups fit a CU's LDS (19 / 28 passes of 64
 *                     samples: 35 x 34 / 41 x 41); any other launch takes the automatic choice instead, with the same bits.
 *                     For queues >= 32768 POIs the automatic choice takes them in place of 5 / 4 wherever they apply.  0, 6, 8 (the split launch shape) and 9 (the workgroup's
 *                     coefficient band staged in LDS, icgn2d_band.hip) are measured losers that only the A/B build of the
 *                     library contains
 *   "icgn2d_xcd"      1: workgroups of one XCD serve a contiguous range of the POI queue
 *   "icgn2d_tile_px"  side of the square image tiles the ICGN2D / NR2D1 queue is visited by (L1 / L2 locality; 0 = queue order;
 *                     applied to queues >= 16384 POIs)
 *   "icgn2d_setup_cache"  1: ICGN2D1 / ICGN2D2 keep the per-POI set-up of their big-queue launches (variants 10 / 11, 5 / 4) --
 *                     reference mean, norm and inverse Hessian: 152 + 8 B per POI at 6 DoF, 584 + 8 B at 12 -- from one compute()
 *                     to the next and start from it while reference, gradients, radii, arithmetic, count, stride and the
 *                     queue's (x, y) stay what they were: the sequence "overwrite the target in place, prepare_tar(), compute()"
 *                     pays for the set-up once.  set_images / share_images / prepare_ref and any change of those settings make
 *                     the next call rebuild it; the coordinates are compared on the device, no call waits for the host.
 *                     Centre offsets, self-adaptive radii, IC-LM and smaller queues never use it.  0: every call computes its
 *                     set-up.  Same bits either way (oc_hip_icgn2d_setup_cache_last tells which way a call went)
 *   "icgn2d_int_first"  1: while the warp of an ICGN2D1 / ICGN2D2 POI is an INTEGER TRANSLATION -- integral x, y, u, v and
 *                     zero gradients: the first iteration of every FFTCC2D guess -- the interpolation sweep reads each sample's
 *                     value from a value plane that prepare() / prepare_tar() store behind the coefficient table (the
 *                     interpolant at every pixel's own position, evaluated by the sweep's own polynomial code at zero
 *                     fractions: 4 B per pixel on top of the table's 64, field "lut_val" of oc_hip_get_field) instead of
 *                     gathering 16 coefficients and evaluating 15 products with zero.  Every other sweep, centre offsets,
 *                     self-adaptive radii, IC-LM and the one-pass contract are untouched.  0: every sweep is the full one
 *                     (the behaviour before the plane existed).  Same bits either way, NaN / Inf pixels included
 *                     (tests/test_gpu_int_first.py); the key exists for that comparison and for measurements
 *   "icgn2d_split_chunks"  A/B build, variant 8 only: chunks of the two-stream pipeline (0 = the two kernels back to back)
 *   "fftcc2d_fused"   1: single-kernel FFTCC2D (register / LDS FFT) for EVERY window with both radii in 4 ... 32 (even
 *                     sides 8 ... 64): a template instance per square side and for the 42 rectangular pairs (radius_x !=
 *                     radius_y) out of sides 16, 20, 24, 32, 40, 48, 64, one kernel with run-time sides (fftcc2d_rect.hip) for
 *                     every other rectangular pair; larger windows run the rocFFT pipeline.  0: rocFFT pipeline always.  2: as
 *                     1, but 32 x 32 windows run the generic NR x NC kernel instead of their own (an A/B switch).  3: as 1, but
 *                     the 32 x 32 kernel runs its body without the scalar row stepping of integral POIs and with a full complex
 *                     last inverse pass (the kernel before those two changes); 4 / 5: with the first / the second of the two
 *                     alone (A/B switches: same integers, ZNCC of 3 and 4 bit-identical)
 *   "fftcc3d_fused"   1: single-kernel FFTCC3D for every cubic window of even side 8 ... 64 (radius 4 ... 32): LDS kernel
 *                     up to 26^3, register kernel at 32^3, plane-wise kernel for 28^3 ... 64^3; and for every NON-cubic window
 *                     with all three radii in 4 ... 16 whose complex volume [2rx][2ry][2rz + 1] fits 160 KB of LDS (one kernel,
 *                     sides as run-time values: fftcc3d_box.hip); other non-cubic windows and larger sides run the rocFFT
 *                     pipeline.  0: rocFFT pipeline always.  2 (A/B build of the library only): as 1, but 32^3 windows run the
 *                     kernel of rounds 1 - 5 (fftcc3d_fused_r5.hip: same integers, ZNCC within 1e-6, 1.45 x the time)
 *   "fftcc3d_planes_blocks"  persistent workgroups (= private scratch volumes) of the plane-wise FFTCC3D kernel; 0 = 256 of them
 *   "fftcc3d_tile_vox"  FFTCC3D single-kernel paths: queues >= 2048 POIs are visited in cubic blocks of this many voxels (0 = queue order)
 *   "icgn3d_tile_vox" the same for ICGN3D1
 *   "icgn3d_mapping"  0: sample s of a subvolume is owned by thread
 *                     s mod 512 (icgn3d.hip; oracle OC_ORDER_LANES, lanes = 512); 1 (A/B build): one half-wave per subvolume row
 *                     (oracle OC_ORDER_ROWS; 12 - 25 % slower; no fused-arithmetic form)
 *   "single_combine"  1: concurrent compute_one calls on an engine are combined into one launch per batch; 0: every
 *                     call is a launch of its own (the behaviour up to round 5).  Same bits either way.
 *   "host_chunk"      POIs per chunk of the host-queue pipeline (copies of one chunk overlap the kernels of its
 *                     neighbours); 0 = whole queue at once
 *   "group_allgather" 1: device groups leave the complete result queue on every member (see oc_hip_set_devices)
 *   "group_force_rccl" 1 (with "group_allgather"): an engine WITHOUT a group sends its DEVICE queues down the group path
 *                     as a group of one, whose all-gather is an ncclAllGather on a one-rank communicator (queue ->
 *                     oc_hip_group_queue(engine, 0)); fails instead of falling back when librccl is unusable.  Exists
 *                     so that the RCCL binding (dlopen, version check, ncclCommInitAll, ncclAllGather) can be executed
 *                     on a one-GPU machine
 *   "match_splits"    descriptor matcher only: parts the candidate range of the distance kernel is cut into; 0 = automatic
 *                     (enough parts for two workgroups per CU), else that many.  Same bits for every value.  The
 *                     matcher also takes "arith_fma" (see oc_hip_matcher_create); every other engine refuses this key with
 *                     OC_HIP_ERR_UNSUPPORTED
 * A device group (oc_hip_set_devices) hands every key on to its members. */
int oc_hip_set_tuning(oc_hip_engine* engine, const char* key, int value);

/* ---- precompute ----------------------------------------------------------- */
/* ICGN2D1::prepare()  src/oc_icgn.cpp:138-142 (prepareRef + prepareTar); FFTCC::prepare() is a no-op
 * in the reference (src/oc_fftcc.cpp:175) and here. */
int oc_hip_prepare(oc_hip_engine* engine);
/* ICGN2D1::prepareRef()  src/oc_icgn.cpp:115-125: reference gradients (Gradient2D4 / Gradient3D4) */
int oc_hip_prepare_ref(oc_hip_engine* engine);
/* ICGN2D1::prepareTar()  src/oc_icgn.cpp:127-136: target B-spline coefficients */
int oc_hip_prepare_tar(oc_hip_engine* engine);

/* ---- compute --------------------------------------------------------------- */
/* FFTCC2D::compute(std::vector<POI2D>&)  src/oc_fftcc.cpp:277-285
 * ICGN2D1::compute(std::vector<POI2D>&)  src/oc_icgn.cpp:343-351   (2D2 :900-908, 3D1 :1492-1500,
 * FFTCC3D :429-436).  `pois` = poi_queue.data(), `count` = poi_queue.size().
 * With OC_HIP_HOST the call returns after the results are back in `pois` (the queue travels in chunks: H2D, kernels
 * and D2H of neighbouring chunks overlap); with OC_HIP_DEVICE it only enqueues work on the engine's stream. */
int oc_hip_compute(oc_hip_engine* engine, void* pois, size_t count, size_t stride_bytes, int memory);
/* Several engines over ONE queue, in the given order -- what examples/test_2d_dic_fftcc_icgn1.cpp:80-99 does with two
 * calls (fftcc2d->compute(poi_queue); icgn2d1->compute(poi_queue);) as ONE: an OC_HIP_HOST queue then crosses PCIe once
 * in each direction instead of once per engine (per chunk: one copy in, every engine's kernels, one copy out; config B:
 * two crossings of the 25 MB AoS instead of four).  Results are bit-identical to the separate calls.  All engines live
 * on one device and take the same record type (POI2D or POI3D); for the duration of the call they run on engines[0]'s
 * stream (device-ordered behind whatever their own streams still hold, and handed back afterwards).  Centre offsets,
 * device groups and Strain / RegionFit are not part of a chain. */
int oc_hip_compute_chain(oc_hip_engine* const* engines, int n_engines, void* pois, size_t count, size_t stride_bytes, int memory);
/* FFTCC2D::compute(POI2D*) / ICGN2D1::compute(POI2D*)  src/oc_fftcc.cpp:177, src/oc_icgn.cpp:144: safe to call from the
 * caller's own OpenMP region (src/oc_epipolar_search.cpp:184-188; the reference keeps one scratch instance per thread,
 * src/oc_icgn.cpp:61-69,147).  Calls that arrive while a launch is in flight are COMBINED: they queue up, one of the waiting
 * threads hands the whole batch to the engine as one queue and every caller returns with its own record filled in -- T
 * concurrent threads cost one launch per ~T POIs.  A POI's result does not depend on the batch it travels in.  A strictly
 * sequential caller still pays a launch and two PCIe copies per POI.  Tuning key "single_combine" = 0 restores one launch per
 * call. */
int oc_hip_compute_one(oc_hip_engine* engine, void* poi);
/* batches / POIs served by the combining front end of compute_one on this engine so far (either pointer may be null) */
int oc_hip_single_stats(oc_hip_engine* engine, unsigned long long* batches, unsigned long long* pois);
/* ICGN2D1::compute(std::vector<POI2D>&, std::vector<Point2D>& center_offset_queue)  src/oc_icgn.cpp:549-557
 * (ICGN2D2 :1128-1136): local subset coordinates are shifted by center_offsets[i] = {x, y} (two floats per POI,
 * the reference's Point2D) and the target subset is centred at POI + offset.  The offsets live in the same
 * memory space as the POIs. */
int oc_hip_compute_with_offsets(oc_hip_engine* engine, void* pois, const float* center_offsets, size_t count,
                                size_t stride_bytes, int memory);
/* ICGN2D1::compute(POI2D*, Point2D& center_offset)  src/oc_icgn.cpp:353 (ICGN2D2 :910) */
int oc_hip_compute_one_with_offset(oc_hip_engine* engine, void* poi, const float* center_offset);
/* DIC::setSelfAdaptive(bool)  src/oc_dic.cpp:34-37: when on, ICGN2D1/2D2 take the subset radius of every POI from
 * poi->subset_radius instead of the engine's (src/oc_icgn.cpp:152-158, 697-703) */
int oc_hip_set_self_adaptive(oc_hip_engine* engine, int enable);
/* wait for everything enqueued on the engine's stream */
int oc_hip_synchronize(oc_hip_engine* engine);

/* ---- descriptor matching (SIFT3D's brute-force keypoint matching) --------- */
/* The matching stage of SIFT3D::compute (src/oc_sift.cpp:625-674, 1251-1418, 1420-1487) for descriptors computed anywhere:
 * rows of `dim` float32 (the reference's SIFT3D: 768; OpenCV's SIFT: 128).  `dim` is fixed at creation and must be a
 * multiple of 32 in [32, 1024] (anything else: OC_HIP_ERR_INVALID).  The squared distance of a pair is the sequential
 * float32 sum of :643-648 (acc = acc + d * d over k ascending; fmaf(d, d, acc) under oc_hip_set_tuning("arith_fma", 1)), so
 * every result equals the reference's loop bit for bit.  The handle supports set_stream, synchronize, profile_* (the
 * distance kernel), set_tuning ("arith_fma", "match_splits": 0 = automatic, 1 ... 64 = the number of parts the candidate
 * range is cut into; results do not depend on it) and destroy.  Not supported (OC_HIP_ERR_UNSUPPORTED): oc_hip_set_devices
 * with more than one device, oc_hip_compute*, oc_hip_set_images*.
 * matching_ratio = SIFT3D::matching_ratio (:629); must be >= 0 and finite. */
int oc_hip_matcher_create(int dim, float matching_ratio, int device, oc_hip_engine** out);
/* SIFT3D::setMatchingRatio(float matching_ratio)  src/oc_sift.cpp:204-207 (default 0.85, :154) */
int oc_hip_matcher_set_ratio(oc_hip_engine* engine, float matching_ratio);
/* descriptor1 / descriptor2 of :625, :1251, :1420 as ONE row-major block rows[count][dim] (the reference's float** rows
 * gathered).  side 0 = reference keypoints, 1 = target keypoints.  OC_HIP_HOST blocks are copied; OC_HIP_DEVICE blocks
 * are used in place (16-byte aligned) until the side is set again.  A second call replaces the side.  count 0 is legal. */
int oc_hip_matcher_set_descriptors(oc_hip_engine* engine, int side, const float* rows, size_t count, int memory);
/* SIFT3D::bruteforceMatch (:625-674).  direction 0: every reference keypoint against all target keypoints, 1: the other
 * way round.  matched_idx[i] = the nearest candidate when best < ratio^2 * second (:666), else -1 -- EVERY entry is written
 * (the reference leaves failing entries as the caller initialised them); best_sq / second_sq (may be null): the two
 * smallest squared distances under (distance, index), FLT_MAX where no candidate exists; *n_matched (may be null; a host
 * variable, the call waits for the stream when it is given): the reference's return value.  The three arrays have one
 * entry per query and live where `memory` says. */
int oc_hip_matcher_nearest(oc_hip_engine* engine, int direction, int* matched_idx, float* best_sq, float* second_sq,
                           size_t* n_matched, int memory);
/* mode 0 = SIFT3D::monodirectionalMatch (:1251-1418): ratio test, then of the reference keypoints that chose the same
 * target the one with the smallest (distance, index) stays when it passes the ratio test against the group's second
 * (:1361-1387); pairs in descending target index.  mode 1 = SIFT3D::bidirectionalMatch (:1420-1487): pairs (i, r2t[i])
 * with t2r[r2t[i]] == i in ascending i.  ref_idx / tar_idx: `capacity` entries each, where `memory` says; *n_pairs (host,
 * required) receives the number of pairs.  capacity smaller than that: OC_HIP_ERR_INVALID, nothing is written and
 * *n_pairs carries the needed size (min(count_ref, count_tar) always suffices).  The call waits for the stream. */
int oc_hip_matcher_match(oc_hip_engine* engine, int mode, int* ref_idx, int* tar_idx, size_t capacity, size_t* n_pairs,
                         int memory);

/* ---- SIFT3D's scale space: Gaussian / DoG pyramids and extrema ------------ */
/* The front half of SIFT3D::compute(): createGaussianPyramid (src/oc_sift.cpp:676-754), createDogPyramid (:756-793) and
 * detectExtrema (:795-847).  Volumes are [z][y][x], x contiguous, float32 (Image3D::vol_mat).  Arithmetic contract: the blur
 * weights are the reference's (:371-399, computed on the host); every blurred voxel is acc = w[0] * s[c], then for
 * r = 1 ... R in that order acc = acc + w[r] * (s[lo(c - r)] + s[hi(c + r)]) in float32 (fmaf(w[r], s_lo + s_hi, acc) under
 * oc_hip_set_tuning("arith_fma", 1)), passes x, y, z; lo / hi are mirrorLow / mirrorHigh (:1505-1517).  One deviation, where the
 * reference reads outside the array (axis radius > dim - 1): the reflected index is clamped into [0, dim - 1].  Non-finite
 * voxels are outside the contract (they cannot affect addressing).  Supported: axis radii up to 32, up to 16 layers per octave,
 * volumes up to 2^31-1 voxels; anything else is refused with OC_HIP_ERR_UNSUPPORTED before anything is launched.  The handle
 * supports set_stream, synchronize, set_tuning ("arith_fma") and destroy; oc_hip_set_devices, oc_hip_compute* and
 * oc_hip_set_images* are refused (OC_HIP_ERR_UNSUPPORTED).  Settings at creation: those of SIFT3D::SIFT3D() (:142-159). */
typedef struct oc_hip_sift3d_candidate {
    int x, y, z;      /* Keypoint3D::coor_layer (:833-835) */
    int octave, layer; /* :836-837; layer = position of the DoG layer in its octave */
    float scale;      /* the DoG layer's (:838) */
} oc_hip_sift3d_candidate;
int oc_hip_sift3d_create(int device, oc_hip_engine** out);
/* the members of Sift3dConfig (src/oc_sift.h:71-83) the scale space reads; SIFT3D::setSiftConfig (:192-195) */
int oc_hip_sift3d_set_config(oc_hip_engine* engine, int n_octave_layers, int min_dimension, float alpha, float sigma_source,
                             float sigma_base);
/* SIFT3D::setPhysicalUnit (:197-202) */
int oc_hip_sift3d_set_physical_unit(oc_hip_engine* engine, float unit_x, float unit_y, float unit_z);
/* The Image3D the pyramid is built from (:676).  OC_HIP_HOST volumes are copied; OC_HIP_DEVICE volumes are used in place and
 * must stay valid until oc_hip_sift3d_build has returned. */
int oc_hip_sift3d_set_volume(oc_hip_engine* engine, const float* data, int dim_x, int dim_y, int dim_z, int memory);
/* createGaussianPyramid + createDogPyramid with max_abs of every DoG layer (:676-793).  Both pyramids stay on the device.
 * The call waits for the stream. */
int oc_hip_sift3d_build(oc_hip_engine* engine);
/* pyramid 0 = Gaussian (n_octave * (n_octave_layers + 3) layers, :685-686), 1 = DoG (n_octave * (n_octave_layers + 2), :758-759) */
int oc_hip_sift3d_layer_count(const oc_hip_engine* engine, int pyramid, int* n_layers, int* n_octave);
/* The members of Layer3D (src/oc_sift.h:85-94) but vol_mat; every output may be null.  dims / units: { x, y, z }.  sigma: the
 * value of :706 / :728 (0 for the bottom layer of an octave above the first and for DoG layers, which the reference leaves
 * unset); max_abs: :777-787 for DoG layers, -1 for Gaussian ones. */
int oc_hip_sift3d_layer_info(const oc_hip_engine* engine, int pyramid, int index, int* dims, float* units, int* octave,
                             float* scale, float* sigma, float* max_abs);
/* vol_mat of one layer as dims[2] * dims[1] * dims[0] floats where `memory` says */
int oc_hip_sift3d_get_layer(oc_hip_engine* engine, int pyramid, int index, float* out, int memory);
/* detectExtrema (:795-847): the candidates in the reference's scan order (octave, layer, z, y, x ascending), identical from
 * run to run.  out: `capacity` records where `memory` says; *n (host, required) receives the number of candidates.  capacity
 * smaller than that: OC_HIP_ERR_INVALID, nothing is written and *n carries the needed size.  The call waits for the stream. */
int oc_hip_sift3d_detect(oc_hip_engine* engine, oc_hip_sift3d_candidate* out, size_t capacity, size_t* n, int memory);

/* ---- SIFT3D's orientation and descriptor stages --------------------------- */
/* SIFT3D::assignOrientation (src/oc_sift.cpp:849-1049) and constructDescriptor (:1051-1249) on the pyramid of
 * oc_hip_sift3d_build, on the same handle.  Arithmetic contract:
 * 1. Per-voxel terms are the reference's float32 expressions in its order, each operation rounded on its own: the window bounds
 *    as written (:863-876 -- :870 multiplies by unit_y where the other five bounds divide -- and :1066-1079), the IMG_BORDER
 *    clamp, the sphere test norm <= radius, gradients (`0.5 * (a - b) / unit` as (0.5f * (a - b)) / unit: the same bits),
 *    rotation, subregion coordinates, (int) truncation for the cube index against floor for the fraction (:1174-1187),
 *    the 10 FLT_EPSILON magnitude test, cartisan2Barycentric (:579-623) over the 20 tiles of prepare() (:212-231) in ascending
 *    order with the first hit winning, the trilinear weights and the three products per bin (:1209-1211).  Unqualified exp,
 *    pow, sqrt, floor and fabs of float arguments are the float overloads.
 * 2. Gaussian weights come from the host's libm, as tables over (|dx|, |dy|, |dz|) per layer: expf(-0.5f * (q * q)) with
 *    q = norm / sigma_w in float (:902), (float)exp(-0.5 * (q * q)) with q = (double)(norm / sigma) (:1129); pow(q, 2) is q * q.
 * 3. Sums over voxels are exact (the deliberate departure: the reference adds sequentially in float32 inside one thread).
 *    With A = max |v| of the volume and E the smallest integer with 2^E >= 2 A / min(unit) (0 for A = 0), a term t becomes
 *    the integer llrintf(ldexpf(t, -q)), q = E - 40 for the three d sums, 2 E - 40 for the six tensor sums, E - 39 for the
 *    descriptor bins; the integers add up in 64 bits.  Back: int64 -> float32 with one rounding, times 2^q (d, the reported
 *    sums, the bins); the tensor enters the eigen-decomposition as int64 -> double, times 2^q.  No result depends on the
 *    order of the voxels, on the launch shape or on the run; a keypoint's bits depend on the rest of the volume through E only.
 * 4. The eigen-decomposition (the reference calls Eigen::EigenSolver<Matrix3f>, :948) is a cyclic Jacobi iteration on the
 *    symmetric 3 x 3 in double (pairs (0,1), (0,2), (1,2); t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)); a pair with
 *    |a_pq| <= 2^-62 (|a_pp| + |a_qq|) is skipped; stop after a sweep without rotation or 16 sweeps).  Values and vectors
 *    are rounded to float32; then :952-1048 follow as written.
 * 5. Normalise / truncate / normalise (:1219-1247): the two 768-term sums are sequential float32 in ascending i.
 * "arith_fma" keeps selecting how the Gaussian layers were blurred; these stages have one mode.
 * Refused before any launch: OC_HIP_ERR_INVALID for a volume with non-finite voxels and for a record that names no layer
 * keypoints lie in (octave in range, layer in 1 ... n_octave_layers), whose scale bits are not that layer's, whose coor_layer
 * is not an integer inside the layer, or (keypoints) with a rotation entry that is not finite or beyond +-2 (no orthonormal
 * matrix has one, and the grid has no room for it); OC_HIP_ERR_UNSUPPORTED for |E| > 60, a window of more than 2^20 voxels
 * after clamping, a window half-extent above 80 voxels.  These three verdicts are the pyramid's: one layer beyond a limit refuses
 * orient and describe for every record, also for records of layers that would fit.  Lists on the device are checked by a kernel
 * that raises a flag.
 * Cost on the entry points of the scale space: oc_hip_sift3d_build also finds A (one read of the volume and a 4-byte read-back),
 * and oc_hip_sift3d_detect makes its list in the engine, where orient(candidates = NULL) reads it, and copies it out -- for an
 * OC_HIP_DEVICE list that is one device-to-device copy and a second copy of the list (24 bytes per candidate) more than before. */
typedef struct oc_hip_sift3d_keypoint {   /* Keypoint3D, src/oc_sift.h:96-103; 72 bytes */
    float coor_layer[3];  /* x, y, z */
    float coor_img[3];    /* coor_layer * 2^octave (:1044-1045) */
    int octave, layer;
    float scale;
    float rotation_matrix[9];
} oc_hip_sift3d_keypoint;
/* The number of candidates of the pyramid as built -- what oc_hip_sift3d_detect reports in *n -- without a list buffer:
 * the size of the status and sums arrays of oc_hip_sift3d_orient(candidates = NULL).  The count is made once per build. */
int oc_hip_sift3d_candidate_count(oc_hip_engine* engine, size_t* n);
/* beta, gamma, gradient_threshold, truncate_threshold of Sift3dConfig (src/oc_sift.h:71-83); at creation the values of
 * SIFT3D::SIFT3D() (:147-152): 0.9, 0.4, 1e-10, 0.2 * 128 / 768.  Takes effect with the next orient / describe. */
int oc_hip_sift3d_set_feature_config(oc_hip_engine* engine, float beta, float gamma, float gradient_threshold, float truncate_threshold);
/* SIFT3D::assignOrientation (:849-1049).  candidates == NULL: the candidates of the pyramid as built, the list
 * oc_hip_sift3d_detect returns, which is made on the device and stays there (n_candidates and candidates_memory are ignored;
 * the count is oc_hip_sift3d_candidate_count's); otherwise n_candidates records where candidates_memory says.
 * status (may be null, one int per candidate): 0 accepted, 1 gradient threshold (:930), 2 eigenvalues (:973-977), 3 angle
 * (:1006).  sums (may be null, 9 floats per candidate): d_x d_y d_z, then the tensor xx xy xz yy yz zz.  out: the accepted
 * keypoints in candidate order (:1039-1048), `capacity` records; out, status and sums live where `memory` says.  *n (host,
 * required) receives the number of keypoints; capacity smaller than that: OC_HIP_ERR_INVALID, nothing is written and *n
 * carries the needed size (n_candidates always suffices).  Either way the keypoints stay on the device for
 * oc_hip_sift3d_describe(keypoints = NULL).  The call waits for the stream. */
int oc_hip_sift3d_orient(oc_hip_engine* engine, const oc_hip_sift3d_candidate* candidates, size_t n_candidates, int candidates_memory,
                         oc_hip_sift3d_keypoint* out, size_t capacity, size_t* n, int* status, float* sums, int memory);
/* SIFT3D::constructDescriptor (:1051-1249).  keypoints == NULL: the output of the engine's last oc_hip_sift3d_orient (n must be
 * its *n); otherwise n records where keypoints_memory says.  descriptors: n x 768 float32, row-major, where `memory` says -- an
 * OC_HIP_DEVICE block (16-byte aligned) is directly usable by oc_hip_matcher_set_descriptors.  descriptors == NULL with
 * OC_HIP_DEVICE: the block stays in the engine, oc_hip_get_field(engine, "descriptors", ...) hands it out, and it is valid
 * until the next oc_hip_sift3d_describe on this handle or its destruction.  Process a long list in chunks: the descriptors of a
 * million keypoints are 3 GB. */
int oc_hip_sift3d_describe(oc_hip_engine* engine, const oc_hip_sift3d_keypoint* keypoints, size_t n, int keypoints_memory,
                           float* descriptors, int memory);

/* ---- SIFT2D's detector: scale space and located keypoints ------------------ */
/* The front half of SIFT2D::compute() (src/oc_sift.cpp:60-93): what cv::SIFT::detect does before it assigns orientations, for
 * the cv::SIFT that SIFT2D creates (:65-79) from its Sift2dConfig (:22-30) -- the 2x upscaled base image, the Gaussian and DoG
 * pyramids, the 26-neighbour extrema scan and the sub-pixel localisation with its contrast and edge rejections.  The
 * arithmetic contract is DESIGN.md section 4.13: float32, every multiply and add rounding on its own ("arith_fma" is refused:
 * this engine has one arithmetic).  The output is the list of located keypoints in the scan order of the extremum each one
 * started from (octave, layer, row, column), the same from run to run; two starts that end in one cell both stay.  Orientation,
 * descriptors, duplicate removal, n_features trimming and matching are not part of this engine.  Refused before anything is
 * launched: image sides below 2, n_octave_layers outside [1, 8], a sigma that is not finite or not > 0 (OC_HIP_ERR_INVALID);
 * a doubled base image above 2^31-1 pixels, a blur radius above 32 or below 1 (a
 * blur sigma below 0.0625), n_features != 0 (OC_HIP_ERR_UNSUPPORTED); oc_hip_sift2d_build
 * refuses an image with a non-finite pixel (OC_HIP_ERR_INVALID).  The handle takes oc_hip_set_stream, oc_hip_set_tuning (the keys
 * every kind accepts) and oc_hip_destroy; oc_hip_compute*, oc_hip_set_images* and oc_hip_set_devices are refused
 * (OC_HIP_ERR_UNSUPPORTED).  Settings at creation: those of SIFT2D::SIFT2D() (:22-30). */
typedef struct oc_hip_sift2d_keypoint {   /* 48 bytes */
    float x, y;             /* cv::KeyPoint::pt in pixels of the input image */
    float size, response;   /* cv::KeyPoint::size, ::response */
    int octave, layer;      /* octave as cv::SIFT counts it (-1 = the doubled base), layer 1 ... n_octave_layers */
    int row, col;           /* the cell of that octave the localisation ended in */
    float xc, xr, xi;       /* its offsets from the cell: column, row, layer */
    int packed_octave;      /* cv::KeyPoint::octave */
} oc_hip_sift2d_keypoint;
/* SIFT2D::SIFT2D() (src/oc_sift.cpp:22-30) */
int oc_hip_sift2d_create(int device, oc_hip_engine** out);
/* the members of Sift2dConfig (src/oc_sift.h:30-37); SIFT2D::setSiftConfig (src/oc_sift.cpp:44-47), cv::SIFT::create (:65-70) */
int oc_hip_sift2d_set_config(oc_hip_engine* engine, int n_features, int n_octave_layers, float contrast_threshold, float edge_threshold,
                             float sigma);
/* the image cv::SIFT::detect is given (:86): [row][col], pixel_type 0 = uint8, 1 = float32 on the 0 ... 255 scale; a HOST image
 * is copied, a DEVICE image (4-byte aligned when float32) is used in place and must stay valid until oc_hip_sift2d_build has returned */
int oc_hip_sift2d_set_image(oc_hip_engine* engine, const void* data, int pixel_type, int width, int height, int memory);
/* the pyramids of cv::SIFT::detect (:86); they stay on the device */
int oc_hip_sift2d_build(oc_hip_engine* engine);
/* pyramid 0 = Gaussian, 1 = DoG (:86) */
int oc_hip_sift2d_layer_count(const oc_hip_engine* engine, int pyramid, int* n_layers, int* n_octave);
/* dims = { cols, rows }; octave counts from 0 at the doubled base; sigma and radius of the blur that made a Gaussian layer (0 for
 * a resampled one and for DoG layers); threshold: the integer the extrema scan compares fabsf(v) with (:86) */
int oc_hip_sift2d_layer_info(const oc_hip_engine* engine, int pyramid, int index, int* dims, int* octave, float* sigma, int* radius,
                             int* threshold);
/* one layer, cols x rows float32, where `memory` says (:86) */
int oc_hip_sift2d_get_layer(oc_hip_engine* engine, int pyramid, int index, float* out, int memory);
/* the number of located keypoints of the pyramid as built (:86); the detection runs once per build */
int oc_hip_sift2d_keypoint_count(oc_hip_engine* engine, size_t* n);
/* The located keypoints (:86) where `memory` says, at most `capacity` records; *n (required) receives their number.  capacity
 * smaller than that: OC_HIP_ERR_INVALID, nothing is written and *n carries the needed size.  The list also stays in the engine.
 * The call waits for the stream. */
int oc_hip_sift2d_detect(oc_hip_engine* engine, oc_hip_sift2d_keypoint* out, size_t capacity, size_t* n, int memory);

/* ---- FeatureAffine2D / FeatureAffine3D: the keypoint-guided affine initial guess ---- */
/* src/oc_feature_affine.{h,cpp}: per POI the matched keypoints inside the search radius (the neighbor_number_min nearest when
 * fewer are found), a RANSAC loop of affine fits over samples of them, and the least-squares affine map of the largest
 * consensus set as the POI's first-order deformation.  The reference seeds std::mt19937_64 from std::random_device and walks
 * nanoflann's result order, so its output differs from run to run; this engine is deterministic.  The contract:
 * 1. Candidates: every reference keypoint with d2 < r * r, d2 the float32 sum dx * dx + dy * dy (+ dz * dz) in that order and
 *    r * r rounded to float, in the order of Strain's walk (the 3 x 3 (x 3) block of grid cells row-major, ascending keypoint
 *    index inside a cell); fewer than neighbor_number_min (but at least sample_number): the neighbor_number_min nearest by
 *    ascending (d2, index) (:204-221 / :461-478).  Fewer than sample_number: zncc = -1, the record otherwise untouched.
 * 2. Coordinates are taken relative to the POI in float32 (:226-230 / :481-485).
 * 3. The sample of trial t = 0, 1, ... is a partial Fisher-Yates over the candidate positions 0 ... n-1 that starts from the
 *    identity every trial: for j = 0 ... s-1, k = j + (uint32)(((h >> 32) * (uint64)(n - j)) >> 32), swap positions j and k,
 *    h = splitmix64(base + ((uint64)t << 8 | j)), base = splitmix64(seed ^ (bits(x) | (uint64)bits(y) << 32)), in 3D
 *    base = splitmix64(base ^ bits(z)); x, y, z are the coordinates the POI came with.  A POI's record therefore does not
 *    depend on where it stands in the queue or on how the queue is split.
 * 4. Sample solve and final fit are one routine: the normal equations of [x y (z) 1] X = [x' y' (z')] accumulated in double
 *    over the rows in the order given (sample order; candidate order for the final fit), Gaussian elimination with partial
 *    pivoting in double (first largest |entry| of the column wins; a pivot below 2^-40 times the largest |entry| of A^T A:
 *    singular; rows are scaled by 1.0 / pivot), X rounded to float32 once.  The reference calls Eigen's float
 *    colPivHouseholderQr: a stated deviation.  A singular sample gives an empty consensus set and the trial counts; a
 *    singular final fit gives zncc = -2.
 * 5. Consensus (:262-282 / :519-543): the reference's float32 expressions in its order, every operation rounded on its own,
 *    strict < error_threshold; the set is kept in candidate order; its error sum is float32, candidate position j added by
 *    lane j % 64 in ascending j, the 64 partials combined by an xor butterfly with offsets 1, 2, ... 32; mean = sum / count
 *    (NaN for an empty set, which compares false); the replacement of the largest set and the exit rule are the reference's
 *    (:284-292 / :545-551, the mean being the current trial's).
 * 6. Output (:296-330 / :555-596): fewer than ndim + 1 inliers: zncc = -2; otherwise the deformation, result.iteration = trials,
 *    result.feature = inliers (POI3D: the float behind convergence, src/oc_poi.h:93-99) and zncc = 0.
 * 7. Self-adaptive subsets, 2D (:128-179): the subset_feature_min nearest keypoints, their bounding box, the reference's update
 *    of the POI's x, y and subset_radius; relative coordinates after the update, the generator's key before it.
 * "arith_fma" is refused: this engine has one arithmetic.  oc_hip_set_devices is refused (OC_HIP_ERR_UNSUPPORTED).
 * Limits, OC_HIP_ERR_UNSUPPORTED: sample_number outside [ndim + 1, 8], trial_number outside [1, 1024], neighbor_number_min or
 * subset_feature_min above 64, more than 2^31-1 keypoints, a POI with more than 16384 keypoints inside the radius (compute
 * names the POI and writes nothing).  A queue with a NaN POI coordinate: OC_HIP_ERR_INVALID, nothing is written. */
/* FeatureAffine2D(radius_x, radius_y, thread_number) :34-55 (ndim 2; radius_z ignored) / FeatureAffine3D(radius_x, radius_y,
 * radius_z, thread_number) :357-374 (ndim 3), with their defaults: search radius sqrt(rx^2 + ry^2 (+ rz^2)), neighbor_number_min
 * 7 / 16, error_threshold 1.5 / 3.2, sample_number 3 / 4, trial_number 20 / 32. */
int oc_hip_feature_affine_create(int ndim, int radius_x, int radius_y, int radius_z, int device, oc_hip_engine** out);
/* setSearch :81-85 / :400-404.  A new radius needs oc_hip_feature_affine_prepare again. */
int oc_hip_feature_affine_set_search(oc_hip_engine* engine, float neighbor_search_radius, int neighbor_number_min);
/* setRansacConfig :87-90 / :406-409 (RansacConfig: trial_number, sample_mumber, error_threshold, src/oc_feature_affine.h:26-31) */
int oc_hip_feature_affine_set_ransac(oc_hip_engine* engine, int trial_number, int sample_number, float error_threshold);
/* the seed of the sample generator (0 at creation); the reference has none (:241-242 / :496-497) */
int oc_hip_feature_affine_set_seed(oc_hip_engine* engine, unsigned long long seed);
/* DIC::setSelfAdaptive + setSubsetAdjustment :92-96 + the size of the reference image (:130-133); FeatureAffine2D only */
int oc_hip_feature_affine_set_self_adaptive(oc_hip_engine* engine, int enable, int feature_min, int radius_min, int width, int height);
/* setKeypointPair :98-102 / :411-415: `count` matched pairs, packed ndim floats per point, where `memory` says.  Copied. */
int oc_hip_feature_affine_set_keypoints(oc_hip_engine* engine, const float* ref, const float* tar, size_t count, int memory);
/* setKeypointPair from the pairs oc_hip_matcher_match returned: pair k is (ref_kp[ref_idx[k]], tar_kp[tar_idx[k]]), the
 * keypoint arrays packed ndim floats per point; everything on the device (memory must be OC_HIP_DEVICE), gathered there.
 * A negative index (the matcher's -1, a stale list) is refused with OC_HIP_ERR_INVALID and nothing is read through it; the engine
 * then holds no keypoints.  Indices are not checked against the arrays' lengths, which this call does not know. */
int oc_hip_feature_affine_set_matched(oc_hip_engine* engine, const float* ref_kp, const float* tar_kp, const int* ref_idx,
                                      const int* tar_idx, size_t n_pairs, int memory);
/* prepare :104-116 / :417-429: the grid over the reference keypoints */
int oc_hip_feature_affine_prepare(oc_hip_engine* engine);
/* compute(std::vector<POI2D>&) :334-342 / compute(std::vector<POI3D>&) :600-608, in place */
int oc_hip_feature_affine_compute(oc_hip_engine* engine, void* pois, size_t count, size_t stride_bytes, int memory);

/* ---- introspection (tests, bench, profiling) ------------------------------ */
int oc_hip_get_kind(const oc_hip_engine* engine, int* kind);
/* Device pointers of the precomputed fields (row-major float32):
 *   "ref","tar"           height*width            (3D: dz*dy*dx)
 *   "gx","gy"[,"gz"]      same shape              ICGN engines after prepare_ref
 *   "lut"                 4*height*width*4        ICGN2D* / NR2D1 after prepare_tar: the bicubic coefficient table of
 *                                                 src/oc_cubic_bspline.cpp:123-129, stored planar as [k][y][x][l]
 *                                                 (plane k = coef[k][0..3] of every pixel)  (3D: "coef", dz*dy*dx)
 *   "lut_gx","lut_gy"     4*height*width*4        NR2D1 after prepare: tables of the target gradients, same layout
 *   "descriptors"         n*768                   SIFT3D after oc_hip_sift3d_describe(descriptors = NULL, OC_HIP_DEVICE)
 * Returns OC_HIP_ERR_INVALID for an unknown name or a field not built yet. */
int oc_hip_get_field(const oc_hip_engine* engine, const char* name, const float** device_ptr, size_t* count);
/* Copy a field to host memory (test helper). */
int oc_hip_read_field(oc_hip_engine* engine, const char* name, float* host_dst, size_t count);
/* Per-kernel timing with hipEvents recorded on the engine's stream around every
 * launch of the engine's dominant kernel ("icgn" / "fftcc" pipeline).  Enable,
 * run compute() any number of times, synchronize, then read.  */
int oc_hip_profile_enable(oc_hip_engine* engine, int enable);
int oc_hip_profile_read(oc_hip_engine* engine, double* total_ms, long* launches);
int oc_hip_profile_reset(oc_hip_engine* engine);
/* How the engine's last ICGN2D compute() treated the set-up cache ("icgn2d_setup_cache"): OC_HIP_SETUP_CACHE_NONE = it went
 * around the cache, _FILL = it computed every POI's set-up and filed it, _USE = it started from the filed records.
 * Waits for the engine's work (the coordinate comparison happens on the device). */
#define OC_HIP_SETUP_CACHE_NONE 0
#define OC_HIP_SETUP_CACHE_FILL 1
#define OC_HIP_SETUP_CACHE_USE 2
int oc_hip_icgn2d_setup_cache_last(oc_hip_engine* engine, int* state);
/* The on-chip limits of an "icgn2d_variant" id (no engine, no device needed): *max_samples = the largest (2 rx + 1) (2 ry + 1)
 * its LDS layout holds (0 for variant 9, which has its own rule); *compact_admissible = 0 when the id is not 10 or 11 or the
 * radii do not fit it (see the key), 1 when they fit but `count` is below what the automatic choice asks for (the id still
 * runs when it is named), 2 when the automatic choice may take it. */
int oc_hip_icgn2d_variant_limits(int variant, int radius_x, int radius_y, size_t count, int* max_samples, int* compact_admissible);

#ifdef __cplusplus
}
#endif
#endif /* OPENCORR_HIP_H_ */

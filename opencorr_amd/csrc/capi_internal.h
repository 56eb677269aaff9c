// capi_internal.h -- what the translation units of the C-ABI (capi.hip: engines and entry points; capi_host.hip: the chunked
// host-queue pipeline; capi_group.hip: device groups + the RCCL binding; capi_strain.hip: Strain / RegionFit and the reliable /
// unreliable selection) share: the engine object, device buffers, error reporting, the stream / tail-event helpers.
// host/*.h: host logic without HIP calls (the tuning keys and settings, the single-POI combiner, the chunk schedule and hand-off).
#pragma once
#include "../../include/opencorr_hip.h"

#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

// RCCL: types and enumerators only -- the library itself is loaded with dlopen on first use (struct Rccl), and a
// single-GPU host needs neither the library nor its development headers: without <rccl/rccl.h> the few declarations the
// binding uses are restated here (the stable NCCL 2.x C API: opaque communicator handle, ncclResult_t with ncclSuccess = 0,
// ncclUint8 = 1 in ncclDataType_t) and the version check against the loaded library is what guards them.
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#define OC_HIP_RCCL_HEADER 1
#else
#define OC_HIP_RCCL_HEADER 0
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0, ncclUint8 = 1 } ncclDataType_t;
ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist);
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclGroupStart();
ncclResult_t ncclGroupEnd();
ncclResult_t ncclCommDestroy(ncclComm_t comm);
const char* ncclGetErrorString(ncclResult_t result);
ncclResult_t ncclGetVersion(int* version);
}
#define NCCL_MAJOR 2
#endif

#include "oc_kernels.h"
#include "host/chunk_pipeline.h"
#include "host/engine_tuning.h"
#include "host/sift3d_plan.h"
#include "host/sift3d_feature_plan.h"
#include "host/sift2d_plan.h"
#include "host/single_combiner.h"

namespace ochip_capi {

// the last error message of the calling thread (oc_hip_last_error) and the one way to set it: defined in capi.hip
extern thread_local std::string g_last_error;
int fail(int code, const char* fmt, ...);

#define OC_HIP_TRY(expr)                                                                              \
    do {                                                                                              \
        hipError_t err__ = (expr);                                                                    \
        if (err__ != hipSuccess)                                                                      \
            return fail(err__ == hipErrorOutOfMemory ? OC_HIP_ERR_NOMEM : OC_HIP_ERR_HIP,             \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

#define OC_FFT_TRY(expr)                                                                               \
    do {                                                                                               \
        rocfft_status st__ = (expr);                                                                   \
        if (st__ != rocfft_status_success)                                                             \
            return fail(OC_HIP_ERR_ROCFFT, "%s failed: rocfft_status %d (%s:%d)", #expr, (int)st__, __FILE__, __LINE__); \
    } while (0)

#define OC_TRY(expr)                  \
    do {                              \
        int rc__ = (expr);            \
        if (rc__ != OC_HIP_OK) return rc__; \
    } while (0)

// DevBuf, PinnedBuf and FftPlans free what they hold in their destructors: move-only, and a move leaves the source empty.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        DevBuf taken(std::move(o));  // (what this one held goes with `taken`)
        std::swap(p, taken.p);
        std::swap(bytes, taken.bytes);
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only allocation
    int reserve(size_t n) {
        if (n <= bytes) return OC_HIP_OK;
        release();
        hipError_t err = hipMalloc(&p, n);
        if (err != hipSuccess) {
            p = nullptr;
            return fail(OC_HIP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(err));
        }
        bytes = n;
        return OC_HIP_OK;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// grow-only page-locked host buffer (the combining front end of compute(POI*) stages its batches here: copies from / to
// pinned memory are plain asynchronous DMA, pageable ones go through the runtime's own staging with a wait each)
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        PinnedBuf taken(std::move(o));  // (what this one held goes with `taken`)
        std::swap(p, taken.p);
        std::swap(bytes, taken.bytes);
        return *this;
    }
    ~PinnedBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    int reserve(size_t n) {
        if (n <= bytes) return OC_HIP_OK;
        release();
        n = (n + 65535) & ~(size_t)65535;
        hipError_t err = hipHostMalloc(&p, n, hipHostMallocDefault);
        if (err != hipSuccess) {
            p = nullptr;
            return fail(OC_HIP_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", n, hipGetErrorString(err));
        }
        bytes = n;
        return OC_HIP_OK;
    }
};

// device copy of a reference/target image pair (2D) or volume pair (3D), row-major, x fastest
struct ImagePair {
    int ndim = 0;
    int dx = 0, dy = 0, dz = 1;  // width, height, depth
    DevBuf ref, tar;
    const float* ref_ext = nullptr;  // used in place when the caller handed device memory
    const float* tar_ext = nullptr;
    const float* ref_ptr() const { return ref_ext ? ref_ext : ref.as<float>(); }
    const float* tar_ptr() const { return tar_ext ? tar_ext : tar.as<float>(); }
    size_t count() const { return (size_t)dx * dy * dz; }
};

struct FftPlans {
    int n0 = 0, n1 = 0, n2 = 0;  // slowest .. fastest (n2 == 0 for 2D)
    size_t chunk = 0;
    rocfft_plan fwd = nullptr, inv = nullptr;
    rocfft_execution_info info_fwd = nullptr, info_inv = nullptr;
    DevBuf work_fwd, work_inv;
    FftPlans() = default;
    FftPlans(FftPlans&& o) noexcept { *this = std::move(o); }
    FftPlans& operator=(FftPlans&& o) noexcept {
        if (this == &o) return *this;
        destroy();
        n0 = o.n0, n1 = o.n1, n2 = o.n2, chunk = std::exchange(o.chunk, 0);
        fwd = std::exchange(o.fwd, nullptr), inv = std::exchange(o.inv, nullptr);
        info_fwd = std::exchange(o.info_fwd, nullptr), info_inv = std::exchange(o.info_inv, nullptr);
        work_fwd = std::move(o.work_fwd), work_inv = std::move(o.work_inv);
        return *this;
    }
    void destroy() {
        if (fwd) rocfft_plan_destroy(fwd);
        if (inv) rocfft_plan_destroy(inv);
        if (info_fwd) rocfft_execution_info_destroy(info_fwd);
        if (info_inv) rocfft_execution_info_destroy(info_inv);
        fwd = inv = nullptr;
        info_fwd = info_inv = nullptr;
        chunk = 0;
    }
    ~FftPlans() { destroy(); }
};

template <class T> constexpr bool kMoveOnly = std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value &&
                                            !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value;
static_assert(kMoveOnly<DevBuf> && kMoveOnly<PinnedBuf> && kMoveOnly<FftPlans>, "a copy would free twice");

void rocfft_init_once();   // capi.hip

}  // namespace ochip_capi
using namespace ochip_capi;

// Everything an engine holds that is bound to its device or to its streams.  reset_device_state (capi.hip) is the one teardown:
// oc_hip_destroy ends with it, a move to another device (oc_hip_set_devices) starts from it -- a member added here is covered by both.
struct DeviceState {
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t order_ev = nullptr;  // orders the private stream behind the caller's default-stream work
    // Orders a newly chosen stream behind the work this engine left on the previous one.  On a CALLER-owned stream the
    // event is recorded at the end of every entry point that returns with work still enqueued (mark_tail): the caller may
    // destroy its stream at any time afterwards, and HIP aborts the process when a destroyed stream is handed to ANY
    // API call -- so a stream switch, destroy() and set_devices() never touch a caller's stream again, they wait for
    // this event instead.
    hipEvent_t switch_ev = nullptr;
    bool tail_marked = false;  // switch_ev holds the tail of this engine's work on the current (caller-owned) stream
    std::shared_ptr<ImagePair> img;
    DevBuf gx, gy, gz, coef;  // coef: 2D LUT (16 floats / px) or 3D coefficient volume
    DevBuf coef_gx, coef_gy;  // NR2D1: LUTs of the target gradients
    DevBuf tmp;               // scratch for layout conversion / the warped subvolumes of ICGN3D1
    DevBuf prefilter_tmp;     // second volume of the 3D B-spline prefilter (x pass -> here -> y pass -> coef -> z pass)
    bool ref_ready = false, tar_ready = false;
    DevBuf poi_stage, off_stage;
    DevBuf cursors;  // small device scratch (batch maxima)
    DevBuf perm, tiles, perm_slots;  // locality schedule of the ICGN2D queue (poi_order.hip)
    DevBuf setup_recs;               // icgn2d variant 8 (split launch shape): mean, norm, H^-1 per POI between the two kernels
    // ICGN2D set-up cache (run_icgn2d, icgn2d.hip CACHE): { reference mean, norm, H^-1 } per POI of the last big-queue launch, the
    // (x, y) bit patterns they were built for, and the word the coordinate check stamps.  What the host can know -- reference
    // and its gradients re-prepared, radii, arithmetic, count, stride, variant -- lives in setup_cache_key; the coordinates are
    // compared on the device, so no call waits for the host.  Grow-only, per engine (group members own theirs).
    DevBuf setup_cache_recs, setup_cache_xy, setup_cache_word;
    struct SetupCacheKey {
        size_t count = 0;
        int stride_f = 0, variant = -1, dof = 0, rx = 0, ry = 0, arith_fma = 0, height = 0, width = 0;
        const void *ref = nullptr, *gx = nullptr, *gy = nullptr;
        unsigned long long ref_generation = 0;
        bool operator==(const SetupCacheKey& o) const {
            return count == o.count && stride_f == o.stride_f && variant == o.variant && dof == o.dof && rx == o.rx && ry == o.ry &&
                   arith_fma == o.arith_fma && height == o.height && width == o.width && ref == o.ref && gx == o.gx && gy == o.gy &&
                   ref_generation == o.ref_generation;
        }
    } setup_cache_key;
    bool setup_cache_valid = false;          // the records belong to setup_cache_key
    unsigned setup_cache_epoch = 0;          // one per cached launch; the coordinate check stamps the word with it
    int setup_cache_last = 0;                // last run_icgn2d: 0 = went around the cache, 1 = fill (host's decision), 2 = the device word decided
    bool coef_has_val = false;               // 2D: the value plane (im.count() floats) lies behind the 16 coefficient floats per pixel in `coef`
    DevBuf split_scratch, split_tmp; // oc_hip_split_reliable / oc_hip_merge_recovered (poi_split.hip)
    // Strain
    size_t st_count = 0;  // queue length the grid was prepared for (0 = not prepared)
    ochip::StrainGrid st_grid{};
    DevBuf st_box, st_counts, st_start, st_cursor, st_slots, st_order, st_recs, st_fallback;
    // FeatureAffine (capi_feature_affine.hip): the engine's copy of the matched keypoints (packed, fa_ndim floats per point), the
    // verdict words of the count pass and the global slices of candidate lists beyond the LDS part.  The grid over the reference
    // keypoints lives in the st_* buffers above (st_count = keypoints it was prepared for).
    size_t fa_count = 0;
    DevBuf fa_ref, fa_tar, fa_verdict, fa_scratch;
    DevBuf cal_map_x, cal_map_y, cal_stage;  // Calibration: the undistortion map
    // Descriptor matcher: side 0 = reference, 1 = target.  HOST descriptors are copied into mt_desc, DEVICE ones are used in place (mt_ext).
    size_t mt_count[2] = {0, 0};
    const float* mt_ext[2] = {nullptr, nullptr};
    DevBuf mt_desc[2], mt_idx[2], mt_best[2], mt_second[2];   // [direction] for the results: 0 = ref -> tar, 1 = tar -> ref
    DevBuf mt_part, mt_keys, mt_scan, mt_pairs, mt_counter;
    // SIFT3D scale space (capi_sift3d.hip): the volume (a HOST volume is copied into sf_vol, a DEVICE one is used in place), both
    // pyramids resident for the later stages, ONE scratch volume of octave-0 size (the y pass of every blur), the DoG maxima,
    // the scan scratch and the staged list of oc_hip_sift3d_detect
    const float* sf_ext = nullptr;
    DevBuf sf_vol, sf_scratch, sf_max, sf_scan, sf_list;
    std::vector<DevBuf> sf_gauss, sf_dog;
    bool sf_built = false;
    bool sf_counted = false;  // sf_scan holds the scanned per-workgroup counts of the pyramid as built, sf_total their sum
    unsigned sf_total = 0;
    // ... and its orientation / descriptor stages: the weight tables and the layer records of the pyramid as built (sf_ftables,
    // sf_flayers), max |v| of the volume, the per-candidate results of the last orient (status, nine sums, keypoint slots), its
    // compacted output (sf_kp, what describe(NULL) reads), staged inputs and outputs of HOST calls
    std::vector<DevBuf> sf_ftables;
    DevBuf sf_flayers, sf_vmax, sf_status, sf_sums, sf_slots, sf_kp, sf_fscan, sf_flag, sf_in, sf_desc;
    bool sf_listed = false;    // sf_list holds the list of the last detect (sf_total records)
    bool sf_features = false;  // sf_ftables / sf_flayers belong to the pyramid as built
    bool sf_oriented = false;  // sf_kp holds sf_kp_count keypoints of the pyramid as built
    size_t sf_kp_count = 0;
    size_t sf_desc_floats = 0;  // what the last describe(descriptors = NULL, OC_HIP_DEVICE) left in sf_desc ("descriptors" of oc_hip_get_field)
    // SIFT2D detector (capi_sift2d.hip): the image (a HOST image is copied into s2_img, a DEVICE one is used in place), both pyramids
    // resident for the later stages, ONE scratch image of base size (the rows pass of every blur; the upscaled input before the
    // first one lies in s2_base), the table of DoG layers the localisation reads, the scan scratch, the starts, their verdicts
    // and records, the list of located keypoints
    const void* s2_ext = nullptr;
    DevBuf s2_img, s2_base, s2_scratch, s2_table, s2_flag, s2_scan, s2_starts, s2_status, s2_slots, s2_kscan, s2_kp;
    std::vector<DevBuf> s2_gauss, s2_dog;
    bool s2_built = false;
    bool s2_detected = false;  // s2_kp holds the s2_kp_count keypoints of the pyramid as built
    size_t s2_kp_count = 0;
    // FFTCC working set
    FftPlans fft;
    DevBuf win, freq, norms, flags;
    // host-queue pipeline (compute_host): the queue travels in chunks, copies of one chunk overlap the kernels of
    // its neighbours; one event per chunk orders the copy-out stream behind the kernels
    hipStream_t copy_stream = nullptr, copy_in_stream = nullptr;
    // icgn2d variant 8 with "icgn2d_split_chunks" >= 2: the set-up kernels run on this second stream, one or two chunks ahead
    // of the iteration kernels on the engine's stream, so that workgroups of both kinds are resident together
    hipStream_t aux_stream = nullptr;
    std::vector<hipEvent_t> split_ev;
    std::vector<hipEvent_t> chunk_done, chunk_in;
    DevBuf group_mirror;         // device groups: full-size copy of a DEVICE queue (members other than the leader work in theirs)
    DevBuf group_off_mirror;
    size_t group_mirror_block = 0;  // bytes per member block of the last all-gathered queue
    hipEvent_t group_ev = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;  // profiling
};

// The engine: its settings (host/engine_tuning.h: what oc_hip_set_tuning, set_self_adaptive and set_damping write, and what a
// group member takes from its leader as a whole), its device-bound state, and what belongs to neither.
struct oc_hip_engine : ochip_host::EngineTuning, DeviceState {
    int kind = 0;
    int device = 0;
    int rx = 0, ry = 0, rz = 0;
    float conv = 0.001f, stop = 10.f;
    unsigned long long ref_generation = 0;   // bumped by set_images / share_images / prepare_ref: the reference or its gradients changed
    // Strain (src/oc_strain.cpp:31-46: radius, min neighbours; ZNCC threshold 0.9, Cauchy approximation)
    float st_radius = 0.f, st_zncc = 0.9f;
    int st_nmin = 0, st_approx = 1, st_ndim = 0;
    // Calibration (src/oc_calibration.h:47-97): the 13 + 6 numbers, the four small matrices (host code, row-major), the
    // undistortion map on the device.  Stereovision (src/oc_stereovision.h): the two cameras (handles the caller keeps alive,
    // like the reference's Calibration pointers) and the fundamental matrix.  Handles of these two kinds are created without
    // touching the device (the matrices are host arithmetic); the stream is made by the first call that needs the GPU.
    float cal_i[13] = {}, cal_e[6] = {};
    float cal_K[9] = {}, cal_R[9] = {}, cal_T[3] = {}, cal_P[12] = {};
    float cal_conv = 0.001f;
    int cal_iter = 40, cal_h = 0, cal_w = 0;
    oc_hip_engine* stereo_cam[2] = {nullptr, nullptr};
    float stereo_F[9] = {};
    // Descriptor matcher (capi_match.hip; SIFT3D::bruteforceMatch and the two match modes, src/oc_sift.cpp:625-674, 1251-1487)
    int mt_dim = 0;
    float mt_ratio = 0.f;
    // FeatureAffine2D/3D (capi_feature_affine.hip; src/oc_feature_affine.cpp:34-55, 357-374): search, RANSAC, seed, self-adaptive subsets
    int fa_ndim = 0;
    float fa_radius = 0.f, fa_threshold = 0.f;
    int fa_nmin = 0, fa_samples = 0, fa_trials = 0;
    unsigned long long fa_seed = 0;
    bool fa_adaptive = false;
    int fa_feature_min = 14, fa_radius_min = 10, fa_width = 0, fa_height = 0;
    // SIFT3D scale space (capi_sift3d.hip; SIFT3D::createGaussianPyramid, createDogPyramid, detectExtrema, src/oc_sift.cpp:676-847):
    // the settings, the volume's dims, the plan of the last build (host/sift3d_plan.h) and max_abs of every DoG layer
    ochip_host::Sift3dSettings sf_cfg;
    float sf_unit[3] = {1.f, 1.f, 1.f};
    int sf_dim[3] = {0, 0, 0};
    ochip_host::Sift3dPlan sf_plan;
    std::vector<float> sf_max_abs;
    // its orientation / descriptor stages (SIFT3D::assignOrientation, constructDescriptor, :849-1249): the settings, max |v| of
    // the volume the pyramid was built from, the plan (host/sift3d_feature_plan.h)
    ochip_host::Sift3dFeatureSettings sf_fcfg;
    float sf_vol_max = 0.f;
    ochip_host::Sift3dFeaturePlan sf_fplan;
    // SIFT2D detector (capi_sift2d.hip; cv::SIFT as SIFT2D::compute() creates it, src/oc_sift.cpp:22-30, 60-93): the settings, the
    // image's sides and pixel type, the plan of the last build (host/sift2d_plan.h)
    ochip_host::Sift2dSettings s2_cfg;
    int s2_width = 0, s2_height = 0;
    bool s2_u8 = false;
    ochip_host::Sift2dPlan s2_plan;
    ochip_host::ChunkHandoff chunk_handoff;  // the copy-out thread sleeps here until the next chunk has been handed over
    std::atomic<unsigned> single_calls{0};  // compute(POI*) calls on this engine (one hint on stderr when a caller loops over them)
    // Combining front end of compute(POI*) (host/single_combiner.h): callers that arrive while a launch is in flight are queued;
    // one of them (the leader) hands the whole batch to the engine as ONE queue (serve_single_batch, capi.hip).
    struct SinglePoi {
        void* poi;
        const float* offset;
        int rc = OC_HIP_OK;
        std::string error;
        SinglePoi(void* p, const float* o) : poi(p), offset(o) {}
    };
    using SingleCombiner = ochip_host::SingleCombiner<SinglePoi>;
    SingleCombiner single_combiner;
    std::atomic<unsigned long long> single_batches{0}, single_batched_pois{0}, single_engine_ns{0};   // (engine_ns: time inside the engine calls)
    PinnedBuf single_buf, single_off;            // the leader's contiguous, page-locked copy of a batch's records (and offsets)
    // device group (oc_hip_set_devices): this engine leads, replicas[i] is a full engine of the same kind on
    // group_devices[i + 1]; every setter, set_images, prepare and compute fans out
    std::vector<oc_hip_engine*> replicas;
    std::vector<int> group_devices;
    bool is_replica = false;
    void* rccl_comm = nullptr;   // ncclComm_t of this member (group_allgather with distinct devices)
    bool prof = false;           // profiling
    mutable std::mutex mu;

    bool is_matcher() const { return kind == OC_HIP_MATCHER; }
    bool is_sift3d() const { return kind == OC_HIP_SIFT3D; }
    bool is_sift2d() const { return kind == OC_HIP_SIFT2D; }
    bool is_feature_affine() const { return kind == OC_HIP_FEATURE_AFFINE; }
    bool is3d() const { return kind == OC_HIP_FFTCC3D || kind == OC_HIP_ICGN3D1; }
    bool is_iclm() const { return kind == OC_HIP_ICLM2D1 || kind == OC_HIP_ICLM2D2; }
    bool is_icgn2d() const { return kind == OC_HIP_ICGN2D1 || kind == OC_HIP_ICGN2D2 || is_iclm(); }
    bool is_icgn() const { return is_icgn2d() || kind == OC_HIP_ICGN3D1 || kind == OC_HIP_NR2D1; }
    size_t poi_bytes() const { return is3d() ? OC_HIP_POI3D_BYTES : OC_HIP_POI2D_BYTES; }
};

namespace ochip_capi {

void group_drop_comms(oc_hip_engine* e);  // RCCL communicators of a device group (capi_group.hip)

inline int check_engine(const oc_hip_engine* e) {
    if (!e) return fail(OC_HIP_ERR_INVALID, "null engine handle");
    return OC_HIP_OK;
}

int make_own_stream(oc_hip_engine* e);  // capi_stereo.hip

inline int activate(const oc_hip_engine* e) {
    OC_TRY(check_engine(e));
    OC_HIP_TRY(hipSetDevice(e->device));
    // Calibration / Stereovision handles are created on the host alone: their stream comes with the first device call
    if (!e->own_stream) OC_TRY(make_own_stream(const_cast<oc_hip_engine*>(e)));
    return OC_HIP_OK;
}

// Entry points make the engine's device current for the calling thread and give the caller's device back on the way
// out (a host that drives several GPUs from one thread -- torch with more than one device, say -- must not find its
// current device changed by a library call).
struct DeviceScope {
    int saved = -1;
    DeviceScope() {
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
    }
    ~DeviceScope() {
        int now = -1;
        if (saved >= 0 && hipGetDevice(&now) == hipSuccess && now != saved) (void)hipSetDevice(saved);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
#define OC_ACTIVATE(e)        \
    DeviceScope device_scope; \
    OC_TRY(activate(e))

// The engine's private stream is non-blocking: nothing the caller enqueued is ordered against it.  Inputs that
// live on the device (OC_HIP_DEVICE queues, offsets, images used in place) are usually produced on the legacy
// default stream -- hipMemcpy, plain launches, torch unless told otherwise -- so every entry point that enqueues work
// on the private stream first makes it wait for what the default stream holds at that moment.  Producers on OTHER
// streams must be complete, or be named with oc_hip_set_stream (documented in opencorr_hip.h).
inline int order_after_default_stream(oc_hip_engine* e) {
    if (e->stream != e->own_stream) return OC_HIP_OK;  // caller-chosen stream: stream order is the caller's
    if (!e->order_ev) OC_HIP_TRY(hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming));
    OC_HIP_TRY(hipEventRecord(e->order_ev, nullptr));
    OC_HIP_TRY(hipStreamWaitEvent(e->own_stream, e->order_ev, 0));
    return OC_HIP_OK;
}

// See oc_hip_engine::switch_ev.  Entry points that return with work enqueued on a caller-owned stream end with this.
inline int mark_tail(oc_hip_engine* e) {
    if (e->stream == e->own_stream) return OC_HIP_OK;  // the engine's own stream can always be asked later
    if (!e->switch_ev) OC_HIP_TRY(hipEventCreateWithFlags(&e->switch_ev, hipEventDisableTiming));
    OC_HIP_TRY(hipEventRecord(e->switch_ev, e->stream));
    e->tail_marked = true;
    return OC_HIP_OK;
}

// Scope guard of the entry points that enqueue work: whatever way the function leaves -- also an error exit after some
// kernels or copies were already enqueued on a CALLER-owned stream -- the engine's tail event covers that work, so a later
// set_stream / destroy / set_devices drains it through the event instead of relying on hipFree's implicit device
// synchronisation.  Quiet: a failure to record never replaces the error message the function itself reports, and the
// success paths' own mark_tail (finish_device_call) simply records the same point twice.
struct TailGuard {
    oc_hip_engine* e;
    explicit TailGuard(oc_hip_engine* engine) : e(engine) {}
    TailGuard(const TailGuard&) = delete;
    TailGuard& operator=(const TailGuard&) = delete;
    ~TailGuard() {
        if (!e || e->stream == e->own_stream) return;
        if (!e->switch_ev && hipEventCreateWithFlags(&e->switch_ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        if (hipEventRecord(e->switch_ev, e->stream) == hipSuccess) e->tail_marked = true;
        else (void)hipGetLastError();
    }
};

// Host-side wait for everything this engine has enqueued, without ever touching a caller's (possibly destroyed) stream.
inline void drain_engine(oc_hip_engine* e) {
    if (e->stream == e->own_stream) {
        if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
    } else {
        if (e->tail_marked && e->switch_ev) (void)hipEventSynchronize(e->switch_ev);
        if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
    }
    (void)hipGetLastError();
}

inline void clear_events(oc_hip_engine* e) {
    for (auto& ev : e->events) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    e->events.clear();
}

struct ProfScope {
    oc_hip_engine* e;
    hipEvent_t stop = nullptr;
    explicit ProfScope(oc_hip_engine* e_) : e(e_) {
        if (!e->prof) return;
        hipEvent_t start = nullptr;
        if (hipEventCreate(&start) != hipSuccess) return;
        if (hipEventCreate(&stop) != hipSuccess) { (void)hipEventDestroy(start); stop = nullptr; return; }
        (void)hipEventRecord(start, e->stream);
        e->events.emplace_back(start, stop);
    }
    ~ProfScope() {
        if (stop) (void)hipEventRecord(stop, e->stream);
    }
};

// ---- functions one translation unit defines and another one calls ----------------------------------------------------
// capi.hip
int create_engine(int kind, int rx, int ry, int rz, float conv, float stop, int device, oc_hip_engine** out);
int run_compute_device(oc_hip_engine* e, float* d_pois, int stride_f, size_t count, const float* d_offsets = nullptr);
// capi_host.hip: the chunked host-queue pipeline
int compute_host(oc_hip_engine* e, char* pois, const float* offsets, size_t count, size_t stride_bytes, oc_hip_engine* const* chain = nullptr,
                 int n_chain = 0);
// capi_group.hip: device groups
int compute_group_device(oc_hip_engine* e, char* pois, const float* offsets, size_t count, size_t stride_bytes);
int compute_group_host(oc_hip_engine* e, char* pois, const float* offsets, size_t count, size_t stride_bytes);

// a DEVICE-queue call returns with its work enqueued: on a caller-owned stream the tail event covers it, on the engine's own
// stream the call completes here
inline int finish_device_call(oc_hip_engine* e) {
    if (e->stream == e->own_stream) OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return mark_tail(e);
}

}  // namespace ochip_capi
using namespace ochip_capi;

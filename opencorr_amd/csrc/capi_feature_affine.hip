// capi_feature_affine.hip -- FeatureAffine2D / FeatureAffine3D (part of the C-ABI of include/opencorr_hip.h): the keypoint-guided
// RANSAC affine initial guess of the reference (src/oc_feature_affine.cpp) over the kernels of feature_affine.hip and the grid
// launches of strain.hip.  Everything runs on the engine's stream.
#include "capi_internal.h"

namespace {

int check_fa(const oc_hip_engine* e, const char* what) {
    OC_TRY(check_engine(e));
    if (!e->is_feature_affine()) return fail(OC_HIP_ERR_INVALID, "%s: not a FeatureAffine handle", what);
    return OC_HIP_OK;
}

int check_memory(int memory, const char* what) {
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "%s: bad memory kind %d", what, memory);
    return OC_HIP_OK;
}

int check_search(float radius, int nmin) {
    if (!(radius > 0.f) || !std::isfinite(radius)) return fail(OC_HIP_ERR_INVALID, "FeatureAffine: neighbor_search_radius must be > 0 and finite (got %g)", (double)radius);
    if (nmin < 1) return fail(OC_HIP_ERR_INVALID, "FeatureAffine: neighbor_number_min must be >= 1 (got %d)", nmin);
    if (nmin > ochip::strain_knn_max())
        return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: neighbor_number_min %d exceeds the KNN path's limit of %d", nmin, ochip::strain_knn_max());
    return OC_HIP_OK;
}

hipMemcpyKind to_device(int memory) { return memory == OC_HIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }

}  // namespace

extern "C" {

int oc_hip_feature_affine_create(int ndim, int radius_x, int radius_y, int radius_z, int device, oc_hip_engine** out) {
    if (out) *out = nullptr;
    if (ndim != 2 && ndim != 3) return fail(OC_HIP_ERR_INVALID, "feature_affine_create: ndim must be 2 or 3, got %d", ndim);
    if (radius_x < 1 || radius_y < 1 || (ndim == 3 && radius_z < 1))
        return fail(OC_HIP_ERR_INVALID, "feature_affine_create: subset radius must be >= 1 (got %d, %d, %d)", radius_x, radius_y, radius_z);
    OC_TRY(create_engine(OC_HIP_FEATURE_AFFINE, radius_x, radius_y, ndim == 3 ? radius_z : 0, 0.f, 0.f, device, out));
    oc_hip_engine* e = *out;
    e->fa_ndim = ndim;
    if (ndim == 2) {  // src/oc_feature_affine.cpp:34-47
        e->fa_radius = sqrtf((float)(radius_x * radius_x + radius_y * radius_y));
        e->fa_nmin = 7;
        e->fa_threshold = 1.5f;
        e->fa_samples = 3;
        e->fa_trials = 20;
    } else {  // :357-366
        e->fa_radius = sqrtf((float)(radius_x * radius_x + radius_y * radius_y + radius_z * radius_z));
        e->fa_nmin = 16;
        e->fa_threshold = 3.2f;
        e->fa_samples = 4;
        e->fa_trials = 32;
    }
    return OC_HIP_OK;
}

int oc_hip_feature_affine_set_search(oc_hip_engine* e, float neighbor_search_radius, int neighbor_number_min) {
    OC_TRY(check_fa(e, "feature_affine_set_search"));
    OC_TRY(check_search(neighbor_search_radius, neighbor_number_min));
    std::lock_guard<std::mutex> lock(e->mu);
    if (neighbor_search_radius != e->fa_radius) e->st_count = 0;  // the grid pitch follows the radius: prepare() again
    e->fa_radius = neighbor_search_radius;
    e->fa_nmin = neighbor_number_min;
    return OC_HIP_OK;
}

int oc_hip_feature_affine_set_ransac(oc_hip_engine* e, int trial_number, int sample_number, float error_threshold) {
    OC_TRY(check_fa(e, "feature_affine_set_ransac"));
    if (sample_number < e->fa_ndim + 1 || sample_number > 8)
        return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: sample_number must be %d ... 8 (got %d)", e->fa_ndim + 1, sample_number);
    if (trial_number < 1 || trial_number > 1024) return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: trial_number must be 1 ... 1024 (got %d)", trial_number);
    if (!(error_threshold > 0.f) || !std::isfinite(error_threshold))
        return fail(OC_HIP_ERR_INVALID, "FeatureAffine: error_threshold must be > 0 and finite (got %g)", (double)error_threshold);
    std::lock_guard<std::mutex> lock(e->mu);
    e->fa_trials = trial_number;
    e->fa_samples = sample_number;
    e->fa_threshold = error_threshold;
    return OC_HIP_OK;
}

int oc_hip_feature_affine_set_seed(oc_hip_engine* e, unsigned long long seed) {
    OC_TRY(check_fa(e, "feature_affine_set_seed"));
    std::lock_guard<std::mutex> lock(e->mu);
    e->fa_seed = seed;
    return OC_HIP_OK;
}

int oc_hip_feature_affine_set_self_adaptive(oc_hip_engine* e, int enable, int feature_min, int radius_min, int width, int height) {
    OC_TRY(check_fa(e, "feature_affine_set_self_adaptive"));
    if (enable && e->fa_ndim != 2) return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine3D has no self-adaptive subsets in the reference");
    if (enable) {
        if (feature_min < 1) return fail(OC_HIP_ERR_INVALID, "FeatureAffine: subset_feature_min must be >= 1 (got %d)", feature_min);
        if (feature_min > ochip::strain_knn_max())
            return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: subset_feature_min %d exceeds the KNN path's limit of %d", feature_min, ochip::strain_knn_max());
        if (radius_min < 0 || width < 1 || height < 1)
            return fail(OC_HIP_ERR_INVALID, "FeatureAffine: subset_radius_min must be >= 0 and the image %d x %d at least 1 x 1", width, height);
    }
    std::lock_guard<std::mutex> lock(e->mu);
    e->fa_adaptive = enable != 0;
    if (enable) {
        e->fa_feature_min = feature_min;
        e->fa_radius_min = radius_min;
        e->fa_width = width;
        e->fa_height = height;
    }
    return OC_HIP_OK;
}

int oc_hip_feature_affine_set_keypoints(oc_hip_engine* e, const float* ref, const float* tar, size_t count, int memory) {
    OC_TRY(check_fa(e, "feature_affine_set_keypoints"));
    OC_ACTIVATE(e);
    OC_TRY(check_memory(memory, "feature_affine_set_keypoints"));
    if (count > 0 && (!ref || !tar)) return fail(OC_HIP_ERR_INVALID, "feature_affine_set_keypoints: null keypoint array");
    if (count > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: at most 2^31-1 keypoints");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->fa_count = 0;
    e->st_count = 0;
    if (count == 0) return OC_HIP_OK;
    OC_TRY(order_after_default_stream(e));
    const size_t bytes = count * (size_t)e->fa_ndim * sizeof(float);
    drain_engine(e);  // (a grow releases the old block: nothing may still read it)
    OC_TRY(e->fa_ref.reserve(bytes));
    OC_TRY(e->fa_tar.reserve(bytes));
    OC_HIP_TRY(hipMemcpyAsync(e->fa_ref.p, ref, bytes, to_device(memory), e->stream));
    OC_HIP_TRY(hipMemcpyAsync(e->fa_tar.p, tar, bytes, to_device(memory), e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));  // the caller's arrays may be released
    e->fa_count = count;
    return OC_HIP_OK;
}

int oc_hip_feature_affine_set_matched(oc_hip_engine* e, const float* ref_kp, const float* tar_kp, const int* ref_idx, const int* tar_idx,
                                      size_t n_pairs, int memory) {
    OC_TRY(check_fa(e, "feature_affine_set_matched"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "feature_affine_set_matched: the arrays live on the device (host pairs: gather them and call set_keypoints)");
    if (n_pairs > 0 && (!ref_kp || !tar_kp || !ref_idx || !tar_idx)) return fail(OC_HIP_ERR_INVALID, "feature_affine_set_matched: null array");
    if (n_pairs > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: at most 2^31-1 keypoints");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->fa_count = 0;
    e->st_count = 0;
    if (n_pairs == 0) return OC_HIP_OK;
    OC_TRY(order_after_default_stream(e));
    const size_t bytes = n_pairs * (size_t)e->fa_ndim * sizeof(float);
    drain_engine(e);
    OC_TRY(e->fa_ref.reserve(bytes));
    OC_TRY(e->fa_tar.reserve(bytes));
    OC_TRY(e->fa_verdict.reserve(3 * sizeof(unsigned)));
    OC_HIP_TRY(ochip::launch_feature_affine_pairs(e->fa_ndim, ref_kp, tar_kp, ref_idx, tar_idx, n_pairs, e->fa_ref.as<float>(),
                                                  e->fa_tar.as<float>(), e->fa_verdict.as<unsigned>(), e->stream));
    unsigned negative = 0;
    OC_HIP_TRY(hipMemcpyAsync(&negative, e->fa_verdict.p, sizeof(negative), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    if (negative != 0xffffffffu)
        return fail(OC_HIP_ERR_INVALID, "feature_affine_set_matched: pair %u has a negative index (the engine holds no keypoints now)", negative);
    e->fa_count = n_pairs;
    return OC_HIP_OK;
}

int oc_hip_feature_affine_prepare(oc_hip_engine* e) {
    OC_TRY(check_fa(e, "feature_affine_prepare"));
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->st_count = 0;
    const size_t count = e->fa_count;
    if (count == 0) return fail(OC_HIP_ERR_INVALID, "FeatureAffine: prepare() needs keypoints (oc_hip_feature_affine_set_keypoints / _set_matched)");
    const int ndim = e->fa_ndim;
    const float* ref = e->fa_ref.as<float>();
    // bounding box -> grid (the cell count is needed on the host to size the tables): Strain's launches on the packed array
    OC_TRY(e->st_box.reserve(6 * sizeof(unsigned)));
    OC_HIP_TRY(ochip::launch_strain_bbox(ndim, ref, ndim, count, e->st_box.as<unsigned>(), e->stream));
    unsigned box[6];
    OC_HIP_TRY(hipMemcpyAsync(box, e->st_box.p, sizeof(box), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    const ochip::StrainGrid g = ochip::strain_make_grid(ndim, box, e->fa_radius);
    const size_t ncell = ochip::strain_cell_count(g);
    OC_TRY(e->st_counts.reserve(ncell * sizeof(unsigned)));
    OC_TRY(e->st_cursor.reserve(ncell * sizeof(unsigned)));
    OC_TRY(e->st_start.reserve((ncell + 1) * sizeof(unsigned)));
    OC_TRY(e->st_slots.reserve(count * sizeof(unsigned)));
    OC_TRY(e->st_order.reserve(count * sizeof(unsigned)));
    OC_TRY(e->st_recs.reserve(count * 32));
    OC_HIP_TRY(ochip::launch_strain_sort(ndim, ref, ndim, count, g, e->st_counts.as<unsigned>(), e->st_start.as<unsigned>(),
                                         e->st_cursor.as<unsigned>(), e->st_slots.as<unsigned>(), e->st_order.as<unsigned>(), e->stream));
    OC_HIP_TRY(ochip::launch_feature_affine_gather(ndim, ref, e->fa_tar.as<float>(), count, e->st_order.as<unsigned>(), e->st_recs.p,
                                                   e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    e->st_grid = g;
    e->st_ndim = ndim;
    e->st_count = count;
    return OC_HIP_OK;
}

int oc_hip_feature_affine_compute(oc_hip_engine* e, void* pois, size_t count, size_t stride_bytes, int memory) {
    OC_TRY(check_fa(e, "feature_affine_compute"));
    OC_ACTIVATE(e);
    OC_TRY(check_memory(memory, "feature_affine_compute"));
    if (count == 0) return OC_HIP_OK;
    if (!pois) return fail(OC_HIP_ERR_INVALID, "null POI buffer");
    const int ndim = e->fa_ndim;
    const size_t rec = ndim == 2 ? OC_HIP_POI2D_BYTES : OC_HIP_POI3D_BYTES;
    if (stride_bytes < rec || (stride_bytes & 3))
        return fail(OC_HIP_ERR_INVALID, "bad POI stride %zu (record is %zu bytes, stride must be a multiple of 4)", stride_bytes, rec);
    if (count > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: at most 2^31-1 POIs per queue");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    if (e->st_count == 0)
        return fail(OC_HIP_ERR_INVALID, "FeatureAffine: prepare() has not been called (or the keypoints or the search radius changed since)");
    OC_TRY(order_after_default_stream(e));
    float* d_pois = static_cast<float*>(pois);
    if (memory == OC_HIP_HOST) {
        OC_TRY(e->poi_stage.reserve(count * stride_bytes));
        OC_HIP_TRY(hipMemcpyAsync(e->poi_stage.p, pois, count * stride_bytes, hipMemcpyHostToDevice, e->stream));
        d_pois = e->poi_stage.as<float>();
    }
    const int stride_f = (int)(stride_bytes / 4);
    ochip::FeatureAffineParams P;
    P.radius2 = e->fa_radius * e->fa_radius;
    P.error_threshold = e->fa_threshold;
    P.neighbor_min = e->fa_nmin;
    P.sample_number = e->fa_samples;
    P.trial_number = e->fa_trials;
    P.self_adaptive = e->fa_adaptive ? 1 : 0;
    P.feature_min = e->fa_feature_min;
    P.radius_min = e->fa_radius_min;
    P.width = (float)e->fa_width;
    P.height = (float)e->fa_height;
    P.seed = e->fa_seed;
    // the verdict of the queue before a record is touched: NaN coordinates, a candidate list beyond the limit
    OC_TRY(e->fa_verdict.reserve(3 * sizeof(unsigned)));
    OC_HIP_TRY(ochip::launch_feature_affine_count(ndim, d_pois, stride_f, count, e->st_grid, P, e->st_start.as<unsigned>(), e->st_recs.p,
                                                  e->fa_verdict.as<unsigned>(), e->stream));
    unsigned verdict[3];
    OC_HIP_TRY(hipMemcpyAsync(verdict, e->fa_verdict.p, sizeof(verdict), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    if (verdict[2] != 0xffffffffu)
        return fail(OC_HIP_ERR_INVALID, "FeatureAffine: POI %u has a NaN coordinate (nothing was written)", verdict[2]);
    if (verdict[1] != 0xffffffffu)
        return fail(OC_HIP_ERR_UNSUPPORTED, "FeatureAffine: POI %u has more than %d keypoints inside the search radius (%u is the queue's largest count; nothing was written)",
                    verdict[1], ochip::kFeatureAffineListMax, verdict[0]);
    const size_t scratch = ochip::feature_affine_scratch_bytes(ndim, count, verdict[0]);
    if (scratch) OC_TRY(e->fa_scratch.reserve(scratch));
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_feature_affine_compute(ndim, d_pois, stride_f, count, e->st_grid, P, e->st_start.as<unsigned>(), e->st_recs.p,
                                                        verdict[0], scratch ? e->fa_scratch.as<float>() : nullptr, e->stream));
    }
    if (memory == OC_HIP_HOST) {
        OC_HIP_TRY(hipMemcpyAsync(pois, d_pois, count * stride_bytes, hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return OC_HIP_OK;
    }
    return finish_device_call(e);
}

}  // extern "C"

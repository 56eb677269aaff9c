// capi_match.hip -- the descriptor matcher (part of the C-ABI of include/opencorr_hip.h): SIFT3D::bruteforceMatch,
// monodirectionalMatch and bidirectionalMatch of the reference (src/oc_sift.cpp:625-674, 1251-1418, 1420-1487) over the kernels
// of match.hip.  Everything runs on the engine's stream.
#include "capi_internal.h"

namespace {

int check_matcher(const oc_hip_engine* e, const char* what) {
    OC_TRY(check_engine(e));
    if (!e->is_matcher()) return fail(OC_HIP_ERR_INVALID, "%s: not a descriptor matcher handle", what);
    return OC_HIP_OK;
}

int check_ratio(float ratio) {
    if (!(ratio >= 0.f) || !std::isfinite(ratio)) return fail(OC_HIP_ERR_INVALID, "matcher: matching_ratio must be >= 0 and finite (got %g)", (double)ratio);
    return OC_HIP_OK;
}

const float* side_ptr(const oc_hip_engine* e, int side) { return e->mt_ext[side] ? e->mt_ext[side] : e->mt_desc[side].as<float>(); }

// Parts of the candidate range (gridDim.y).  A workgroup owns 64 queries; when the query tiles alone do not give every CU two
// workgroups, the candidate tiles are shared out -- at most one part per candidate tile, at most kMatchMaxSplits.
int choose_splits(const oc_hip_engine* e, size_t nq, size_t nc) {
    const size_t ctiles = std::max<size_t>(1, (nc + ochip::kMatchTile - 1) / ochip::kMatchTile);
    if (e->mt_splits > 0) return e->mt_splits;
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    else (void)hipGetLastError();
    const size_t qtiles = (nq + ochip::kMatchTile - 1) / ochip::kMatchTile, want = 2 * (size_t)cus;
    if (qtiles >= want) return 1;
    const size_t s = (want + qtiles - 1) / qtiles;
    return (int)std::min<size_t>(std::min<size_t>(s, ctiles), (size_t)ochip::kMatchMaxSplits);
}

// nearest + second nearest + ratio test of one direction into the engine's buffers; the match count lands in mt_counter
int run_nearest(oc_hip_engine* e, int direction) {
    const int qs = direction == 0 ? 0 : 1, cs = 1 - qs;
    const size_t nq = e->mt_count[qs], nc = e->mt_count[cs];
    OC_TRY(e->mt_counter.reserve(sizeof(unsigned)));
    OC_TRY(e->mt_idx[direction].reserve(nq * sizeof(int)));
    OC_TRY(e->mt_best[direction].reserve(nq * sizeof(float)));
    OC_TRY(e->mt_second[direction].reserve(nq * sizeof(float)));
    const int splits = choose_splits(e, nq, nc);
    OC_TRY(e->mt_part.reserve((size_t)splits * nq * 16));
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_match_top2(side_ptr(e, qs), nq, side_ptr(e, cs), nc, e->mt_dim, splits, e->arith_fma != 0, e->mt_part.p,
                                            e->stream));
    }
    const float ratio_sq = e->mt_ratio * e->mt_ratio;  // src/oc_sift.cpp:629
    OC_HIP_TRY(ochip::launch_match_finalize(e->mt_part.p, nq, splits, ratio_sq, e->mt_idx[direction].as<int>(),
                                            e->mt_best[direction].as<float>(), e->mt_second[direction].as<float>(),
                                            e->mt_counter.as<unsigned>(), e->stream));
    return OC_HIP_OK;
}

int copy_out(oc_hip_engine* e, void* dst, const void* src, size_t bytes, int memory) {
    if (!dst || bytes == 0) return OC_HIP_OK;
    OC_HIP_TRY(hipMemcpyAsync(dst, src, bytes, memory == OC_HIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    return OC_HIP_OK;
}

}  // namespace

extern "C" {

int oc_hip_matcher_create(int dim, float matching_ratio, int device, oc_hip_engine** out) {
    if (out) *out = nullptr;
    if (!ochip::match_dim_supported(dim))
        return fail(OC_HIP_ERR_INVALID, "matcher: descriptor length must be a multiple of 32 in [32, 1024] (got %d)", dim);
    OC_TRY(check_ratio(matching_ratio));
    OC_TRY(create_engine(OC_HIP_MATCHER, 1, 1, 0, 0.f, 0.f, device, out));
    (*out)->mt_dim = dim;
    (*out)->mt_ratio = matching_ratio;
    return OC_HIP_OK;
}

int oc_hip_matcher_set_ratio(oc_hip_engine* e, float matching_ratio) {
    OC_TRY(check_matcher(e, "matcher_set_ratio"));
    OC_TRY(check_ratio(matching_ratio));
    std::lock_guard<std::mutex> lock(e->mu);
    e->mt_ratio = matching_ratio;
    return OC_HIP_OK;
}

int oc_hip_matcher_set_descriptors(oc_hip_engine* e, int side, const float* rows, size_t count, int memory) {
    OC_TRY(check_matcher(e, "matcher_set_descriptors"));
    OC_ACTIVATE(e);
    if (side != 0 && side != 1) return fail(OC_HIP_ERR_INVALID, "matcher_set_descriptors: side must be 0 (reference) or 1 (target), got %d", side);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "matcher_set_descriptors: bad memory kind %d", memory);
    if (count > 0 && !rows) return fail(OC_HIP_ERR_INVALID, "matcher_set_descriptors: null descriptor block");
    if (count > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "matcher: at most 2^31-1 keypoints per side");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->mt_count[side] = 0;
    e->mt_ext[side] = nullptr;
    if (count == 0) return OC_HIP_OK;
    if (memory == OC_HIP_DEVICE) {
        if (reinterpret_cast<uintptr_t>(rows) & 15) return fail(OC_HIP_ERR_INVALID, "matcher_set_descriptors: a device block must be 16-byte aligned");
        e->mt_ext[side] = rows;
    } else {
        const size_t bytes = count * (size_t)e->mt_dim * sizeof(float);
        drain_engine(e);  // (a grow releases the old block: nothing may still read it)
        OC_TRY(e->mt_desc[side].reserve(bytes));
        OC_HIP_TRY(hipMemcpyAsync(e->mt_desc[side].p, rows, bytes, hipMemcpyHostToDevice, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));  // host buffers may be released by the caller
    }
    e->mt_count[side] = count;
    return OC_HIP_OK;
}

int oc_hip_matcher_nearest(oc_hip_engine* e, int direction, int* matched_idx, float* best_sq, float* second_sq, size_t* n_matched,
                           int memory) {
    OC_TRY(check_matcher(e, "matcher_nearest"));
    OC_ACTIVATE(e);
    if (direction != 0 && direction != 1) return fail(OC_HIP_ERR_INVALID, "matcher_nearest: direction must be 0 (ref -> tar) or 1 (tar -> ref), got %d", direction);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "matcher_nearest: bad memory kind %d", memory);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    if (n_matched) *n_matched = 0;
    const size_t nq = e->mt_count[direction == 0 ? 0 : 1];
    if (nq == 0) return OC_HIP_OK;
    OC_TRY(order_after_default_stream(e));
    OC_TRY(run_nearest(e, direction));
    OC_TRY(copy_out(e, matched_idx, e->mt_idx[direction].p, nq * sizeof(int), memory));
    OC_TRY(copy_out(e, best_sq, e->mt_best[direction].p, nq * sizeof(float), memory));
    OC_TRY(copy_out(e, second_sq, e->mt_second[direction].p, nq * sizeof(float), memory));
    if (n_matched || memory == OC_HIP_HOST) {
        unsigned n = 0;
        OC_HIP_TRY(hipMemcpyAsync(&n, e->mt_counter.p, sizeof(n), hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        if (n_matched) *n_matched = n;
        return OC_HIP_OK;
    }
    return finish_device_call(e);
}

int oc_hip_matcher_match(oc_hip_engine* e, int mode, int* ref_idx, int* tar_idx, size_t capacity, size_t* n_pairs, int memory) {
    OC_TRY(check_matcher(e, "matcher_match"));
    OC_ACTIVATE(e);
    if (mode != 0 && mode != 1) return fail(OC_HIP_ERR_INVALID, "matcher_match: mode must be 0 (monodirectional) or 1 (bidirectional), got %d", mode);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "matcher_match: bad memory kind %d", memory);
    if (!n_pairs) return fail(OC_HIP_ERR_INVALID, "matcher_match: null n_pairs");
    *n_pairs = 0;
    if (capacity > 0 && (!ref_idx || !tar_idx)) return fail(OC_HIP_ERR_INVALID, "matcher_match: null output buffer");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    const size_t nr = e->mt_count[0], nt = e->mt_count[1];
    if (nr == 0 || nt == 0) return OC_HIP_OK;
    OC_TRY(order_after_default_stream(e));
    OC_TRY(run_nearest(e, 0));
    const float ratio_sq = e->mt_ratio * e->mt_ratio;
    const int* r2t = e->mt_idx[0].as<int>();
    const int* t2r = nullptr;
    const unsigned long long* keys = nullptr;
    if (mode == 1) {
        OC_TRY(run_nearest(e, 1));
        t2r = e->mt_idx[1].as<int>();
    } else {
        OC_TRY(e->mt_keys.reserve(2 * nt * sizeof(unsigned long long)));
        OC_HIP_TRY(ochip::launch_match_many_to_one(r2t, e->mt_best[0].as<float>(), nr, nt, e->mt_keys.as<unsigned long long>(), e->stream));
        keys = e->mt_keys.as<unsigned long long>();
    }
    const size_t words = ochip::match_pairs_scratch_words(nr, nt, mode);
    OC_TRY(e->mt_scan.reserve(words * sizeof(unsigned)));
    unsigned* scratch = e->mt_scan.as<unsigned>();
    OC_HIP_TRY(ochip::launch_match_pairs_count(mode, r2t, t2r, keys, nr, nt, ratio_sq, scratch, e->stream));
    unsigned total = 0;
    OC_HIP_TRY(hipMemcpyAsync(&total, scratch + (words - 2), sizeof(total), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    *n_pairs = total;
    if (total > capacity)
        return fail(OC_HIP_ERR_INVALID, "matcher_match: %u pairs do not fit the capacity of %zu (n_pairs carries the needed size)", total, capacity);
    if (total == 0) return OC_HIP_OK;
    int *d_ref = ref_idx, *d_tar = tar_idx;
    if (memory == OC_HIP_HOST) {
        OC_TRY(e->mt_pairs.reserve(2 * (size_t)total * sizeof(int)));
        d_ref = e->mt_pairs.as<int>();
        d_tar = d_ref + total;
    }
    OC_HIP_TRY(ochip::launch_match_pairs_scatter(mode, r2t, t2r, keys, nr, nt, ratio_sq, scratch, d_ref, d_tar, e->stream));
    if (memory == OC_HIP_HOST) {
        OC_HIP_TRY(hipMemcpyAsync(ref_idx, d_ref, total * sizeof(int), hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipMemcpyAsync(tar_idx, d_tar, total * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    }
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

}  // extern "C"

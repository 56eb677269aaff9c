// capi_sift3d.hip -- SIFT3D's scale space (part of the C-ABI of include/opencorr_hip.h): SIFT3D::createGaussianPyramid,
// createDogPyramid and detectExtrema of the reference (src/oc_sift.cpp:676-754, 756-793, 795-847) over the kernels of sift3d.hip.
// The layer table, the blur weights and the support verdict come from host/sift3d_plan.h.  Everything runs on the engine's stream.
#include "capi_internal.h"

static_assert(ochip::kSiftMaxRadius == ochip_host::kSift3dMaxRadius, "the plan admits what the kernels take");
static_assert(sizeof(oc_hip_sift3d_candidate) == 24 && sizeof(ochip::SiftCandidate) == 24, "a candidate is 24 bytes");

namespace {

int check_sift3d(const oc_hip_engine* e, const char* what) {
    OC_TRY(check_engine(e));
    if (!e->is_sift3d()) return fail(OC_HIP_ERR_INVALID, "%s: not a SIFT3D scale-space handle", what);
    return OC_HIP_OK;
}

int check_built(const oc_hip_engine* e, const char* what) {
    if (!e->sf_built) return fail(OC_HIP_ERR_INVALID, "%s: no pyramid yet (oc_hip_sift3d_build)", what);
    return OC_HIP_OK;
}

int check_layer(const oc_hip_engine* e, const char* what, int pyramid, int index) {
    if (pyramid != 0 && pyramid != 1) return fail(OC_HIP_ERR_INVALID, "%s: pyramid must be 0 (Gaussian) or 1 (DoG), got %d", what, pyramid);
    const int n = pyramid == 0 ? (int)e->sf_plan.gauss.size() : e->sf_plan.dog_layers();
    if (index < 0 || index >= n) return fail(OC_HIP_ERR_INVALID, "%s: layer %d out of range [0,%d)", what, index, n);
    return OC_HIP_OK;
}

ochip::SiftWeights weights_of(const std::vector<float>& w) {
    ochip::SiftWeights W{};
    for (size_t i = 0; i < w.size() && i <= (size_t)ochip::kSiftMaxRadius; i++) W.w[i] = w[i];
    return W;
}

// SIFT3D::gaussianBlur (:365-547): x pass src -> dst, y pass dst -> scratch, z pass scratch -> dst
int blur_layer(oc_hip_engine* e, const ochip_host::Sift3dLayer& g, const float* src, float* dst) {
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    float* scratch = e->sf_scratch.as<float>();
    const bool fma = e->arith_fma != 0;
    OC_HIP_TRY(ochip::launch_sift_blur_x(src, dst, nx, (size_t)ny * nz, weights_of(g.weight[0]), g.radius[0], fma, e->stream));
    OC_HIP_TRY(ochip::launch_sift_blur_strided(dst, scratch, (size_t)nz, ny, (size_t)nx, weights_of(g.weight[1]), g.radius[1], fma, e->stream));
    OC_HIP_TRY(ochip::launch_sift_blur_strided(scratch, dst, 1, nz, (size_t)nx * ny, weights_of(g.weight[2]), g.radius[2], fma, e->stream));
    return OC_HIP_OK;
}

// the DoG layers detectExtrema visits (:797-802), in its order, each with its place among the workgroups of all of them
std::vector<ochip::SiftExtremaLayer> extrema_layers(const oc_hip_engine* e, size_t* total_blocks) {
    const ochip_host::Sift3dPlan& p = e->sf_plan;
    std::vector<ochip::SiftExtremaLayer> layers;
    size_t blocks = 0;
    for (int m = 0; m < p.n_octave; m++)
        for (int n = 1; n < p.n_octave_layers + 1; n++) {
            const int d = m * p.dog_per_octave() + n;
            const ochip_host::Sift3dLayer& g = p.gauss[(size_t)p.dog_gauss(d)];
            if (g.dim[0] < 3 || g.dim[1] < 3 || g.dim[2] < 3) continue;  // (no voxel with 1 <= index <= dim - 2)
            ochip::SiftExtremaLayer L{};
            L.below = e->sf_dog[(size_t)d - 1].as<float>();
            L.here = e->sf_dog[(size_t)d].as<float>();
            L.above = e->sf_dog[(size_t)d + 1].as<float>();
            L.nx = g.dim[0], L.ny = g.dim[1], L.nz = g.dim[2];
            L.octave = m, L.layer = n;
            L.scale = g.scale;
            L.threshold = e->sf_cfg.alpha * e->sf_max_abs[(size_t)d];  // :812, a float32 product
            L.first_block = (unsigned)blocks;
            blocks += ochip::sift_extrema_blocks(g.voxels());
            layers.push_back(L);
        }
    *total_blocks = blocks;
    return layers;
}

}  // namespace

extern "C" {

int oc_hip_sift3d_create(int device, oc_hip_engine** out) {
    if (out) *out = nullptr;
    return create_engine(OC_HIP_SIFT3D, 1, 1, 0, 0.f, 0.f, device, out);
}

int oc_hip_sift3d_set_config(oc_hip_engine* e, int n_octave_layers, int min_dimension, float alpha, float sigma_source, float sigma_base) {
    OC_TRY(check_sift3d(e, "sift3d_set_config"));
    if (n_octave_layers < 1 || min_dimension < 1)
        return fail(OC_HIP_ERR_INVALID, "sift3d_set_config: n_octave_layers and min_dimension must be >= 1 (got %d, %d)", n_octave_layers, min_dimension);
    if (!std::isfinite(alpha) || !std::isfinite(sigma_source) || !std::isfinite(sigma_base))
        return fail(OC_HIP_ERR_INVALID, "sift3d_set_config: alpha, sigma_source and sigma_base must be finite");
    std::lock_guard<std::mutex> lock(e->mu);
    e->sf_cfg.n_octave_layers = n_octave_layers;
    e->sf_cfg.min_dimension = min_dimension;
    e->sf_cfg.alpha = alpha;
    e->sf_cfg.sigma_source = sigma_source;
    e->sf_cfg.sigma_base = sigma_base;
    e->sf_built = false;
    return OC_HIP_OK;
}

int oc_hip_sift3d_set_physical_unit(oc_hip_engine* e, float unit_x, float unit_y, float unit_z) {
    OC_TRY(check_sift3d(e, "sift3d_set_physical_unit"));
    const float u[3] = {unit_x, unit_y, unit_z};
    for (float v : u)
        if (!(v > 0) || !std::isfinite(v))
            return fail(OC_HIP_ERR_INVALID, "sift3d_set_physical_unit: units must be positive and finite (got %g, %g, %g)", (double)unit_x, (double)unit_y, (double)unit_z);
    std::lock_guard<std::mutex> lock(e->mu);
    for (int a = 0; a < 3; a++) e->sf_unit[a] = u[a];
    e->sf_built = false;
    return OC_HIP_OK;
}

int oc_hip_sift3d_set_volume(oc_hip_engine* e, const float* data, int dim_x, int dim_y, int dim_z, int memory) {
    OC_TRY(check_sift3d(e, "sift3d_set_volume"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift3d_set_volume: bad memory kind %d", memory);
    if (!data) return fail(OC_HIP_ERR_INVALID, "sift3d_set_volume: null volume");
    if (dim_x < 1 || dim_y < 1 || dim_z < 1) return fail(OC_HIP_ERR_INVALID, "sift3d_set_volume: dimensions must be >= 1 (got %d x %d x %d)", dim_x, dim_y, dim_z);
    if ((long long)dim_x * dim_y * dim_z > ochip_host::kSift3dMaxVoxels) return fail(OC_HIP_ERR_UNSUPPORTED, "sift3d: volumes of at most 2^31-1 voxels");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->sf_built = false;
    e->sf_ext = nullptr;
    e->sf_dim[0] = e->sf_dim[1] = e->sf_dim[2] = 0;
    if (memory == OC_HIP_DEVICE) {
        if (reinterpret_cast<uintptr_t>(data) & 3) return fail(OC_HIP_ERR_INVALID, "sift3d_set_volume: a device volume must be 4-byte aligned");
        e->sf_ext = data;
    } else {
        const size_t bytes = (size_t)dim_x * dim_y * dim_z * sizeof(float);
        drain_engine(e);  // (a grow releases the old block: nothing may still read it)
        OC_TRY(e->sf_vol.reserve(bytes));
        OC_HIP_TRY(hipMemcpyAsync(e->sf_vol.p, data, bytes, hipMemcpyHostToDevice, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));  // host buffers may be released by the caller
    }
    e->sf_dim[0] = dim_x, e->sf_dim[1] = dim_y, e->sf_dim[2] = dim_z;
    return OC_HIP_OK;
}

int oc_hip_sift3d_build(oc_hip_engine* e) {
    OC_TRY(check_sift3d(e, "sift3d_build"));
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->sf_built = false;
    e->sf_counted = false;
    if (e->sf_dim[0] < 1) return fail(OC_HIP_ERR_INVALID, "sift3d_build: no volume (oc_hip_sift3d_set_volume)");
    // the verdict comes first: nothing is allocated or launched for a volume or a setting outside the supported range
    ochip_host::Sift3dPlan plan = ochip_host::sift3d_plan(e->sf_cfg, e->sf_dim[0], e->sf_dim[1], e->sf_dim[2], e->sf_unit[0], e->sf_unit[1], e->sf_unit[2]);
    if (plan.status != OC_HIP_OK) return fail(plan.status, "%s", plan.why.c_str());
    const size_t n_gauss = plan.gauss.size(), n_dog = (size_t)plan.dog_layers();
    drain_engine(e);  // (a grow releases old blocks: nothing may still read them)
    if (e->sf_gauss.size() < n_gauss) e->sf_gauss.resize(n_gauss);
    if (e->sf_dog.size() < n_dog) e->sf_dog.resize(n_dog);
    OC_TRY(e->sf_scratch.reserve(plan.gauss[0].voxels() * sizeof(float)));
    OC_TRY(e->sf_max.reserve(n_dog * sizeof(unsigned)));
    for (size_t i = 0; i < n_gauss; i++) OC_TRY(e->sf_gauss[i].reserve(plan.gauss[i].voxels() * sizeof(float)));
    for (size_t d = 0; d < n_dog; d++) OC_TRY(e->sf_dog[d].reserve(plan.gauss[(size_t)plan.dog_gauss((int)d)].voxels() * sizeof(float)));
    OC_TRY(order_after_default_stream(e));
    const float* volume = e->sf_ext ? e->sf_ext : e->sf_vol.as<float>();
    for (size_t i = 0; i < n_gauss; i++) {
        const ochip_host::Sift3dLayer& g = plan.gauss[i];
        const float* src = g.source < 0 ? volume : e->sf_gauss[(size_t)g.source].as<float>();
        float* dst = e->sf_gauss[i].as<float>();
        if (g.blurred) {
            OC_TRY(blur_layer(e, g, src, dst));
        } else {
            const ochip_host::Sift3dLayer& s = plan.gauss[(size_t)g.source];
            OC_HIP_TRY(ochip::launch_sift_downsample(src, s.dim[0], s.dim[1], dst, g.dim[0], g.dim[1], g.dim[2], e->stream));
        }
    }
    OC_HIP_TRY(hipMemsetAsync(e->sf_max.p, 0, n_dog * sizeof(unsigned), e->stream));
    for (size_t d = 0; d < n_dog; d++) {
        const size_t gi = (size_t)plan.dog_gauss((int)d);
        OC_HIP_TRY(ochip::launch_sift_dog(e->sf_gauss[gi].as<float>(), e->sf_gauss[gi + 1].as<float>(), e->sf_dog[d].as<float>(), plan.gauss[gi].voxels(),
                                          e->sf_max.as<unsigned>() + d, e->stream));
    }
    std::vector<unsigned> bits(n_dog);
    OC_HIP_TRY(hipMemcpyAsync(bits.data(), e->sf_max.p, n_dog * sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    e->sf_max_abs.resize(n_dog);
    std::memcpy(e->sf_max_abs.data(), bits.data(), n_dog * sizeof(float));
    e->sf_plan = std::move(plan);
    e->sf_built = true;
    return OC_HIP_OK;
}

int oc_hip_sift3d_layer_count(const oc_hip_engine* e, int pyramid, int* n_layers, int* n_octave) {
    OC_TRY(check_sift3d(e, "sift3d_layer_count"));
    std::lock_guard<std::mutex> lock(e->mu);
    OC_TRY(check_built(e, "sift3d_layer_count"));
    if (pyramid != 0 && pyramid != 1) return fail(OC_HIP_ERR_INVALID, "sift3d_layer_count: pyramid must be 0 (Gaussian) or 1 (DoG), got %d", pyramid);
    if (n_layers) *n_layers = pyramid == 0 ? (int)e->sf_plan.gauss.size() : e->sf_plan.dog_layers();
    if (n_octave) *n_octave = e->sf_plan.n_octave;
    return OC_HIP_OK;
}

int oc_hip_sift3d_layer_info(const oc_hip_engine* e, int pyramid, int index, int* dims, float* units, int* octave, float* scale, float* sigma,
                             float* max_abs) {
    OC_TRY(check_sift3d(e, "sift3d_layer_info"));
    std::lock_guard<std::mutex> lock(e->mu);
    OC_TRY(check_built(e, "sift3d_layer_info"));
    OC_TRY(check_layer(e, "sift3d_layer_info", pyramid, index));
    const ochip_host::Sift3dLayer& g = e->sf_plan.gauss[(size_t)(pyramid == 0 ? index : e->sf_plan.dog_gauss(index))];
    for (int a = 0; a < 3; a++) {
        if (dims) dims[a] = g.dim[a];
        if (units) units[a] = g.unit[a];
    }
    if (octave) *octave = g.octave;
    if (scale) *scale = g.scale;
    if (sigma) *sigma = pyramid == 0 ? g.sigma : 0.f;
    if (max_abs) *max_abs = pyramid == 0 ? -1.f : e->sf_max_abs[(size_t)index];
    return OC_HIP_OK;
}

int oc_hip_sift3d_get_layer(oc_hip_engine* e, int pyramid, int index, float* out, int memory) {
    OC_TRY(check_sift3d(e, "sift3d_get_layer"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift3d_get_layer: bad memory kind %d", memory);
    if (!out) return fail(OC_HIP_ERR_INVALID, "sift3d_get_layer: null output buffer");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built(e, "sift3d_get_layer"));
    OC_TRY(check_layer(e, "sift3d_get_layer", pyramid, index));
    const size_t bytes = e->sf_plan.gauss[(size_t)(pyramid == 0 ? index : e->sf_plan.dog_gauss(index))].voxels() * sizeof(float);
    const void* src = pyramid == 0 ? e->sf_gauss[(size_t)index].p : e->sf_dog[(size_t)index].p;
    OC_TRY(order_after_default_stream(e));
    OC_HIP_TRY(hipMemcpyAsync(out, src, bytes, memory == OC_HIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    if (memory == OC_HIP_HOST) {
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return OC_HIP_OK;
    }
    return finish_device_call(e);
}

int oc_hip_sift3d_detect(oc_hip_engine* e, oc_hip_sift3d_candidate* out, size_t capacity, size_t* n, int memory) {
    OC_TRY(check_sift3d(e, "sift3d_detect"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift3d_detect: bad memory kind %d", memory);
    if (!n) return fail(OC_HIP_ERR_INVALID, "sift3d_detect: null n");
    *n = 0;
    if (capacity > 0 && !out) return fail(OC_HIP_ERR_INVALID, "sift3d_detect: null output buffer");
    if (memory == OC_HIP_DEVICE && (reinterpret_cast<uintptr_t>(out) & 3)) return fail(OC_HIP_ERR_INVALID, "sift3d_detect: a device list must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built(e, "sift3d_detect"));
    size_t blocks = 0;
    const std::vector<ochip::SiftExtremaLayer> layers = extrema_layers(e, &blocks);
    if (layers.empty()) return OC_HIP_OK;
    OC_TRY(order_after_default_stream(e));
    OC_TRY(e->sf_scan.reserve((2 * blocks + 2) * sizeof(unsigned)));
    unsigned* counts = e->sf_scan.as<unsigned>();
    unsigned* totals = counts + 2 * blocks;
    // (a caller that asks for the size first and for the list next pays for the count and the scan once: they belong to the
    // pyramid as built, and every build starts over)
    if (!e->sf_counted) {
        for (const ochip::SiftExtremaLayer& L : layers) OC_HIP_TRY(ochip::launch_sift_extrema_count(L, counts, e->stream));
        OC_HIP_TRY(ochip::launch_block_count_scan(counts, blocks, totals, e->stream));
        OC_HIP_TRY(hipMemcpyAsync(&e->sf_total, totals, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        e->sf_counted = true;
    }
    const unsigned total = e->sf_total;
    *n = total;
    if (total > capacity)
        return fail(OC_HIP_ERR_INVALID, "sift3d_detect: %u candidates do not fit the capacity of %zu (n carries the needed size)", total, capacity);
    if (total == 0) return OC_HIP_OK;
    ochip::SiftCandidate* d_out = reinterpret_cast<ochip::SiftCandidate*>(out);
    if (memory == OC_HIP_HOST) {
        OC_TRY(e->sf_list.reserve((size_t)total * sizeof(ochip::SiftCandidate)));
        d_out = e->sf_list.as<ochip::SiftCandidate>();
    }
    for (const ochip::SiftExtremaLayer& L : layers) OC_HIP_TRY(ochip::launch_sift_extrema_fill(L, counts, d_out, e->stream));
    if (memory == OC_HIP_HOST) OC_HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)total * sizeof(ochip::SiftCandidate), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

}  // extern "C"

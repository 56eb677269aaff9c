// capi_sift3d.hip -- SIFT3D's scale space (part of the C-ABI of include/opencorr_hip.h): SIFT3D::createGaussianPyramid,
// createDogPyramid and detectExtrema of the reference (src/oc_sift.cpp:676-754, 756-793, 795-847) over the kernels of sift3d.hip,
// and its orientation and descriptor stages, assignOrientation and constructDescriptor (:849-1049, 1051-1249), over those of
// sift3d_features.hip.  The layer table, the blur weights and the support verdict come from host/sift3d_plan.h; the Gaussian weight
// tables, the grid of the exact sums and what is refused from host/sift3d_feature_plan.h.  Everything runs on the engine's stream.
#include "capi_internal.h"

static_assert(ochip::kSiftMaxRadius == ochip_host::kSift3dMaxRadius, "the plan admits what the kernels take");
static_assert(sizeof(oc_hip_sift3d_candidate) == 24 && sizeof(ochip::SiftCandidate) == 24, "a candidate is 24 bytes");
static_assert(sizeof(oc_hip_sift3d_keypoint) == 72 && sizeof(ochip::SiftKeypoint) == 72, "a keypoint is 72 bytes");
static_assert(ochip::kSiftDescriptorLength == ochip_host::kSiftDescriptorLength, "one descriptor length");

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

// The candidates of the pyramid as built: their number in sf_total (count and scan happen once per build: a caller that asks for
// the size first and for the list next pays for them once) and, with `fill`, the list in sf_list, where it stays for
// oc_hip_sift3d_orient(candidates = NULL).
int candidate_list(oc_hip_engine* e, bool fill) {
    size_t blocks = 0;
    const std::vector<ochip::SiftExtremaLayer> layers = extrema_layers(e, &blocks);
    if (layers.empty()) {
        e->sf_total = 0;
        e->sf_counted = e->sf_listed = true;  // (an empty list is a list)
        return OC_HIP_OK;
    }
    OC_TRY(order_after_default_stream(e));
    OC_TRY(e->sf_scan.reserve((2 * blocks + 2) * sizeof(unsigned)));
    unsigned* counts = e->sf_scan.as<unsigned>();
    unsigned* totals = counts + 2 * blocks;
    if (!e->sf_counted) {
        for (const ochip::SiftExtremaLayer& L : layers) OC_HIP_TRY(ochip::launch_sift_extrema_count(L, counts, e->stream));
        OC_HIP_TRY(ochip::launch_block_count_scan(counts, blocks, totals, e->stream));
        OC_HIP_TRY(hipMemcpyAsync(&e->sf_total, totals, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        e->sf_counted = true;
    }
    if (!fill || e->sf_listed) return OC_HIP_OK;
    if (e->sf_total > 0) {
        OC_TRY(e->sf_list.reserve((size_t)e->sf_total * sizeof(ochip::SiftCandidate)));
        for (const ochip::SiftExtremaLayer& L : layers)
            OC_HIP_TRY(ochip::launch_sift_extrema_fill(L, counts, e->sf_list.as<ochip::SiftCandidate>(), e->stream));
    }
    e->sf_listed = true;
    return OC_HIP_OK;
}

// The weight tables and the layer records of the pyramid as built, on the device; the verdict of host/sift3d_feature_plan.h
// first: nothing is allocated or launched for a volume outside the supported range.
int ensure_features(oc_hip_engine* e) {
    if (e->sf_features) return OC_HIP_OK;
    ochip_host::Sift3dFeaturePlan plan = ochip_host::sift3d_feature_plan(e->sf_plan, e->sf_vol_max);
    if (plan.status != OC_HIP_OK) return fail(plan.status, "%s", plan.why.c_str());
    const size_t n = e->sf_plan.gauss.size();
    drain_engine(e);  // (a grow releases old blocks: nothing may still read them)
    // the uploads below read `plan`'s vectors and `layers`: whichever way this function leaves, they have completed first
    struct Settle {
        oc_hip_engine* e;
        ~Settle() {
            (void)hipStreamSynchronize(e->stream);
        }
    } settle{e};
    if (e->sf_ftables.size() < 2 * n) e->sf_ftables.resize(2 * n);
    std::vector<ochip::SiftFeatureLayer> layers(n);
    for (size_t i = 0; i < n; i++) {
        const ochip_host::Sift3dLayer& g = e->sf_plan.gauss[i];
        ochip::SiftFeatureLayer& L = layers[i];
        L = ochip::SiftFeatureLayer{};
        L.vol = e->sf_gauss[i].as<float>();
        L.scale = g.scale;
        for (int a = 0; a < 3; a++) {
            L.dim[a] = g.dim[a];
            L.unit[a] = g.unit[a];
        }
        const ochip_host::Sift3dFeatureTable* tables[2] = {&plan.orient[i], &plan.describe[i]};
        for (int s = 0; s < 2; s++) {
            const ochip_host::Sift3dFeatureTable& t = *tables[s];
            if (t.weight.empty()) continue;
            DevBuf& buf = e->sf_ftables[2 * i + (size_t)s];
            OC_TRY(buf.reserve(t.weight.size() * sizeof(float)));
            OC_HIP_TRY(hipMemcpyAsync(buf.p, t.weight.data(), t.weight.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
            (s == 0 ? L.orient : L.describe) = buf.as<float>();
            for (int a = 0; a < 3; a++) (s == 0 ? L.orient_half : L.describe_half)[a] = t.half[a];
        }
        L.orient_radius = plan.orient[i].radius;
        L.describe_radius = plan.describe[i].radius;
        L.cube_radius = plan.describe[i].cube_radius;
    }
    OC_TRY(e->sf_flayers.reserve(n * sizeof(ochip::SiftFeatureLayer)));
    OC_TRY(e->sf_flag.reserve(sizeof(unsigned)));
    OC_HIP_TRY(hipMemcpyAsync(e->sf_flayers.p, layers.data(), n * sizeof(ochip::SiftFeatureLayer), hipMemcpyHostToDevice, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    e->sf_fplan = std::move(plan);
    e->sf_features = true;
    return OC_HIP_OK;
}

ochip::SiftFeatureParams feature_params(const oc_hip_engine* e) {
    ochip::SiftFeatureParams p{};
    p.layers = e->sf_flayers.as<ochip::SiftFeatureLayer>();
    p.n_octave = e->sf_plan.n_octave;
    p.n_octave_layers = e->sf_plan.n_octave_layers;
    p.exponent = e->sf_fplan.exponent;
    p.beta = e->sf_fcfg.beta;
    p.gamma = e->sf_fcfg.gamma;
    p.gradient_threshold = e->sf_fcfg.gradient_threshold;
    p.truncate_threshold = e->sf_fcfg.truncate_threshold;
    return p;
}

// a HOST list staged in sf_in, a DEVICE list in place
template <class Record> int stage_list(oc_hip_engine* e, const char* what, const void* list, size_t n, int memory, const Record** d_list) {
    if (memory == OC_HIP_DEVICE) {
        if (reinterpret_cast<uintptr_t>(list) & 3) return fail(OC_HIP_ERR_INVALID, "%s: a device list must be 4-byte aligned", what);
        *d_list = static_cast<const Record*>(list);
        return OC_HIP_OK;
    }
    if (e->sf_in.bytes < n * sizeof(Record)) drain_engine(e);
    OC_TRY(e->sf_in.reserve(n * sizeof(Record)));
    OC_HIP_TRY(hipMemcpyAsync(e->sf_in.p, list, n * sizeof(Record), hipMemcpyHostToDevice, e->stream));
    *d_list = e->sf_in.as<Record>();
    return OC_HIP_OK;
}

// the records index the pyramid: a kernel reads the list where it lies and raises a flag, and nothing else is launched on a raised one
template <class Record, class Launch>
int check_list(oc_hip_engine* e, const char* what, const Record* d_list, size_t n, const ochip::SiftFeatureParams& p, Launch launch) {
    unsigned flag = 0;
    OC_HIP_TRY(hipMemsetAsync(e->sf_flag.p, 0, sizeof(unsigned), e->stream));
    OC_HIP_TRY(launch(d_list, n, p, e->sf_flag.as<unsigned>(), e->stream));
    OC_HIP_TRY(hipMemcpyAsync(&flag, e->sf_flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    if (flag)
        return fail(OC_HIP_ERR_INVALID,
                    "%s: a record names no layer keypoints lie in (octave, layer 1 ... n_octave_layers), a scale that is not that layer's, a "
                    "coordinate that is not an integer inside it, or a rotation entry that is not finite or beyond +-2", what);
    return OC_HIP_OK;
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
    e->sf_listed = e->sf_features = e->sf_oriented = false;
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
    OC_TRY(e->sf_vmax.reserve(sizeof(unsigned)));
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
    // max |v| of the volume: the grid of the exact sums of the orientation and descriptor stages (host/sift3d_feature_plan.h)
    unsigned volume_bits = 0;
    OC_HIP_TRY(hipMemsetAsync(e->sf_vmax.p, 0, sizeof(unsigned), e->stream));
    OC_HIP_TRY(ochip::launch_sift_max_abs(volume, plan.gauss[0].voxels(), e->sf_vmax.as<unsigned>(), e->stream));
    OC_HIP_TRY(hipMemcpyAsync(&volume_bits, e->sf_vmax.p, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    std::vector<unsigned> bits(n_dog);
    OC_HIP_TRY(hipMemcpyAsync(bits.data(), e->sf_max.p, n_dog * sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    std::memcpy(&e->sf_vol_max, &volume_bits, sizeof(float));
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
    OC_TRY(candidate_list(e, false));
    const unsigned total = e->sf_total;
    *n = total;
    if (total > capacity)
        return fail(OC_HIP_ERR_INVALID, "sift3d_detect: %u candidates do not fit the capacity of %zu (n carries the needed size)", total, capacity);
    if (total == 0) return OC_HIP_OK;
    OC_TRY(candidate_list(e, true));
    OC_HIP_TRY(hipMemcpyAsync(out, e->sf_list.p, (size_t)total * sizeof(ochip::SiftCandidate),
                              memory == OC_HIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

int oc_hip_sift3d_candidate_count(oc_hip_engine* e, size_t* n) {
    OC_TRY(check_sift3d(e, "sift3d_candidate_count"));
    OC_ACTIVATE(e);
    if (!n) return fail(OC_HIP_ERR_INVALID, "sift3d_candidate_count: null n");
    *n = 0;
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built(e, "sift3d_candidate_count"));
    OC_TRY(candidate_list(e, false));
    *n = e->sf_total;
    return OC_HIP_OK;
}

int oc_hip_sift3d_set_feature_config(oc_hip_engine* e, float beta, float gamma, float gradient_threshold, float truncate_threshold) {
    OC_TRY(check_sift3d(e, "sift3d_set_feature_config"));
    if (!std::isfinite(beta) || !std::isfinite(gamma) || !std::isfinite(gradient_threshold) || !std::isfinite(truncate_threshold))
        return fail(OC_HIP_ERR_INVALID, "sift3d_set_feature_config: beta, gamma, gradient_threshold and truncate_threshold must be finite");
    std::lock_guard<std::mutex> lock(e->mu);
    e->sf_fcfg.beta = beta;
    e->sf_fcfg.gamma = gamma;
    e->sf_fcfg.gradient_threshold = gradient_threshold;
    e->sf_fcfg.truncate_threshold = truncate_threshold;
    return OC_HIP_OK;
}

int oc_hip_sift3d_orient(oc_hip_engine* e, const oc_hip_sift3d_candidate* candidates, size_t n_candidates, int candidates_memory,
                         oc_hip_sift3d_keypoint* out, size_t capacity, size_t* n, int* status, float* sums, int memory) {
    OC_TRY(check_sift3d(e, "sift3d_orient"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift3d_orient: bad memory kind %d", memory);
    if (candidates && candidates_memory != OC_HIP_HOST && candidates_memory != OC_HIP_DEVICE)
        return fail(OC_HIP_ERR_INVALID, "sift3d_orient: bad memory kind %d of the candidates", candidates_memory);
    if (!n) return fail(OC_HIP_ERR_INVALID, "sift3d_orient: null n");
    *n = 0;
    if (capacity > 0 && !out) return fail(OC_HIP_ERR_INVALID, "sift3d_orient: null output buffer");
    if (memory == OC_HIP_DEVICE && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(sums)) & 3))
        return fail(OC_HIP_ERR_INVALID, "sift3d_orient: device outputs must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built(e, "sift3d_orient"));
    if (!candidates) {
        OC_TRY(candidate_list(e, true));
        n_candidates = e->sf_total;
    }
    if (n_candidates > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "sift3d_orient: at most 2^31-1 candidates per call");
    e->sf_oriented = false;
    if (n_candidates == 0) {
        e->sf_kp_count = 0;
        e->sf_oriented = true;
        return OC_HIP_OK;
    }
    OC_TRY(ensure_features(e));
    OC_TRY(order_after_default_stream(e));
    const ochip::SiftCandidate* d_list = e->sf_list.as<ochip::SiftCandidate>();
    if (candidates) OC_TRY(stage_list<ochip::SiftCandidate>(e, "sift3d_orient", candidates, n_candidates, candidates_memory, &d_list));
    const ochip::SiftFeatureParams p = feature_params(e);
    OC_TRY(check_list(e, "sift3d_orient", d_list, n_candidates, p, ochip::launch_sift_check_candidates));
    const size_t blocks = ochip::sift_orient_blocks(n_candidates);
    drain_engine(e);  // (a grow releases old blocks: nothing may still read them)
    OC_TRY(e->sf_status.reserve(n_candidates * sizeof(int)));
    OC_TRY(e->sf_sums.reserve(n_candidates * 9 * sizeof(float)));
    OC_TRY(e->sf_slots.reserve(n_candidates * sizeof(ochip::SiftKeypoint)));
    OC_TRY(e->sf_fscan.reserve((2 * blocks + 2) * sizeof(unsigned)));
    int* d_status = e->sf_status.as<int>();
    unsigned* counts = e->sf_fscan.as<unsigned>();
    unsigned* totals = counts + 2 * blocks;
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_sift_orient(d_list, n_candidates, p, d_status, e->sf_sums.as<float>(), e->sf_slots.as<ochip::SiftKeypoint>(), e->stream));
    }
    OC_HIP_TRY(ochip::launch_sift_orient_count(d_status, n_candidates, counts, e->stream));
    OC_HIP_TRY(ochip::launch_block_count_scan(counts, blocks, totals, e->stream));
    unsigned total = 0;
    OC_HIP_TRY(hipMemcpyAsync(&total, totals, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    OC_TRY(e->sf_kp.reserve((size_t)total * sizeof(ochip::SiftKeypoint)));
    if (total > 0)
        OC_HIP_TRY(ochip::launch_sift_orient_fill(d_status, e->sf_slots.as<ochip::SiftKeypoint>(), n_candidates, counts, e->sf_kp.as<ochip::SiftKeypoint>(),
                                                  e->stream));
    e->sf_kp_count = total;
    e->sf_oriented = true;
    *n = total;
    if (total > capacity) {
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return fail(OC_HIP_ERR_INVALID, "sift3d_orient: %u keypoints do not fit the capacity of %zu (n carries the needed size)", total, capacity);
    }
    const hipMemcpyKind kind = memory == OC_HIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (total > 0) OC_HIP_TRY(hipMemcpyAsync(out, e->sf_kp.p, (size_t)total * sizeof(ochip::SiftKeypoint), kind, e->stream));
    if (status) OC_HIP_TRY(hipMemcpyAsync(status, d_status, n_candidates * sizeof(int), kind, e->stream));
    if (sums) OC_HIP_TRY(hipMemcpyAsync(sums, e->sf_sums.p, n_candidates * 9 * sizeof(float), kind, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

int oc_hip_sift3d_describe(oc_hip_engine* e, const oc_hip_sift3d_keypoint* keypoints, size_t n, int keypoints_memory, float* descriptors, int memory) {
    OC_TRY(check_sift3d(e, "sift3d_describe"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift3d_describe: bad memory kind %d", memory);
    if (keypoints && keypoints_memory != OC_HIP_HOST && keypoints_memory != OC_HIP_DEVICE)
        return fail(OC_HIP_ERR_INVALID, "sift3d_describe: bad memory kind %d of the keypoints", keypoints_memory);
    if (memory == OC_HIP_DEVICE && (reinterpret_cast<uintptr_t>(descriptors) & 3))
        return fail(OC_HIP_ERR_INVALID, "sift3d_describe: a device block must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built(e, "sift3d_describe"));
    if (!keypoints) {
        if (!e->sf_oriented) return fail(OC_HIP_ERR_INVALID, "sift3d_describe: no keypoints on the device yet (oc_hip_sift3d_orient)");
        if (n != e->sf_kp_count) return fail(OC_HIP_ERR_INVALID, "sift3d_describe: the last orient left %zu keypoints, not %zu", e->sf_kp_count, n);
    }
    if (n > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "sift3d_describe: at most 2^31-1 keypoints per call");
    const bool keep = !descriptors && memory == OC_HIP_DEVICE;  // the block stays in the engine ("descriptors" of oc_hip_get_field)
    if (keep) e->sf_desc_floats = 0;
    if (n == 0) return OC_HIP_OK;
    if (!descriptors && !keep) return fail(OC_HIP_ERR_INVALID, "sift3d_describe: null output buffer");
    OC_TRY(ensure_features(e));
    OC_TRY(order_after_default_stream(e));
    const ochip::SiftKeypoint* d_list = e->sf_kp.as<ochip::SiftKeypoint>();
    if (keypoints) OC_TRY(stage_list<ochip::SiftKeypoint>(e, "sift3d_describe", keypoints, n, keypoints_memory, &d_list));
    const ochip::SiftFeatureParams p = feature_params(e);
    OC_TRY(check_list(e, "sift3d_describe", d_list, n, p, ochip::launch_sift_check_keypoints));
    float* d_out = descriptors;
    const size_t bytes = n * ochip::kSiftDescriptorLength * sizeof(float);
    if (memory == OC_HIP_HOST || keep) {
        e->sf_desc_floats = 0;  // (a HOST call stages in the same block)
        if (e->sf_desc.bytes < bytes) drain_engine(e);
        OC_TRY(e->sf_desc.reserve(bytes));
        d_out = e->sf_desc.as<float>();
    }
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_sift_describe(d_list, n, p, d_out, e->stream));
    }
    if (memory == OC_HIP_HOST) {
        OC_HIP_TRY(hipMemcpyAsync(descriptors, d_out, bytes, hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return OC_HIP_OK;
    }
    if (keep) e->sf_desc_floats = n * ochip::kSiftDescriptorLength;
    return finish_device_call(e);
}

}  // extern "C"

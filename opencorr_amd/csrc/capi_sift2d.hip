// capi_sift2d.hip -- SIFT2D's detector (part of the C-ABI of include/opencorr_hip.h): what cv::SIFT::detect does before it
// assigns orientations, for the cv::SIFT the reference's SIFT2D::compute() creates (src/oc_sift.cpp:22-30, 60-93), over the
// kernels of sift2d.hip.  The octave count, the layer table, the blur weights, the threshold and every refusal come from
// host/sift2d_plan.h.  Everything runs on the engine's stream; both pyramids and the keypoint list stay on the device.
#include "capi_internal.h"

static_assert(sizeof(oc_hip_sift2d_keypoint) == 48 && sizeof(ochip::Sift2dKeypoint) == 48, "a keypoint is 48 bytes");

namespace {

int check_sift2d(const oc_hip_engine* e, const char* what) {
    OC_TRY(check_engine(e));
    if (!e->is_sift2d()) return fail(OC_HIP_ERR_INVALID, "%s: not a SIFT2D detector handle", what);
    return OC_HIP_OK;
}

int check_built2d(const oc_hip_engine* e, const char* what) {
    if (!e->s2_built) return fail(OC_HIP_ERR_INVALID, "%s: no pyramid yet (oc_hip_sift2d_build)", what);
    return OC_HIP_OK;
}

int check_layer2d(const oc_hip_engine* e, const char* what, int pyramid, int index) {
    if (pyramid != 0 && pyramid != 1) return fail(OC_HIP_ERR_INVALID, "%s: pyramid must be 0 (Gaussian) or 1 (DoG), got %d", what, pyramid);
    const int n = pyramid == 0 ? (int)e->s2_plan.gauss.size() : e->s2_plan.dog_layers();
    if (index < 0 || index >= n) return fail(OC_HIP_ERR_INVALID, "%s: layer %d out of range [0,%d)", what, index, n);
    return OC_HIP_OK;
}

ochip::SiftWeights weights2d(const std::vector<float>& w) {
    ochip::SiftWeights W{};
    for (size_t i = 0; i < w.size() && i <= (size_t)ochip::kSift2dMaxRadius; i++) W.w[i] = w[i];
    return W;
}

// the DoG layers the scan visits, in its order (octave, layer 1 ... n_octave_layers), each with its place among the workgroups
std::vector<ochip::Sift2dExtremaLayer> scan_layers(const oc_hip_engine* e, size_t* total_blocks) {
    const ochip_host::Sift2dPlan& p = e->s2_plan;
    std::vector<ochip::Sift2dExtremaLayer> layers;
    size_t blocks = 0;
    for (int o = 0; o < p.n_octave; o++)
        for (int n = 1; n <= p.n_octave_layers; n++) {
            const int d = o * p.dog_per_octave() + n;
            const ochip_host::Sift2dLayer& g = p.gauss[(size_t)p.dog_gauss(d)];
            if (g.cols <= 2 * ochip_host::kSift2dBorder || g.rows <= 2 * ochip_host::kSift2dBorder) continue;  // (an empty scan region)
            ochip::Sift2dExtremaLayer L{};
            L.below = e->s2_dog[(size_t)d - 1].as<float>();
            L.here = e->s2_dog[(size_t)d].as<float>();
            L.above = e->s2_dog[(size_t)d + 1].as<float>();
            L.cols = g.cols, L.rows = g.rows, L.octave = o, L.layer = n;
            L.threshold = (float)p.threshold;
            L.first_block = (unsigned)blocks;
            blocks += ochip::sift_extrema_blocks(g.pixels());
            layers.push_back(L);
        }
    *total_blocks = blocks;
    return layers;
}

// The located keypoints of the pyramid as built, in s2_kp, once per build: scan (count, exclusive scan, fill), localisation with
// one thread per start, and the order-preserving compaction of the located ones.
int detect_list(oc_hip_engine* e) {
    if (e->s2_detected) return OC_HIP_OK;
    size_t blocks = 0;
    const std::vector<ochip::Sift2dExtremaLayer> layers = scan_layers(e, &blocks);
    e->s2_kp_count = 0;
    if (layers.empty()) {
        e->s2_detected = true;
        return OC_HIP_OK;
    }
    OC_TRY(order_after_default_stream(e));
    drain_engine(e);  // (a grow releases old blocks: nothing may still read them)
    OC_TRY(e->s2_scan.reserve((2 * blocks + 2) * sizeof(unsigned)));
    unsigned* counts = e->s2_scan.as<unsigned>();
    unsigned* totals = counts + 2 * blocks;
    unsigned n_starts = 0;
    for (const ochip::Sift2dExtremaLayer& L : layers) OC_HIP_TRY(ochip::launch_sift2d_extrema_count(L, counts, e->stream));
    OC_HIP_TRY(ochip::launch_block_count_scan(counts, blocks, totals, e->stream));
    OC_HIP_TRY(hipMemcpyAsync(&n_starts, totals, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    if (n_starts == 0) {
        e->s2_detected = true;
        return OC_HIP_OK;
    }
    const size_t kblocks = ochip::sift_orient_blocks(n_starts);
    OC_TRY(e->s2_starts.reserve((size_t)n_starts * sizeof(ochip::Sift2dStart)));
    OC_TRY(e->s2_status.reserve((size_t)n_starts * sizeof(int)));
    OC_TRY(e->s2_slots.reserve((size_t)n_starts * sizeof(ochip::Sift2dKeypoint)));
    OC_TRY(e->s2_kscan.reserve((2 * kblocks + 2) * sizeof(unsigned)));
    for (const ochip::Sift2dExtremaLayer& L : layers)
        OC_HIP_TRY(ochip::launch_sift2d_extrema_fill(L, counts, e->s2_starts.as<ochip::Sift2dStart>(), e->stream));
    ochip::Sift2dLocalizeParams p{};
    p.dog = e->s2_table.as<ochip::Sift2dDogLayer>();
    p.n_octave = e->s2_plan.n_octave;
    p.n_octave_layers = e->s2_plan.n_octave_layers;
    p.contrast_threshold = e->s2_cfg.contrast_threshold;
    p.edge_threshold = e->s2_cfg.edge_threshold;
    p.sigma = e->s2_cfg.sigma;
    int* status = e->s2_status.as<int>();
    unsigned* kcounts = e->s2_kscan.as<unsigned>();
    unsigned* ktotals = kcounts + 2 * kblocks;
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_sift2d_localize(e->s2_starts.as<ochip::Sift2dStart>(), n_starts, p, status, e->s2_slots.as<ochip::Sift2dKeypoint>(), e->stream));
    }
    OC_HIP_TRY(ochip::launch_sift_orient_count(status, n_starts, kcounts, e->stream));
    OC_HIP_TRY(ochip::launch_block_count_scan(kcounts, kblocks, ktotals, e->stream));
    unsigned total = 0;
    OC_HIP_TRY(hipMemcpyAsync(&total, ktotals, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    if (total > 0) {
        OC_TRY(e->s2_kp.reserve((size_t)total * sizeof(ochip::Sift2dKeypoint)));
        OC_HIP_TRY(ochip::launch_sift2d_fill(status, e->s2_slots.as<ochip::Sift2dKeypoint>(), n_starts, kcounts, e->s2_kp.as<ochip::Sift2dKeypoint>(), e->stream));
    }
    e->s2_kp_count = total;
    e->s2_detected = true;
    return OC_HIP_OK;
}

}  // namespace

extern "C" {

// SIFT2D::SIFT2D() (src/oc_sift.cpp:22-30)
int oc_hip_sift2d_create(int device, oc_hip_engine** out) {
    if (out) *out = nullptr;
    return create_engine(OC_HIP_SIFT2D, 1, 1, 0, 0.f, 0.f, device, out);
}

// SIFT2D::setSiftConfig (:44-47), cv::SIFT::create (:65-70)
int oc_hip_sift2d_set_config(oc_hip_engine* e, int n_features, int n_octave_layers, float contrast_threshold, float edge_threshold, float sigma) {
    OC_TRY(check_sift2d(e, "sift2d_set_config"));
    ochip_host::Sift2dSettings cfg;
    cfg.n_features = n_features, cfg.n_octave_layers = n_octave_layers, cfg.contrast_threshold = contrast_threshold;
    cfg.edge_threshold = edge_threshold, cfg.sigma = sigma;
    // the verdict on the settings alone (any image the plan accepts shows it)
    const ochip_host::Sift2dPlan verdict = ochip_host::sift2d_plan(cfg, 16, 16);
    if (verdict.status != OC_HIP_OK) return fail(verdict.status, "%s", verdict.why.c_str());
    std::lock_guard<std::mutex> lock(e->mu);
    e->s2_cfg = cfg;
    e->s2_built = e->s2_detected = false;
    return OC_HIP_OK;
}

// the image cv::SIFT::detect is given (:86)
int oc_hip_sift2d_set_image(oc_hip_engine* e, const void* data, int pixel_type, int width, int height, int memory) {
    OC_TRY(check_sift2d(e, "sift2d_set_image"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift2d_set_image: bad memory kind %d", memory);
    if (pixel_type != 0 && pixel_type != 1) return fail(OC_HIP_ERR_INVALID, "sift2d_set_image: pixel_type must be 0 (uint8) or 1 (float32), got %d", pixel_type);
    if (!data) return fail(OC_HIP_ERR_INVALID, "sift2d_set_image: null image");
    if (width < 2 || height < 2) return fail(OC_HIP_ERR_INVALID, "sift2d_set_image: image sides must be >= 2 (got %d x %d)", width, height);
    if (4ll * width * height > ochip_host::kSift2dMaxPixels) return fail(OC_HIP_ERR_UNSUPPORTED, "sift2d: doubled base images of at most 2^31-1 pixels");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->s2_built = e->s2_detected = false;
    e->s2_ext = nullptr;
    e->s2_width = e->s2_height = 0;
    if (memory == OC_HIP_DEVICE) {
        if (pixel_type == 1 && (reinterpret_cast<uintptr_t>(data) & 3)) return fail(OC_HIP_ERR_INVALID, "sift2d_set_image: a float32 device image must be 4-byte aligned");
        e->s2_ext = data;
    } else {
        const size_t bytes = (size_t)width * height * (pixel_type == 1 ? sizeof(float) : 1);
        drain_engine(e);  // (a grow releases the old block: nothing may still read it)
        OC_TRY(e->s2_img.reserve(bytes));
        OC_HIP_TRY(hipMemcpyAsync(e->s2_img.p, data, bytes, hipMemcpyHostToDevice, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));  // host buffers may be released by the caller
    }
    e->s2_u8 = pixel_type == 0;
    e->s2_width = width, e->s2_height = height;
    return OC_HIP_OK;
}

// the pyramids of cv::SIFT::detect (:86)
int oc_hip_sift2d_build(oc_hip_engine* e) {
    OC_TRY(check_sift2d(e, "sift2d_build"));
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->s2_built = e->s2_detected = false;
    if (e->s2_width < 1) return fail(OC_HIP_ERR_INVALID, "sift2d_build: no image (oc_hip_sift2d_set_image)");
    // the verdict comes first: nothing is allocated or launched for an image or a setting outside the supported range
    ochip_host::Sift2dPlan plan = ochip_host::sift2d_plan(e->s2_cfg, e->s2_width, e->s2_height);
    if (plan.status != OC_HIP_OK) return fail(plan.status, "%s", plan.why.c_str());
    const size_t n_gauss = plan.gauss.size(), n_dog = (size_t)plan.dog_layers();
    drain_engine(e);  // (a grow releases old blocks: nothing may still read them)
    if (e->s2_gauss.size() < n_gauss) e->s2_gauss.resize(n_gauss);
    if (e->s2_dog.size() < n_dog) e->s2_dog.resize(n_dog);
    const size_t base_bytes = plan.gauss[0].pixels() * sizeof(float);
    OC_TRY(e->s2_base.reserve(base_bytes));
    OC_TRY(e->s2_scratch.reserve(base_bytes));
    OC_TRY(e->s2_flag.reserve(sizeof(unsigned)));
    OC_TRY(e->s2_table.reserve(n_dog * sizeof(ochip::Sift2dDogLayer)));
    for (size_t i = 0; i < n_gauss; i++) OC_TRY(e->s2_gauss[i].reserve(plan.gauss[i].pixels() * sizeof(float)));
    std::vector<ochip::Sift2dDogLayer> table(n_dog);
    for (size_t d = 0; d < n_dog; d++) {
        const ochip_host::Sift2dLayer& g = plan.gauss[(size_t)plan.dog_gauss((int)d)];
        OC_TRY(e->s2_dog[d].reserve(g.pixels() * sizeof(float)));
        table[d] = ochip::Sift2dDogLayer{e->s2_dog[d].as<float>(), g.cols, g.rows};
    }
    OC_TRY(order_after_default_stream(e));
    // the upload below reads `table`, the read-back writes `flag`: whichever way this function leaves, they have completed first
    struct Settle {
        oc_hip_engine* e;
        ~Settle() {
            (void)hipStreamSynchronize(e->stream);
        }
    } settle{e};
    const void* image = e->s2_ext ? e->s2_ext : e->s2_img.p;
    float* scratch = e->s2_scratch.as<float>();
    unsigned flag = 0;
    OC_HIP_TRY(hipMemsetAsync(e->s2_flag.p, 0, sizeof(unsigned), e->stream));
    OC_HIP_TRY(hipMemcpyAsync(e->s2_table.p, table.data(), n_dog * sizeof(ochip::Sift2dDogLayer), hipMemcpyHostToDevice, e->stream));
    OC_HIP_TRY(ochip::launch_sift2d_upscale(image, e->s2_u8, e->s2_width, e->s2_height, e->s2_base.as<float>(), e->s2_flag.as<unsigned>(), e->stream));
    OC_HIP_TRY(hipMemcpyAsync(&flag, e->s2_flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));  // (`table` and `flag` have been read and written)
    if (flag) return fail(OC_HIP_ERR_INVALID, "sift2d_build: the image has a pixel that is not finite");
    {
        ProfScope prof(e);
        for (size_t i = 0; i < n_gauss; i++) {
            const ochip_host::Sift2dLayer& g = plan.gauss[i];
            const float* src = g.source < 0 ? e->s2_base.as<float>() : e->s2_gauss[(size_t)g.source].as<float>();
            float* dst = e->s2_gauss[i].as<float>();
            if (!g.blurred) {
                const ochip_host::Sift2dLayer& s = plan.gauss[(size_t)g.source];
                OC_HIP_TRY(ochip::launch_sift2d_resample(src, s.cols, s.rows, dst, g.cols, g.rows, e->stream));
                continue;
            }
            const ochip::SiftWeights W = weights2d(g.weight);
            OC_HIP_TRY(ochip::launch_sift2d_blur_rows(src, scratch, g.cols, g.rows, W, g.radius, e->stream));
            // dog[i - 1] = gauss[i] - gauss[i - 1] leaves with the write of gauss[i]
            float* dog = g.index > 0 ? e->s2_dog[(size_t)(g.octave * plan.dog_per_octave() + g.index - 1)].as<float>() : nullptr;
            OC_HIP_TRY(ochip::launch_sift2d_blur_cols(scratch, dst, g.cols, g.rows, W, g.radius, dog ? src : nullptr, dog, e->stream));
        }
    }
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    e->s2_plan = std::move(plan);
    e->s2_built = true;
    return OC_HIP_OK;
}

// (:86)
int oc_hip_sift2d_layer_count(const oc_hip_engine* e, int pyramid, int* n_layers, int* n_octave) {
    OC_TRY(check_sift2d(e, "sift2d_layer_count"));
    std::lock_guard<std::mutex> lock(e->mu);
    OC_TRY(check_built2d(e, "sift2d_layer_count"));
    if (pyramid != 0 && pyramid != 1) return fail(OC_HIP_ERR_INVALID, "sift2d_layer_count: pyramid must be 0 (Gaussian) or 1 (DoG), got %d", pyramid);
    if (n_layers) *n_layers = pyramid == 0 ? (int)e->s2_plan.gauss.size() : e->s2_plan.dog_layers();
    if (n_octave) *n_octave = e->s2_plan.n_octave;
    return OC_HIP_OK;
}

// (:86)
int oc_hip_sift2d_layer_info(const oc_hip_engine* e, int pyramid, int index, int* dims, int* octave, float* sigma, int* radius, int* threshold) {
    OC_TRY(check_sift2d(e, "sift2d_layer_info"));
    std::lock_guard<std::mutex> lock(e->mu);
    OC_TRY(check_built2d(e, "sift2d_layer_info"));
    OC_TRY(check_layer2d(e, "sift2d_layer_info", pyramid, index));
    const ochip_host::Sift2dLayer& g = e->s2_plan.gauss[(size_t)(pyramid == 0 ? index : e->s2_plan.dog_gauss(index))];
    if (dims) dims[0] = g.cols, dims[1] = g.rows;
    if (octave) *octave = g.octave;
    if (sigma) *sigma = pyramid == 0 ? g.sigma : 0.f;
    if (radius) *radius = pyramid == 0 ? g.radius : 0;
    if (threshold) *threshold = e->s2_plan.threshold;
    return OC_HIP_OK;
}

// (:86)
int oc_hip_sift2d_get_layer(oc_hip_engine* e, int pyramid, int index, float* out, int memory) {
    OC_TRY(check_sift2d(e, "sift2d_get_layer"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift2d_get_layer: bad memory kind %d", memory);
    if (!out) return fail(OC_HIP_ERR_INVALID, "sift2d_get_layer: null output buffer");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built2d(e, "sift2d_get_layer"));
    OC_TRY(check_layer2d(e, "sift2d_get_layer", pyramid, index));
    const size_t bytes = e->s2_plan.gauss[(size_t)(pyramid == 0 ? index : e->s2_plan.dog_gauss(index))].pixels() * sizeof(float);
    const void* src = pyramid == 0 ? e->s2_gauss[(size_t)index].p : e->s2_dog[(size_t)index].p;
    OC_TRY(order_after_default_stream(e));
    OC_HIP_TRY(hipMemcpyAsync(out, src, bytes, memory == OC_HIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    if (memory == OC_HIP_HOST) {
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return OC_HIP_OK;
    }
    return finish_device_call(e);
}

// (:86)
int oc_hip_sift2d_keypoint_count(oc_hip_engine* e, size_t* n) {
    OC_TRY(check_sift2d(e, "sift2d_keypoint_count"));
    OC_ACTIVATE(e);
    if (!n) return fail(OC_HIP_ERR_INVALID, "sift2d_keypoint_count: null n");
    *n = 0;
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built2d(e, "sift2d_keypoint_count"));
    OC_TRY(detect_list(e));
    *n = e->s2_kp_count;
    return OC_HIP_OK;
}

// (:86)
int oc_hip_sift2d_detect(oc_hip_engine* e, oc_hip_sift2d_keypoint* out, size_t capacity, size_t* n, int memory) {
    OC_TRY(check_sift2d(e, "sift2d_detect"));
    OC_ACTIVATE(e);
    if (memory != OC_HIP_HOST && memory != OC_HIP_DEVICE) return fail(OC_HIP_ERR_INVALID, "sift2d_detect: bad memory kind %d", memory);
    if (!n) return fail(OC_HIP_ERR_INVALID, "sift2d_detect: null n");
    *n = 0;
    if (capacity > 0 && !out) return fail(OC_HIP_ERR_INVALID, "sift2d_detect: null output buffer");
    if (memory == OC_HIP_DEVICE && (reinterpret_cast<uintptr_t>(out) & 3)) return fail(OC_HIP_ERR_INVALID, "sift2d_detect: a device list must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    OC_TRY(check_built2d(e, "sift2d_detect"));
    OC_TRY(detect_list(e));
    const size_t total = e->s2_kp_count;
    *n = total;
    if (total > capacity)
        return fail(OC_HIP_ERR_INVALID, "sift2d_detect: %zu keypoints do not fit the capacity of %zu (n carries the needed size)", total, capacity);
    if (total == 0) return OC_HIP_OK;
    OC_HIP_TRY(hipMemcpyAsync(out, e->s2_kp.p, total * sizeof(ochip::Sift2dKeypoint), memory == OC_HIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                              e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

}  // extern "C"

// capi_stereo.hip -- Calibration and Stereovision (part of the C-ABI of include/opencorr_hip.h): the small matrices are host
// code in float32, the undistortion map, the undistortion of points and the reconstruction are the kernels of stereo.hip.
#include "capi_internal.h"

namespace ochip_capi {

// Calibration / Stereovision handles are created by host arithmetic; their stream is made by the first entry point that
// activates the device (capi_internal.h activate()).
int make_own_stream(oc_hip_engine* e) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (e->own_stream) return OC_HIP_OK;
    hipStream_t s = nullptr;
    OC_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (e->stream == nullptr) e->stream = s;
    e->own_stream = s;
    return OC_HIP_OK;
}

}  // namespace ochip_capi

namespace {

// coefficient-wise product with ascending inner index: first term, then the others added one by one
void matmul(const float* a, const float* b, float* out, int rows, int inner, int cols) {
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++) {
            float v = a[i * inner] * b[j];
            for (int k = 1; k < inner; k++) v = v + a[i * inner + k] * b[k * cols + j];
            out[i * cols + j] = v;
        }
}

// 3 x 3 inverse as cofactors over the determinant (Eigen's compute_inverse for size 3)
float cof3(const float* m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}

void inverse3(const float* m, float* r) {
    const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
    const float det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
    const float invdet = 1.f / det;
    r[0] = c0 * invdet;
    r[1] = c1 * invdet;
    r[2] = c2 * invdet;
    for (int i = 1; i < 3; i++)
        for (int j = 0; j < 3; j++) r[i * 3 + j] = cof3(m, j, i) * invdet;
}

// Calibration::updateMatrices, src/oc_calibration.cpp:36-85
int update_matrices(oc_hip_engine* e) {
    const float* ci = e->cal_i;  // fx fy fs cx cy ...
    const float* ce = e->cal_e;  // tx ty tz rx ry rz
    float* K = e->cal_K;
    // :36-48
    K[0] = ci[0]; K[1] = ci[2]; K[2] = ci[3];
    K[3] = 0.f;   K[4] = ci[1]; K[5] = ci[4];
    K[6] = 0.f;   K[7] = 0.f;   K[8] = 1.f;
    // isIdentity() with Eigen's default precision: an off-diagonal entry counts as zero when it is <= 1e-5 beside 1
    if (std::fabs(K[0] - 1.f) <= 1e-5f && std::fabs(K[4] - 1.f) <= 1e-5f && std::fabs(K[1]) <= 1e-5f && std::fabs(K[2]) <= 1e-5f &&
        std::fabs(K[5]) <= 1e-5f)
        return fail(OC_HIP_ERR_INVALID, "Null intrinsics matrix");
    // :50-60 -- angle |r| about r / |r|, AngleAxisf::toRotationMatrix.  The zero vector is the identity: the reference gets it
    // from normalize() leaving a zero vector alone (sin 0 = 0, cos 0 = 1); here it is a case of its own
    float* R = e->cal_R;
    float ax[3] = {ce[3], ce[4], ce[5]};
    float n2 = 0.f;
    for (int i = 0; i < 3; i++) n2 = n2 + ax[i] * ax[i];
    if (!(n2 > 0.f) && n2 == n2) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
    } else {
        const float theta = std::sqrt(n2);
        for (int i = 0; i < 3; i++) ax[i] = ax[i] / theta;
        const float s = std::sin(theta), c = std::cos(theta);
        const float sx = s * ax[0], sy = s * ax[1], sz = s * ax[2];
        const float cx = (1.f - c) * ax[0], cy = (1.f - c) * ax[1], cz = (1.f - c) * ax[2];
        float tmp = cx * ax[1];
        R[1] = tmp - sz;
        R[3] = tmp + sz;
        tmp = cx * ax[2];
        R[2] = tmp + sy;
        R[6] = tmp - sy;
        tmp = cy * ax[2];
        R[5] = tmp - sx;
        R[7] = tmp + sx;
        R[0] = cx * ax[0] + c;
        R[4] = cy * ax[1] + c;
        R[8] = cz * ax[2] + c;
    }
    // :62-67
    for (int i = 0; i < 3; i++) e->cal_T[i] = ce[i];
    // :69-77
    float rt[12];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) rt[i * 4 + j] = R[i * 3 + j];
        rt[i * 4 + 3] = e->cal_T[i];
    }
    matmul(K, rt, e->cal_P, 3, 3, 4);
    return OC_HIP_OK;
}

ochip::CameraParams camera_params(const oc_hip_engine* e) {
    const float* c = e->cal_i;
    return ochip::CameraParams{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12]};
}

int camera_view(const oc_hip_engine* cam, ochip::CameraView* v) {
    if (cam->cal_h < 2 || cam->cal_w < 2 || !cam->cal_map_x.p || !cam->cal_map_y.p)
        return fail(OC_HIP_ERR_INVALID, "Calibration: prepare(height, width) has not been called");
    v->cam = camera_params(cam);
    v->map_x = cam->cal_map_x.as<float>();
    v->map_y = cam->cal_map_y.as<float>();
    v->height = cam->cal_h;
    v->width = cam->cal_w;
    for (int i = 0; i < 12; i++) v->proj[i] = cam->cal_P[i];
    return OC_HIP_OK;
}

int check_kind(const oc_hip_engine* e, int kind, const char* what) {
    OC_TRY(check_engine(e));
    if (e->kind != kind) return fail(OC_HIP_ERR_INVALID, "%s: not a %s handle", what, kind == OC_HIP_CALIBRATION ? "Calibration" : "Stereovision");
    return OC_HIP_OK;
}

int check_stride(size_t stride_bytes, size_t rec_bytes, const char* what) {
    if (stride_bytes < rec_bytes || (stride_bytes & 3))
        return fail(OC_HIP_ERR_INVALID, "%s: bad stride %zu (record is %zu bytes, stride must be a multiple of 4)", what, stride_bytes, rec_bytes);
    return OC_HIP_OK;
}

int stereo_views(oc_hip_engine* e, ochip::CameraView* v1, ochip::CameraView* v2) {
    OC_TRY(camera_view(e->stereo_cam[0], v1));
    OC_TRY(camera_view(e->stereo_cam[1], v2));
    return OC_HIP_OK;
}

}  // namespace

extern "C" {

int oc_hip_calibration_create(const float intrinsics[13], const float extrinsics[6], int device, oc_hip_engine** out) {
    if (!out) return fail(OC_HIP_ERR_INVALID, "null output handle");
    *out = nullptr;
    if (!intrinsics || !extrinsics) return fail(OC_HIP_ERR_INVALID, "Calibration: null intrinsics / extrinsics");
    if (device < 0) return fail(OC_HIP_ERR_INVALID, "device %d out of range", device);
    std::unique_ptr<oc_hip_engine> e(new oc_hip_engine);
    e->kind = OC_HIP_CALIBRATION;
    e->device = device;
    std::memcpy(e->cal_i, intrinsics, sizeof(e->cal_i));
    std::memcpy(e->cal_e, extrinsics, sizeof(e->cal_e));
    OC_TRY(update_matrices(e.get()));
    *out = e.release();
    return OC_HIP_OK;
}

int oc_hip_calibration_set_undistortion(oc_hip_engine* e, float convergence, int iteration) {
    OC_TRY(check_kind(e, OC_HIP_CALIBRATION, "set_undistortion"));
    std::lock_guard<std::mutex> lock(e->mu);
    e->cal_conv = convergence;
    e->cal_iter = iteration;
    return OC_HIP_OK;
}

int oc_hip_calibration_get(const oc_hip_engine* e, int what, float* out) {
    OC_TRY(check_kind(e, OC_HIP_CALIBRATION, "calibration_get"));
    if (!out) return fail(OC_HIP_ERR_INVALID, "calibration_get: null output");
    switch (what) {
    case OC_HIP_CAL_INTRINSIC: std::memcpy(out, e->cal_K, sizeof(e->cal_K)); break;
    case OC_HIP_CAL_ROTATION: std::memcpy(out, e->cal_R, sizeof(e->cal_R)); break;
    case OC_HIP_CAL_TRANSLATION: std::memcpy(out, e->cal_T, sizeof(e->cal_T)); break;
    case OC_HIP_CAL_PROJECTION: std::memcpy(out, e->cal_P, sizeof(e->cal_P)); break;
    default: return fail(OC_HIP_ERR_INVALID, "calibration_get: unknown matrix %d", what);
    }
    return OC_HIP_OK;
}

int oc_hip_calibration_prepare(oc_hip_engine* e, int height, int width) {
    OC_TRY(check_kind(e, OC_HIP_CALIBRATION, "calibration_prepare"));
    if (height < 2 || width < 2 || (size_t)height * (size_t)width > 0x7fffffffull)
        return fail(OC_HIP_ERR_INVALID, "Calibration::prepare: height and width must be >= 2 (got %d x %d)", height, width);
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    e->cal_h = e->cal_w = 0;
    const size_t bytes = (size_t)height * width * sizeof(float);
    OC_TRY(e->cal_map_x.reserve(bytes));
    OC_TRY(e->cal_map_y.reserve(bytes));
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_undistort_map(camera_params(e), height, width, e->cal_conv, e->cal_iter, e->cal_map_x.as<float>(),
                                               e->cal_map_y.as<float>(), e->stream));
    }
    // a Stereovision handle reads the map on a stream of its own: the map is complete when this call returns
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    e->cal_h = height;
    e->cal_w = width;
    return OC_HIP_OK;
}

int oc_hip_calibration_maps(oc_hip_engine* e, float* map_x, float* map_y, int memory) {
    OC_TRY(check_kind(e, OC_HIP_CALIBRATION, "calibration_maps"));
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    if (e->cal_h < 2) return fail(OC_HIP_ERR_INVALID, "Calibration: prepare(height, width) has not been called");
    const size_t bytes = (size_t)e->cal_h * e->cal_w * sizeof(float);
    const hipMemcpyKind kind = memory == OC_HIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (map_x) OC_HIP_TRY(hipMemcpyAsync(map_x, e->cal_map_x.p, bytes, kind, e->stream));
    if (map_y) OC_HIP_TRY(hipMemcpyAsync(map_y, e->cal_map_y.p, bytes, kind, e->stream));
    if (memory == OC_HIP_DEVICE) return finish_device_call(e);
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

int oc_hip_calibration_undistort(oc_hip_engine* e, const void* in, void* out, size_t count, size_t stride_bytes, int memory) {
    OC_TRY(check_kind(e, OC_HIP_CALIBRATION, "calibration_undistort"));
    if (count == 0) return OC_HIP_OK;
    if (!in || !out) return fail(OC_HIP_ERR_INVALID, "calibration_undistort: null buffer");
    OC_TRY(check_stride(stride_bytes, 8, "calibration_undistort"));
    if (count > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "calibration_undistort: at most 2^31-1 points per call");
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    ochip::CameraView v;
    OC_TRY(camera_view(e, &v));
    OC_TRY(order_after_default_stream(e));
    const int stride_f = (int)(stride_bytes / 4);
    if (memory == OC_HIP_DEVICE) {
        OC_HIP_TRY(ochip::launch_undistort_points(v, static_cast<const float*>(in), static_cast<float*>(out), stride_f, count, e->stream));
        return finish_device_call(e);
    }
    const size_t bytes = count * stride_bytes;
    OC_TRY(e->cal_stage.reserve(bytes));
    OC_HIP_TRY(hipMemcpyAsync(e->cal_stage.p, in, bytes, hipMemcpyHostToDevice, e->stream));
    OC_HIP_TRY(ochip::launch_undistort_points(v, e->cal_stage.as<float>(), e->cal_stage.as<float>(), stride_f, count, e->stream));
    // only the coordinate pairs travel back: what the caller keeps between them stays
    OC_HIP_TRY(hipMemcpy2DAsync(out, stride_bytes, e->cal_stage.p, stride_bytes, 8, count, hipMemcpyDeviceToHost, e->stream));
    OC_HIP_TRY(hipStreamSynchronize(e->stream));
    return OC_HIP_OK;
}

int oc_hip_stereo_create(oc_hip_engine* cam1, oc_hip_engine* cam2, oc_hip_engine** out) {
    if (!out) return fail(OC_HIP_ERR_INVALID, "null output handle");
    *out = nullptr;
    OC_TRY(check_kind(cam1, OC_HIP_CALIBRATION, "stereo_create"));
    OC_TRY(check_kind(cam2, OC_HIP_CALIBRATION, "stereo_create"));
    if (cam1->device != cam2->device)
        return fail(OC_HIP_ERR_INVALID, "Stereovision: the two cameras live on devices %d and %d", cam1->device, cam2->device);
    std::unique_ptr<oc_hip_engine> e(new oc_hip_engine);
    e->kind = OC_HIP_STEREOVISION;
    e->device = cam1->device;
    e->stereo_cam[0] = cam1;
    e->stereo_cam[1] = cam2;
    *out = e.release();
    return OC_HIP_OK;
}

int oc_hip_stereo_fundamental(oc_hip_engine* e, float out[9]) {
    OC_TRY(check_kind(e, OC_HIP_STEREOVISION, "stereo_fundamental"));
    if (!out) return fail(OC_HIP_ERR_INVALID, "stereo_fundamental: null output");
    std::lock_guard<std::mutex> lock(e->mu);
    const oc_hip_engine* c1 = e->stereo_cam[0];
    const oc_hip_engine* c2 = e->stereo_cam[1];
    // src/oc_stereovision.cpp:36-54
    float inv2[9], right_invK_t[9];
    inverse3(c2->cal_K, inv2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) right_invK_t[i * 3 + j] = inv2[j * 3 + i];
    const float* t = c2->cal_T;
    const float anti[9] = {0.f, -t[2], t[1], t[2], 0.f, -t[0], -t[1], t[0], 0.f};
    float right_E[9], left_K[9], tmp[9];
    matmul(anti, c2->cal_R, right_E, 3, 3, 3);
    inverse3(c1->cal_K, left_K);
    matmul(right_invK_t, right_E, tmp, 3, 3, 3);
    matmul(tmp, left_K, e->stereo_F, 3, 3, 3);
    std::memcpy(out, e->stereo_F, sizeof(e->stereo_F));
    return OC_HIP_OK;
}

int oc_hip_stereo_reconstruct(oc_hip_engine* e, const void* p1, size_t stride1, const void* p2, size_t stride2, void* out,
                              size_t stride_out, size_t count, int memory) {
    OC_TRY(check_kind(e, OC_HIP_STEREOVISION, "stereo_reconstruct"));
    if (count == 0) return OC_HIP_OK;
    if (!p1 || !p2 || !out) return fail(OC_HIP_ERR_INVALID, "stereo_reconstruct: null buffer");
    OC_TRY(check_stride(stride1, 8, "stereo_reconstruct (view 1)"));
    OC_TRY(check_stride(stride2, 8, "stereo_reconstruct (view 2)"));
    OC_TRY(check_stride(stride_out, 12, "stereo_reconstruct (3D points)"));
    if (count > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "stereo_reconstruct: at most 2^31-1 points per call");
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    ochip::CameraView v1, v2;
    OC_TRY(stereo_views(e, &v1, &v2));
    OC_TRY(order_after_default_stream(e));
    if (memory == OC_HIP_DEVICE) {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_reconstruct(v1, v2, static_cast<const float*>(p1), (int)(stride1 / 4), static_cast<const float*>(p2),
                                             (int)(stride2 / 4), static_cast<float*>(out), (int)(stride_out / 4), count, e->stream));
    } else {
        // packed copies on the device: 2 + 2 floats in, 3 floats out per point
        OC_TRY(e->cal_stage.reserve(count * 28));
        float* d1 = e->cal_stage.as<float>();
        float* d2 = d1 + 2 * count;
        float* d3 = d2 + 2 * count;
        OC_HIP_TRY(hipMemcpy2DAsync(d1, 8, p1, stride1, 8, count, hipMemcpyHostToDevice, e->stream));
        OC_HIP_TRY(hipMemcpy2DAsync(d2, 8, p2, stride2, 8, count, hipMemcpyHostToDevice, e->stream));
        {
            ProfScope prof(e);
            OC_HIP_TRY(ochip::launch_reconstruct(v1, v2, d1, 2, d2, 2, d3, 3, count, e->stream));
        }
        OC_HIP_TRY(hipMemcpy2DAsync(out, stride_out, d3, 12, 12, count, hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return OC_HIP_OK;
    }
    return finish_device_call(e);
}

int oc_hip_stereo_reconstruct_pois(oc_hip_engine* e, void* pois, size_t count, size_t stride_bytes, int memory) {
    OC_TRY(check_kind(e, OC_HIP_STEREOVISION, "stereo_reconstruct_pois"));
    if (count == 0) return OC_HIP_OK;
    if (!pois) return fail(OC_HIP_ERR_INVALID, "stereo_reconstruct_pois: null POI buffer");
    OC_TRY(check_stride(stride_bytes, OC_HIP_POI2DS_BYTES, "stereo_reconstruct_pois"));
    if (count > 0x7fffffffull) return fail(OC_HIP_ERR_UNSUPPORTED, "stereo_reconstruct_pois: at most 2^31-1 POIs per queue");
    OC_ACTIVATE(e);
    std::lock_guard<std::mutex> lock(e->mu);
    TailGuard tail(e);
    ochip::CameraView v1, v2;
    OC_TRY(stereo_views(e, &v1, &v2));
    OC_TRY(order_after_default_stream(e));
    const int stride_f = (int)(stride_bytes / 4);
    float* d_pois = static_cast<float*>(pois);
    if (memory == OC_HIP_HOST) {
        OC_TRY(e->poi_stage.reserve(count * stride_bytes));
        OC_HIP_TRY(hipMemcpyAsync(e->poi_stage.p, pois, count * stride_bytes, hipMemcpyHostToDevice, e->stream));
        d_pois = e->poi_stage.as<float>();
    }
    {
        ProfScope prof(e);
        OC_HIP_TRY(ochip::launch_reconstruct_pois(v1, v2, d_pois, stride_f, count, e->stream));
    }
    if (memory == OC_HIP_HOST) {
        OC_HIP_TRY(hipMemcpy2DAsync(pois, stride_bytes, d_pois, stride_bytes, OC_HIP_POI2DS_BYTES, count, hipMemcpyDeviceToHost, e->stream));
        OC_HIP_TRY(hipStreamSynchronize(e->stream));
        return OC_HIP_OK;
    }
    return finish_device_call(e);
}

}  // extern "C"

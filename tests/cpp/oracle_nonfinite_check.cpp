// oracle_nonfinite_check.cpp -- a stand-alone program around oracle/oc_oracle.cpp and the two one-pass twins
// (tests/cpp/icgn2d_onepass_twin.cpp, tests/cpp/icgn3d_onepass_twin.cpp): it solves the queues of a job file and prints every
// record as hexadecimal words.  tests/test_oracle_nonfinite.py builds it twice with g++ -- as it is, and with
// -fsanitize=undefined,address,float-cast-overflow -- and feeds it the queues of tests/nonfinite_cases.py: both builds must
// print the same records, and the sanitized one must stay silent, i.e. no (int)NaN, no index formed from one, is reachable.
//
// Job file (native endianness): any number of jobs, each
//   int32 x 16: engine, order, lanes, self_adaptive, has_offsets, d0, d1, d2 (2D: height, width, 0; 3D: dz, dy, dx), rx, ry, rz,
//               n, stop, stride (25 / 31), 0, 0
//   float conv
//   float ref[d0 * d1 (* d2)], tar[same], queue[n * stride], offsets[n * 2] if has_offsets
// engine: 0 ICGN2D1, 1 ICGN2D2, 2 ICLM2D1, 3 ICLM2D2 (default damping), 4 NR2D1, 5 ICGN3D1, 6 FFTCC2D, 7 / 8 the one-pass twin of
// ICGN2D1 / ICGN2D2, 9 the one-pass twin of ICGN3D1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oracle/oc_oracle.h"

extern "C" void oc_twin_icgn2d_onepass(int dof, const float* ref, const float* gx, const float* gy, const float* lut, int height,
                                       int width, int rx, int ry, float conv, float stop, float* pois, long n, int stride_floats);
extern "C" void oc_twin_icgn3d_onepass(const float* ref, const float* gx, const float* gy, const float* gz, const float* coef, int dz,
                                       int dy, int dx, int rx, int ry, int rz, float conv, float stop, float* pois, long n,
                                       int stride_floats);

namespace {

bool read_exact(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

bool read_floats(std::FILE* f, std::vector<float>& v, size_t n) {
    v.resize(n);
    return n == 0 || read_exact(f, v.data(), n * sizeof(float));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s JOBFILE\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t h[16];
    int job = 0;
    while (std::fread(h, sizeof(int32_t), 16, f) == 16) {
        const int engine = h[0], order = h[1], lanes = h[2], self_adaptive = h[3], has_offsets = h[4];
        const int d0 = h[5], d1 = h[6], d2 = h[7], rx = h[8], ry = h[9], rz = h[10], n = h[11], stop = h[12], stride = h[13];
        const bool is3d = engine == 5 || engine == 9;
        if (d0 <= 0 || d1 <= 0 || d2 < 0 || n < 0 || (is3d ? d2 <= 0 : d2 != 0) || stride != (is3d ? OC_POI3D_FLOATS : OC_POI2D_FLOATS)) {
            std::fprintf(stderr, "job %d: bad header\n", job);
            return 2;
        }
        float conv;
        std::vector<float> ref, tar, q, off;
        const size_t vox = (size_t)d0 * d1 * (is3d ? d2 : 1);
        if (!read_exact(f, &conv, sizeof conv) || !read_floats(f, ref, vox) || !read_floats(f, tar, vox) ||
            !read_floats(f, q, (size_t)n * stride) || !read_floats(f, off, has_offsets ? (size_t)n * 2 : 0)) {
            std::fprintf(stderr, "job %d: truncated\n", job);
            return 2;
        }
        const float* offp = has_offsets ? off.data() : nullptr;
        if (is3d) {
            std::vector<float> gx(vox), gy(vox), gz(vox), coef(vox);
            oc_oracle_gradient3d(ref.data(), d0, d1, d2, gx.data(), gy.data(), gz.data(), 1);
            oc_oracle_bspline3d_prefilter(tar.data(), d0, d1, d2, coef.data(), 1);
            if (engine == 5)
                oc_oracle_icgn3d1(ref.data(), gx.data(), gy.data(), gz.data(), coef.data(), d0, d1, d2, rx, ry, rz, conv, (float)stop,
                                  q.data(), n, order, lanes, 1);
            else
                oc_twin_icgn3d_onepass(ref.data(), gx.data(), gy.data(), gz.data(), coef.data(), d0, d1, d2, rx, ry, rz, conv, (float)stop,
                                       q.data(), n, stride);
        } else if (engine == 6) {
            oc_oracle_fftcc2d(ref.data(), tar.data(), d0, d1, rx, ry, q.data(), n, 1, nullptr);
        } else if (engine == 4) {
            std::vector<float> tgx(vox), tgy(vox), lut(vox * 16), lgx(vox * 16), lgy(vox * 16);
            oc_oracle_gradient2d(tar.data(), d0, d1, tgx.data(), tgy.data(), 1);
            oc_oracle_bspline2d_lut(tar.data(), d0, d1, lut.data(), 1);
            oc_oracle_bspline2d_lut(tgx.data(), d0, d1, lgx.data(), 1);
            oc_oracle_bspline2d_lut(tgy.data(), d0, d1, lgy.data(), 1);
            oc_oracle_nr2d1(ref.data(), lut.data(), lgx.data(), lgy.data(), d0, d1, rx, ry, conv, (float)stop, q.data(), n, order, lanes, 1);
        } else {
            std::vector<float> gx(vox), gy(vox), lut(vox * 16);
            oc_oracle_gradient2d(ref.data(), d0, d1, gx.data(), gy.data(), 1);
            oc_oracle_bspline2d_lut(tar.data(), d0, d1, lut.data(), 1);
            const float damping[3] = {100.f, 0.1f, 10.f};
            switch (engine) {
                case 0:
                    oc_oracle_icgn2d1_ex(ref.data(), gx.data(), gy.data(), lut.data(), d0, d1, rx, ry, conv, (float)stop, q.data(), n, order,
                                         lanes, 1, offp, self_adaptive);
                    break;
                case 1:
                    oc_oracle_icgn2d2_ex(ref.data(), gx.data(), gy.data(), lut.data(), d0, d1, rx, ry, conv, (float)stop, q.data(), n, order,
                                         lanes, 1, offp, self_adaptive);
                    break;
                case 2:
                case 3:
                    oc_oracle_iclm2d(engine == 2 ? 6 : 12, ref.data(), gx.data(), gy.data(), lut.data(), d0, d1, rx, ry, conv, (float)stop,
                                     damping, self_adaptive, q.data(), n, stride, order, lanes, 1);
                    break;
                case 7:
                case 8:
                    oc_twin_icgn2d_onepass(engine == 7 ? 6 : 12, ref.data(), gx.data(), gy.data(), lut.data(), d0, d1, rx, ry, conv,
                                           (float)stop, q.data(), n, stride);
                    break;
                default:
                    std::fprintf(stderr, "job %d: unknown engine %d\n", job, engine);
                    return 2;
            }
        }
        std::printf("job %d engine %d n %d\n", job, engine, n);
        for (int i = 0; i < n; i++) {
            for (int k = 0; k < stride; k++) {
                uint32_t w;
                std::memcpy(&w, &q[(size_t)i * stride + k], sizeof w);
                std::printf(k ? " %08x" : "%08x", w);
            }
            std::printf("\n");
        }
        job++;
    }
    std::fclose(f);
    return 0;
}

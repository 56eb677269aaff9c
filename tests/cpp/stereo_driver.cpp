// stereo_driver.cpp -- exercises the stereo classes of include/opencorr_compat/oc_stereo.h (Calibration, Stereovision,
// EpipolarSearch), Strain for POI2DS and IO2D::loadTable2DS / saveTable2DS on data handed over by pytest.
//
//   stereo_driver io <in.csv> <out.csv>          loadTable2DS -> saveTable2DS                                   (no GPU)
//   stereo_driver matrices <in.bin> <out.bin>    in: 2 x (13 + 6) floats; out: K, R, t, P of both cameras, then F (no GPU)
//   stereo_driver epipolar <in.bin> <out.bin>    in: int32 height, width, rx, ry, n, search_radius, search_step; float32 conv, stop;
//                                                2 x (13 + 6) camera floats; parallax_x[3], parallax_y[3]; ref[h*w], tar[h*w]
//                                                (row-major); x[n], y[n]
//                                                out: F (9 floats); n POI2D of EpipolarSearch::compute(poi_queue); n POI2D of
//                                                epipolarCandidates + ICGN2D1::computeBestOf with Stereovision's F; n POI2D of
//                                                EpipolarSearch::compute(POI2D*) for the first 3 POIs (the others zero)
//   stereo_driver chain <in.bin> <out.bin>       in: int32 height, width, n; float32 radius; int32 neighbours; 2 x (13 + 6)
//                                                camera floats; n POI2DS records
//                                                out: n POI2DS after Stereovision::reconstruct(queue) + Strain::prepare / compute
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "opencorr_compat/opencorr.h"

using namespace opencorr;

static bool read_all(FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

static void cameras(const float* c, Calibration& cam1, Calibration& cam2) {
    CameraIntrinsics i1, i2;
    CameraExtrinsics e1, e2;
    std::memcpy(i1.cam_i, c, 52);
    std::memcpy(e1.cam_e, c + 13, 24);
    std::memcpy(i2.cam_i, c + 19, 52);
    std::memcpy(e2.cam_e, c + 32, 24);
    cam1.updateCalibration(i1, e1);
    cam2.updateCalibration(i2, e2);
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "io") {
            IO2D in_out;
            in_out.setDelimiter(",");
            in_out.setPath(argv[2]);
            std::vector<POI2DS> q = in_out.loadTable2DS();
            in_out.setPath(argv[3]);
            in_out.saveTable2DS(q);
            return 0;
        }
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) return 3;
        FILE* out = std::fopen(argv[3], "wb");
        if (!out) return 3;
        if (mode == "matrices") {
            float c[38];
            if (!read_all(f, c, sizeof(c))) return 4;
            Calibration cam1, cam2;
            cameras(c, cam1, cam2);
            Stereovision stereo(&cam1, &cam2, 1);
            stereo.prepare();
            for (Calibration* cam : {&cam1, &cam2}) {
                std::fwrite(cam->intrinsic_matrix.data(), 4, 9, out);
                std::fwrite(cam->rotation_matrix.data(), 4, 9, out);
                std::fwrite(cam->translation_vector.data(), 4, 3, out);
                std::fwrite(cam->projection_matrix.data(), 4, 12, out);
            }
            std::fwrite(stereo.fundamental_matrix.data(), 4, 9, out);
            // the reference's accessors
            if (cam1.intrinsic_matrix(0, 2) != cam1.intrinsics.cx || cam2.translation_vector(1) != cam2.extrinsics.ty || cam1.projection_matrix.cols() != 4) return 9;
        } else if (mode == "epipolar") {
            int hdr[7];
            float it[2], c[38], px[3], py[3];
            if (!read_all(f, hdr, sizeof(hdr)) || !read_all(f, it, sizeof(it)) || !read_all(f, c, sizeof(c)) || !read_all(f, px, 12) || !read_all(f, py, 12)) return 4;
            const int h = hdr[0], w = hdr[1], rx = hdr[2], ry = hdr[3], n = hdr[4];
            std::vector<float> ref((size_t)h * w), tar((size_t)h * w), xs(n), ys(n);
            if (!read_all(f, ref.data(), ref.size() * 4) || !read_all(f, tar.data(), tar.size() * 4) || !read_all(f, xs.data(), n * 4) || !read_all(f, ys.data(), n * 4)) return 5;
            Image2D ref_img(w, h), tar_img(w, h);
            ref_img.fromRowMajor(ref.data());
            tar_img.fromRowMajor(tar.data());
            std::vector<POI2D> start;
            for (int i = 0; i < n; i++) start.push_back(POI2D(Point2D(xs[i], ys[i])));
            Calibration cam1, cam2;
            cameras(c, cam1, cam2);
            // the class, called as examples/test_3d_reconstruction_epipolar.cpp:139-171 calls it
            EpipolarSearch* epipolar_search = new EpipolarSearch(cam1, cam2, 4);
            epipolar_search->setParallax(px, py);
            epipolar_search->setSearch(hdr[5], hdr[6]);
            epipolar_search->createICGN(rx, ry, it[0], it[1]);
            epipolar_search->setImages(ref_img, tar_img);
            epipolar_search->prepare();
            std::vector<POI2D> by_class = start;
            epipolar_search->compute(by_class);
            // its parts: Stereovision's fundamental matrix -> epipolarCandidates -> computeBestOf
            Stereovision stereo(&cam1, &cam2, 4);
            stereo.prepare();
            EpipolarSearchSetting s;
            for (int i = 0; i < 9; i++) s.fundamental_matrix[i] = stereo.fundamental_matrix.data()[i];
            for (int i = 0; i < 3; i++) {
                s.parallax_x[i] = px[i];
                s.parallax_y[i] = py[i];
            }
            s.search_radius = hdr[5];
            s.search_step = hdr[6];
            s.subset_radius_x = rx;
            s.subset_radius_y = ry;
            s.image_width = w;
            s.image_height = h;
            std::vector<POI2D> by_parts = start, candidates;
            std::vector<unsigned> segment_starts;
            epipolarCandidates(by_parts, s, candidates, segment_starts);
            ICGN2D1 icgn1(rx, ry, it[0], it[1], 4);
            icgn1.setImages(ref_img, tar_img);
            icgn1.prepare();
            icgn1.computeBestOf(candidates, segment_starts, by_parts);
            // the single-POI form
            std::vector<POI2D> singles = start;
            for (POI2D& p : singles) p.x = p.y = 0.f;
            for (int i = 0; i < 3 && i < n; i++) {
                singles[i] = start[i];
                epipolar_search->compute(&singles[i]);
            }
            std::fwrite(stereo.fundamental_matrix.data(), 4, 9, out);
            std::fwrite(by_class.data(), sizeof(POI2D), by_class.size(), out);
            std::fwrite(by_parts.data(), sizeof(POI2D), by_parts.size(), out);
            std::fwrite(singles.data(), sizeof(POI2D), singles.size(), out);
            delete epipolar_search;
        } else if (mode == "chain") {
            int hdr[3], nmin;
            float radius, c[38];
            if (!read_all(f, hdr, sizeof(hdr)) || !read_all(f, &radius, 4) || !read_all(f, &nmin, 4) || !read_all(f, c, sizeof(c))) return 4;
            std::vector<POI2DS> q((size_t)hdr[2], POI2DS(0.f, 0.f));
            if (!read_all(f, q.data(), q.size() * sizeof(POI2DS))) return 5;
            Calibration cam1, cam2;
            cameras(c, cam1, cam2);
            cam1.prepare(hdr[0], hdr[1]);
            cam2.prepare(hdr[0], hdr[1]);
            Stereovision stereo(&cam1, &cam2, 4);
            stereo.prepare();
            stereo.reconstruct(q);
            // the array form and the single-pair form agree with the record form
            std::vector<Point2D> v1, v2;
            for (const POI2DS& p : q) {
                v1.push_back(Point2D(p.x, p.y));
                v2.push_back(Point2D(p.result.r2_x, p.result.r2_y));
            }
            std::vector<Point3D> pts(q.size());
            stereo.reconstruct(v1, v2, pts);
            for (size_t i = 0; i < q.size(); i++)
                if (std::memcmp(&pts[i], &q[i].ref_coor, sizeof(Point3D)) != 0) return 9;
            if (!q.empty()) {
                Point3D one = stereo.reconstruct(v1[0], v2[0]);
                if (std::memcmp(&one, &pts[0], sizeof(Point3D)) != 0) return 10;
            }
            Strain* strain = new Strain(radius, nmin, 4);
            strain->prepare(q);
            strain->compute(q);
            delete strain;
            std::fwrite(q.data(), sizeof(POI2DS), q.size(), out);
        } else {
            return 2;
        }
        std::fclose(f);
        std::fclose(out);
    } catch (const std::string& msg) {
        std::cerr << "stereo_driver: " << msg << std::endl;
        return 7;
    }
    return 0;
}

"""The host side of the stereo chain (no GPU): exported symbols, the Calibration matrices, the fundamental matrix, the POI2DS
table format, and the NumPy restatement (tests/stereo_numpy.py) pinned on the reference's own GT4 result table BEFORE the
GPU is measured against it.

Figures the restatement has to keep against the table (maxima over all 9 997 rows; the measurement that picked the GT4 table
as the anchor): float32 undistortion + least-squares triangulation reproduces ref_x, ref_y, ref_z within 6.2e-5, 1.8e-5,
3.1e-4 and tar_x, tar_y, tar_z within 7.3e-5, 2.3e-5, 2.5e-4 (z is about 393, float32 ulp 3e-5); solving in float64 or float32
makes no visible difference; u, v, w equal tar - ref within 2.5e-7; the float64 strain fit reproduces the six strains of the
9 987 rows that pass the three ZNCC gates within 2.7e-4, 8.2e-6, 2.4e-4, 1.4e-4, 6.9e-4, 7.0e-4.  The other 10 rows fail their
own gate; the program that wrote the table had no per-POI gate, the source as it stands has one (src/oc_strain.cpp:363-365):
they are not compared.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import opencorr_amd
from opencorr_amd import capi, io
from oracle import ref as oref

import epipolar_case as ec
import stereo_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "opencorr_amd", "lib")
T = sn.T

# the first rows of examples/3d_dic/GT4-0273_0_epipolar_sift_r16.csv as the reference's program wrote them
CSV_HEAD = """x,y,u,v,w,r1r2 ZNCC,r1t1 ZNCC,r1t2 ZNCC,r2_x,r2_y,t1_x,t1_y,t2_x,t2_y,ref_x,ref_y,ref_z,tar_x,tar_y,tar_z,exx,eyy,ezz,exy,eyz,ezx
234,135,-4.04184341,-0.76217842,0.88442993,0.96850073,0.99491721,0.95749855,188.2503662,74.72184753,166.9600067,123.1402206,115.4577637,60.4112854,-37.60477829,-26.23824501,393.3672485,-41.6466217,-27.00042343,394.2516785,-0.0015749,-0.00211355,-0.05832024,-0.00481462,-0.02333627,-0.02186193
234,144,-4.03266907,-0.76305962,0.87860107,0.97191882,0.99503356,0.96278977,188.2015381,84.04255676,167.1051025,132.0861359,115.5844269,69.73632812,-37.60469055,-25.70654869,393.3648987,-41.63735962,-26.46960831,394.2434998,-0.00588725,-0.00186241,0.01785528,0.00846684,0.05169706,-0.02846305
234,153,-4.02384186,-0.76404762,0.88046265,0.97181445,0.99471194,0.9627524,188.1716003,93.30827332,167.2576904,141.0367889,115.6952591,79.01472473,-37.60427475,-25.17622948,393.3592529,-41.62811661,-25.9402771,394.2397156,-0.01263448,-0.00162354,0.37401003,0.01018812,0.06174982,-0.01422531
"""
HEADER_2DS = ("x,y,u,v,w,r1r2 ZNCC,r1t1 ZNCC,r1t2 ZNCC,r2_x,r2_y,t1_x,t1_y,t2_x,t2_y,ref_x,ref_y,ref_z,tar_x,tar_y,tar_z,exx,eyy,ezz,"
              "exy,eyz,ezx,subset_rx,subset_ry,")


@pytest.fixture(scope="module")
def fx():
    return sn.load_fixture()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stereo") / "stereo_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stereo_driver.cpp"), "-o", exe, "-L" + LIBDIR, "-lopencorr_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_library_exports_the_stereo_entry_points():
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("oc_hip_calibration_create", "oc_hip_calibration_set_undistortion", "oc_hip_calibration_prepare",
                 "oc_hip_calibration_get", "oc_hip_calibration_maps", "oc_hip_calibration_undistort", "oc_hip_stereo_create",
                 "oc_hip_stereo_fundamental", "oc_hip_stereo_reconstruct", "oc_hip_stereo_reconstruct_pois"):
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert capi.lib().oc_hip_abi_version() == 3          # entries were added, none changed
    assert capi.POI2DS not in (2, 3) and capi.POI2DS_BYTES == 112 and len(opencorr_amd.P2S) == 28


def _ulps(got, want64):
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / ulp


def test_calibration_matrices_against_float64_rodrigues(fx):
    for k in ("cam1", "cam2"):
        cam = opencorr_amd.Calibration(fx[k + "_intrinsics"], fx[k + "_extrinsics"])
        K, R, t, P = sn.matrices64(fx[k + "_intrinsics"], fx[k + "_extrinsics"])
        assert np.array_equal(cam.intrinsic_matrix, K.astype(np.float32))
        assert np.array_equal(cam.translation_vector, t.astype(np.float32))
        assert _ulps(cam.rotation_matrix, R).max() <= 2
        assert _ulps(cam.projection_matrix, P).max() <= 2
        kind = ctypes.c_int()
        capi.check(capi.lib().oc_hip_get_kind(cam._h, ctypes.byref(kind)))
        assert kind.value == capi.CALIBRATION
        cam.close()


def test_zero_rotation_vector_is_the_exact_identity(fx):
    cam = opencorr_amd.Calibration(fx["cam1_intrinsics"], np.array([1.5, -2.0, 3.0, 0, 0, 0], dtype=np.float32))
    assert np.array_equal(cam.rotation_matrix.view(np.uint32), np.eye(3, dtype=np.float32).view(np.uint32))
    P = cam.projection_matrix
    assert np.array_equal(P[:, :3], cam.intrinsic_matrix)
    # a tiny rotation vector is NOT treated as zero
    cam2 = opencorr_amd.Calibration(fx["cam1_intrinsics"], np.array([0, 0, 0, 1e-20, 0, 0], dtype=np.float32))
    assert np.isfinite(cam2.rotation_matrix).all() and np.allclose(cam2.rotation_matrix, np.eye(3), atol=1e-7)


def test_null_intrinsics_are_an_error_code():
    bad = np.zeros(13, dtype=np.float32)
    bad[0] = bad[1] = 1.0     # fx = fy = 1, everything else 0: the intrinsic matrix is the identity (src/oc_calibration.cpp:44-47)
    with pytest.raises(capi.OpenCorrHipError) as err:
        opencorr_amd.Calibration(bad, np.zeros(6, dtype=np.float32))
    assert err.value.status == capi.ERR_INVALID and "Null intrinsics" in str(err.value)
    h = ctypes.c_void_p()
    assert capi.lib().oc_hip_calibration_create(None, None, 0, ctypes.byref(h)) == capi.ERR_INVALID
    # maps / reconstruct before prepare and wrong handle kinds are refused before any device work
    cam = opencorr_amd.Calibration(np.array([800, 800, 0, 320, 240, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32), np.zeros(6, dtype=np.float32))
    out = np.zeros(9, dtype=np.float32)
    assert capi.lib().oc_hip_stereo_fundamental(cam._h, ctypes.c_void_p(out.ctypes.data)) == capi.ERR_INVALID
    assert capi.lib().oc_hip_calibration_get(cam._h, 7, ctypes.c_void_p(out.ctypes.data)) == capi.ERR_INVALID
    assert capi.lib().oc_hip_calibration_prepare(cam._h, 1, 640) == capi.ERR_INVALID


def test_fundamental_matrix_satisfies_the_epipolar_constraint(fx):
    """x2^T F x1 on the table's undistorted (x, y) / (r2_x, r2_y) pairs, to the accuracy a float64 evaluation of the same F gives."""
    cams = [opencorr_amd.Calibration(fx[k + "_intrinsics"], fx[k + "_extrinsics"]) for k in ("cam1", "cam2")]
    F = opencorr_amd.Stereovision(cams[0], cams[1]).fundamental_matrix
    K1, _, _, _ = sn.matrices64(fx["cam1_intrinsics"], fx["cam1_extrinsics"])
    K2, R2, t2, _ = sn.matrices64(fx["cam2_intrinsics"], fx["cam2_extrinsics"])
    tx = np.array([[0, -t2[2], t2[1]], [t2[2], 0, -t2[0]], [-t2[1], t2[0], 0]])
    F64 = np.linalg.inv(K2).T @ tx @ R2 @ np.linalg.inv(K1)
    scale = np.abs(F64).max()
    assert np.abs(F - F64).max() <= 1e-5 * scale          # float32 products and two 3 x 3 inverses
    t = fx["table"]
    h, w = int(fx["height"]), int(fx["width"])
    ncams = [sn.Camera(fx[k + "_intrinsics"], fx[k + "_extrinsics"]) for k in ("cam1", "cam2")]
    maps = [c.undistortion_map(h, w) for c in ncams]
    x1, y1 = ncams[0].undistort(maps[0][0], maps[0][1], t[:, T["x"]], t[:, T["y"]])
    x2, y2 = ncams[1].undistort(maps[1][0], maps[1][1], t[:, T["r2_x"]], t[:, T["r2_y"]])
    p1 = np.stack([x1, y1, np.ones_like(x1)], axis=1).astype(np.float64)
    p2 = np.stack([x2, y2, np.ones_like(x2)], axis=1).astype(np.float64)

    def distance(Fm):   # pixels between the second point and the epipolar line of the first
        line = p1 @ Fm.T
        return np.abs((p2 * line).sum(axis=1)) / np.hypot(line[:, 0], line[:, 1])

    d32, d64 = distance(F.astype(np.float64)), distance(F64)
    print("epipolar distance of the matched pairs: float32 F median %.3g max %.3g px, float64 F median %.3g max %.3g px"
          % (np.median(d32), d32.max(), np.median(d64), d64.max()))
    assert np.median(d64) < 1.0                            # the matches do lie on their epipolar lines
    assert np.abs(d32 - d64).max() <= 0.05                 # and the float32 matrix says the same to a twentieth of a pixel


@pytest.mark.skipif(not (oref.available() and hasattr(oref.lib(), "oc_ref_epipolar_search")),
                    reason="needs oracle/_ref/liboc_ref.so (make -C oracle ref, where the reference tree is present)")
def test_fundamental_matrix_equals_the_reference_build_bit_for_bit(fx, driver, tmp_path):
    from opencorr_amd import synth
    ref, tar = synth.speckle_pair_2d(64, 72, seed=5)
    pois = np.zeros((1, 25), dtype=np.float32)
    pois[0, :2] = 36, 32
    for cam1, cam2 in (ec.cameras(72, 64),
                       ((fx["cam1_intrinsics"], fx["cam1_extrinsics"]), (fx["cam2_intrinsics"], fx["cam2_extrinsics"]))):
        want = oref.epipolar_search(ref, tar, cam1, cam2, 4, 3, ec.PARALLAX_X, ec.PARALLAX_Y, 8, 8, 0.001, 3, pois.copy())
        c1, c2 = opencorr_amd.Calibration(*cam1), opencorr_amd.Calibration(*cam2)
        got = opencorr_amd.Stereovision(c1, c2).fundamental_matrix
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
        # ... and through the C++ classes
        blob = np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a in (cam1[0], cam1[1], cam2[0], cam2[1])])
        (tmp_path / "cams.bin").write_bytes(blob.tobytes())
        subprocess.check_call([driver, "matrices", str(tmp_path / "cams.bin"), str(tmp_path / "m.bin")])
        m = np.fromfile(tmp_path / "m.bin", dtype=np.float32)
        assert m.size == 2 * 33 + 9
        assert np.array_equal(m[66:].view(np.uint32), want.ravel().view(np.uint32))
        assert np.array_equal(m[:9].reshape(3, 3), c1.intrinsic_matrix) and np.array_equal(m[9:18].reshape(3, 3), c1.rotation_matrix)
        assert np.array_equal(m[33 + 21:66].reshape(3, 4), c2.projection_matrix) and np.array_equal(m[33 + 18:33 + 21], c2.translation_vector)


def test_table2ds_round_trip_and_format(fx, driver, tmp_path):
    t = fx["table"]
    # the reference's own file parses into the fixture's floats (26 columns: the subset radius stays 0)
    (tmp_path / "head.csv").write_text(CSV_HEAD)
    head = io.load_table2ds(tmp_path / "head.csv")
    assert head.shape == (3, 28) and np.array_equal(head[:, :26], t[:3]) and (head[:, 26:] == 0).all()
    subprocess.check_call([driver, "io", str(tmp_path / "head.csv"), str(tmp_path / "head_out.csv")])
    lines = (tmp_path / "head_out.csv").read_text().splitlines()
    # written in the format of the source as it stands (src/oc_io.cpp:588-672): 28 columns, fixed notation with 8 decimals, a
    # delimiter after every field.  The example file predates it (26 columns, shortest general notation) and cannot be
    # reproduced character for character by that code; value for value it is.
    assert lines[0] == HEADER_2DS
    assert lines[1].startswith("234.00000000,135.00000000,-4.04184341,-0.76217842,0.88442993,0.96850073,0.99491721,0.95749855,188.25036621,")
    assert lines[1].endswith(",-0.00157490,-0.00211355,-0.05832024,-0.00481462,-0.02333627,-0.02186193,0.00000000,0.00000000,")
    assert all(ln.count(",") == 28 for ln in lines)
    assert np.array_equal(io.load_table2ds(tmp_path / "head_out.csv"), head)
    # the whole queue through the C++ loader and writer, and through the Python twin: the same text, the same floats back
    q = sn.table_to_pois(t)
    q[:, 26:] = 16
    io.save_table2ds(tmp_path / "py.csv", q)
    subprocess.check_call([driver, "io", str(tmp_path / "py.csv"), str(tmp_path / "cpp.csv")])
    assert (tmp_path / "py.csv").read_text() == (tmp_path / "cpp.csv").read_text()
    back = io.load_table2ds(tmp_path / "cpp.csv")
    assert np.array_equal(back.view(np.uint32), q.view(np.uint32))


def test_restatement_reproduces_the_table(fx):
    t = fx["table"]
    h, w = int(fx["height"]), int(fx["width"])
    ncams = [sn.Camera(fx[k + "_intrinsics"], fx[k + "_extrinsics"]) for k in ("cam1", "cam2")]
    maps = [c.undistortion_map(h, w) for c in ncams]
    assert max(m[2].max() for m in maps) <= 3            # iterations of the undistortion loop
    P = [opencorr_amd.Calibration(fx[k + "_intrinsics"], fx[k + "_extrinsics"]).projection_matrix for k in ("cam1", "cam2")]
    bounds = dict(ref=(6.2e-5, 1.8e-5, 3.1e-4), tar=(7.3e-5, 2.3e-5, 2.5e-4))
    sets = dict(ref=(t[:, 0:2], t[:, T["r2_x"]:T["r2_x"] + 2], t[:, T["ref_x"]:T["ref_x"] + 3]),
                tar=(t[:, T["t1_x"]:T["t1_x"] + 2], t[:, T["t2_x"]:T["t2_x"] + 2], t[:, T["tar_x"]:T["tar_x"] + 3]))
    for name, (p1, p2, want) in sets.items():
        for dtype in (np.float64, np.float32):
            got = sn.reconstruct(ncams[0], maps[0], P[0], ncams[1], maps[1], P[1], p1, p2, dtype)
            d = np.abs(got - want).max(axis=0)
            print(name, dtype.__name__, d)
            assert (d <= np.array(bounds[name])).all(), (name, d)
    assert np.abs(t[:, 2:5] - (t[:, 17:20] - t[:, 14:17])).max() <= 2.5e-7
    radius, nmin, thr, approx = [float(v) for v in fx["strain_settings"]]
    gate = (t[:, 5:8] >= np.float32(thr)).all(axis=1)
    assert gate.sum() == 9987
    s = sn.strain_poi2ds(t[:, :2], t[:, 14:17], t[:, 2:5], t[:, 5:8], radius, int(nmin), thr, int(approx))
    assert np.array_equal(s["fitted"], gate)
    d = np.abs(s["strain"][gate] - t[gate, 20:26]).max(axis=0)
    print("strain", d)
    assert (d <= np.array([2.7e-4, 8.2e-6, 2.4e-4, 1.4e-4, 6.9e-4, 7.0e-4])).all(), d

"""Stereo DIC on the GPU: Calibration::prepare / undistort, Stereovision::reconstruct (arrays and POI2DS records) and Strain for
POI2DS, against the float32 / float64 NumPy restatement of tests/stereo_numpy.py and against the reference's own result table of
the GT4 example (tests/golden/gt4_stereo_r16.npz; 9 997 rows written by the reference's programs).

Bounds (none of them is taken from what the GPU returns):
  * maps and undistorted coordinates hold no reduction: bit-identical to the float32 restatement.  Two NaNs count as equal
    whatever their sign and payload (inf - inf is -NaN on x86 and +NaN on the GPU; IEEE 754 leaves that open).
  * reconstruct: within 1 float32 ulp of the float64 least-squares solution of the same float32 system (Householder QR in
    double on a 4 x 3 system is exact far below that; rounding it once can land on the neighbour of the rounded LAPACK
    solution).  Against the table: 1.5e-4, 5e-5, 6.5e-4 in x, y, z -- twice what the restatement itself measures against it
    (test_stereo_host.py pins those figures), the factor two allowing the reference's float32 QR to lie on the other side of
    the exact solution.
  * Strain on POI2DS: against the table twice 2.7e-4, 8.2e-6, 2.4e-4, 1.4e-4, 6.9e-4, 7.0e-4 (the restatement's own measured
    distances); against the float64 restatement over the same neighbour sets 1e-6 absolute (double normal equations at
    cond^2 <= 3e7 and one float32 rounding of values up to 6 leave less than 5e-7).
"""
import numpy as np
import pytest

import opencorr_amd
from opencorr_amd import P2S

import stereo_numpy as sn

pytestmark = pytest.mark.gpu

T = sn.T
SENTINEL = np.float32(-7.5)
TABLE_XYZ = np.array([1.5e-4, 5e-5, 6.5e-4])
TABLE_STRAIN = 2 * np.array([2.7e-4, 8.2e-6, 2.4e-4, 1.4e-4, 6.9e-4, 7.0e-4])


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_bits(got, want, what):
    ok = same_bits(got, want)
    bad = np.argwhere(~ok)
    assert bad.size == 0, "%s: %d differ, first %s: %r vs %r" % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def fx():
    return sn.load_fixture()


@pytest.fixture(scope="module")
def rig(fx):
    """Both GT4 cameras: engine objects (prepared), NumPy cameras and their maps."""
    h, w = int(fx["height"]), int(fx["width"])
    cams, ncams, maps = [], [], []
    for k in ("cam1", "cam2"):
        c = opencorr_amd.Calibration(fx[k + "_intrinsics"], fx[k + "_extrinsics"])
        c.prepare(h, w)
        cams.append(c)
        n = sn.Camera(fx[k + "_intrinsics"], fx[k + "_extrinsics"])
        ncams.append(n)
        maps.append(n.undistortion_map(h, w))
    stereo = opencorr_amd.Stereovision(cams[0], cams[1])
    return dict(cams=cams, ncams=ncams, maps=maps, stereo=stereo, h=h, w=w)


def test_gt4_maps_are_bit_identical(rig):
    for cam, (mx, my, used) in zip(rig["cams"], rig["maps"]):
        gx, gy = cam.maps()
        assert used.max() <= 3          # "at most 3 of its 40 iterations on both cameras"
        assert_same_bits(gx, mx, "map_x")
        assert_same_bits(gy, my, "map_y")


def test_map_with_every_coefficient_on_an_odd_sized_image():
    intr = np.array([812.5, 799.25, 1.75, 257.3, 166.9, -0.21, 0.083, -0.011, 0.013, -0.0047, 0.0009, 0.0012, -0.0008], dtype=np.float32)
    cam = opencorr_amd.Calibration(intr, np.zeros(6, dtype=np.float32))
    cam.prepare(331, 517)
    mx, my, used = sn.Camera(intr, np.zeros(6)).undistortion_map(331, 517)
    assert used.max() > 3 and used.max() < 40
    gx, gy = cam.maps()
    assert_same_bits(gx, mx, "map_x")
    assert_same_bits(gy, my, "map_y")


def test_map_under_strong_distortion_runs_out_of_iterations_and_overflows():
    """Barrel distortion strong enough that the fixed-point loop diverges towards the corners: pixels that use all 40
    iterations, and pixels whose deviation overflows (the `isinf` reset, after which the source still applies the update)."""
    intr = np.array([300.0, 300.0, 0.0, 320.0, 240.0, -0.9, 0.0, 40.0, 0, 0, 0, 0, 0], dtype=np.float32)
    ncam = sn.Camera(intr, np.zeros(6))
    mx, my, used = ncam.undistortion_map(480, 640)
    assert (used == 40).any(), "the case must reach the iteration limit somewhere"
    assert (~np.isfinite(mx)).any(), "the case must overflow somewhere"
    assert np.isfinite(mx).mean() > 0.2
    cam = opencorr_amd.Calibration(intr, np.zeros(6, dtype=np.float32))
    cam.prepare(480, 640)
    gx, gy = cam.maps()
    assert_same_bits(gx, mx, "map_x")
    assert_same_bits(gy, my, "map_y")
    # a lower iteration limit and a coarser criterion are honoured too
    cam.set_undistortion(0.05, 7)
    cam.prepare(480, 640)
    mx, my, used = ncam.undistortion_map(480, 640, 0.05, 7)
    assert used.max() == 7
    gx, gy = cam.maps()
    assert_same_bits(gx, mx, "map_x (7 iterations)")
    assert_same_bits(gy, my, "map_y (7 iterations)")


def test_undistorted_coordinates_are_bit_identical(fx, rig):
    t = fx["table"]
    h, w = rig["h"], rig["w"]
    edge = np.array([[-5.0, -3.0], [-0.25, 10.5], [w - 2.0, h - 2.0], [w - 2.0 + 0.5, 17.25], [33.5, h - 2.0 + 0.75], [w - 1.0, h - 1.0],
                     [w + 40.0, h + 90.0], [w - 2.0 - 0.125, h - 2.0 - 0.125], [0.0, 0.0], [np.inf, -np.inf], [1e9, 1e9]], dtype=np.float32)
    sets = [t[:, [T["x"], T["y"]]], t[:, [T["r2_x"], T["r2_y"]]], t[:, [T["t1_x"], T["t1_y"]]], t[:, [T["t2_x"], T["t2_y"]]], edge]
    for k, (cam, ncam, (mx, my, _)) in enumerate(zip(rig["cams"], rig["ncams"], rig["maps"])):
        for j, pts in enumerate(sets):
            pts = np.ascontiguousarray(pts)
            before = pts.copy()
            got = cam.undistort(pts)
            assert np.array_equal(pts, before)          # the input is not clamped in place
            wx, wy = ncam.undistort(mx, my, pts[:, 0], pts[:, 1])
            assert_same_bits(got, np.stack([wx, wy], axis=1), "camera %d, point set %d" % (k + 1, j))
    got = rig["cams"][0].undistort(np.array([[np.nan, 5.0], [5.0, np.nan], [7.0, 9.0]], dtype=np.float32))
    assert np.isnan(got[:2]).all() and np.isfinite(got[2]).all()
    # a device-resident point list gives the same bits
    import torch
    pts = np.ascontiguousarray(t[:, 0:2])
    dev = rig["cams"][1].undistort(torch.from_numpy(pts).cuda())
    torch.cuda.synchronize()
    assert_same_bits(dev.cpu().numpy(), rig["cams"][1].undistort(pts), "device tensor")


def _pairs(t):
    """(view 1 points, view 2 points, the table's 3D points) of the reference and the target state, as column views of the table."""
    return ((t[:, 0:2], t[:, T["r2_x"]:T["r2_x"] + 2], t[:, T["ref_x"]:T["ref_x"] + 3]),
            (t[:, T["t1_x"]:T["t1_x"] + 2], t[:, T["t2_x"]:T["t2_x"] + 2], t[:, T["tar_x"]:T["tar_x"] + 3]))


def test_reconstruct_against_the_restatement_and_the_table(fx, rig):
    t = fx["table"]
    st = rig["stereo"]
    P1, P2 = rig["cams"][0].projection_matrix, rig["cams"][1].projection_matrix
    for name, (p1, p2, want_table) in zip(("ref", "tar"), _pairs(t)):
        got = st.reconstruct(p1, p2)        # column views of the table: strides of 104 bytes
        assert got.shape == (len(t), 3) and got.dtype == np.float32
        exact = sn.reconstruct(rig["ncams"][0], rig["maps"][0], P1, rig["ncams"][1], rig["maps"][1], P2, p1, p2, np.float64, rounded=False)
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - exact) / ulp
        equal = (got == exact.astype(np.float32)).mean()
        dist = np.abs(got - want_table).max(axis=0)
        print("%s: max distance to the float64 solution %.3f ulp, %.4f of the coordinates equal its float32 rounding; "
              "max distance to the table %s" % (name, err.max(), equal, dist))
        assert err.max() <= 1.0
        assert (dist <= TABLE_XYZ).all(), dist


def test_reconstruct_nan_inputs_and_device_tensors(fx, rig):
    import torch
    t = fx["table"][:257]
    p1 = np.ascontiguousarray(t[:, [T["x"], T["y"]]])
    p2 = np.ascontiguousarray(t[:, [T["r2_x"], T["r2_y"]]])
    want = rig["stereo"].reconstruct(p1, p2)
    for col, arr in ((0, p1), (1, p1), (0, p2), (1, p2)):
        arr[3 + 5 * col + (arr is p2), col] = np.nan
    nan_rows = np.isnan(p1).any(axis=1) | np.isnan(p2).any(axis=1)
    assert nan_rows.sum() == 4
    got = rig["stereo"].reconstruct(p1, p2)
    assert (got[nan_rows] == 0).all()
    assert_same_bits(got[~nan_rows], want[~nan_rows], "rows without NaN")
    dev = rig["stereo"].reconstruct(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda())
    torch.cuda.synchronize()
    assert_same_bits(dev.cpu().numpy(), got, "device tensors")


def _bare_queue(t):
    """POI2DS records holding only the table's 2D columns; everything else a sentinel."""
    q = np.full((len(t), 28), SENTINEL, dtype=np.float32)
    for name in ("x", "y", "r2_x", "r2_y", "t1_x", "t1_y", "t2_x", "t2_y"):
        q[:, P2S[name]] = t[:, T[name]]
    return q


def test_reconstruct_pois(fx, rig):
    import torch
    t = fx["table"]
    st = rig["stereo"]
    (r1, r2, _), (t1, t2, _) = _pairs(t)
    ref, tar = st.reconstruct(r1, r2), st.reconstruct(t1, t2)
    start = _bare_queue(t)
    start[11, P2S["t2_x"]] = np.nan            # tar_coor = 0, deformation = -ref_coor
    tar[11] = 0
    written = [P2S[k] for k in ("u", "v", "w", "ref_x", "ref_y", "ref_z", "tar_x", "tar_y", "tar_z")]
    kept = [c for c in range(28) if c not in written]

    def check(q, what):
        assert_same_bits(q[:, 14:17], ref, what + ": ref_coor")
        assert_same_bits(q[:, 17:20], tar, what + ": tar_coor")
        assert_same_bits(q[:, 2:5], tar - ref, what + ": deformation")
        assert_same_bits(q[:, kept], start[:, kept], what + ": untouched fields")

    host = start.copy()
    assert st.reconstruct_pois(host) is host
    check(host, "host queue")
    dev = torch.from_numpy(start).cuda()
    st.reconstruct_pois(dev)
    torch.cuda.synchronize()
    check(dev.cpu().numpy(), "device queue")
    # a stream of the caller's own
    side = torch.cuda.Stream()
    st2 = opencorr_amd.Stereovision(rig["cams"][0], rig["cams"][1])
    with torch.cuda.stream(side):
        dev2 = torch.from_numpy(start).cuda()
        st2.reconstruct_pois(dev2)
        out = dev2.cpu()
    side.synchronize()
    check(out.numpy(), "device queue on a side stream")
    st2.close()
    # records embedded in wider rows keep what lies between them
    wide = np.full((len(t), 33), np.float32(3.25), dtype=np.float32)
    wide[:, :28] = start
    st.reconstruct_pois(wide)
    check(wide[:, :28], "stride of 132 bytes")
    assert (wide[:, 28:] == np.float32(3.25)).all()


def _strain_queue(t):
    q = sn.table_to_pois(t)
    q[:, 20:26] = SENTINEL
    q[:, 26:28] = 16
    return q


def test_strain_poi2ds_on_the_table(fx):
    t = fx["table"]
    radius, nmin, thr, approx = [float(v) for v in fx["strain_settings"]]
    gate = (t[:, 5:8] >= np.float32(thr)).all(axis=1)
    assert gate.sum() == 9987
    want = sn.strain_poi2ds(t[:, :2], t[:, 14:17], t[:, 2:5], t[:, 5:8], radius, int(nmin), thr, int(approx))
    assert want["fitted"].sum() == 9987 and not want["knn"][gate].any()
    assert want["cond"].max() ** 2 <= 3.5e7
    nb, _ = sn.strain_neighbours(t[:, :2], gate, radius, int(nmin))
    filtered = sum(1 for i in np.nonzero(gate)[0] if len(nb[i]) < ((t[:, 0] - t[i, 0]) ** 2 + (t[:, 1] - t[i, 1]) ** 2 < radius * radius).sum())
    assert filtered == 118                                 # the neighbour filter is exercised
    st = opencorr_amd.Strain(radius, int(nmin))
    st.set_zncc_threshold(thr)
    st.set_approximation(int(approx))
    q = _strain_queue(t)
    st.prepare(q)
    st.compute(q)
    got = q[:, 20:26]
    assert (got[~gate] == SENTINEL).all()                  # the 10 rows that fail their own gate are left untouched
    assert_same_bits(q[:, :20], _strain_queue(t)[:, :20], "fields before the strains")
    assert (q[:, 26:28] == 16).all()
    d_table = np.abs(got[gate] - t[gate, 20:26]).max(axis=0)
    d_twin = np.abs(got[gate].astype(np.float64) - want["strain"][gate]).max(axis=0)
    print("POI2DS strain: max distance to the table %s, to the float64 restatement %s" % (d_table, d_twin))
    assert (d_table <= TABLE_STRAIN).all(), d_table
    assert d_twin.max() <= 1e-6, d_twin
    # Green strains.  They are float32 polynomials of the gradients g (|d e / d g| <= 1 + sum |g|), whose two roundings differ
    # by at most the 1e-6 above; the evaluation itself adds a few roundings of the result
    st.set_approximation(2)
    q2 = _strain_queue(t)
    st.compute(q2)
    green = sn.strain_poi2ds(t[:, :2], t[:, 14:17], t[:, 2:5], t[:, 5:8], radius, int(nmin), thr, 2)
    tol = 1e-6 * (1 + np.abs(green["grad"]).sum(axis=1, keepdims=True)) + 8 * np.spacing(np.abs(green["strain"]))
    err = np.abs(q2[:, 20:26].astype(np.float64) - green["strain"])
    assert (err[gate] <= tol[gate]).all(), (err[gate] / tol[gate]).max()
    assert (q2[~gate, 20:26] == SENTINEL).all()
    assert np.abs(q2[gate, 20:26] - got[gate]).max() > 1e-3      # the second mode really is another formula
    st.close()


def test_strain_poi2ds_device_chain(fx, rig):
    """reconstruct_pois -> Strain on one device-resident queue equals the same two steps on a host queue."""
    import torch
    t = fx["table"]
    radius, nmin, thr, approx = [float(v) for v in fx["strain_settings"]]
    start = _bare_queue(t)
    start[:, 5:8] = t[:, 5:8]
    st = opencorr_amd.Strain(radius, int(nmin))
    host = start.copy()
    rig["stereo"].reconstruct_pois(host)
    st.prepare(host)
    st.compute(host)
    dev = torch.from_numpy(start).cuda()
    rig["stereo"].reconstruct_pois(dev)
    st.prepare(dev)
    st.compute(dev)
    torch.cuda.synchronize()
    assert_same_bits(dev.cpu().numpy(), host, "device chain")
    assert (host[:, 20:26] != SENTINEL).any(axis=1).sum() == 9987
    st.close()


def test_strain_poi2ds_sparse_cloud_takes_the_k_nearest_path(fx):
    t = fx["table"]
    rng = np.random.default_rng(20261016)
    s = t[rng.random(len(t)) < 0.08]
    radius, nmin, thr = 20.0, 8, 0.9
    want = sn.strain_poi2ds(s[:, :2], s[:, 14:17], s[:, 2:5], s[:, 5:8], radius, nmin, thr, 1)
    gate = (s[:, 5:8] >= np.float32(thr)).all(axis=1)
    assert want["knn"].mean() > 0.9 and want["fitted"].sum() > 0.9 * len(s)
    st = opencorr_amd.Strain(radius, nmin)
    q = _strain_queue(s)
    st.prepare(q)
    st.compute(q)
    got = q[:, 20:26]
    fitted = want["fitted"]
    assert (got[~fitted] == SENTINEL).all() and (got[fitted] != SENTINEL).all()
    assert not fitted[~gate].any()
    # normal equations in double: relative error of the gradients about cond^2 * 2^-53 per unit of |g| and of the right-hand
    # sides' scale; one float32 rounding on top (the 1e-6 of the dense case is this bound at cond^2 <= 3e7)
    g = np.abs(want["grad"]).max(axis=1)
    tol = np.maximum(1e-6, 16 * want["cond"] ** 2 * 2.0 ** -53 * np.maximum(g, 1.0)) + np.spacing(np.float32(np.maximum(g, 1e-30)))
    err = np.abs(got.astype(np.float64) - want["strain"]).max(axis=1)
    print("sparse cloud: cond max %.3g, max error %.3g, max error / bound %.3g" % (want["cond"][fitted].max(), err[fitted].max(), (err / tol)[fitted].max()))
    assert (err[fitted] <= tol[fitted]).all()
    st.close()


def test_strain_rejects_other_record_kinds():
    st = opencorr_amd.Strain(20.0, 5)
    with pytest.raises(ValueError):
        st.prepare(np.zeros((10, 27), dtype=np.float32))
    from opencorr_amd import capi
    import ctypes
    q = np.zeros((10, 28), dtype=np.float32)
    for ndim in (0, 1, 4, 28):
        assert capi.lib().oc_hip_strain_prepare(st._h, ctypes.c_void_p(q.ctypes.data), 10, 112, ndim, capi.HOST) == capi.ERR_INVALID
    rf = opencorr_amd.RegionFit(20.0, 5)
    assert capi.lib().oc_hip_region_fit_prepare(rf._h, ctypes.c_void_p(q.ctypes.data), 10, 112, capi.POI2DS, capi.HOST) == capi.ERR_INVALID
    st.close()


# ---- the C++ classes of include/opencorr_compat/oc_stereo.h (tests/cpp/stereo_driver.cpp) --------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "opencorr_amd", "lib")
    exe = str(tmp_path_factory.mktemp("stereo") / "stereo_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "stereo_driver.cpp"), "-o", exe, "-L" + libdir, "-lopencorr_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_epipolar_search_class_equals_its_parts(driver, tmp_path):
    """EpipolarSearch (C++ shim) on a synthetic stereo-like pair returns bit for bit what epipolarCandidates + computeBestOf
    return with the fundamental matrix of Stereovision -- and what the Python classes return for the same batch."""
    import struct
    import subprocess
    import epipolar_case as ec
    from opencorr_amd import synth
    ref, tar = synth.speckle_pair_2d(300, 320, seed=20260925)
    h, w = ref.shape
    xs, ys = synth.poi_grid_2d(h, w, 17, 15, 30)
    xs = np.concatenate([xs, [w - 22.0, w - 19.0, 40.0]]).astype(np.float32)   # fans cut by the bounds tests
    ys = np.concatenate([ys, [150.0, 60.0, h - 18.0]]).astype(np.float32)
    n = len(xs)
    cam1, cam2 = ec.cameras(w, h)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<7i2f", h, w, ec.RX, ec.RY, n, ec.SEARCH_RADIUS, ec.SEARCH_STEP, ec.CONV, ec.STOP))
        for a in (cam1[0], cam1[1], cam2[0], cam2[1], ec.PARALLAX_X, ec.PARALLAX_Y, ref, tar, xs, ys):
            f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    subprocess.run([driver, "epipolar", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=300)
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float32)
    assert raw.size == 9 + 3 * n * 25
    F = raw[:9].reshape(3, 3)
    by_class, by_parts, singles = raw[9:].reshape(3, n, 25)
    assert_same_bits(by_class, by_parts, "EpipolarSearch::compute(queue) vs its parts")
    assert_same_bits(singles[:3], by_class[:3], "EpipolarSearch::compute(POI2D*)")
    ok = by_class[:, 16] > 0.9
    assert ok.mean() > 0.9
    assert np.abs(by_class[ok, 2] - 2.3).max() < 1.0 and np.abs(by_class[ok, 8] + 1.7).max() < 1.0   # the pair's displacement
    # the Python classes: the same matrix, the same batch, the same winners
    c1, c2 = opencorr_amd.Calibration(*cam1), opencorr_amd.Calibration(*cam2)
    assert_same_bits(opencorr_amd.Stereovision(c1, c2).fundamental_matrix, F, "fundamental matrix")
    pois = opencorr_amd.make_pois2d(xs, ys)
    cand, starts = ec.candidates(ec.candidate_lib(tmp_path), pois, F, w, h)
    icgn = opencorr_amd.ICGN2D1(ec.RX, ec.RY, ec.CONV, ec.STOP)
    icgn.set_images(ref, tar)
    icgn.prepare()
    got = icgn.select_best(icgn.compute(cand), starts, pois)
    assert_same_bits(got, by_class, "Python classes vs the C++ class")


def test_cpp_chain_reconstruct_and_strain(fx, rig, driver, tmp_path):
    """Calibration -> Stereovision::reconstruct(queue) -> Strain::prepare / compute through the C++ classes equal the Python ones."""
    import struct
    import subprocess
    t = fx["table"][:1500]
    radius, nmin, thr, approx = [float(v) for v in fx["strain_settings"]]
    start = _bare_queue(t)
    start[:, 5:8] = t[:, 5:8]
    start[:, 20:26] = 0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3ifi", rig["h"], rig["w"], len(start), radius, int(nmin)))
        for k in ("cam1", "cam2"):
            f.write(fx[k + "_intrinsics"].astype(np.float32).tobytes())
            f.write(fx[k + "_extrinsics"].astype(np.float32).tobytes())
        f.write(start.tobytes())
    subprocess.run([driver, "chain", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=300)
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float32).reshape(-1, 28)
    want = start.copy()
    rig["stereo"].reconstruct_pois(want)
    st = opencorr_amd.Strain(radius, int(nmin))
    st.prepare(want)
    st.compute(want)
    st.close()
    assert_same_bits(got, want, "C++ chain vs Python chain")
    assert (got[:, 20:26] != 0).any(axis=1).mean() > 0.99

"""ctypes wrapper of tests/cpp/icgn3d_onepass_twin.cpp: the CPU restatement of the one-pass arithmetic contract of ICGN3D1
(oc_hip_set_tuning "arith_onepass3d").  Shared by tests/test_onepass3d_twin_cpu.py (CPU) and tests/test_gpu_arith_onepass3d.py
(GPU == twin bit for bit); the queues both files run are built here, so that the CPU file can state what the GPU file relies on."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None

SHAPE = (72, 76, 80)   # dz, dy, dx: the pair of tests/test_gpu_parity_3d.py (seed 21)
BIG = (96, 100, 104)   # its larger pair (seed 23)


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="onepass3d_twin_")
        so = os.path.join(_dir.name, "libicgn3d_onepass_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "icgn3d_onepass_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        i, f = ctypes.c_int, ctypes.c_float
        L.oc_twin_icgn3d_onepass.argtypes = [fp, fp, fp, fp, fp, i, i, i, i, i, i, f, f, fp, ctypes.c_long, i]
        L.oc_twin_icgn3d_onepass.restype = None
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def icgn3d1(prep, rx, ry, rz, conv, stop, pois):
    """In place on ``pois`` (n x 31 float32): ICGN3D1 under the one-pass contract.  ``prep`` is an oracle.Prepared3D."""
    assert pois.dtype == np.float32 and pois.flags.c_contiguous and pois.ndim == 2 and pois.shape[1] == 31
    dz, dy, dx = prep.ref.shape
    lib().oc_twin_icgn3d_onepass(_fp(prep.ref), _fp(prep.gx), _fp(prep.gy), _fp(prep.gz), _fp(prep.coef), dz, dy, dx, int(rx), int(ry),
                                 int(rz), float(conv), float(stop), _fp(pois), pois.shape[0], pois.shape[1])
    return pois


def codes(p):
    """Failure code of every record (-3 / -4 / -5 / whatever a rejected record carried), 0 where it converged."""
    z = p[:, 18]
    return np.where(z < 0, z, np.float32(0))


def vs_reference_order(got, seq):
    """`got` against the oracle in the reference's loop order (ORDER_SEQ) on the same guesses: records whose failure code differs,
    fraction of commonly converged POIs with equal iteration counts and -- over those -- max |d u|, |d v|, |d w| and max |d ZNCC|."""
    cg, cs = codes(got), codes(seq)
    both = (cg == 0) & (cs == 0)
    same_it = both & (got[:, 19] == seq[:, 19])
    dd = np.abs(got[same_it][:, [3, 7, 11]].astype(np.float64) - seq[same_it][:, [3, 7, 11]].astype(np.float64))
    dz = np.abs(got[same_it, 18].astype(np.float64) - seq[same_it, 18].astype(np.float64))
    return dict(code_mismatch=(cg != cs), iteration_agreement=float(same_it.sum() / max(1, both.sum())),
                max_abs_d_disp=float(dd.max()) if dd.size else 0.0, max_abs_d_zncc=float(dz.max()) if dz.size else 0.0,
                same_it=int(same_it.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# queues
# ---------------------------------------------------------------------------------------------------------------------------------
def small_pair():
    from opencorr_amd import synth
    return synth.speckle_pair_3d(*SHAPE, seed=21)


def big_pair():
    from opencorr_amd import synth
    return synth.speckle_pair_3d(*BIG, seed=23)


def grid_queue(ref, tar):
    """The queue of tests/test_gpu_parity_3d.py::test_icgn3d1_bit_exact_vs_oracle: the 4 x 3 x 3 grid with FFTCC3D guesses and the
    four trippers (guard reject, out of the volume inside the loop, rejected on entry with its flag kept, NaN guess)."""
    import oracle
    from opencorr_amd import synth
    xs, ys, zs = synth.poi_grid_3d(*SHAPE, 4, 3, 3, 26)
    pois = oracle.make_pois3d(xs, ys, zs)
    oracle.fftcc3d(ref, tar, 8, 8, 8, pois)
    P = oracle.P3
    extra = oracle.make_pois3d([3, 40, 40, 40], [38, 38, 38, 38], [36, 36, 36, 36])
    extra[1, P["u"]] = 60.0
    extra[2, P["zncc"]] = -1.0
    extra[3, P["w"]] = np.nan
    return np.concatenate([pois, extra]).astype(np.float32)


ELEMENT_PATH_X, ELEMENT_PATH_RX = np.float32(13.0) - np.float32(2.0 ** -20), 5


def reference_indices(c, r):
    """(per-element float32 indices of Subset3D::fill along one axis, the indices of the box that starts at int(c - r))."""
    start = np.float32(c) - np.float32(r)
    e = np.arange(2 * r + 1)
    per_element = (start + e.astype(np.float32)).astype(np.float32).astype(np.int64)   # float32 addition, truncated
    return per_element, int(start) + e


def offgrid_queue():
    """Non-integer centres on the small pair for radii (5, 7, 6), and one POI whose reference subvolume is NOT a box: at
    x = 13 - 2^-20 with rx = 5 the float32 sum start + 10 rounds up to 18 (tests/test_onepass3d_twin_cpu.py asserts it)."""
    import oracle
    from opencorr_amd import synth
    P = oracle.P3
    rng = np.random.default_rng(3305)
    n = 9
    xs = rng.uniform(12, SHAPE[2] - 13, n).astype(np.float32)
    ys = rng.uniform(14, SHAPE[1] - 15, n).astype(np.float32)
    zs = rng.uniform(13, SHAPE[0] - 14, n).astype(np.float32)
    xs[0] = ELEMENT_PATH_X
    xs[1], ys[1], zs[1] = 33.5, 30.25, 28.75
    pois = oracle.make_pois3d(xs, ys, zs)
    w = synth.DEFAULT_WARP_3D
    pois[:, P["u"]], pois[:, P["v"]], pois[:, P["w"]] = round(w["u"]), round(w["v"]), round(w["w"])
    return pois.astype(np.float32)


def config_e_queue(ref, tar, fftcc=None):
    """The queue of test_icgn3d1_config_e_shape_multi_pass_staging (r = 16 on the big pair): 27 FFTCC3D-guessed POIs plus border,
    out-of-volume, rejected and NaN records.  ``fftcc``: a callable filling the guesses in place (default: the oracle's FFTCC3D,
    whose integers are the GPU engine's)."""
    import oracle
    from opencorr_amd import synth
    xs, ys, zs = synth.poi_grid_3d(*BIG, 3, 3, 3, 24)
    pois = oracle.make_pois3d(xs, ys, zs)
    if fftcc is None:
        oracle.fftcc3d(ref, tar, 16, 16, 16, pois)
    else:
        fftcc(pois)
    P = oracle.P3
    extra = oracle.make_pois3d([16, 60, 60, 60, BIG[2] - 17.0], [50, 50, 50, 50, 50], [48, 48, 48, 48, 48])
    extra[1, P["u"]] = 80.0
    extra[2, P["zncc"]] = -2.0
    extra[3, P["v"]] = np.nan
    return np.concatenate([pois, extra]).astype(np.float32)


def rotated_queue():
    """The four rotated / stretched guesses of test_icgn3d1_global_tap_fallback (r = 16, stop = 6): passes take global taps."""
    import oracle
    P = oracle.P3
    cx, cy, cz = BIG[2] // 2, BIG[1] // 2, BIG[0] // 2
    pois = oracle.make_pois3d([cx, cx + 3, cx - 2, cx], [cy, cy - 2, cy + 1, cy], [cz, cz + 1, cz - 1, cz])
    ang = np.deg2rad(30.0)
    for i, a in enumerate([ang, -ang, 0.6 * ang]):
        pois[i, P["ux"]] = np.cos(a) - 1.0
        pois[i, P["uy"]] = -np.sin(a)
        pois[i, P["vx"]] = np.sin(a)
        pois[i, P["vy"]] = np.cos(a) - 1.0
    pois[3, P["ux"]] = 0.35
    pois[3, P["wz"]] = 0.2
    return pois.astype(np.float32)


def large_radius_queue(r):
    """4 - 6 POIs with integer guesses for r = 21, 25, 30, as test_icgn3d1_large_radii_kernels builds them."""
    import oracle
    from opencorr_amd import synth
    c = [BIG[2] // 2, BIG[1] // 2, BIG[0] // 2]
    span = [BIG[2] - 2 * (r + 4), BIG[1] - 2 * (r + 4), BIG[0] - 2 * (r + 4)]
    rng = np.random.default_rng(r)
    n = 6 if r < 30 else 4
    xs = [c[0] + int(rng.integers(-span[0] // 2, span[0] // 2 + 1)) for _ in range(n)]
    ys = [c[1] + int(rng.integers(-span[1] // 2, span[1] // 2 + 1)) for _ in range(n)]
    zs = [c[2] + int(rng.integers(-span[2] // 2, span[2] // 2 + 1)) for _ in range(n)]
    pois = oracle.make_pois3d(xs, ys, zs)
    P = oracle.P3
    w = synth.DEFAULT_WARP_3D
    pois[:, P["u"]], pois[:, P["v"]], pois[:, P["w"]] = round(w["u"]), round(w["v"]), round(w["w"])
    return pois.astype(np.float32)


def schedule_queue():
    """The 2 191-POI queue of test_icgn3d1_block_schedule_changes_no_bits (r = 5 on the small pair)."""
    import oracle
    from opencorr_amd import synth
    P = oracle.P3
    xs, ys, zs = synth.poi_grid_3d(*SHAPE, 13, 13, 13, 14)
    pois = oracle.make_pois3d(xs, ys, zs)[:2191]
    w = synth.DEFAULT_WARP_3D
    pois[:, P["u"]], pois[:, P["v"]], pois[:, P["w"]] = round(w["u"]), round(w["v"]), round(w["w"])
    pois[5::97, P["zncc"]] = -1.0
    pois[11::131, P["u"]] = 70.0
    pois[17::151, P["x"]] = 2.0
    return pois.astype(np.float32)

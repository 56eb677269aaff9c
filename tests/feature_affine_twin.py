"""ctypes wrapper of tests/cpp/feature_affine_twin.cpp: the CPU restatement of the FeatureAffine2D/3D contract.
Shared by tests/test_feature_affine_twin_cpu.py (twin against the float64 model) and tests/test_gpu_feature_affine.py
(kernel == twin bit for bit)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None

(SLIP_NONE, SLIP_CONSENSUS_LE, SLIP_RADIUS_LE, SLIP_REPLACEMENT, SLIP_NO_KNN, SLIP_NO_DIAGONAL, SLIP_NOT_LOCAL,
 SLIP_EXIT_MAX_MEAN) = range(8)

DEFAULTS = {2: dict(nmin=7, trials=20, samples=3, threshold=1.5), 3: dict(nmin=16, trials=32, samples=4, threshold=3.2)}


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="feature_affine_twin_")
        so = os.path.join(_dir.name, "libfeature_affine_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "feature_affine_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        i, f, n = ctypes.c_int, ctypes.c_float, ctypes.c_long
        L.oc_twin_fa_set_slip.argtypes = [i]
        L.oc_twin_fa_set_slip.restype = None
        L.oc_twin_fa_compute.argtypes = [i, fp, fp, n, fp, n, i, f, i, i, i, f, ctypes.c_ulonglong, i, i, i, i, i, i]
        L.oc_twin_fa_compute.restype = None
        _lib = L
    return _lib


class slip:
    """``with slip(SLIP_...):`` the twin runs with one planted error."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        lib().oc_twin_fa_set_slip(self.which)

    def __exit__(self, *exc):
        lib().oc_twin_fa_set_slip(SLIP_NONE)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def default_radius(ndim, subset_radius):
    """The search radius of the reference's constructors: sqrt of the float of the integer sum of squares."""
    return float(np.sqrt(np.float32(sum(int(r) * int(r) for r in subset_radius[:ndim]))))


def compute(ref, tar, pois, radius, nmin=None, trials=None, samples=None, threshold=None, seed=0, adaptive=None, threads=0):
    """A copy of the (n, 25) / (n, 31) float32 queue ``pois`` after FeatureAffine over the matched keypoints ``ref`` -> ``tar``
    ((m, 2) / (m, 3) float32).  ``adaptive``: None or (feature_min, radius_min, width, height); ``threads``: OpenMP
    threads (0: the runtime's default)."""
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    tar = np.ascontiguousarray(tar, dtype=np.float32)
    ndim = ref.shape[1]
    assert ndim in (2, 3) and tar.shape == ref.shape and pois.dtype == np.float32 and pois.shape[1] == (25 if ndim == 2 else 31)
    d = DEFAULTS[ndim]
    out = np.array(pois, dtype=np.float32, order="C")
    ad = (1,) + tuple(int(v) for v in adaptive) if adaptive else (0, 14, 10, 0, 0)
    lib().oc_twin_fa_compute(ndim, _fp(ref), _fp(tar), ref.shape[0], _fp(out), out.shape[0], out.shape[1], float(radius),
                             int(d["nmin"] if nmin is None else nmin), int(d["trials"] if trials is None else trials),
                             int(d["samples"] if samples is None else samples), float(d["threshold"] if threshold is None else threshold),
                             int(seed), *ad, int(threads))
    return out


_qr = None


def qr32(rows_ref, rows_tar):
    """The (ndim + 1, ndim) affine matrix of the final fit in the reference's arithmetic: float32 Householder QR with column
    pivoting (tests/cpp/feature_affine_qr32.cpp over the stand-in of oracle/ref_stubs/Eigen)."""
    global _qr
    if _qr is None:
        lib()
        so = os.path.join(_dir.name, "libfeature_affine_qr32.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
                               "-I", os.path.join(ROOT, "oracle", "ref_stubs", "Eigen"),
                               os.path.join(ROOT, "tests", "cpp", "feature_affine_qr32.cpp"), "-o", so])
        _qr = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        _qr.oc_fa_qr32.argtypes = [ctypes.c_int, fp, fp, ctypes.c_int, fp]
        _qr.oc_fa_qr32.restype = None
    r = np.ascontiguousarray(rows_ref, dtype=np.float32)
    t = np.ascontiguousarray(rows_tar, dtype=np.float32)
    ndim = r.shape[1]
    X = np.zeros((ndim + 1, ndim), np.float32)
    _qr.oc_fa_qr32(ndim, _fp(r), _fp(t), r.shape[0], _fp(X))
    return X


def qr32_distance(model_records):
    """The largest |entry| of (model's affine matrix - the same fit by float32 QR) over the fitted POIs of a model run."""
    worst = 0.0
    for rec in model_records:
        if rec["X"] is not None:
            worst = max(worst, float(np.abs(qr32(*rec["rows"]).astype(np.float64) - rec["X"]).max()))
    return worst

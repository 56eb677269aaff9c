"""ctypes wrapper of tests/cpp/sift3d_twin.cpp: the CPU restatement of the arithmetic contract of SIFT3D's scale space
(createGaussianPyramid, createDogPyramid, detectExtrema; src/oc_sift.cpp:676-847).  Shared by tests/test_sift3d_twin_cpu.py (twin
against the float64 model), tests/test_sift3d_plan_cpu.py (plan header against twin and model) and tests/test_gpu_sift3d.py
(kernel == twin bit for bit)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None

SLIP_NONE, SLIP_NOT_STRICT, SLIP_NO_SCALE_NEIGHBOURS, SLIP_BORDER_0, SLIP_REFLECTION, SLIP_DESCENDING, SLIP_THRESHOLD = 0, 1, 2, 3, 4, 5, 6
SLIPS = (SLIP_NOT_STRICT, SLIP_NO_SCALE_NEIGHBOURS, SLIP_BORDER_0, SLIP_REFLECTION, SLIP_DESCENDING, SLIP_THRESHOLD)

CANDIDATE = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32), ("octave", np.int32), ("layer", np.int32), ("scale", np.float32)])


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="sift3d_twin_")
        so = os.path.join(_dir.name, "libsift3d_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "sift3d_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.oc_twin_sift3d_set_slip.argtypes = [i]
        L.oc_twin_sift3d_set_slip.restype = None
        L.oc_twin_sift3d_build.argtypes = [vp, i, i, i, i, i, f, f, f, f, f, f, i]
        L.oc_twin_sift3d_build.restype = vp
        L.oc_twin_sift3d_free.argtypes = [vp]
        L.oc_twin_sift3d_free.restype = None
        L.oc_twin_sift3d_layers.argtypes = [vp, i]
        L.oc_twin_sift3d_layers.restype = i
        L.oc_twin_sift3d_octaves.argtypes = [vp]
        L.oc_twin_sift3d_octaves.restype = i
        L.oc_twin_sift3d_info.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, vp]
        L.oc_twin_sift3d_info.restype = ctypes.POINTER(ctypes.c_float)
        L.oc_twin_sift3d_weights.argtypes = [vp, i, i, vp]
        L.oc_twin_sift3d_weights.restype = i
        L.oc_twin_sift3d_detect.argtypes = [vp, vp, ctypes.c_long]
        L.oc_twin_sift3d_detect.restype = ctypes.c_long
        _lib = L
    return _lib


class slip:
    """``with slip(SLIP_...):`` the twin runs with one planted error."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        lib().oc_twin_sift3d_set_slip(self.which)

    def __exit__(self, *exc):
        lib().oc_twin_sift3d_set_slip(SLIP_NONE)


class Layer:
    """dims / units / radius are (x, y, z); vol is (z, y, x); weights: three float32 arrays for a blurred Gaussian layer."""

    def __init__(self, dims, units, octave, scale, sigma, max_abs, radius, vol, weights):
        self.dims, self.units, self.octave, self.scale, self.sigma, self.max_abs = dims, units, octave, scale, sigma, max_abs
        self.radius, self.vol, self.weights = radius, vol, weights


class Result:
    def __init__(self, n_octave, gauss, dog, candidates):
        self.n_octave, self.gauss, self.dog, self.candidates = n_octave, gauss, dog, candidates


def _layer(L, h, pyramid, index):
    dims, units, radius = (ctypes.c_int * 3)(), (ctypes.c_float * 3)(), (ctypes.c_int * 3)()
    octave, scale, sigma, max_abs = ctypes.c_int(), ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    ptr = L.oc_twin_sift3d_info(h, pyramid, index, dims, units, ctypes.byref(octave), ctypes.byref(scale), ctypes.byref(sigma),
                                ctypes.byref(max_abs), radius)
    shape = (dims[2], dims[1], dims[0])
    vol = np.ctypeslib.as_array(ptr, shape=shape).copy()
    weights = []
    if pyramid == 0 and radius[0] > 0:
        for axis in range(3):
            buf = np.zeros(64, np.float32)
            n = L.oc_twin_sift3d_weights(h, index, axis, buf.ctypes.data)
            weights.append(buf[:n].copy())
    return Layer(tuple(dims), tuple(np.float32(u) for u in units), octave.value, np.float32(scale.value), np.float32(sigma.value),
                 np.float32(max_abs.value), tuple(radius), vol, weights)


def scale_space(volume, n_octave_layers=3, min_dimension=8, alpha=0.1, sigma_source=1.15, sigma_base=1.6, units=(1.0, 1.0, 1.0), fma=0):
    """Both pyramids and the candidate list of a (z, y, x) float32 volume; ``units`` = (x, y, z)."""
    v = np.ascontiguousarray(volume, dtype=np.float32)
    assert v.ndim == 3
    L = lib()
    h = L.oc_twin_sift3d_build(v.ctypes.data, v.shape[2], v.shape[1], v.shape[0], int(n_octave_layers), int(min_dimension), float(alpha),
                               float(sigma_source), float(sigma_base), float(units[0]), float(units[1]), float(units[2]), int(fma))
    try:
        gauss = [_layer(L, h, 0, i) for i in range(L.oc_twin_sift3d_layers(h, 0))]
        dog = [_layer(L, h, 1, i) for i in range(L.oc_twin_sift3d_layers(h, 1))]
        n = L.oc_twin_sift3d_detect(h, None, 0)
        cand = np.zeros(n, dtype=CANDIDATE)
        if n:
            L.oc_twin_sift3d_detect(h, cand.ctypes.data, n)
        return Result(L.oc_twin_sift3d_octaves(h), gauss, dog, cand)
    finally:
        L.oc_twin_sift3d_free(h)

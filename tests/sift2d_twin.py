"""ctypes wrapper of tests/cpp/sift2d_twin.cpp: the float32 CPU restatement of the arithmetic contract of SIFT2D's detector
(cv::SIFT as SIFT2D::compute() creates it, src/oc_sift.cpp:22-30, 60-93).  Shared by
tests/test_sift2d_twin_cpu.py (twin against the float64 model), tests/test_sift2d_golden.py (the reference's own keypoint table)
and tests/test_gpu_sift2d.py (kernel == twin bit for bit)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None

(SLIP_NONE, SLIP_STRICT, SLIP_NO_LAYER_NEIGHBOURS, SLIP_BORDER_4, SLIP_PLAIN_REFLECT, SLIP_TRUNCATE, SLIP_THRESHOLD, SLIP_NO_HALF,
 SLIP_EDGE_INVERTED) = range(9)
SLIPS = {"strict": SLIP_STRICT, "no_layer_neighbours": SLIP_NO_LAYER_NEIGHBOURS, "border_4": SLIP_BORDER_4,
         "plain_reflect": SLIP_PLAIN_REFLECT, "truncate": SLIP_TRUNCATE, "threshold_not_floored": SLIP_THRESHOLD,
         "no_half": SLIP_NO_HALF, "edge_inverted": SLIP_EDGE_INVERTED}

KEYPOINT = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("response", np.float32),
                     ("octave", np.int32), ("layer", np.int32), ("row", np.int32), ("col", np.int32),
                     ("xc", np.float32), ("xr", np.float32), ("xi", np.float32), ("packed_octave", np.int32)])
START = np.dtype([("octave", np.int32), ("layer", np.int32), ("row", np.int32), ("col", np.int32), ("accepted", np.int32)])
assert KEYPOINT.itemsize == 48

DEFAULTS = dict(n_features=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6)


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="sift2d_twin_")
        so = os.path.join(_dir.name, "libsift2d_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "sift2d_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        vp, i, f, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
        L.oc_twin_sift2d_set_slip.argtypes = [i]
        L.oc_twin_sift2d_set_slip.restype = None
        L.oc_twin_sift2d_build.argtypes = [vp, i, i, i, i, i, f, f, f, vp]
        L.oc_twin_sift2d_build.restype = vp
        L.oc_twin_sift2d_free.argtypes = [vp]
        L.oc_twin_sift2d_free.restype = None
        L.oc_twin_sift2d_layers.argtypes = [vp, i]
        L.oc_twin_sift2d_octaves.argtypes = [vp]
        L.oc_twin_sift2d_threshold.argtypes = [vp]
        L.oc_twin_sift2d_info.argtypes = [vp, i, i, vp, vp, vp, vp, vp]
        L.oc_twin_sift2d_info.restype = ctypes.POINTER(ctypes.c_float)
        L.oc_twin_sift2d_weights.argtypes = [vp, i, vp]
        L.oc_twin_sift2d_detect.argtypes = [vp, vp, lg, vp, lg, vp]
        L.oc_twin_sift2d_detect.restype = lg
        for name in ("oc_twin_sift2d_pow2", "oc_twin_sift2d_powf"):
            getattr(L, name).argtypes = [f]
            getattr(L, name).restype = f
        _lib = L
    return _lib


class slip:
    """``with slip(SLIP_...):`` the twin runs with one planted error."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        lib().oc_twin_sift2d_set_slip(self.which)

    def __exit__(self, *exc):
        lib().oc_twin_sift2d_set_slip(SLIP_NONE)


class Layer:
    """One layer: data is (rows, cols) float32; weights: radius + 1 float32 for a blurred Gaussian layer."""

    def __init__(self, cols, rows, octave, sigma, radius, data, weights):
        self.cols, self.rows, self.octave, self.sigma, self.radius, self.data, self.weights = cols, rows, octave, sigma, radius, data, weights


class Result:
    def __init__(self, n_octave, threshold, gauss, dog, keypoints, starts):
        self.n_octave, self.threshold, self.gauss, self.dog, self.keypoints, self.starts = n_octave, threshold, gauss, dog, keypoints, starts


class Refused(Exception):
    def __init__(self, status):
        super().__init__("the plan refuses with status %d" % status)
        self.status = status


def _layer(L, h, pyramid, index):
    cols, rows, octave, radius, sigma = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    ptr = L.oc_twin_sift2d_info(h, pyramid, index, ctypes.byref(cols), ctypes.byref(rows), ctypes.byref(octave), ctypes.byref(sigma),
                                ctypes.byref(radius))
    data = np.ctypeslib.as_array(ptr, shape=(rows.value, cols.value)).copy()
    weights = None
    if pyramid == 0 and radius.value > 0:
        buf = np.zeros(64, np.float32)
        n = L.oc_twin_sift2d_weights(h, index, buf.ctypes.data)
        weights = buf[:n].copy()
    return Layer(cols.value, rows.value, octave.value, np.float32(sigma.value), radius.value, data, weights)


def detector(image, layers=True, **cfg):
    """Both pyramids (``layers``), the located keypoints and every starting extremum of a (rows, cols) uint8 or float32 image."""
    c = dict(DEFAULTS, **cfg)
    img = np.ascontiguousarray(image)
    if img.dtype != np.uint8:
        img = np.ascontiguousarray(img, dtype=np.float32)
    assert img.ndim == 2
    L = lib()
    status = ctypes.c_int()
    h = L.oc_twin_sift2d_build(img.ctypes.data, int(img.dtype == np.uint8), img.shape[1], img.shape[0], int(c["n_features"]),
                               int(c["n_octave_layers"]), float(c["contrast_threshold"]), float(c["edge_threshold"]), float(c["sigma"]),
                               ctypes.byref(status))
    if not h:
        raise Refused(status.value)
    try:
        gauss = [_layer(L, h, 0, i) for i in range(L.oc_twin_sift2d_layers(h, 0))] if layers else None
        dog = [_layer(L, h, 1, i) for i in range(L.oc_twin_sift2d_layers(h, 1))] if layers else None
        n_starts = ctypes.c_long()
        n = L.oc_twin_sift2d_detect(h, None, 0, None, 0, ctypes.byref(n_starts))
        kps, starts = np.zeros(n, dtype=KEYPOINT), np.zeros(n_starts.value, dtype=START)
        L.oc_twin_sift2d_detect(h, kps.ctypes.data, n, starts.ctypes.data, n_starts.value, ctypes.byref(n_starts))
        return Result(L.oc_twin_sift2d_octaves(h), L.oc_twin_sift2d_threshold(h), gauss, dog, kps, starts)
    finally:
        L.oc_twin_sift2d_free(h)

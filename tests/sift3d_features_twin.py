"""ctypes wrapper of tests/cpp/sift3d_features_twin.cpp: the CPU restatement of the arithmetic contract of SIFT3D's orientation and
descriptor stages (assignOrientation, constructDescriptor; src/oc_sift.cpp:849-1249) over the Gaussian layers of the scale-space twin
(tests/sift3d_twin.py).  Shared by tests/test_sift3d_features_cpu.py (twin against the float64 model, the planted slips, the pipeline
property) and tests/test_gpu_sift3d_features.py (kernel == twin bit for bit).  ``mode`` 0 is the contract (exact sums), 1 the
reference's sequential float32 accumulation, which only measures."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import match_twin
import sift3d_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None

SLIP_NONE, SLIP_FLOOR_INDEX, SLIP_DIVIDE_870, SLIP_LAST_TILE, SLIP_STRICT_SPHERE, SLIP_NO_TRUNCATION, SLIP_TRANSPOSED, SLIP_ASCENDING = range(8)
ORIENT_SLIPS = (SLIP_DIVIDE_870, SLIP_STRICT_SPHERE, SLIP_TRANSPOSED, SLIP_ASCENDING)
DESCRIBE_SLIPS = (SLIP_FLOOR_INDEX, SLIP_LAST_TILE, SLIP_STRICT_SPHERE, SLIP_NO_TRUNCATION)

CANDIDATE = sift3d_twin.CANDIDATE
KEYPOINT = np.dtype([("coor_layer", np.float32, 3), ("coor_img", np.float32, 3), ("octave", np.int32), ("layer", np.int32), ("scale", np.float32),
                     ("rotation_matrix", np.float32, 9)])
assert KEYPOINT.itemsize == 72
ACCEPTED, REJECT_GRADIENT, REJECT_EIGENVALUES, REJECT_ANGLE = 0, 1, 2, 3
# beta, gamma, gradient_threshold, truncate_threshold: the defaults of SIFT3D::SIFT3D() (src/oc_sift.cpp:147-152)
FEATURE_DEFAULTS = dict(beta=0.9, gamma=0.4, gradient_threshold=0.0000000001, truncate_threshold=float(np.float32(0.2) * np.float32(128) / np.float32(768)))


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="sift3d_features_twin_")
        so = os.path.join(_dir.name, "libsift3d_features_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "sift3d_features_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        vp, i, f, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
        L.oc_twin_features_set_slip.argtypes = [i]
        L.oc_twin_features_set_slip.restype = None
        L.oc_twin_features_grid_exponent.argtypes = [f, f]
        L.oc_twin_features_grid_exponent.restype = i
        L.oc_twin_features_gradient_forms.argtypes = [f, f, f, vp, vp]
        L.oc_twin_features_gradient_forms.restype = None
        L.oc_twin_features_orient.argtypes = [vp, vp, vp, i, vp, lg, i, f, f, f, i, vp, vp, vp]
        L.oc_twin_features_orient.restype = None
        L.oc_twin_features_describe.argtypes = [vp, vp, vp, i, vp, lg, i, f, i, vp]
        L.oc_twin_features_describe.restype = None
        _lib = L
    return _lib


class slip:
    """``with slip(SLIP_...):`` the twin runs with one planted error."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        lib().oc_twin_features_set_slip(self.which)

    def __exit__(self, *exc):
        lib().oc_twin_features_set_slip(SLIP_NONE)


def grid_exponent(volume, units):
    """E of the exact sums' grid: the smallest integer with 2^E >= 2 max|v| / min(unit); None for a volume with non-finite voxels."""
    e = lib().oc_twin_features_grid_exponent(float(np.max(np.abs(np.asarray(volume, np.float32)))), float(min(units)))
    return None if e == -1000 else e


class Pyramid:
    """The Gaussian layers of a sift3d_twin.Result in the form the C functions take."""

    def __init__(self, gauss, n_octave_layers):
        self.n_octave_layers = int(n_octave_layers)
        self.gauss = gauss
        self._vols = [np.ascontiguousarray(g.vol, np.float32) for g in gauss]
        self.pointers = (ctypes.c_void_p * len(gauss))(*[v.ctypes.data for v in self._vols])
        self.dims = np.array([g.dims for g in gauss], np.int32)
        self.units = np.array([g.units for g in gauss], np.float32)

    def layer_index(self, octave, layer):
        return int(layer) + int(octave) * (self.n_octave_layers + 3)


def orient(pyramid, candidates, exponent, beta=0.9, gamma=0.4, gradient_threshold=0.0000000001, mode=0, **_):
    """(status, sums (n, 9), slots): one entry per candidate; the accepted keypoints are ``slots[status == 0]``."""
    cand = np.ascontiguousarray(candidates, dtype=CANDIDATE)
    n = len(cand)
    status = np.zeros(n, np.int32)
    sums = np.zeros((n, 9), np.float32)
    slots = np.zeros(n, KEYPOINT)
    if n:
        lib().oc_twin_features_orient(pyramid.pointers, pyramid.dims.ctypes.data, pyramid.units.ctypes.data, pyramid.n_octave_layers, cand.ctypes.data, n,
                                      int(exponent), float(beta), float(gamma), float(gradient_threshold), int(mode), status.ctypes.data,
                                      sums.ctypes.data, slots.ctypes.data)
    return status, sums, slots


def describe(pyramid, keypoints, exponent, truncate_threshold=FEATURE_DEFAULTS["truncate_threshold"], mode=0, **_):
    """(n, 768) float32"""
    kp = np.ascontiguousarray(keypoints, dtype=KEYPOINT)
    out = np.zeros((len(kp), 768), np.float32)
    if len(kp):
        lib().oc_twin_features_describe(pyramid.pointers, pyramid.dims.ctypes.data, pyramid.units.ctypes.data, pyramid.n_octave_layers, kp.ctypes.data,
                                        len(kp), int(exponent), float(truncate_threshold), int(mode), out.ctypes.data)
    return out


class Features:
    def __init__(self, scale_space, pyramid, exponent, status, sums, slots, keypoints, descriptors):
        self.scale_space, self.pyramid, self.exponent = scale_space, pyramid, exponent
        self.status, self.sums, self.slots, self.keypoints, self.descriptors = status, sums, slots, keypoints, descriptors


def extract(volume, settings, features=None, fma=0, mode=0, candidates=None, with_descriptors=True):
    """The whole extraction of one (z, y, x) volume: scale space, orientation of its candidates (or of ``candidates``), descriptors."""
    features = dict(FEATURE_DEFAULTS, **(features or {}))
    ss = sift3d_twin.scale_space(volume, fma=fma, **settings)
    pyr = Pyramid(ss.gauss, settings["n_octave_layers"])
    e = grid_exponent(volume, settings["units"])
    cand = ss.candidates if candidates is None else candidates
    status, sums, slots = orient(pyr, cand, e, mode=mode, **features)
    kp = slots[status == ACCEPTED]
    desc = describe(pyr, kp, e, features["truncate_threshold"], mode=mode) if with_descriptors else None
    return Features(ss, pyr, e, status, sums, slots, kp, desc)


def pipeline(ref, tar, settings, ratio=0.85, bidirectional=False, features=None):
    """SIFT3D::compute (src/oc_sift.cpp:234-293) on the twins: the matched coor_img pairs, (n, 3) each."""
    a, b = extract(ref, settings, features), extract(tar, settings, features)
    ri, ti = match_twin.pairs(a.descriptors, b.descriptors, ratio, 1 if bidirectional else 0)
    return a.keypoints["coor_img"][ri], b.keypoints["coor_img"][ti], a, b

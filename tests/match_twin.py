"""ctypes wrapper of tests/cpp/match_twin.cpp: the CPU restatement of the descriptor matcher's arithmetic contract (the
sequential scan of SIFT3D::bruteforceMatch, src/oc_sift.cpp:625-674, and the two match modes).  Shared by
tests/test_match_twin_cpu.py (twin against the float64 model) and tests/test_gpu_match.py (kernel == twin bit for bit)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None

SLIP_NONE, SLIP_LESS_EQUAL, SLIP_RATIO_UNSQUARED, SLIP_ASCENDING = 0, 1, 2, 3


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="match_twin_")
        so = os.path.join(_dir.name, "libmatch_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "match_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
        i, f, n = ctypes.c_int, ctypes.c_float, ctypes.c_long
        L.oc_twin_match_set_slip.argtypes = [i]
        L.oc_twin_match_set_slip.restype = None
        L.oc_twin_match_nearest.argtypes = [fp, n, fp, n, i, f, i, ip, fp, fp]
        L.oc_twin_match_nearest.restype = n
        L.oc_twin_match_pairs.argtypes = [fp, n, fp, n, i, f, i, i, ip, ip]
        L.oc_twin_match_pairs.restype = n
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _rows(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2
    return a


class slip:
    """``with slip(SLIP_...):`` the twin runs with one planted error."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        lib().oc_twin_match_set_slip(self.which)

    def __exit__(self, *exc):
        lib().oc_twin_match_set_slip(SLIP_NONE)


def nearest(query, cand, ratio, fma=0):
    """(matched_idx, best_sq, second_sq, n_matched) of every query row against all candidate rows."""
    q, c = _rows(query), _rows(cand)
    assert q.shape[1] == c.shape[1]
    idx = np.empty(q.shape[0], np.int32)
    best = np.empty(q.shape[0], np.float32)
    second = np.empty(q.shape[0], np.float32)
    n = lib().oc_twin_match_nearest(_fp(q), q.shape[0], _fp(c), c.shape[0], q.shape[1], float(ratio), int(fma), _ip(idx), _fp(best),
                                    _fp(second))
    return idx, best, second, int(n)


def pairs(ref, tar, ratio, mode, fma=0):
    """(ref_idx, tar_idx): mode 0 = monodirectional, 1 = bidirectional."""
    r, t = _rows(ref), _rows(tar)
    assert r.shape[1] == t.shape[1]
    cap = min(r.shape[0], t.shape[0])
    ri = np.empty(cap, np.int32)
    ti = np.empty(cap, np.int32)
    n = lib().oc_twin_match_pairs(_fp(r), r.shape[0], _fp(t), t.shape[0], r.shape[1], float(ratio), int(fma), int(mode), _ip(ri), _ip(ti))
    return ri[:n].copy(), ti[:n].copy()

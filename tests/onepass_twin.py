"""ctypes wrapper of tests/cpp/icgn2d_onepass_twin.cpp: the CPU restatement of the one-pass arithmetic contract of
ICGN2D1 / ICGN2D2 (oc_hip_set_tuning "arith_onepass").  Shared by tests/test_onepass_twin_cpu.py (CPU) and
tests/test_gpu_arith_onepass.py / tests/test_gpu_fullsize_onepass.py (GPU == twin bit for bit)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="onepass_twin_")
        so = os.path.join(_dir.name, "libicgn2d_onepass_twin.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "icgn2d_onepass_twin.cpp"), "-o", so])
        L = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        i, f = ctypes.c_int, ctypes.c_float
        L.oc_twin_icgn2d_onepass.argtypes = [i, fp, fp, fp, fp, i, i, i, i, f, f, fp, ctypes.c_long, i]
        L.oc_twin_icgn2d_onepass.restype = None
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def icgn2d(dof, prep, rx, ry, conv, stop, pois):
    """In place on ``pois`` (n x 25 float32): ICGN2D1 (dof 6) / ICGN2D2 (dof 12) under the one-pass contract.  ``prep`` is an
    oracle.Prepared2D."""
    assert dof in (6, 12)
    assert pois.dtype == np.float32 and pois.flags.c_contiguous and pois.ndim == 2 and pois.shape[1] == 25
    h, w = prep.ref.shape
    lib().oc_twin_icgn2d_onepass(dof, _fp(prep.ref), _fp(prep.gx), _fp(prep.gy), _fp(prep.lut), h, w, int(rx), int(ry), float(conv),
                                 float(stop), _fp(pois), pois.shape[0], pois.shape[1])
    return pois


def icgn2d1(prep, rx, ry, conv, stop, pois):
    return icgn2d(6, prep, rx, ry, conv, stop, pois)


def icgn2d2(prep, rx, ry, conv, stop, pois):
    return icgn2d(12, prep, rx, ry, conv, stop, pois)


def codes(p):
    """Failure code of every record (-3 / -4 / -5 / whatever a rejected record carried), 0 where it converged."""
    z = p[:, 16]
    return np.where(z < 0, z, np.float32(0))


def vs_reference_order(got, seq):
    """`got` against the oracle in the reference's loop order (ORDER_SEQ) on the same guesses: records whose failure code differs,
    fraction of commonly converged POIs with equal iteration counts and -- over those -- max |d u|, |d v| and max |d ZNCC|."""
    cg, cs = codes(got), codes(seq)
    both = (cg == 0) & (cs == 0)
    same_it = both & (got[:, 17] == seq[:, 17])
    dd = np.abs(got[same_it][:, [2, 8]].astype(np.float64) - seq[same_it][:, [2, 8]].astype(np.float64))
    dz = np.abs(got[same_it, 16].astype(np.float64) - seq[same_it, 16].astype(np.float64))
    return dict(code_mismatch=(cg != cs), iteration_agreement=float(same_it.sum() / max(1, both.sum())),
                max_abs_d_disp=float(dd.max()) if dd.size else 0.0, max_abs_d_zncc=float(dz.max()) if dz.size else 0.0,
                over_1e4=int((dd.max(axis=1) > 1e-4).sum()) if dd.size else 0, same_it=int(same_it.sum()))


def check_golden_oht(got, seq, guesses, golden):
    """The assertions on the reference's OHT example: the four of test_golden_oht_on_gpu_fma against the golden table, and
    identical codes against ORDER_SEQ except where ORDER_SEQ's own convergence value lies within 5 % of the criterion (a POI
    that ends its last iteration on the criterion; ORDER_LANES uses the exception for one POI of 30 000)."""
    tab = golden["table"]   # x y u v u0 v0 zncc iteration convergence
    same = (guesses[:, 2] == tab[:, 4]) & (guesses[:, 8] == tab[:, 5])
    m = (tab[:, 7] < golden["stop"]) & same
    du, dv = np.abs(got[m, 2] - tab[m, 2]).max(), np.abs(got[m, 8] - tab[m, 3]).max()
    dz = np.abs(got[m, 16] - tab[m, 6]).max()
    it = (got[m, 17] == tab[m, 7]).mean()
    r = vs_reference_order(got, seq)
    mism = r["code_mismatch"]
    near = np.abs(seq[:, 18] - golden["conv"]) <= 0.05 * golden["conv"]
    used = int((mism & near).sum())
    print("golden OHT: m = %d, max |du| %.3e |dv| %.3e |dzncc| %.3e, equal iterations %.5f; vs ORDER_SEQ: code exceptions used %d of %d "
          "(outside the exception: %d), equal iterations %.5f, max |d disp| %.3e (%d beyond 1e-4), max |d zncc| %.3e"
          % (m.sum(), du, dv, dz, it, used, len(got), int((mism & ~near).sum()), r["iteration_agreement"], r["max_abs_d_disp"],
             r["over_1e4"], r["max_abs_d_zncc"]))
    assert m.sum() > 28000
    assert du <= 2e-4 and dv <= 2e-4
    assert dz <= 1e-5
    assert it >= 0.99
    assert not (mism & ~near).any(), np.flatnonzero(mism & ~near)[:10].tolist()
    assert used <= 0.0005 * len(got), used

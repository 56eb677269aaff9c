"""opencorr::FeatureAffine2D / FeatureAffine3D (include/opencorr_compat/oc_feature_affine.h) through the umbrella header.

* The reference's examples/test_dvc_sift_icgn1.cpp -- SIFT3D -> FeatureAffine3D -> ICGN3D1 -- compiles UNMODIFIED against the
  compat headers (CPU, compile only; the recipe of tests/test_stereo_examples_compile.py, skipped without the reference tree).
* A small main of ours that uses both classes as the reference's examples do compiles and links against the C-ABI library (CPU);
  on the GPU it reproduces the CPU twin's records bit for bit, compute(POI*) and self-adaptive mode included."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import feature_affine_cases as cases
import feature_affine_twin as twin
from oracle.ref import REFERENCE_ROOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "opencorr_amd", "lib")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC)")


def test_reference_dvc_sift_icgn1_example_compiles_unmodified():
    src = os.path.join(REFERENCE_ROOT, "examples", "test_dvc_sift_icgn1.cpp")
    if not os.path.exists(src):
        pytest.skip("reference tree not mounted")
    cmd = ["g++", "-std=c++17", "-fopenmp", "-fsyntax-only", "-w", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "include", "opencorr_compat"), src]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]


def _build(tmp_path):
    exe = str(tmp_path / "feature_affine_compat_main")
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "feature_affine_compat_main.cpp"), "-o", exe, "-L" + LIBDIR, "-lopencorr_hip",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    return exe


def test_feature_affine_main_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # wrong usage exits with its own code before touching the GPU
    assert subprocess.call([exe]) == 2


def _records(lines, tag):
    rows = [[int(w, 16) for w in l.split()[2:]] for l in lines if l.startswith(tag + " ")]
    return np.array(rows, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("ndim", [2, 3])
def test_feature_affine_main_reproduces_the_twin(tmp_path, ndim):
    exe = _build(tmp_path)
    case = cases.noisy(ndim, 2001 if ndim == 2 else 3001)
    path = str(tmp_path / "keypoints.f32")
    np.concatenate([np.array([case["ref"].shape[0]], np.float32), case["ref"].ravel(), case["tar"].ravel()]).tofile(path)
    out = subprocess.run([exe, str(ndim), path, "77"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    lines = out.stdout.decode().splitlines()
    if ndim == 3:
        pts = [(15 + 15 * x, 15 + 15 * y, 15 + 15 * z) for z in range(3) for y in range(3) for x in range(3)]
        want = twin.compute(case["ref"], case["tar"], cases.queue(np.array(pts, np.float32)), case["radius"], trials=24, seed=77)
    else:
        pts = [(40 + 60 * x, 40 + 60 * y) for y in range(3) for x in range(3)]
        want = twin.compute(case["ref"], case["tar"], cases.queue(np.array(pts, np.float32)), case["radius"], seed=77)
        adaptive = twin.compute(case["ref"], case["tar"], cases.queue(np.array(pts, np.float32)), case["radius"], seed=77, adaptive=(14, 10, 200, 200))
        assert np.array_equal(_records(lines, "adaptive"), adaptive.view(np.uint32))
    assert np.array_equal(_records(lines, "poi"), want.view(np.uint32))
    assert (want[:, cases.ZNCC[ndim]] == 0).all()

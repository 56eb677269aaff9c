"""opencorr::SIFT2DScaleSpace and Sift2dConfig (include/opencorr_compat/oc_feature_detect.h) through the umbrella header: a small
main compiles with hipcc and links against the C-ABI library (CPU); on the GPU it reproduces the twin's -- and so the Python
binding's -- keypoints for the "odd_sides" case of tests/sift2d_cases.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sift2d_cases as cases
import sift2d_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "opencorr_amd", "lib")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC)")


def _build(tmp_path):
    exe = str(tmp_path / "sift2d_compat_main")
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "sift2d_compat_main.cpp"), "-o", exe, "-L" + LIBDIR, "-lopencorr_hip",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    return exe


def test_detector_main_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # wrong usage exits with its own code before touching the GPU
    assert subprocess.call([exe]) == 2


@pytest.mark.gpu
def test_detector_main_reproduces_the_twin(tmp_path):
    exe = _build(tmp_path)
    image = cases.CASE_BY_NAME["odd_sides"].image().astype(np.float32)
    path = str(tmp_path / "image.f32")
    image.tofile(path)
    out = subprocess.run([exe, path, str(image.shape[1]), str(image.shape[0])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    lines = out.stdout.decode().splitlines()
    want = twin.detector(image)
    assert lines[0].split() == ["octaves", str(want.n_octave), "keypoints", str(len(want.keypoints))] and len(want.keypoints) >= 10
    got = [l.split()[1:] for l in lines if l.startswith("kp ")]
    assert got == [["%08x" % int(np.float32(k[f]).view(np.uint32)) for f in ("x", "y", "size", "response")]
                   + [str(int(k[f])) for f in ("octave", "layer", "row", "col", "packed_octave")] for k in want.keypoints]

"""opencorr::SIFT3DScaleSpace (include/opencorr_compat/oc_feature_detect.h) through the umbrella header: a small main compiles
with hipcc and links against the C-ABI library (CPU); on the GPU it reproduces the twin's -- and so the Python binding's --
result for the first case of tests/sift3d_cases.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sift3d_cases as cases
import sift3d_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "opencorr_amd", "lib")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC)")


def _build(tmp_path):
    exe = str(tmp_path / "sift3d_compat_main")
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "sift3d_compat_main.cpp"), "-o", exe, "-L" + LIBDIR, "-lopencorr_hip",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    return exe


def test_scale_space_main_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # wrong usage exits with its own code before touching the GPU
    assert subprocess.call([exe]) == 2


@pytest.mark.gpu
def test_scale_space_main_reproduces_case_1(tmp_path):
    exe = _build(tmp_path)
    case = cases.CASES[0]
    volume = case.volume()
    path = str(tmp_path / "volume.f32")
    volume.tofile(path)
    out = subprocess.run([exe, path, str(volume.shape[2]), str(volume.shape[1]), str(volume.shape[0])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    lines = out.stdout.decode().splitlines()
    want = twin.scale_space(volume, **case.settings)
    assert lines[0].split() == ["octaves", str(want.n_octave), "gauss", str(len(want.gauss)), "dog", str(len(want.dog))]
    assert lines[1].split()[1:] == ["%08x" % int(np.float32(d.max_abs).view(np.uint32)) for d in want.dog]
    kps = [l.split()[1:] for l in lines if l.startswith("kp ")]
    assert kps == [[str(int(c[f])) for f in ("x", "y", "z", "octave", "layer")] + ["%08x" % int(np.float32(c["scale"]).view(np.uint32))]
                   for c in want.candidates] and len(kps) >= 1
    sums = {(int(l.split()[1]), int(l.split()[2])): int(l.split()[3]) for l in lines if l.startswith("sum ")}
    for pyramid, layers in ((0, want.gauss), (1, want.dog)):
        for i, t in enumerate(layers):
            assert sums[(pyramid, i)] == int(t.vol.view(np.uint32).astype(np.uint64).sum()), (pyramid, i)

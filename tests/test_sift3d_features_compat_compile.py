"""opencorr::SIFT3D and the orientation / descriptor methods of opencorr::SIFT3DScaleSpace (include/opencorr_compat/oc_feature_detect.h)
through the umbrella header: a main that uses the class as lines 82-104 of the reference's examples/test_dvc_sift_icgn1.cpp do compiles
with hipcc and links against the C-ABI library (CPU); on the GPU it reproduces the twin pipeline's matched pairs and descriptors."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sift3d_features_cases as cases
import sift3d_features_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "opencorr_amd", "lib")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC)")


def _build(tmp_path):
    exe = str(tmp_path / "sift3d_features_compat_main")
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "sift3d_features_compat_main.cpp"), "-o", exe, "-L" + LIBDIR, "-lopencorr_hip",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    return exe


def test_sift3d_main_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # wrong usage exits with its own code before touching the GPU
    assert subprocess.call([exe]) == 2


def _fmt(v):
    """a float32 as ``std::ostream << float`` prints it (6 significant digits)"""
    return "%g" % float(v)


@pytest.mark.gpu
def test_sift3d_main_reproduces_the_twin_pipeline(tmp_path):
    exe = _build(tmp_path)
    ref, tar = cases.shift_pair()
    paths = [str(tmp_path / "ref.f32"), str(tmp_path / "tar.f32")]
    ref.tofile(paths[0])
    tar.tofile(paths[1])
    out = subprocess.run([exe, *paths, str(ref.shape[2]), str(ref.shape[1]), str(ref.shape[0])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    lines = out.stdout.decode().splitlines()
    want_ref, want_tar, a, _ = twin.pipeline(ref, tar, cases.SETTINGS)
    assert len(want_ref) >= 5
    assert lines[0].split() == ["pairs", str(len(want_ref))]
    pairs = [l.split()[1:] for l in lines if l.startswith("pair ")]
    assert pairs == [[",".join(_fmt(c) for c in r), ",".join(_fmt(c) for c in t)] for r, t in zip(want_ref, want_tar)]
    kps = [l.split()[1:] for l in lines if l.startswith("kp ")]
    assert kps == [[str(int(k["coor_img"][0])), str(int(k["coor_img"][1])), str(int(k["coor_img"][2])), str(int(k["octave"])), str(int(k["layer"])),
                    str(int(d.view(np.uint32).astype(np.uint64).sum()))] for k, d in zip(a.keypoints, a.descriptors)]

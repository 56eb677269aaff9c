"""opencorr::DescriptorMatcher3D (include/opencorr_compat/oc_feature_match.h) through the umbrella header: a small main compiles
with plain g++ and links against the C-ABI library (CPU; the recipe of tests/test_cpp_shim.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "opencorr_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "match_compat_main")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "match_compat_main.cpp"), "-o", exe, "-L" + LIBDIR, "-lopencorr_hip",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    return exe


def test_descriptor_matcher_main_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # wrong usage exits with its own code before touching the GPU
    assert subprocess.call([exe]) == 2


@pytest.mark.gpu
def test_descriptor_matcher_main_runs(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe, "70"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    assert out.stdout.decode().split() == ["70", "70", "70"]

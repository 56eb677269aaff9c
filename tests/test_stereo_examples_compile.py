"""The reference's stereo example mains compile UNMODIFIED against include/opencorr_compat (CPU, compile only; the recipe of
tests/test_reference_examples_compile.py).  Needs the reference tree (oracle.ref.REFERENCE_ROOT): skipped without it.
examples/test_3d_dic_epipolar_sift.cpp needs SIFT2D and FeatureAffine2D, which this project does not have."""
import os
import subprocess

import pytest

from oracle.ref import REFERENCE_ROOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXAMPLES = ["test_3d_reconstruction_epipolar", "test_3d_dic_strain"]


@pytest.mark.parametrize("name", EXAMPLES)
def test_stereo_example_compiles_unmodified(name):
    src = os.path.join(REFERENCE_ROOT, "examples", name + ".cpp")
    if not os.path.exists(src):
        pytest.skip("reference tree not mounted")
    cmd = ["g++", "-std=c++17", "-fopenmp", "-fsyntax-only", "-w", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "include", "opencorr_compat"), src]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]

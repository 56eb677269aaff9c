"""opencorr_amd/csrc/host/sift3d_plan.h -- the layer table, blur radii and weights and the support verdict of SIFT3D's scale
space -- against the float64 model's plan (tests/sift3d_model.py, written independently) and, for the weights, bit for bit
against the twin (tests/cpp/sift3d_twin.cpp), whose weights come from the same libm.  CPU only: tests/cpp/sift3d_plan_check.cpp
is a stand-alone program over the header, built with plain g++ (-ffp-contract=off like the library) and once more with
-fsanitize=undefined,address.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import sift3d_model as model
import sift3d_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, 1, 5
SHAPES = [(8, 8, 8), (9, 9, 9), (15, 15, 15), (16, 16, 16), (17, 17, 17), (64, 64, 64), (100, 100, 100), (18, 33, 40)]   # (z, y, x)
LAYERS = (2, 3, 4)
UNITS = ((1.0, 1.0, 1.0), (1.0, 1.0, 2.0))   # (x, y, z)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("sift3d_plan")
    built = []
    for tag, flags in (("", ("-O2",)), ("_san", ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(out / ("sift3d_plan_check" + tag))
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "opencorr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sift3d_plan_check.cpp"), "-o", exe], check=True, timeout=600)
        built.append(exe)
    return built


def _f(word):
    return struct.unpack("<f", struct.pack("<I", int(word, 16)))[0]


def _ask(exe, shape, n_octave_layers=3, min_dimension=8, sigma_source=1.15, sigma_base=1.6, units=(1.0, 1.0, 1.0)):
    args = [*shape, n_octave_layers, min_dimension, sigma_source, sigma_base, *units]
    out = subprocess.run([exe, *(repr(a) for a in args)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    status = int(lines[0].split()[1])
    plan = {"status": status, "why": lines[0].split(" ", 2)[2] if len(lines[0].split(" ", 2)) > 2 else "", "layers": [], "weights": {}}
    if status != OK:
        return plan
    plan["octaves"] = int(lines[1].split()[1])
    for line in lines[2:]:
        t = line.split()
        if t[0] == "layer":
            plan["layers"].append(dict(dims=tuple(int(v) for v in t[3:6]), units=tuple(_f(v) for v in t[7:10]), octave=int(t[11]), scale=_f(t[13]),
                                       sigma=_f(t[15]), source=int(t[17]), blurred=int(t[19]), radius=tuple(int(v) for v in t[21:24])))
        else:
            plan["weights"][(int(t[1]), int(t[2]))] = np.array([int(v, 16) for v in t[3:]], dtype=np.uint32).view(np.float32)
    return plan


def _check_against_model_and_twin(plan, shape, n_octave_layers, units, sigma_source=1.15, sigma_base=1.6):
    n_octave, layers = model.plan(shape, n_octave_layers, 8, sigma_source, sigma_base, units)
    assert plan["status"] == OK and plan["octaves"] == n_octave and len(plan["layers"]) == len(layers)
    tw = twin.scale_space(np.zeros(shape, np.float32), n_octave_layers=n_octave_layers, sigma_source=sigma_source, sigma_base=sigma_base, units=units)
    assert tw.n_octave == n_octave
    for i, (got, want, t) in enumerate(zip(plan["layers"], layers, tw.gauss)):
        assert got["dims"] == want.dims == t.dims, i
        assert got["units"] == tuple(float(u) for u in want.units), i
        assert got["octave"] == want.octave and got["source"] == want.source and got["blurred"] == int(want.blurred), i
        assert got["scale"] == pytest.approx(float(want.scale), rel=1e-6) and np.float32(got["scale"]) == t.scale, i
        if want.blurred:
            assert got["radius"] == tuple(want.radius) == t.radius, i
            if np.isnan(want.sigma):
                assert np.isnan(got["sigma"])
            else:
                assert got["sigma"] == pytest.approx(float(want.sigma), rel=1e-5) and np.float32(got["sigma"]) == t.sigma, i
            for axis in range(3):
                w = plan["weights"][(i, axis)]
                assert w.tobytes() == t.weights[axis].tobytes(), (i, axis)                  # the twin's, bit for bit
                np.testing.assert_allclose(w, want.weights[axis], rtol=2e-6, atol=1e-12)      # float32 rounding of a few operations
        else:
            assert got["radius"] == (0, 0, 0) and got["sigma"] == 0.0, i


@pytest.mark.parametrize("units", UNITS)
@pytest.mark.parametrize("n_octave_layers", LAYERS)
def test_plan_equals_model_and_twin(exes, n_octave_layers, units):
    for shape in SHAPES:
        _check_against_model_and_twin(_ask(exes[0], shape, n_octave_layers, units=units), shape, n_octave_layers, units)


def test_expected_octaves_and_radii(exes):
    """the figures the kernel cases rest on, stated by hand"""
    p = _ask(exes[0], (18, 33, 40))
    assert p["octaves"] == 2 and len(p["layers"]) == 12
    assert p["layers"][6]["dims"] == (20, 16, 9) and p["layers"][6]["source"] == 3 and p["layers"][6]["units"] == (2.0, 2.0, 2.0)
    assert [l["radius"][2] for l in p["layers"][:6]] == [2, 3, 4, 5, 6, 8]        # R = 8 = dim_z - 1 of octave 1: the last defined reflection
    assert p["layers"][11]["radius"] == (8, 8, 8)
    assert _ask(exes[0], (16, 16, 16))["layers"][11]["dims"] == (8, 8, 8)          # ... and R = 8 > 7: the clamp rule
    assert _ask(exes[0], (20, 40, 40), units=(1.0, 1.0, 2.0))["layers"][5]["radius"] == (16, 16, 8)
    assert _ask(exes[0], (8, 8, 8))["octaves"] == 1 and _ask(exes[0], (7, 9, 9))["octaves"] == 1 and _ask(exes[0], (64, 64, 64))["octaves"] == 4
    assert [l["dims"] for l in _ask(exes[0], (19, 21, 37))["layers"]][6] == (18, 10, 9)


def test_sigma_base_below_sigma_source(exes):
    """sqrtf of a negative number is NaN, which is not > 0: radius 1, weights {1, 0} (src/oc_sift.cpp:373-381)"""
    p = _ask(exes[0], (16, 16, 16), sigma_source=1.6, sigma_base=1.15)
    assert np.isnan(p["layers"][0]["sigma"]) and p["layers"][0]["radius"] == (1, 1, 1)
    for axis in range(3):
        assert p["weights"][(0, axis)].tolist() == [1.0, 0.0]
    _check_against_model_and_twin(p, (16, 16, 16), 3, (1.0, 1.0, 1.0), sigma_source=1.6, sigma_base=1.15)


def test_refusals(exes):
    # radius 8 * floor(4.125 + 0.5) = 32 is the limit, 8 * floor(4.5 + 0.5) = 40 and 11 * 3 = 33 are beyond it
    assert _ask(exes[0], (16, 16, 16), units=(1.0, 1.0, 4.125))["layers"][5]["radius"] == (32, 32, 8)
    for kwargs in (dict(units=(1.0, 1.0, 4.5)), dict(sigma_base=2.2, units=(1.0, 1.0, 3.0))):
        p = _ask(exes[0], (16, 16, 16), **kwargs)
        assert p["status"] == ERR_UNSUPPORTED and "radius" in p["why"], p
    p = _ask(exes[0], (16, 16, 16), sigma_base=2.2, units=(1.0, 1.0, 3.0))
    assert "radius 33" in p["why"]
    assert _ask(exes[0], (2048, 1024, 1024))["status"] == ERR_UNSUPPORTED          # 2^31 voxels
    assert _ask(exes[0], (2047, 1024, 1024), min_dimension=512)["status"] == OK    # 2^31 - 2^20
    assert _ask(exes[0], (16, 16, 16), n_octave_layers=17)["status"] == ERR_UNSUPPORTED
    for kwargs in (dict(n_octave_layers=0), dict(min_dimension=0), dict(units=(0.0, 1.0, 1.0)), dict(units=(1.0, float("nan"), 1.0))):
        assert _ask(exes[0], (16, 16, 16), **kwargs)["status"] == ERR_INVALID
    assert _ask(exes[0], (0, 16, 16))["status"] == ERR_INVALID


def test_sanitized_build_agrees(exes):
    for kwargs in (dict(), dict(units=(1.0, 1.0, 2.0), n_octave_layers=4), dict(sigma_source=1.6, sigma_base=1.15), dict(units=(1.0, 1.0, 4.5))):
        for shape in ((18, 33, 40), (8, 8, 8)):
            a, b = _ask(exes[0], shape, **kwargs), _ask(exes[1], shape, **kwargs)
            assert a["status"] == b["status"] and a["layers"] == b["layers"] or np.isnan(a["layers"][0]["sigma"])
            assert all(a["weights"][k].tobytes() == b["weights"][k].tobytes() for k in a["weights"])

"""opencorr_amd/csrc/host/sift2d_plan.h -- the octave count, layer table, sigmas, blur radii and weights, the extrema threshold and
every refusal of SIFT2D's detector -- against the float64 model's plan (tests/sift2d_model.py, written independently from the
contract of DESIGN.md section 4.13).  CPU only: tests/cpp/sift2d_plan_check.cpp is a stand-alone program over the header, built
with plain g++ (-ffp-contract=off like the library) and once more with -fsanitize=undefined,address.
"""
import os
import subprocess

import numpy as np
import pytest

import sift2d_cases as cases
import sift2d_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
SHAPES = [(2, 2), (20, 24), (29, 37), (16, 16), (33, 200), (200, 33), (130, 130), (512, 512), (4096, 4096), (3, 1000), (11, 11), (12, 12)]   # (rows, cols)
SETTINGS = [dict(), dict(n_octave_layers=1, sigma=1.1), dict(n_octave_layers=2), dict(n_octave_layers=5), dict(n_octave_layers=8),
            dict(sigma=1.2), dict(sigma=0.5), dict(sigma=2.5), dict(contrast_threshold=0.09), dict(n_octave_layers=8, contrast_threshold=0.01)]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("sift2d_plan")
    built = []
    for tag, flags in (("", ("-O2",)), ("_san", ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(out / ("sift2d_plan_check" + tag))
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "opencorr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sift2d_plan_check.cpp"), "-o", exe], check=True, timeout=600)
        built.append(exe)
    return built


def _words(tokens):
    return np.array([int(v, 16) for v in tokens], dtype=np.uint32).view(np.float32)


def _ask(exe, shape, n_features=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
    args = [shape[1], shape[0], n_features, n_octave_layers, contrast_threshold, edge_threshold, sigma]
    out = subprocess.run([exe, *(repr(a) for a in args)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    plan = {"status": int(lines[0].split()[1]), "layers": [], "weights": {}, "reflect": {}, "nearest": {}}
    if plan["status"] != OK:
        return plan
    t = lines[1].split()
    plan["octaves"], plan["threshold"] = int(t[1]), int(t[5])
    for line in lines[2:]:
        t = line.split()
        if t[0] == "layer":
            plan["layers"].append(dict(dims=(int(t[3]), int(t[4])), octave=int(t[6]), index=int(t[8]), sigma=_words([t[10]])[0], source=int(t[12]),
                                       blurred=int(t[14]), radius=int(t[16])))
        elif t[0] == "w":
            plan["weights"][int(t[1])] = _words(t[2:])
        elif t[0] == "reflect":
            plan["reflect"][int(t[1])] = [int(v) for v in t[2:]]
        elif t[0] == "nearest":
            plan["nearest"][int(t[1])] = [int(v) for v in t[3:]]
        elif t[0] == "pow2":
            w = _words(t[1:])
            plan["pow2"] = (w[0::2], w[1::2])
    return plan


@pytest.mark.parametrize("settings", SETTINGS, ids=repr)
def test_plan_equals_model(exes, settings):
    for shape in SHAPES:
        for exe in exes[:1] if shape[0] > 600 else exes:
            got = _ask(exe, shape, **settings)
            n = settings.get("n_octave_layers", 3)
            n_octave, dims, sig, base, threshold = model.plan(shape[1], shape[0], n, settings.get("sigma", 1.6), settings.get("contrast_threshold", 0.04))
            assert got["status"] == OK and got["octaves"] == n_octave and got["threshold"] == threshold, (shape, settings)
            assert len(got["layers"]) == n_octave * (n + 3)
            for i, g in enumerate(got["layers"]):
                o, k = divmod(i, n + 3)
                assert g["dims"] == dims[o] and g["octave"] == o and g["index"] == k, (shape, i)
                if k == 0 and o > 0:
                    assert g["blurred"] == 0 and g["source"] == (o - 1) * (n + 3) + n and g["radius"] == 0 and i not in got["weights"]
                    continue
                want_sigma = base if i == 0 else sig[k]
                assert g["blurred"] == 1 and g["source"] == i - 1, (shape, i)
                assert g["sigma"].view(np.uint32) == np.float32(want_sigma).view(np.uint32), (shape, i)
                assert g["radius"] == model.radius_of(want_sigma), (shape, i)
                w = got["weights"][i]
                assert np.array_equal(w.view(np.uint32), model.weights_of(want_sigma, g["radius"]).view(np.uint32)), (shape, i)
                assert abs(float(w[0]) + 2 * float(w[1:].astype(np.float64).sum()) - 1) < (g["radius"] + 1) * 2.0 ** -24


def test_index_maps_and_pow2(exes):
    for exe in exes:
        got = _ask(exe, (16, 16))
        i = np.arange(-30, 31)
        for n in (1, 2, 8):
            assert got["reflect"][n] == model.reflect101(i, n).tolist(), n
        assert got["reflect"][8][30 - 1] == 1 and got["reflect"][8][30 + 8] == 6 and got["reflect"][8][30 + 14] == 0 and got["reflect"][8][30 + 15] == 1
        for src in (37, 74, 9):
            want = np.minimum(np.floor(np.arange(src // 2) * (src / (src // 2))).astype(int), src - 1).tolist()
            assert got["nearest"][src] == want
        # 2^t of the keypoint size: the correctly rounded float32 of the exact value
        t, p = got["pow2"]
        assert len(t) == 4001 and np.array_equal(p.view(np.uint32), np.exp2(t.astype(np.float64)).astype(np.float32).view(np.uint32))


def test_nearest_rule_on_halved_sides(exes):
    """floor(x * src / dst) with dst = src / 2 by integer division is 2 x + floor(x * (src % 2) / dst) = 2 x for every x < dst: on odd
    sides too the rule picks every second pixel and never the last one.  The rule is kept as the contract states it."""
    got = _ask(exes[0], (16, 16))
    for src in (37, 74, 9):
        assert got["nearest"][src] == [2 * x for x in range(src // 2)]


@pytest.mark.parametrize("settings,status", cases.REFUSED_SETTINGS, ids=lambda v: repr(v))
def test_refused_settings(exes, settings, status):
    for exe in exes:
        assert _ask(exe, (20, 20), **settings)["status"] == status


@pytest.mark.parametrize("shape,status", cases.REFUSED_SHAPES + [((0, 40), cases.INVALID), ((-3, 40), cases.INVALID)], ids=lambda v: repr(v))
def test_refused_shapes(exes, shape, status):
    for exe in exes:
        assert _ask(exe, shape)["status"] == status
    assert _ask(exes[0], (23170, 23170))["status"] == OK   # 4 * 23170^2 = 2 147 395 600 <= 2^31 - 1

"""Which kernel serves an FFTCC window, on the CPU (no GPU): opencorr_amd/csrc/host/fftcc_plan.h -- the kernel, the sizes of the
rocFFT pipeline, the plane-wise kernel's workgroups and scratch -- against tests/fftcc_plan_model.py, an independent restatement
as ranges and arithmetic, over every radius pair / triple around the kernels' ranges.  The header needs nothing but the standard
library; tests/cpp/fftcc_plan_check.cpp is a stand-alone program, built here with plain g++ -- once as it is and once with
-fsanitize=undefined,address.
"""
import collections
import itertools
import os
import subprocess

import pytest

import fftcc_plan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
KEYS_2D = (0, 1, 2, 3, 4, 5)
KEYS_3D = (0, 1, 2)


def _build(out_dir, flags, tag):
    exe = str(out_dir / ("fftcc_plan_check" + tag))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "fftcc_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("fftcc_plan")
    return {"plain": _build(d, ("-O2",), ""), "sanitized": _build(d, SANITIZE, "_san")}


def _run(exe, args=(), text=""):
    out = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


def _both(check, rows, fmt, want):
    """Both binaries on `rows`; each printed line against the model's.  Returns the lines."""
    text = "".join(fmt % r + "\n" for r in rows)
    got = _run(check["plain"], text=text)
    assert len(got) == len(rows)
    assert _run(check["sanitized"], text=text) == got
    bad = [(r, g, want(*r)) for r, g in zip(rows, got) if g != want(*r)]
    assert not bad, "%d of %d rows differ (request, header, model), first: %s" % (len(bad), len(rows), bad[:5])
    return got


@pytest.fixture(scope="module")
def rows2d(check):
    rows = list(itertools.product(range(41), range(41), KEYS_2D))
    return dict(zip(rows, (g.split()[0] for g in _both(check, rows, "2 %d %d %d", model.plan2d))))


@pytest.fixture(scope="module")
def rows3d(check):
    rows = list(itertools.product(range(35), range(35), range(35), KEYS_3D, (0, 1)))
    return dict(zip(rows, (g.split()[0] for g in _both(check, rows, "3 %d %d %d %d %d", model.plan3d))))


def test_every_2d_window_gets_the_models_kernel(rows2d):
    assert len(rows2d) == 41 * 41 * 6
    assert set(rows2d.values()) == {"fused32", "smooth", "prime", "pair", "rect", "rocfft"}
    # today's partition at "fftcc2d_fused" = 1: 29 square sides (one of them 32 x 32), 7 * 6 pairs, the other 29 * 28 - 42 rectangles
    count = collections.Counter(k for (rx, ry, key), k in rows2d.items() if key == 1)
    assert count == {"fused32": 1, "smooth": 15, "prime": 13, "pair": 42, "rect": 29 * 28 - 42, "rocfft": 41 * 41 - 29 * 29}
    assert count["rect"] == 770
    # the bodies of the 32 x 32 kernel (3, 4, 5) choose like 1; 2 moves 32 x 32 alone; 0 is the pipeline everywhere
    for (rx, ry, key), k in rows2d.items():
        assert k == ("rocfft" if key == 0 else "smooth" if key == 2 and rx == ry == 16 else rows2d[rx, ry, 1]), (rx, ry, key)


def test_every_3d_window_gets_the_models_kernel(rows3d):
    assert len(rows3d) == 35 ** 3 * 3 * 2
    assert set(rows3d.values()) == {"fused32", "fused32_r5", "cube", "planes", "box", "rocfft"}
    for ab in (0, 1):
        count = collections.Counter(k for (rx, ry, rz, key, build), k in rows3d.items() if key == 1 and build == ab)
        assert count == {"cube": 10, "fused32": 1, "planes": 18, "box": 2078, "rocfft": 35 ** 3 - 10 - 1 - 18 - 2078}
    assert sum(1 for r in itertools.product(range(4, 17), repeat=3) if len(set(r)) > 1) == 2184   # the non-cubic triples 2 078 are out of
    for (rx, ry, rz, key, ab), k in rows3d.items():
        r5 = key == 2 and ab == 1 and rx == ry == rz == 16
        assert k == ("rocfft" if key == 0 else "fused32_r5" if r5 else rows3d[rx, ry, rz, 1, 0]), (rx, ry, rz, key, ab)


def test_pinned_boundaries(rows2d, rows3d):
    # the box kernel's LDS rule: 32 x 32 x 19 and 18 x 32 x 33 complex values fit, 32 x 32 x 21, 20 x 32 x 33 and 26 x 28 x 31 do not
    assert rows3d[16, 16, 9, 1, 0] == "box" and rows3d[9, 16, 16, 1, 0] == "box"
    assert rows3d[16, 16, 10, 1, 0] == "rocfft" and rows3d[10, 16, 16, 1, 0] == "rocfft" and rows3d[13, 14, 15, 1, 0] == "rocfft"
    assert max(model.box_lds_bytes(16, 16, 9), model.box_lds_bytes(9, 16, 16)) <= model.LDS_LIMIT < min(model.box_lds_bytes(10, 16, 16), model.box_lds_bytes(16, 16, 10))
    assert rows2d[33, 33, 1] == "rocfft" and rows2d[3, 3, 1] == "rocfft" and rows2d[4, 32, 1] == "rect" and rows2d[8, 32, 1] == "pair"
    assert rows2d[16, 16, 2] == "smooth"
    assert rows3d[16, 16, 16, 2, 1] == "fused32_r5" and rows3d[16, 16, 16, 2, 0] == "fused32"


def test_pinned_plans_of_the_bench_configs(rows2d, rows3d):
    assert rows2d[16, 16, 1] == "fused32" and rows2d[20, 20, 1] == "smooth"
    assert rows3d[16, 16, 16, 1, 0] == "fused32" and rows3d[30, 30, 30, 1, 0] == "planes"


def test_pinned_sizes(check):
    rows = [(0, 1, 30), (0, 10 ** 6, 30), (100, 10 ** 6, 30), (0, 9, 14), (7, 10 ** 6, 32), (-3, 255, 17), (4096, 1 << 33, 32)]
    got = _both(check, rows, "p %d %d %d", model.planes)
    assert [int(g.split()[0]) for g in got[:3]] == [8, 256, 104]
    assert got[1] == "256 442368000"
    # the rocFFT pipeline at 2D r = 33, the smallest square window beyond every single-kernel path: 66 x 66 floats, 66 x 34 bins
    assert _both(check, [(33, 33, 1)], "2 %d %d %d", model.plan2d) == ["rocfft 64 4356 2244"]
    assert _run(check["sanitized"], args=("constants",)) == ["%d %d %d 32 32" % (model.ROCFFT_CHUNK_2D, model.ROCFFT_CHUNK_3D, model.MAX_LAUNCH)]
    assert (model.ROCFFT_CHUNK_2D, model.ROCFFT_CHUNK_3D, model.MAX_LAUNCH) == (32768, 1024, 2 ** 30)

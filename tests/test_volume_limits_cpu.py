"""Which volumes ICGN3D1 takes, on the CPU (no GPU): opencorr_amd/csrc/host/volume_limits.h against the exact-integer restatement in
tests/large_volume_cases.py (whose walk model derives the rule: tests/test_oracle_large_volume_cases.py).  The header needs nothing
but the language; tests/cpp/volume_limits_check.cpp is a stand-alone program, built here with plain g++ -- once as it is and once
with -fsanitize=undefined,address.
"""
import itertools
import os
import subprocess

import pytest

import large_volume_cases as lv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
INT_MAX = (1 << 31) - 1
SATURATED = (1 << 64) - 1

RADII = [(0, 0, 0), (1, 1, 1), (3, 3, 4), (3, 3, 7), (3, 3, 30), (5, 7, 6), (8, 8, 8), (16, 16, 16), (30, 30, 30), (1, 1, 4), (16, 16, 3), (4096, 4096, 4096),
         (INT_MAX, INT_MAX, INT_MAX), (-1, 2, 3)]
# (dy, dx): the shapes of tests/large_volume_cases.py and their neighbours, powers of two on both sides of every product, the extremes
PLANES = [lv.INDEX31[1:], lv.SLAB[1:], lv.REFUSED[1:], (lv.REFUSED[1] - 1, lv.REFUSED[2]), (512, 512), (1, 1), (65536, 32768), (65536, 32767),
          (46341, 46341), (46340, 46340), (1 << 16, 1 << 16), (1 << 20, 1 << 11), (1 << 30, (1 << 31) - 3), (INT_MAX, INT_MAX), (0, 0), (-5, 7)]


def _model(rx, ry, rz, dy, dx):
    """the header's answer from exact integers: negative arguments count as 0, anything beyond 64 bits saturates"""
    span = lv.box_span(*(max(v, 0) for v in (rx, ry, rz, dy, dx)))
    return min(span, SATURATED), int(span <= lv.MAX_SPAN)


def _build(out_dir, flags, tag):
    exe = str(out_dir / ("volume_limits_check" + tag))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "volume_limits_check.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("volume_limits")
    return {"plain": _build(d, ("-O2",), ""), "sanitized": _build(d, SANITIZE, "_san")}


def _run(exe, args=(), text=""):
    out = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


def test_every_request_gets_the_models_answer(check):
    rows = [r + p for r, p in itertools.product(RADII, PLANES)]
    text = "".join("%d %d %d %d %d\n" % r for r in rows)
    got = _run(check["plain"], text=text)
    assert len(got) == len(rows) and _run(check["sanitized"], text=text) == got
    bad = [(r, g, _model(*r)) for r, g in zip(rows, got) if tuple(int(v) for v in g.split()) != _model(*r)]
    assert not bad, "%d of %d rows differ (rx ry rz dy dx, header, model), first: %s" % (len(bad), len(rows), bad[:5])
    assert {g.split()[1] for g in got} == {"0", "1"} and any(int(g.split()[0]) == SATURATED for g in got)
    assert _run(check["sanitized"], args=("limit",)) == [str(lv.MAX_SPAN)]


def test_pinned_answers(check):
    def ask(*row):
        (line,) = _run(check["plain"], text="%d %d %d %d %d\n" % row)
        return tuple(int(v) for v in line.split())

    assert ask(*lv.R_SLAB, *lv.SLAB[1:]) == (2148531270, 1)                              # between 2^31 and 2^32: served
    assert all(ask(*r, *lv.INDEX31[1:])[1] == 1 for r in lv.RADII["INDEX31"])
    assert ask(*lv.R_REFUSED, *lv.REFUSED[1:]) == (4295203440, 0)
    assert ask(*lv.R_REFUSED, lv.REFUSED[1] - 1, lv.REFUSED[2]) == (4294958202, 1)       # one row per plane less
    assert ask(16, 16, 6, *lv.REFUSED[1:])[1] == 1                                       # the same volume, a flatter subset
    assert ask(0, 0, 1, 65536, 32768) == (1 << 32, 0) and ask(0, 0, 1, 65536, 32767) == ((1 << 32) - 131072, 1)
    assert ask(16, 16, 16, 512, 512)[1] == 1 and ask(30, 30, 30, 1300, 1300)[1] == 1     # what DVC runs today

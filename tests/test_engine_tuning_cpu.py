"""The tuning keys of oc_hip_set_tuning, on the CPU (no GPU): opencorr_amd/csrc/host/engine_tuning.h -- one table of keys, fields,
rules, engine kinds and A/B-only values -- against tests/engine_tuning_model.py, an independent restatement key by key, for every
engine kind, every key, both builds of the library and the values around every bound.  The header needs nothing but the standard
library; tests/cpp/engine_tuning_check.cpp is a stand-alone program, built here with plain g++ -- once as it is and once with
-fsanitize=undefined,address.
"""
import itertools
import os
import subprocess

import pytest

import engine_tuning_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
VALUES = (-2, -1, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 63, 64, 65, 256, 257, 4096, 4097, 16383, 16384, 65536, 2 ** 31 - 1)
KEYS = model.KEYS + ("xcd", "no_such_key", "")
EXTRA = [(model.FFTCC2D, "fftcc2d_fused", 4, 0), (model.FFTCC2D, "fftcc2d_fused", 4, 1)]   # (4 is a value of this key alone)
DEFAULTS = ("variant=-1 xcd=1 tile_px=128 setup_cache=1 int_first=1 split_chunks=0 arith_fma=0 arith_onepass=0 arith_onepass3d=0 fftcc2d_fused=1 "
            "fftcc3d_fused=1 planes_blocks=0 fftcc3d_tile_vox=64 icgn3d_tile_vox=64 mapping=0 match_splits=0 single_combine=1 host_chunk=65536 "
            "group_allgather=0 group_force_rccl=0 self_adaptive=0 lm=100,0.1,10")


def _build(out_dir, flags, tag):
    exe = str(out_dir / ("engine_tuning_check" + tag))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "engine_tuning_check.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("engine_tuning")
    return {"plain": _build(d, ("-O2",), ""), "sanitized": _build(d, SANITIZE, "_san")}


def _run(exe, args=(), text=""):
    out = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def rows(check):
    """request (kind, key, value, ab_build) -> the line both binaries print for it"""
    requests = list(itertools.product(model.KINDS, KEYS, VALUES, (0, 1))) + EXTRA
    text = "".join("%d %s %d %d\n" % r for r in requests)
    got = _run(check["plain"], text=text)
    assert len(got) == len(requests)
    assert _run(check["sanitized"], text=text) == got
    return dict(zip(requests, got))


def test_every_row_equals_the_model(rows):
    assert len(rows) == 13 * (len(model.KEYS) + 3) * 27 * 2 + len(EXTRA) and len(model.KEYS) == 20
    bad = [(r, g, model.line(*r)) for r, g in rows.items() if g != model.line(*r)]
    assert not bad, "%d of %d rows differ (request, header, model), first: %s" % (len(bad), len(rows), bad[:5])
    assert {g.split()[1] for g in rows.values()} == {"none", "unknown_key", "wrong_kind", "onepass_of_3d", "ab_only", "out_of_range"}


def test_the_table_has_the_models_keys(check):
    assert sorted(_run(check["sanitized"], args=("keys",))) == sorted(model.KEYS)


def test_pinned_defaults(check):
    assert _run(check["plain"], args=("defaults",)) == [DEFAULTS] == _run(check["sanitized"], args=("defaults",))
    assert model.format_settings(dict(model.DEFAULTS)) == DEFAULTS


def test_a_refused_row_changes_nothing(rows):
    refused = [g for g in rows.values() if not g.startswith("0 none ")]
    assert len(refused) > 5000
    assert all(g.split(" ", 2)[2] == DEFAULTS for g in refused)
    assert all(g.split()[0] in ("1", "5") for g in refused)


def _status(rows, kind, key, value, ab):
    g = rows[kind, key, value, ab].split()
    return int(g[0]), g[1]


def _field(rows, request, name):
    return dict(f.split("=") for f in rows[request].split()[2:])[name]


def test_pinned_product_build_refusals(rows):
    for kind in model.KINDS:
        for variant in (0, 6, 8, 9):
            assert _status(rows, kind, "icgn2d_variant", variant, 0) == (model.ERR_UNSUPPORTED, "ab_only")
            assert _status(rows, kind, "icgn2d_variant", variant, 1) == (model.OK, "none")
        for variant in (-1, 1, 2, 3, 5, 7, 10, 11):
            assert _status(rows, kind, "icgn2d_variant", variant, 0) == (model.OK, "none")
        for key, value in (("icgn3d_mapping", 1), ("fftcc3d_fused", 2), ("icgn2d_split_chunks", 1)):
            assert _status(rows, kind, key, value, 0) == (model.ERR_UNSUPPORTED, "ab_only")
            assert _status(rows, kind, key, value, 1) == (model.OK, "none")
        # the product build refuses icgn2d_split_chunks before it looks at the range; the A/B build finds the range
        assert _status(rows, kind, "icgn2d_split_chunks", 257, 0) == (model.ERR_UNSUPPORTED, "ab_only")
        assert _status(rows, kind, "icgn2d_split_chunks", 257, 1) == (model.ERR_INVALID, "out_of_range")
        assert _status(rows, kind, "icgn2d_split_chunks", -1, 0) == (model.ERR_UNSUPPORTED, "ab_only")
        assert _status(rows, kind, "icgn2d_variant", 12, 0) == (model.ERR_INVALID, "out_of_range") == _status(rows, kind, "icgn2d_variant", -2, 1)


def test_pinned_normalisations(rows):
    for ab in (0, 1):
        assert [_field(rows, (model.FFTCC2D, "fftcc2d_fused", v, ab), "fftcc2d_fused") for v in (-1, 0, 1, 2, 3, 4, 5, 6)] == list("10123451")
        assert [_field(rows, (model.FFTCC3D, "fftcc3d_fused", v, ab), "fftcc3d_fused") for v in (-1, 0, 1, 3)] == list("1011")
        assert _field(rows, (model.ICGN2D1, "xcd", 7, ab), "xcd") == "1" and _field(rows, (model.ICGN2D1, "xcd", 0, ab), "xcd") == "0"
        assert _field(rows, (model.ICGN2D1, "host_chunk", 16384, ab), "host_chunk") == "16384"
        assert _status(rows, model.ICGN2D1, "host_chunk", 16383, ab) == (model.ERR_INVALID, "out_of_range")
        assert _status(rows, model.ICGN2D1, "icgn2d_tile_px", 15, ab) == (model.ERR_INVALID, "out_of_range")
        assert _field(rows, (model.ICGN2D1, "icgn2d_tile_px", 16, ab), "tile_px") == "16"
    assert _field(rows, (model.FFTCC3D, "fftcc3d_fused", 2, 1), "fftcc3d_fused") == "2"


def test_pinned_engine_kinds(rows):
    for ab in (0, 1):
        assert _status(rows, model.ICGN3D1, "arith_onepass", 1, ab) == (model.ERR_UNSUPPORTED, "onepass_of_3d")
        assert _status(rows, model.ICGN3D1, "arith_onepass3d", 1, ab) == (model.OK, "none")
        assert _status(rows, model.ICGN2D1, "arith_onepass3d", 1, ab) == (model.ERR_UNSUPPORTED, "wrong_kind")
        assert _status(rows, model.ICLM2D1, "arith_onepass", 1, ab) == (model.ERR_UNSUPPORTED, "wrong_kind")
        for kind in model.KINDS:
            # a key another engine kind owns is accepted with 0 on every kind; match_splits belongs to the matcher whatever the value
            for key in ("arith_fma", "arith_onepass", "arith_onepass3d"):
                assert _status(rows, kind, key, 0, ab) == (model.OK, "none")
            want = (model.OK, "none") if kind == model.MATCHER else (model.ERR_UNSUPPORTED, "wrong_kind")
            assert _status(rows, kind, "match_splits", 0, ab) == want == _status(rows, kind, "match_splits", 64, ab)
            assert _status(rows, kind, "match_splits", 65, ab) == ((model.ERR_INVALID, "out_of_range") if kind == model.MATCHER else want)
            fused = kind in (model.ICGN2D1, model.ICGN2D2, model.ICLM2D1, model.ICLM2D2, model.ICGN3D1, model.MATCHER)
            assert _status(rows, kind, "arith_fma", 1, ab) == ((model.OK, "none") if fused else (model.ERR_UNSUPPORTED, "wrong_kind"))
            assert _status(rows, kind, "no_such_key", 0, ab) == (model.ERR_INVALID, "unknown_key") == _status(rows, kind, "", 1, ab)

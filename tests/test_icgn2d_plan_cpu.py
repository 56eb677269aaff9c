"""What run_icgn2d decides before it enqueues anything, on the CPU (no GPU): opencorr_amd/csrc/host/icgn2d_plan.h -- the variant, the
launch path, the use of the set-up cache, or the refusal -- against tests/icgn2d_plan_model.py, an independent restatement of the
rules, over the full cross product of what a call can bring.  The header needs nothing but the standard library;
tests/cpp/icgn2d_plan_check.cpp is a stand-alone program, built here with plain g++ -- once as it is and once with
-fsanitize=undefined,address.
"""
import itertools
import os
import subprocess

import pytest

import icgn2d_plan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")

# radii on both sides of every boundary (budget 161 792 B; passes of 64 samples)
RADII = [
    (17, 16), (17, 17),      # 19 | 20 passes: the ICGN2D1 table variant and six compact workgroups
    (20, 21), (21, 21),      # 28 | 29 passes: the ICGN2D2 table variant and four compact workgroups
    (127, 1), (1, 150), (128, 1),   # 255 columns | 301 rows, 257 columns: the compact table's 8-bit indices
    (14, 28), (20, 20),      # 26 | 27 passes: self-adaptive, three workgroups of variant 2 fit | do not
    (30, 29), (30, 30),      # 3 599 | 3 721 samples around the 3 648 of variants 4 and 5
    (35, 35), (35, 36),      # 5 041 | 5 183 samples around variant 2's 5 056
    (50, 49), (50, 50),      # 9 999 | 10 201 samples around the 10 112 of variants 0 and 7
    (57, 57), (58, 57),      # 13 225 | 13 455 samples around the one-pass kernel's 13 440
    (71, 70), (71, 71),      # 20 163 | 20 449 samples around variant 1's 20 224
    (0, 0), (16, 16), (4096, 4096),
]
COUNTS = [1, 16383, 16384, 32767, 32768, 1 << 30, (1 << 30) + 1]
VARIANTS = list(range(-1, 12))


def _requests():
    flag = (0, 1)
    # model.REQUEST_FIELDS order: dof lm onepass self_adaptive offsets variant (rx ry) count setup_cache split_chunks ab_build band_supported
    for dof, lm, onepass, sa, offsets, variant, (rx, ry), count, cache, split, ab, band in itertools.product(
            (6, 12), flag, flag, flag, flag, VARIANTS, RADII, COUNTS, flag, (0, 2), flag, flag):
        yield (dof, lm, onepass, sa, offsets, variant, rx, ry, count, cache, split, ab, band)


def _build(out_dir, flags, tag):
    exe = str(out_dir / ("icgn2d_plan_check" + tag))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "icgn2d_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("icgn2d_plan")
    return {"plain": _build(d, ("-O2",), ""), "sanitized": _build(d, SANITIZE, "_san")}


def _run(exe, args=(), text=""):
    out = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


def _plan(check, **kw):
    q = dict(dof=6, lm=0, onepass=0, self_adaptive=0, offsets=0, variant=-1, rx=16, ry=16, count=250000, setup_cache=1, split_chunks=0,
             ab_build=0, band_supported=0)
    q.update(kw)
    row = tuple(q[f] for f in model.REQUEST_FIELDS)
    got = _run(check["plain"], text=" ".join(str(v) for v in row) + "\n")
    assert got == [model.plan(*row)]
    return got[0]


def test_boundary_radii_sit_where_the_comments_say():
    assert [model.passes(*r) for r in RADII[:4]] == [19, 20, 28, 29] and [model.passes(*r) for r in RADII[7:9]] == [26, 27]
    samples = [(2 * rx + 1) * (2 * ry + 1) for rx, ry in RADII]
    assert samples[9:19] == [3599, 3721, 5041, 5183, 9999, 10201, 13225, 13455, 20163, 20449]
    assert [model.max_samples(v) for v in (5, 2, 7, 1)] == [3648, 5056, 10112, 20224] and model.onepass_max_samples() == 13440
    budget = 160 * 1024 - 2048
    assert 3 * 2048 * 26 <= budget < 3 * 2048 * 27 and 3 * 2816 * 19 <= budget < 3 * 2816 * 20 and 2 * 2816 * 28 <= budget < 2 * 2816 * 29


def test_every_request_gets_the_models_plan(check):
    rows = list(_requests())
    assert len(rows) == 2 ** 9 * len(VARIANTS) * len(RADII) * len(COUNTS)
    text = "".join("%d %d %d %d %d %d %d %d %d %d %d %d %d\n" % r for r in rows)
    got = _run(check["plain"], text=text)
    assert len(got) == len(rows)
    assert _run(check["sanitized"], text=text) == got
    bad = [(r, g, model.plan(*r)) for r, g in zip(rows, got) if g != model.plan(*r)]
    assert not bad, "%d of %d rows differ (request %s, header, model), first: %s" % (len(bad), len(rows), model.REQUEST_FIELDS, bad[:5])
    # every outcome occurs
    kinds = {" ".join(g.split()[:2]) if g.startswith("refuse") else g.split()[2] for g in got}
    assert kinds == {"plain", "onepass", "lm", "band", "split_pipelined", "refuse onepass_offsets", "refuse onepass_self_adaptive",
                     "refuse onepass_too_large", "refuse too_large"}
    assert {int(g.split()[1]) for g in got if g.startswith("run")} == {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}


def test_pinned_plans(check):
    # bench.py's config B and config C: 250 000 POIs, r = 16, everything default
    assert _plan(check, dof=6) == "run 10 plain 1 0"
    assert _plan(check, dof=12) == "run 11 plain 1 0"
    # config A's 10 000 POIs: the small-queue variants, around the cache
    assert _plan(check, dof=6, count=10000) == "run 2 plain 0 0"
    assert _plan(check, dof=12, count=10000) == "run 3 plain 0 0"
    assert _plan(check, dof=6, lm=1) == "run 1 lm 0 0" and _plan(check, dof=12, lm=1, variant=10) == "run 1 lm 0 0"
    assert _plan(check, onepass=1, offsets=1) == "refuse onepass_offsets 0"
    assert _plan(check, onepass=1, self_adaptive=1) == "refuse onepass_self_adaptive 0"
    assert _plan(check, onepass=1, rx=58, ry=57) == "refuse onepass_too_large 13440"
    assert _plan(check, onepass=1, dof=12) == "run 4 onepass 0 0"
    # beyond 19 / 28 passes and beyond 8-bit indices the float-table variants and then the table-less ones take over
    assert _plan(check, rx=17, ry=17) == "run 2 plain 0 0" and _plan(check, dof=12, rx=20, ry=21) == "run 11 plain 1 0"
    assert _plan(check, dof=12, rx=21, ry=21) == "run 3 plain 0 0" and _plan(check, rx=1, ry=150) == "run 5 plain 1 0"
    assert _plan(check, variant=10, rx=17, ry=17, count=100) == "run 2 plain 0 0" and _plan(check, variant=10, count=100) == "run 10 plain 1 0"
    assert _plan(check, self_adaptive=1, rx=14, ry=28) == "run 2 plain 0 0" and _plan(check, self_adaptive=1, rx=20, ry=20) == "run 7 plain 0 0"
    assert _plan(check, rx=35, ry=36, count=100) == "run 1 plain 0 0" and _plan(check, rx=71, ry=71) == "refuse too_large 20224"
    assert _plan(check, offsets=1) == "run 10 plain 0 0" and _plan(check, setup_cache=0) == "run 10 plain 0 0"
    assert _plan(check, count=(1 << 30) + 1) == "run 10 plain 0 0"
    # the A/B partners: the band kernel where it has an instantiation, the split shape's pipeline from two chunks and 16 384 POIs on
    assert _plan(check, variant=9, ab_build=1, band_supported=1) == "run 9 band 0 0" and _plan(check, variant=9, ab_build=1) == "run 2 plain 0 0"
    assert _plan(check, variant=8, ab_build=1, split_chunks=2) == "run 8 split_pipelined 0 1"
    assert _plan(check, variant=8, ab_build=1, split_chunks=2, count=16383) == "run 8 plain 0 1"


def test_variant_table_and_limits(check):
    """The shape table's derived answers: which build contains an id, whether it shares a coordinate table, what it holds."""
    got = _run(check["sanitized"], args=("limits",))
    assert got[-1] == "onepass %d" % model.onepass_max_samples()
    table = [tuple(int(v) for v in ln.split()) for ln in got[:-1]]
    assert table == [(v, int(v not in model.AB_ONLY), 1, int(v in model.TABLE_VARIANTS), model.max_samples(v)) for v in range(12)]

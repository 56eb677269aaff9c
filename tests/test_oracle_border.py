"""The ladders of tests/border_cases.py on the oracle alone (CPU, runs everywhere): no ladder passes emptily.

tests/test_gpu_border.py compares the kernels with the oracle bit for bit on these queues; that says something about the range
rule only if the queues hold both outcomes next to each other.  Asserted here, per ladder, for ICGN2D1 / ICGN2D2 / ICGN3D1 in the
order the kernels are compared with: at least 2 abandoned rungs and at least 2 iterated ones; on the inward ladders at least half
of the in-range rungs end with ZNCC > 0.9; the walk-out ladders hold at least 2 records that are abandoned although their first
sample set is in range.  "Iterated" is read from the record where the record can show it (iteration >= 1).  An abandon writes
nothing but ZNCC = -3 (src/oc_icgn.cpp:251-255), so a rung that walks out in its second iteration looks like one that never
started: for the walk-out ladders, and as the exact form of the condition for every ladder, the same queue is solved with stop = 1,
where an in-range rung ends its one iteration with iteration = 1 and nothing can leave later.  There the NumPy restatement of the
rule (border_cases.first_sweep / outside) must predict EVERY record: abandoned <=> first sweep outside.  The four planted slips -- `>=` relaxed to `>` at the high limit, `< 1` relaxed to `< 0`, `inside` with `x0 >= 0`, a 3D
box clipped at D - 2 -- each change records of the ladders (the counts are printed and pinned).
"""
import numpy as np
import pytest

import border_cases as bc
import oracle

Z2, I2, Z3, I3 = oracle.P2["zncc"], oracle.P2["iteration"], oracle.P3["zncc"], oracle.P3["iteration"]


@pytest.fixture(scope="module")
def solved2d():
    """{(solver, ladder name[, "once"]): records}, ORDER_LANES, at stop = 10 and ("once") at stop = 1; computed once, never written to."""
    out = {}
    for (pair, mode), (q, off, at) in bc.group(bc.ladders2d()).items():
        for solver in ("icgn2d1", "icgn2d2"):
            got = bc.oracle2d(solver, pair, q, oracle.ORDER_LANES, offsets=off, adaptive=mode in ("adaptive", "both"))
            once = bc.oracle2d(solver, pair, q, oracle.ORDER_LANES, offsets=off, adaptive=mode in ("adaptive", "both"), stop=1)
            for l, s in at:
                out[solver, l.name] = got[s]
                out[solver, l.name, "once"] = once[s]
    return out


def _solve3d(ladders):
    out = {}
    for l in ladders:
        out[l.name] = bc.oracle3d(l, l.queue, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D)
        out[l.name, "once"] = bc.oracle3d(l, l.queue, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D, stop=1)
    return out


@pytest.fixture(scope="module")
def solved3d():
    return _solve3d(bc.ladders3d())


def _check_ladder(l, got, z, it, what, once):
    """got: the ladder's records at its own stop; once: at stop = 1."""
    lo, hi = bc.first_sweep(l)
    out = bc.outside(l, lo, hi)
    # one iteration: the restatement decides every record -- outside: abandoned, untouched otherwise; inside: exactly one iteration
    assert np.array_equal(once[:, z] == -3, out), (what, "stop = 1: abandoned <=> first sweep outside", once[:, z].tolist(), out.tolist())
    assert (once[out, it] == 0).all() and (once[~out, it] == 1).all(), what
    assert (~out).sum() >= 2, (what, "at least 2 rungs complete an iteration")
    abandoned = got[:, z] == -3
    iterated = got[:, it] >= 1
    # at the ladder's own stop: out of range -> abandoned with nothing else written; in range -> an iteration was counted, or the POI
    # was abandoned in a later one
    assert abandoned[out].all() and (got[out, it] == 0).all(), (what, "first sweep outside but not abandoned")
    assert (iterated | abandoned)[~out].all(), what
    walked = abandoned & ~out
    print("%-28s rungs %2d: first sweep outside %2d, iterated %2d, walked out later %2d, ZNCC > 0.9: %2d; outcome per rung: %s"
          % (what, len(got), out.sum(), iterated.sum(), walked.sum(), (got[:, z] > 0.9).sum(),
             "".join("x" if a else ("w" if w else ".") for a, w in zip(out, walked))))
    assert out.sum() >= 2 and (~out).sum() >= 2, (what, "both outcomes")
    if l.kind == "walkout":
        assert walked.sum() >= 2, (what, "records that start inside and leave later")
    else:
        assert iterated.sum() >= 2, what
    if l.kind == "inward":
        assert (got[~out, z] > 0.9).sum() * 2 >= (~out).sum(), (what, "in-range rungs converge")
    return out


@pytest.mark.parametrize("solver", ["icgn2d1", "icgn2d2"])
def test_2d_ladders_hold_both_outcomes(solved2d, solver):
    for l in bc.ladders2d():
        _check_ladder(l, solved2d[solver, l.name], Z2, I2, "%s %s" % (solver, l.name), solved2d[solver, l.name, "once"])


def test_plain_sides_cross_where_the_spacing_of_the_limit_says(solved2d):
    """Left: x = 10 + (-10 + u) rounds in units of 9.5e-7 (the spacing at 9), u = 1 - 6 .. 1 - 5 steps of 1.2e-7 round down to the
    float below 1, 1 - 4 steps is a tie that rounds to 1: rungs 0-1 abandoned.  Right and bottom: x = 101 + (10 + u) is exact, rung 6
    (u = -1) sits ON size - 2: rungs 0-5 in range."""
    for solver in ("icgn2d1", "icgn2d2"):
        z = solved2d[solver, "left"][:, Z2]
        assert (z[:2] == -3).all() and (z[2:] > 0.9).all(), z
        assert len(set(solved2d[solver, "left"][2:, I2])) == 1       # a few 1e-7 in the guess: the same path
        top = solved2d[solver, "top"][:, Z2]
        assert (top[:4] == -3).all() and (top[4:] > 0.9).all(), top
        for side in ("right", "bottom"):
            z = solved2d[solver, side][:, Z2]
            assert (z[:6] > 0.9).all() and (z[6:] == -3).all(), (side, z)


def test_iclm_solves_out_of_range_rungs_with_the_sentinel_as_data():
    """ICLM2D1 never abandons (src/oc_iclm.cpp has no such check): the rungs ICGN abandons are iterated on -1 samples."""
    for l in bc.ladders2d():
        if l.mode != "plain" or l.name not in ("left", "right", "top", "bottom"):
            continue
        got = bc.oracle2d("iclm2d1", l.pair, l.queue, oracle.ORDER_LANES)
        out = bc.outside(l, *bc.first_sweep(l))
        assert out.sum() >= 2 and not (got[:, Z2] == -3).any() and (got[out, I2] >= 1).all(), l.name


def test_3d_ladders_hold_both_outcomes(solved3d):
    for l in bc.ladders3d():
        lo, hi = bc.first_sweep(l)
        out = _check_ladder(l, solved3d[l.name], Z3, I3, "icgn3d1 " + l.name, solved3d[l.name, "once"])
        # an in-range rung reads the first / last coefficient of the axis
        (axis, side), = l.limits[:1]
        tap = bc.uses_first_tap(l, lo, hi) if side == "low" else bc.uses_last_tap(l, lo, hi)
        assert tap.sum() >= 2 and not (tap & out).any(), l.name
    z = solved3d["low-x"][:, Z3]
    assert (z[:4] == -3).all() and (z[4:] > 0.9).all() and len(set(solved3d["low-x"][4:, I3])) == 1, z


@pytest.mark.parametrize("r", bc.LARGE_R)
def test_3d_large_radius_ladders_hold_both_outcomes(r):
    ladders = bc.ladders3d_large(r)
    got = _solve3d(ladders)
    for l in ladders:
        _check_ladder(l, got[l.name], Z3, I3, "icgn3d1 " + l.name, got[l.name, "once"])
    assert sum(len(l.queue) for l in ladders) == 26


# ---- planted slips: the rule restated in NumPy, relaxed, and the records whose first sweep it would decide otherwise -----------------
# records of all ladders (2D, 3D, the large radii) that each slip decides otherwise; DESIGN.md section 3 quotes them
SLIP_TOTALS = {"high limit > for >=": 44, "low limit < 0 for < 1": 220, "inside with x0 >= 0": 9, "3D box clipped at D - 2": 83}


def _slip_counts():
    all2d, all3d = bc.ladders2d(), bc.ladders3d() + sum((bc.ladders3d_large(r) for r in bc.LARGE_R), ())
    counts = {}
    for name, kw in (("high limit > for >=", dict(high_closed=False)), ("low limit < 0 for < 1", dict(low=0.0))):
        per = {}
        for l in all2d + all3d:
            lo, hi = bc.first_sweep(l)
            n = int((bc.outside(l, lo, hi) != bc.outside(l, lo, hi, **kw)).sum())
            if n:
                per[l.name] = n
        counts[name] = per
    per = {}
    for l in all2d:
        applies, inside = bc.integer_inside(l)
        _, slipped = bc.integer_inside(l, x_low=0)
        n = int((applies & (inside != slipped)).sum())
        if n:
            per[l.name] = n
    counts["inside with x0 >= 0"] = per
    per = {}
    for l in all3d:
        n = int(bc.uses_last_tap(l, *bc.first_sweep(l)).sum())
        if n:
            per[l.name] = n
    counts["3D box clipped at D - 2"] = per
    return counts


def test_planted_slips_change_records():
    counts = _slip_counts()
    for name, per in counts.items():
        print("%-26s %3d records in %2d ladders: %s" % (name, sum(per.values()), len(per), per))
        assert sum(per.values()) >= 1, name
        assert sum(per.values()) == SLIP_TOTALS[name], name
    hi = counts["high limit > for >="]
    # exactly the rung that sits ON size - 2: one per plain high-side ladder
    assert hi["right"] == 1 and hi["bottom"] == 1 and hi["high-x"] == 1 and hi["high-y"] == 1 and hi["high-z"] == 1
    lo = counts["low limit < 0 for < 1"]
    assert lo["left"] == 2 and lo["low-x"] == 4
    # every high-side / low-side ladder is hit by its slip, in 2D and 3D
    for l in bc.ladders2d() + bc.ladders3d() + sum((bc.ladders3d_large(r) for r in bc.LARGE_R), ()):
        if l.kind == "integer":
            continue
        side = l.limits[0][1]
        assert l.name in (lo if side == "low" else hi), (l.name, side)
        if l.dim == 3 and side == "high":
            assert counts["3D box clipped at D - 2"][l.name] >= 2, l.name
    assert counts["inside with x0 >= 0"] == {"integer": counts["inside with x0 >= 0"]["integer"]}
    assert counts["inside with x0 >= 0"]["integer"] >= 4


def test_integer_rungs_decide_the_integer_translation_sweep(solved2d):
    """x0 = 0 against x0 = 1, x0 + 2 rx = width - 3 against width - 2: the records for which `inside` holds are exactly those the
    per-sample rule keeps, so a sweep that read the value plane for any other one would solve a POI from the plane's zero border."""
    l = [l for l in bc.ladders2d() if l.kind == "integer"][0]
    applies, inside = bc.integer_inside(l)
    assert applies.all()
    out = bc.outside(l, *bc.first_sweep(l))
    assert np.array_equal(inside, ~out)
    _, slipped = bc.integer_inside(l, x_low=0)
    changed = slipped & ~inside
    for solver in ("icgn2d1", "icgn2d2"):
        assert (solved2d[solver, l.name][changed, Z2] == -3).all()
    assert inside.sum() >= 8 and out.sum() >= 8

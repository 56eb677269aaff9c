"""ICGN3D1 and ICGN2D2 pinned to a plain float64 model of the iteration (tests/icgn_model64.py), CPU only.

The oracle is bit-exact against the reference's loops over stand-in Eigen / FFTW headers, and the GPU against the oracle;
for these two solvers no result table of the reference closes that chain.  Here an independent float64 restatement of the
algorithm -- NumPy sums, LAPACK inverses -- is compared PER ITERATION: with a convergence criterion of 0 (|dp| >= 0 always
holds) and stop = k the record holds the state after exactly k iterations, k = 1 ... 5, so a wrong Hessian entry, a wrong
steepest-descent column or a wrong update -- which all still converge to nearly the same fixed point -- shows in the path.

Bars: 4 x the distance of the COMPILED REFERENCE from the model, measured per field group and k and committed in
icgn_model64.MEASURED (never taken from oracle or GPU output).  test_reference_within_measured_distances keeps them honest,
test_flawed_models_fall_outside_the_bars shows that they are tight enough to be evidence.
"""
import numpy as np
import pytest

import icgn_model64 as m64
import oracle
from oracle import ref as oref


@pytest.fixture(scope="module")
def cases():
    cs = m64.cases3d() + m64.cases2d2()
    return cs, [m64.model_runs(c) for c in cs]


def _oracle_run(order, lanes3):
    def run(case, conv, stop):
        _, r, _, _, prep, _, pois = case
        p = pois.copy()
        if len(r) == 3:
            oracle.icgn3d1(prep, r[0], r[1], r[2], conv, stop, p, order=order, lanes=lanes3)
        else:
            oracle.icgn2d2(prep, r[0], r[1], conv, stop, p, order=order, lanes=oracle.GPU_LANES_2D)
        return p
    return run


def _check(cases, run, what):
    cs, models = cases
    dist, exc = m64.measure(cs, run, models)   # (asserts flags, iteration counts and the exception's condition)
    lines, bad = m64.check_within_bars(dist, what)
    print("\n".join(lines))
    print(what, "one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)
    return dist, exc


@pytest.mark.skipif(not oref.available(), reason="reference build (oracle/_ref/liboc_ref.so) not present")
def test_reference_within_measured_distances(cases):
    """The compiled reference (its own loops, float32, over the stand-in headers) against the model: within 4 x the
    committed distances, which were measured from exactly this comparison; it used the one-iteration exception on 0 of 148
    (3D), 0 of 8 (3DE) and 0 of 328 (2D2) records."""
    dist, exc = _check(cases, m64.run_reference, "reference")
    for family, (used, n) in exc.items():
        assert (used, n) == tuple(m64.MEASURED_EXCEPTIONS[family]), (family, used, n)


@pytest.mark.parametrize("name,order,lanes3", [
    ("ORDER_SEQ", oracle.ORDER_SEQ, 256), ("ORDER_LANES", oracle.ORDER_LANES, 256),
    ("ORDER_LANES_FMA", oracle.ORDER_LANES_FMA, 256), ("GPU_ORDER_3D", oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D)])
def test_oracle_orders_within_bars(cases, name, order, lanes3):
    """oracle.icgn3d1 / oracle.icgn2d2 in every summation order the tests use (3D: also the GPU kernel's order and lane
    count) against the model: trajectory k = 1 ... 5 and the ordinary run (conv 1e-3; stop 20 in 3D, 10 in 2D)."""
    _check(cases, _oracle_run(order, lanes3), name)


def test_entry_guards_and_exit_flags_agree_with_the_oracle(cases):
    """The rules that the inside-only cases above never reach: guard rejects (flag kept / -3), leaving the volume inside
    the loop (-3, nothing else written), stop-limited (-4) -- the model's records and the oracle's agree field by field."""
    cs, _ = cases
    for case in (cs[0], cs[3]):
        _, r, _, _, prep, fields, pois = case
        ndim = len(r)
        P = m64.P3 if ndim == 3 else m64.P2
        q = pois[:6].copy()
        q[0, P["x"]] = 3.0               # subset leaves the image: -3 on entry
        q[1, P["zncc"]] = -2.0           # rejected earlier: the flag is kept
        q[2, P["u"]] = np.nan            # -3 on entry
        q[3, P["u"]] = fields.ref.shape[-1] - 30.0   # warped subset leaves the target inside the loop: -3
        q[4, P["v"]] = 1e4               # |v| >= size: -3 on entry
        want = q.copy()
        if ndim == 3:
            oracle.icgn3d1(prep, r[0], r[1], r[2], 1e-3, 2, want)
            got, _ = m64.icgn3d1(fields, r[0], r[1], r[2], 1e-3, 2, q)
        else:
            oracle.icgn2d2(prep, r[0], r[1], 1e-3, 2, want)
            got, _ = m64.icgn2d2(fields, r[0], r[1], 1e-3, 2, q)
        assert list(want[:5, P["zncc"]]) == [-3.0, -2.0, -3.0, -3.0, -3.0]
        assert np.array_equal(got[:5], want[:5].astype(np.float64), equal_nan=True)    # untouched records, flags
        assert want[5, P["zncc"]] == -4.0 and got[5, P["zncc"]] == -4.0                # two iterations do not reach 1e-3
        assert got[5, P["iteration"]] == want[5, P["iteration"]] == 2.0


@pytest.mark.parametrize("flaw", m64.FLAWS)
def test_flawed_models_fall_outside_the_bars(cases, flaw):
    """Sharpness: a model with ONE planted mistake must put the oracle's ORDER_SEQ trajectory outside the bars in at least
    one field group by k <= 2, in 3D and in 2D2 -- otherwise the bars would be too loose to be evidence."""
    cs, _ = cases
    run = _oracle_run(oracle.ORDER_SEQ, 256)
    for case in (cs[0], cs[3]):
        family, r, _, _, _, fields, pois = case
        ndim = len(r)
        if ndim == 3:
            flawed = m64.icgn3d1(fields, r[0], r[1], r[2], 0.0, [1, 2], pois, flaw=flaw)[0]
        else:
            flawed = m64.icgn2d2(fields, r[0], r[1], 0.0, [1, 2], pois, flaw=flaw)[0]
        outside = []
        for k in (1, 2):
            for g, v in m64.distances(ndim, run(case, 0.0, k), flawed[k - 1]).items():
                print("%-12s %-4s k=%d %-6s %.3e (bar %.3e)" % (flaw, family, k, g, v, m64.BARS[family][g][k - 1]))
                if v > m64.BARS[family][g][k - 1]:
                    outside.append((k, g))
        assert outside, (flaw, family)

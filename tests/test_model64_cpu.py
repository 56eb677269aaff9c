"""The iterative solvers -- ICGN3D1, ICGN2D2, ICGN2D1, ICLM2D1 / ICLM2D2, NR2D1 -- pinned to plain float64 models of their
iterations (tests/icgn_model64.py), CPU only.

The oracle is bit-exact against the reference's loops over stand-in Eigen / FFTW headers, and the GPU against the oracle;
for these solvers no result table of the reference closes that chain.  Here an independent float64 restatement of the
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


# ---------------------------------------------------------------------------------------------------------------------
# The 6-DoF solvers: ICGN2D1 (its three arithmetic contracts, centre offsets), ICLM2D1 / ICLM2D2 and NR2D1 on the first-order
# pair (icgn_model64.cases2d1 / caseslm / casesnr).  Same rules: bars = 4 x the compiled reference's distance from the model.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases6():
    cs = m64.cases6dof()
    return cs, [m64.model_runs(c) for c in cs]


def oracle_run6(order, lanes=oracle.GPU_LANES_2D):
    """run(case, conv, stop) of the oracle's five 2D solvers in one summation order (shared with tests/test_gpu_model64.py)."""
    def run(case, conv, stop):
        r, prep, pois, extra = case[1], case[4], case[6], case[7]
        p = pois.copy()
        solver = extra["solver"]
        if solver == "icgn2d1":
            oracle.icgn2d1(prep, r[0], r[1], conv, stop, p, order=order, lanes=lanes, center_offsets=extra.get("offsets"))
        elif solver in ("iclm2d1", "iclm2d2"):
            getattr(oracle, solver)(prep, r[0], r[1], conv, stop, p, damping=extra["damping"], order=order, lanes=lanes)
        else:
            oracle.nr2d1(prep, r[0], r[1], conv, stop, p, order=order, lanes=lanes)
        return p
    return run


@pytest.mark.skipif(not oref.available(), reason="reference build (oracle/_ref/liboc_ref.so) not present")
def test_reference_within_measured_distances_6dof(cases6):
    """The compiled reference against the 6-DoF models: within 4 x the committed distances, which were measured from exactly
    this comparison, with the committed number of one-iteration exceptions (1 of 300 in 2D1, none elsewhere) -- and the
    condition the cases were chosen under: at every radius pair but (7, 9) and (9, 12), at least 95 % of the grid POIs
    converge in the reference's ordinary run (measured: all of them)."""
    dist, exc = _check(cases6, m64.run_reference, "reference")
    for family, (used, n) in exc.items():
        assert (used, n) == tuple(m64.MEASURED_EXCEPTIONS[family]), (family, used, n)
    for case in cases6[0]:
        extra = case[7]
        if case[1] in ((7, 9), (9, 12)) or not extra.get("ordinary", True) or extra["queue"] == "offsets":
            continue
        got = m64.run_reference(case, m64.CONV, m64.STOP2)
        assert (got[:40, m64.P2["zncc"]] >= 0).mean() >= 0.95, (case[0], case[1], extra)    # the first 40 records are the grid


@pytest.mark.parametrize("name,order", [("ORDER_SEQ", oracle.ORDER_SEQ), ("ORDER_LANES", oracle.ORDER_LANES),
                                        ("ORDER_LANES_FMA", oracle.ORDER_LANES_FMA)])
def test_oracle_orders_within_bars_6dof(cases6, name, order):
    """oracle.icgn2d1 (also with centre offsets) / iclm2d1 / iclm2d2 / nr2d1 against the model: trajectory k = 1 ... 5 and the
    ordinary run (conv 1e-3, stop 10).  ORDER_LANES at 64 lanes IS the GPU kernels' order (oracle.GPU_ORDER_2D)."""
    assert (oracle.GPU_ORDER_2D, oracle.GPU_LANES_2D) == (oracle.ORDER_LANES, 64)
    _check(cases6, oracle_run6(order), name)


def test_onepass_twin_2d1_within_bars(cases6):
    """The 6-DoF instantiation of the one-pass contract (tests/cpp/icgn2d_onepass_twin.cpp, which the kernel equals in every
    bit) against a reference that does not share its sums: within the 2D1 bars at all three radius pairs."""
    import onepass_twin as twin
    cs, models = cases6
    keep = [i for i, c in enumerate(cs) if c[0] == "2D1"]

    def run(case, conv, stop):
        r = case[1]
        return twin.icgn2d(6, case[4], r[0], r[1], conv, stop, case[6].copy())

    _check(([cs[i] for i in keep], [models[i] for i in keep]), run, "one-pass twin")


def test_entry_guards_and_exit_flags_agree_with_the_oracle_6dof(cases6):
    """What the inside-only cases never reach, model and oracle field by field: guard rejects of ICGN2D1 / ICLM2D1 (-3, an
    earlier flag kept) and of NR2D1 (-1, a flag below -1 kept, -5 with u, v restored for a NaN guess), ICGN2D1's -3 inside the
    loop, the stop-limited -4 of all three, and NR2D1 leaving subset_radius alone."""
    cs, _ = cases6
    P = m64.P2
    for fam in ("2D1", "LM1", "NR1"):
        case = next(c for c in cs if c[0] == fam)
        r, prep, fields, pois, extra = case[1], case[4], case[5], case[6], case[7]
        q = pois[:7].copy()
        q[0, P["x"]] = 3.0               # subset leaves the image
        q[1, P["zncc"]] = -2.0           # rejected earlier: the flag is kept
        q[2, P["u"]] = np.nan
        q[2, P["u0"]], q[2, P["v0"]] = 3.0, -4.0
        q[3, P["v"]] = 1e4               # |v| >= size
        q[4, P["zncc"]] = -0.5           # NR2D1: -1
        if fam == "2D1":
            q[5, P["u"]] = fields.ref.shape[-1] - 60.0   # warped subset leaves the target inside the loop: -3, nothing else written
        want = oracle_run6(oracle.ORDER_SEQ)((fam, r, None, None, prep, fields, q, extra), 1e-3, 2)
        if fam == "2D1":
            got = m64.icgn2d1(fields, r[0], r[1], 1e-3, 2, q)[0]
            flags = [-3.0, -2.0, -3.0, -3.0, -0.5, -3.0]
        elif fam == "LM1":
            got = m64.iclm2d1(fields, r[0], r[1], 1e-3, 2, q, extra["damping"])[0]
            flags = [-3.0, -2.0, -3.0, -3.0, -0.5]
        else:
            got = m64.nr2d1(fields, r[0], r[1], 1e-3, 2, q)[0]
            flags = [-1.0, -2.0, -5.0, -1.0, -1.0]
            assert got[2, P["u"]] == 3.0 and got[2, P["v"]] == -4.0
            assert (want[:, [P["srx"], P["sry"]]] == 0).all() and (got[:, [P["srx"], P["sry"]]] == 0).all()
        assert list(want[:len(flags), P["zncc"]]) == flags, fam
        assert np.array_equal(got[:len(flags)], want[:len(flags)].astype(np.float64), equal_nan=True), fam
        assert want[6, P["zncc"]] == -4.0 and got[6, P["zncc"]] == -4.0, fam           # two iterations do not reach 1e-3
        assert got[6, P["iteration"]] == want[6, P["iteration"]] == 2.0


@pytest.mark.parametrize("flaw", m64.FLAWS)
def test_flawed_2d1_models_fall_outside_the_bars(cases6, flaw):
    """The four planted mistakes of the 3D / 2D2 models in the 2D1 model, with and without centre offsets: the oracle's
    ORDER_SEQ trajectory lies outside the bars in at least one field group by k <= 2."""
    cs, _ = cases6
    run = oracle_run6(oracle.ORDER_SEQ)
    for case in (next(c for c in cs if c[0] == "2D1"), next(c for c in cs if c[0] == "2D1O")):
        family, r, fields, pois = case[0], case[1], case[5], case[6]
        flawed = m64.icgn2d1(fields, r[0], r[1], 0.0, [1, 2], pois, offsets=case[7].get("offsets"), flaw=flaw)[0]
        outside = []
        for k in (1, 2):
            for g, v in m64.distances(21, run(case, 0.0, k), flawed[k - 1]).items():
                print("%-12s %-4s k=%d %-6s %.3e (bar %.3e)" % (flaw, family, k, g, v, m64.BARS[family][g][k - 1]))
                if not v <= m64.BARS[family][g][k - 1]:
                    outside.append((k, g))
        assert outside, (flaw, family)


def _outside(case, run, flaw):
    """What puts ``run`` outside a flawed model: the (group, k index) beyond the bars, or the message of the assertion on flags
    and iteration counts; empty when the flaw goes unnoticed."""
    try:
        dist, _ = m64.measure([case], run, [m64.model_runs(case, flaw)])
    except AssertionError as e:
        return [str(e)[:100]]
    return sorted(set((g, k) for _, g, k, _, _ in m64.check_within_bars(dist, flaw)[1]))


@pytest.mark.parametrize("family,flaw", [(f, w) for f in ("LM1", "LM2") for w in m64.LM_FLAWS] + [("NR1", w) for w in m64.NR_FLAWS])
def test_flawed_lm_and_nr_models_fall_outside_the_bars(cases6, family, flaw):
    """IC-LM (no damping at all; damping on diag(H) instead of I; alpha and beta swapped; znssd0 not replaced on accept; the
    convergence norm only from accepted increments) and NR (the Hessian kept from the first iteration; the gradient tables
    sampled at the unwarped positions; a compositional instead of an additive update): every one puts the oracle outside
    the bars, or breaks the agreement of flags and iteration counts.  IC-LM is judged on the dim pair: on 8-bit gray values
    lambda is 1e-5 ... 1e-7 of the Hessian's diagonal, and the first and third flaw pass there unnoticed."""
    cs, _ = cases6
    case = next(c for c in cs if c[0] == family and (family == "NR1" or c[7].get("dim")))
    found = _outside(case, oracle_run6(oracle.ORDER_SEQ), flaw)
    print(family, flaw, found)
    assert found, (family, flaw)
    if flaw == "lm_zero":      # the reason the dim pair exists
        bright = next(c for c in cs if c[0] == family and not c[7].get("dim") and c[1] == case[1] and c[7]["queue"] == "noisy")
        assert not _outside(bright, oracle_run6(oracle.ORDER_SEQ), flaw)

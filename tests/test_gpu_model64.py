"""The HIP ICGN3D1, ICGN2D2, ICGN2D1, ICLM2D1 / ICLM2D2 and NR2D1 engines against the float64 models of their iterations
(tests/icgn_model64.py).

Same cases, same runs and same committed bars as tests/test_model64_cpu.py: the state after exactly k = 1 ... 5 iterations
(convergence criterion 0, stop = k) and the ordinary run (1e-3; stop 20 in 3D, 10 in 2D), in both arithmetic modes.  The
bars are 4 x the compiled reference's measured distance from the model; nothing in them comes from GPU output.  The 3DE
family is config E's shape (r = 16 on the 96 x 100 x 104 pair), where the float32 sums are longest.
"""
import numpy as np
import pytest

import icgn_model64 as m64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    cs = m64.cases3d() + m64.cases2d2()
    return cs, [m64.model_runs(c) for c in cs]


def _gpu_run(fma):
    import opencorr_amd
    engines = {}

    def run(case, conv, stop):
        family, r, ref, tar, _, _, pois = case
        eng = engines.get((family, r))
        if eng is None:
            eng = opencorr_amd.ICGN3D1(r[0], r[1], r[2], conv, stop) if len(r) == 3 else opencorr_amd.ICGN2D2(r[0], r[1], conv, stop)
            eng.set_images(ref, tar)
            eng.prepare()
            eng.set_tuning("arith_fma", fma)
            engines[(family, r)] = eng
        eng.set_iteration(conv, stop)
        return eng.compute(pois.copy())
    return run


@pytest.mark.parametrize("fma", [0, 1])
def test_gpu_engines_within_bars(cases, fma):
    cs, models = cases
    what = "GPU arith_fma=%d" % fma
    dist, exc = m64.measure(cs, _gpu_run(fma), models)   # (asserts flags, iteration counts and the exception's condition)
    lines, bad = m64.check_within_bars(dist, what)
    print("\n".join(lines))
    print(what, "one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)


@pytest.mark.parametrize("fma", [0, 1])
def test_gpu_trajectory_is_the_oracles(cases, fma):
    """The k-iteration records are also the oracle's, bit for bit, in the kernels' summation order: the stop = k runs take
    the engines through exits that the ordinary parity tests (stop 10 / 20) never take."""
    import numpy as np
    import oracle
    cs, _ = cases
    run = _gpu_run(fma)
    for case in cs:
        _, r, _, _, prep, _, pois = case
        for k in (1, 2, 5):
            want = pois.copy()
            if len(r) == 3:
                oracle.icgn3d1(prep, r[0], r[1], r[2], 0.0, k, want, order=oracle.ORDER_LANES_FMA if fma else oracle.GPU_ORDER_3D,
                               lanes=oracle.GPU_LANES_3D)
            else:
                oracle.icgn2d2(prep, r[0], r[1], 0.0, k, want, order=oracle.ORDER_LANES_FMA if fma else oracle.GPU_ORDER_2D,
                               lanes=oracle.GPU_LANES_2D)
            got = run(case, 0.0, k)
            mism = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            assert mism.size == 0, (case[0], r, k, mism[:10].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# The 6-DoF solvers on the first-order pair (icgn_model64.cases2d1 / caseslm / casesnr): ICGN2D1 in its three arithmetic
# contracts, under named launch shapes, served from the set-up cache, with and without the integer-translation first sweep and
# with centre offsets; ICLM2D1 / ICLM2D2 under every damping of the cases; NR2D1.  Same bars as tests/test_model64_cpu.py.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases6():
    cs = m64.cases6dof()
    return cs, [m64.model_runs(c) for c in cs]


def _pick(cases6, keep):
    cs, models = cases6
    idx = [i for i, c in enumerate(cs) if keep(c)]
    return [cs[i] for i in idx], [models[i] for i in idx]


def _plan(case, tuning, count):
    """What the call launches, from the restated launch plan (tests/icgn2d_plan_model.py): "run <variant> <path> <cached> <records>"."""
    import icgn2d_plan_model as plan
    r, solver = case[1], case[7]["solver"]
    return plan.plan(12 if solver == "iclm2d2" else 6, int(solver.startswith("iclm")), tuning.get("arith_onepass", 0), 0,
                     int(case[7].get("offsets") is not None), tuning.get("icgn2d_variant", -1), r[0], r[1], count,
                     tuning.get("icgn2d_setup_cache", 1), 0, 0, 0)


def _gpu_run6(tuning, second_call=False):
    """run(case, conv, stop) on one engine per (family, radii, pair), re-used across runs; ``tuning`` is set once.  With
    ``second_call`` every run computes the queue twice and returns the second call's records, asserting that the set-up cache
    served it wherever the launch plan says the call is cached."""
    import opencorr_amd
    engines = {}
    kinds = dict(icgn2d1=opencorr_amd.ICGN2D1, iclm2d1=opencorr_amd.ICLM2D1, iclm2d2=opencorr_amd.ICLM2D2, nr2d1=opencorr_amd.NR2D1)

    def run(case, conv, stop):
        family, r, ref, tar, pois, extra = case[0], case[1], case[2], case[3], case[6], case[7]
        key = (family, r, bool(extra.get("dim")))
        eng = engines.get(key)
        if eng is None:
            eng = kinds[extra["solver"]](r[0], r[1], conv, stop)
            eng.set_images(ref, tar)
            eng.prepare()
            for k, v in tuning.items():
                eng.set_tuning(k, v)
            engines[key] = eng
            print("%s %s %s launches: %s" % (family, r, tuning, _plan(case, tuning, len(pois))))
        eng.set_iteration(conv, stop)
        if "damping" in extra:
            eng.set_damping(*extra["damping"])
        if extra.get("offsets") is not None:
            return eng.compute_with_offsets(pois.copy(), extra["offsets"])
        got = eng.compute(pois.copy())
        if second_call:
            got = eng.compute(pois.copy())
            cached = _plan(case, tuning, len(pois)).split()[3] == "1"
            assert eng.setup_cache_last() == ("use" if cached else "none"), (family, r, tuning, eng.setup_cache_last())
        return got
    return run


def _check6(picked, run, what):
    cs, models = picked
    assert cs
    dist, exc = m64.measure(cs, run, models)   # (asserts flags, iteration counts and the exception's condition)
    lines, bad = m64.check_within_bars(dist, what)
    print("\n".join(lines))
    print(what, "one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)


@pytest.mark.parametrize("key,value", [("arith_fma", 0), ("arith_fma", 1), ("arith_onepass", 1)])
def test_gpu_icgn2d1_contracts_within_bars(cases6, key, value):
    """ICGN2D1's three arithmetic contracts at (16, 16), (7, 9) and (36, 36) -- the last beyond what the table shapes admit, so
    whatever the plan falls back to runs (printed) -- against the 2D1 bars."""
    _check6(_pick(cases6, lambda c: c[0] == "2D1"), _gpu_run6({key: value}), "GPU ICGN2D1 %s=%d" % (key, value))


def test_gpu_icgn2d1_center_offsets_within_bars(cases6):
    """compute(poi_queue, center_offset_queue), default contract, against the 2D1O bars."""
    _check6(_pick(cases6, lambda c: c[0] == "2D1O"), _gpu_run6({}), "GPU ICGN2D1 offsets")


@pytest.mark.parametrize("variant", [2, 5, 10])
def test_gpu_icgn2d1_named_launch_shapes_and_the_setup_cache(cases6, variant):
    """Variants 2 (4-wave workgroups, no table), 5 (lockstep, coordinate table) and 10 (compact table), named: a named variant
    runs at any queue length.  Every run is computed twice on the same queue and the SECOND call is judged; for 5 and 10 it
    must have been served by the set-up cache (setup_cache_last() == "use") wherever the shape admits the radii."""
    run = _gpu_run6({"icgn2d_variant": variant}, second_call=True)
    picked = _pick(cases6, lambda c: c[0] == "2D1")
    _check6(picked, run, "GPU ICGN2D1 variant %d, 2nd call" % variant)
    if variant in (5, 10):
        assert _plan(picked[0][0], {"icgn2d_variant": variant}, 50).split()[3] == "1"     # (16, 16) IS cached: the assertion in run() bit


@pytest.mark.parametrize("int_first", [0, 1])
def test_gpu_icgn2d1_integer_translation_first_sweep(cases6, int_first):
    """The integer-guess queues (FFTCC2D output: the first sweep reads the value plane under "icgn2d_int_first" = 1), under the
    lockstep variant that carries the sweep."""
    picked = _pick(cases6, lambda c: c[0] == "2D1" and c[7]["queue"] == "pois")
    P = m64.P2
    for c in picked[0]:
        assert (c[6][:40, [P["x"], P["y"], P["u"], P["v"]]] == np.trunc(c[6][:40, [P["x"], P["y"], P["u"], P["v"]]])).all()
    _check6(picked, _gpu_run6({"icgn2d_int_first": int_first, "icgn2d_variant": 5}), "GPU ICGN2D1 int_first=%d" % int_first)
    _check6(picked, _gpu_run6({"icgn2d_int_first": int_first}), "GPU ICGN2D1 int_first=%d automatic" % int_first)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("family", ["LM1", "LM2"])
def test_gpu_iclm_within_bars(cases6, family, fma):
    """ICLM2D1 / ICLM2D2 under the default damping, (10, 0.5, 4) and -- k-iteration states only -- (1000, 0.2, 5), and on the dim
    pair, where the damping decides the third digit of a step.  Where float32 cannot order znssd and znssd0 the kernel may
    take either branch: it is compared with the model's path it followed (icgn_model64._iterate_lm)."""
    _check6(_pick(cases6, lambda c: c[0] == family), _gpu_run6({"arith_fma": fma}), "GPU %s arith_fma=%d" % (family, fma))


def test_gpu_nr2d1_within_bars(cases6):
    _check6(_pick(cases6, lambda c: c[0] == "NR1"), _gpu_run6({}), "GPU NR2D1")


@pytest.mark.parametrize("fma", [0, 1])
def test_gpu_trajectory_is_the_oracles_6dof(cases6, fma):
    """set_iteration(0, k), k = 1, 2, 5: the oracle's records bit for bit in the matching order, for ICGN2D1 (also with centre
    offsets), ICLM2D1, ICLM2D2 and NR2D1 (its one contract; not repeated under fma) -- exits that the stop-10 parity tests of
    IC-LM and NR never take."""
    import oracle
    from test_model64_cpu import oracle_run6
    cs, _ = cases6
    run = _gpu_run6({"arith_fma": fma} if fma else {})
    want_run = oracle_run6(oracle.ORDER_LANES_FMA if fma else oracle.GPU_ORDER_2D, oracle.GPU_LANES_2D)
    for case in cs:
        if fma and case[0] == "NR1":
            continue
        for k in (1, 2, 5):
            want, got = want_run(case, 0.0, k), run(case, 0.0, k)
            both_nan = np.isnan(got) & np.isnan(want)      # NaN payload bits are not part of the contract
            mism = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~both_nan)
            assert mism.size == 0, (case[0], case[1], case[7], k, mism[:10].tolist())

"""The HIP ICGN3D1 and ICGN2D2 engines against the float64 model of the iteration (tests/icgn_model64.py).

Same cases, same runs and same committed bars as tests/test_model64_cpu.py: the state after exactly k = 1 ... 5 iterations
(convergence criterion 0, stop = k) and the ordinary run (1e-3; stop 20 in 3D, 10 in 2D), in both arithmetic modes.  The
bars are 4 x the compiled reference's measured distance from the model; nothing in them comes from GPU output.  The 3DE
family is config E's shape (r = 16 on the 96 x 100 x 104 pair), where the float32 sums are longest.
"""
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

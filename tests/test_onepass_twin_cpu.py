"""The one-pass arithmetic contract of ICGN2D1 / ICGN2D2 (`oc_hip_set_tuning("arith_onepass", 1)`) on the CPU.

tests/cpp/icgn2d_onepass_twin.cpp restates the contract -- one sweep per iteration over e' = g (t - c) - r~ with 3 + DOF running
sums, the mean / norm / ZNSSD / numerator recovered from them -- and the kernel equals it bit for bit
(tests/test_gpu_arith_onepass.py).  Here the twin itself meets the distance bars the other two contracts meet: against the
reference's loop order (oracle.ORDER_SEQ), against the reference's golden OHT table, and against the float64 model of the
12-DoF iteration.  No GPU.
"""
import numpy as np
import pytest

import icgn_model64 as m64
import onepass_twin as twin
import oracle


@pytest.fixture(scope="module")
def case2d_60(speckle_small):
    from opencorr_amd import synth
    ref, tar = speckle_small
    xs, ys = synth.poi_grid_2d(ref.shape[0], ref.shape[1], 60, 60, 26)
    pois = oracle.make_pois2d(xs, ys)
    oracle.fftcc2d(ref, tar, 16, 16, pois)
    P = oracle.P2
    # the four trippers of tests/test_gpu_arith_fma.py::case2d
    extra = oracle.make_pois2d([3.0, 90.0, 90.0, 90.0], [80.0, 80.0, 80.0, 80.0])
    extra[1, P["u"]] = 200.0      # leaves the image inside the loop: -3
    extra[2, P["zncc"]] = -1.0    # rejected on entry
    extra[3, P["v"]] = np.nan
    pois = np.concatenate([extra[:2], pois, extra[2:]]).astype(np.float32)
    return pois, oracle.Prepared2D(ref, tar)


@pytest.mark.parametrize("dof", [6, 12])
def test_twin_against_the_reference_order_on_the_synthetic_pair(case2d_60, dof):
    """The four conditions the header states for `arith_fma`, for the one-pass contract: identical failure codes, >= 99.5 % identical
    iteration counts, |d u|, |d v| <= 1e-4 and |d ZNCC| <= 1e-5 against ORDER_SEQ."""
    pois, prep = case2d_60
    seq = pois.copy()
    (oracle.icgn2d1 if dof == 6 else oracle.icgn2d2)(prep, 16, 16, 0.001, 10, seq, order=oracle.ORDER_SEQ)
    got = twin.icgn2d(dof, prep, 16, 16, 0.001, 10, pois.copy())
    r = twin.vs_reference_order(got, seq)
    print("dof %d: code mismatches %d, equal iterations %.5f, max |d disp| %.3e, max |d zncc| %.3e, converged %d of %d"
          % (dof, int(r["code_mismatch"].sum()), r["iteration_agreement"], r["max_abs_d_disp"], r["max_abs_d_zncc"],
             int((got[:, 16] >= 0).sum()), len(got)))
    assert (got[[0, 1, -2, -1], 16] < 0).all()             # the trippers fail, with ORDER_SEQ's codes (next line)
    assert not r["code_mismatch"].any()
    assert r["iteration_agreement"] >= 0.995
    assert r["max_abs_d_disp"] <= 1e-4
    assert r["max_abs_d_zncc"] <= 1e-5
    assert (got[:, 16] >= 0).sum() > 0.95 * len(got)
    # records the solver does not write stay untouched, and the contract is a different arithmetic, not a renamed one
    assert np.array_equal(got[:, [0, 1, 19, 20, 21, 22]].view(np.uint32), pois[:, [0, 1, 19, 20, 21, 22]].view(np.uint32))
    fma = pois.copy()
    (oracle.icgn2d1 if dof == 6 else oracle.icgn2d2)(prep, 16, 16, 0.001, 10, fma, order=oracle.ORDER_LANES_FMA, lanes=64)
    assert not np.array_equal(got.view(np.uint32), fma.view(np.uint32))


def test_twin_on_the_golden_oht_pair(golden):
    prep = oracle.Prepared2D(golden["ref"], golden["tar"])
    tab = golden["table"]
    guesses = oracle.make_pois2d(tab[:, 0], tab[:, 1])
    oracle.fftcc2d(golden["ref"], golden["tar"], golden["rx"], golden["ry"], guesses)
    seq = guesses.copy()
    oracle.icgn2d1(prep, golden["rx"], golden["ry"], golden["conv"], golden["stop"], seq, order=oracle.ORDER_SEQ)
    got = twin.icgn2d1(prep, golden["rx"], golden["ry"], golden["conv"], golden["stop"], guesses.copy())
    twin.check_golden_oht(got, seq, guesses, golden)


def test_twin_2d2_within_the_bars_of_the_float64_model():
    """tests/icgn_model64.py, family 2D2: the state after exactly k = 1 ... 5 iterations and the ordinary run, every field group
    (ZNCC included) inside the committed bars -- 4 x the compiled reference's own distance from the model."""
    cs = m64.cases2d2()
    models = [m64.model_runs(c) for c in cs]

    def run(case, conv, stop):
        _, r, _, _, prep, _, pois = case
        return twin.icgn2d2(prep, r[0], r[1], conv, stop, pois.copy())

    dist, exc = m64.measure(cs, run, models)
    lines, bad = m64.check_within_bars(dist, "one-pass twin")
    print("\n".join(lines))
    print("one-pass twin one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)

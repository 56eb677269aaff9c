"""The one-pass arithmetic contract on the GPU (`oc_hip_set_tuning("arith_onepass", 1)`, ICGN2D1 / ICGN2D2).

An iteration is ONE sweep over e' = g (t - c) - r~ with 3 + DOF running sums and no target array; mean, norm, ZNSSD and numerator
are recovered from the sums (opencorr_amd/csrc/icgn2d_onepass.hip).  Not bit-identical to the other two
contracts: it is pinned on its own CPU restatement, tests/cpp/icgn2d_onepass_twin.cpp, which the kernel must equal in EVERY bit,
and it meets the same distance bars against the reference's order, the golden OHT table and the float64 model
(tests/test_onepass_twin_cpu.py asserts those for the twin on the CPU; here for the kernel).  The whole queues of configs B
and C: tests/test_gpu_fullsize_onepass.py.
"""
import numpy as np
import pytest

import icgn_model64 as m64
import onepass_twin as twin

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    return opencorr_amd


@pytest.fixture(scope="module")
def case2d(speckle_small):
    """The queue of tests/test_gpu_arith_fma.py::case2d: a 19 x 23 grid with FFTCC guesses and four trippers."""
    import oracle
    from opencorr_amd import synth
    ref, tar = speckle_small
    xs, ys = synth.poi_grid_2d(ref.shape[0], ref.shape[1], 19, 23, 26)
    pois = oracle.make_pois2d(xs, ys)
    oracle.fftcc2d(ref, tar, 16, 16, pois)
    P = oracle.P2
    extra = oracle.make_pois2d([3.0, 90.0, 90.0, 90.0], [80.0, 80.0, 80.0, 80.0])
    extra[1, P["u"]] = 200.0
    extra[2, P["zncc"]] = -1.0    # rejected on entry
    extra[3, P["v"]] = np.nan
    pois = np.concatenate([extra[:2], pois, extra[2:]]).astype(np.float32)
    return ref, tar, pois, oracle.Prepared2D(ref, tar)


def _engine(eng, dof, rx, ry, ref, tar, conv=0.001, stop=10):
    icgn = (eng.ICGN2D1 if dof == 6 else eng.ICGN2D2)(rx, ry, conv, stop)
    icgn.set_images(ref, tar)
    icgn.prepare()
    icgn.set_tuning("arith_onepass", 1)
    return icgn


def _assert_same_bits(got, want, what=""):
    mism = np.argwhere(_bits(got) != _bits(want))
    assert mism.size == 0, (what, len(mism), mism[:10].tolist())


# samples: 1089 = 17 passes + 1 sample, 513 = 8 passes + 1, 525, 135, 189 (63 x 3) -- an odd x odd subset is never a multiple of 64,
# the partial last pass is the rule
RADII = [(16, 16), (13, 9), (10, 12), (7, 4), (31, 1)]


@pytest.mark.parametrize("radii", RADII)
@pytest.mark.parametrize("dof", [6, 12])
def test_gpu_equals_twin_bit_for_bit(eng, case2d, dof, radii):
    ref, tar, pois, prep = case2d
    rx, ry = radii
    want = twin.icgn2d(dof, prep, rx, ry, 0.001, 10, pois.copy())
    icgn = _engine(eng, dof, rx, ry, ref, tar)
    got = icgn.compute(pois.copy())
    _assert_same_bits(got, want, (dof, radii))
    assert icgn.setup_cache_last() == "none"


def test_subsets_of_less_than_one_pass_and_an_almost_full_last_pass(eng, case2d):
    """9 x 7 = 63 samples: no full pass at all; 21 x 15 = 315 = 4 x 64 + 59."""
    ref, tar, pois, prep = case2d
    for dof in (6, 12):
        for rx, ry in ((10, 7), (4, 3)):
            want = twin.icgn2d(dof, prep, rx, ry, 0.001, 10, pois.copy())
            _assert_same_bits(_engine(eng, dof, rx, ry, ref, tar).compute(pois.copy()), want, (dof, rx, ry))


@pytest.mark.parametrize("dof", [6, 12])
def test_large_queue_takes_the_tile_schedule(eng, speckle_small, dof):
    """33 600 POIs: visited through the tile-order schedule, eight POIs of a tile per workgroup, lockstep sweeps."""
    import oracle
    from opencorr_amd import synth
    ref, tar = speckle_small
    h, w = ref.shape
    xs, ys = synth.poi_grid_2d(h, w, 210, 160, 24)   # 33 600 POIs >= 32 768
    pois = oracle.make_pois2d(xs, ys)
    oracle.fftcc2d(ref, tar, 16, 16, pois)
    r = 16 if dof == 6 else 12
    got = _engine(eng, dof, r, r, ref, tar).compute(pois.copy())
    want = twin.icgn2d(dof, oracle.Prepared2D(ref, tar), r, r, 0.001, 10, pois.copy())
    _assert_same_bits(got, want, dof)
    # a device-resident queue takes the same path
    import torch
    d = torch.from_numpy(pois.copy()).cuda()
    e2 = _engine(eng, dof, r, r, ref, tar)
    e2.compute(d)
    _assert_same_bits(d.cpu().numpy(), want, (dof, "device queue"))


@pytest.mark.parametrize("dof", [6, 12])
def test_trajectories_stop_k(eng, case2d, dof):
    """conv = 0, stop = k: the record after exactly k iterations (k = 1 is the exit with g = 1 and c = the reference mean)."""
    ref, tar, pois, prep = case2d
    r = 16 if dof == 6 else 12
    icgn = _engine(eng, dof, r, r, ref, tar)
    for k in (1, 2, 5):
        icgn.set_iteration(0.0, k)
        want = twin.icgn2d(dof, prep, r, r, 0.0, k, pois.copy())
        _assert_same_bits(icgn.compute(pois.copy()), want, (dof, k))
        assert (want[2:-2, 17] == k).mean() > 0.95 and (want[2:-2, 16] == -4.0).mean() > 0.95


@pytest.mark.parametrize("dof", [6, 12])
def test_switching_contracts(eng, case2d, dof):
    import oracle
    ref, tar, pois, prep = case2d
    r = 16 if dof == 6 else 12
    fn = oracle.icgn2d1 if dof == 6 else oracle.icgn2d2
    want = twin.icgn2d(dof, prep, r, r, 0.001, 10, pois.copy())
    sep = pois.copy()
    fn(prep, r, r, 0.001, 10, sep, order=oracle.ORDER_LANES, lanes=64)
    fma = pois.copy()
    fn(prep, r, r, 0.001, 10, fma, order=oracle.ORDER_LANES_FMA, lanes=64)
    assert not np.array_equal(_bits(want), _bits(sep)) and not np.array_equal(_bits(want), _bits(fma))
    icgn = _engine(eng, dof, r, r, ref, tar)
    _assert_same_bits(icgn.compute(pois.copy()), want)
    icgn.set_tuning("arith_fma", 1)                    # under arith_onepass = 1 the value of arith_fma does not matter
    _assert_same_bits(icgn.compute(pois.copy()), want)
    icgn.set_tuning("arith_onepass", 0)                # back: the fused contract's bits ...
    _assert_same_bits(icgn.compute(pois.copy()), fma)
    icgn.set_tuning("arith_fma", 0)                    # ... and the default's
    _assert_same_bits(icgn.compute(pois.copy()), sep)
    icgn.set_tuning("arith_onepass", 1)
    _assert_same_bits(icgn.compute(pois.copy()), want)


def test_golden_oht_on_gpu_onepass(eng, golden):
    """The reference's own OHT example: GPU == twin bit for bit, the four assertions of test_golden_oht_on_gpu_fma against the
    golden table, and ORDER_SEQ's codes (tests/onepass_twin.py check_golden_oht)."""
    import oracle
    tab = golden["table"]
    guesses = oracle.make_pois2d(tab[:, 0], tab[:, 1])
    f = eng.FFTCC2D(golden["rx"], golden["ry"])
    f.set_images(golden["ref"], golden["tar"])
    f.compute(guesses)
    g = eng.ICGN2D1(golden["rx"], golden["ry"], golden["conv"], golden["stop"])
    g.share_images(f)
    g.prepare()
    g.set_tuning("arith_onepass", 1)
    got = g.compute(guesses.copy())
    prep = oracle.Prepared2D(golden["ref"], golden["tar"])
    want = twin.icgn2d1(prep, golden["rx"], golden["ry"], golden["conv"], golden["stop"], guesses.copy())
    _assert_same_bits(got, want)
    seq = guesses.copy()
    oracle.icgn2d1(prep, golden["rx"], golden["ry"], golden["conv"], golden["stop"], seq, order=oracle.ORDER_SEQ)
    twin.check_golden_oht(got, seq, guesses, golden)


def test_gpu_2d2_within_the_bars_of_the_float64_model(eng):
    cs = m64.cases2d2()
    models = [m64.model_runs(c) for c in cs]
    engines = {}

    def run(case, conv, stop):
        family, r, ref, tar, _, _, pois = case
        e = engines.get((family, r))
        if e is None:
            e = engines[(family, r)] = _engine(eng, 12, r[0], r[1], ref, tar, conv, stop)
        e.set_iteration(conv, stop)
        return e.compute(pois.copy())

    dist, exc = m64.measure(cs, run, models)
    lines, bad = m64.check_within_bars(dist, "GPU arith_onepass")
    print("\n".join(lines))
    print("GPU arith_onepass one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)


def test_key_travels_through_a_device_group_and_is_refused_elsewhere(eng, case2d):
    ref, tar, pois, prep = case2d
    want = twin.icgn2d1(prep, 16, 16, 0.001, 10, pois.copy())
    icgn = eng.ICGN2D1(16, 16, 0.001, 10)
    icgn.set_devices([0, 0, 0])
    icgn.set_tuning("arith_onepass", 1)       # fans out over the members
    icgn.set_images(ref, tar)
    icgn.prepare()
    _assert_same_bits(icgn.compute(pois.copy()), want)
    icgn2 = eng.ICGN2D1(16, 16, 0.001, 10)
    icgn2.set_tuning("arith_onepass", 1)      # set BEFORE the group is formed: the clones inherit it
    icgn2.set_devices([0, 0, 0])
    icgn2.set_images(ref, tar)
    icgn2.prepare()
    _assert_same_bits(icgn2.compute(pois.copy()), want)
    for make in (lambda: eng.FFTCC2D(16, 16), lambda: eng.NR2D1(16, 16, 0.001, 10), lambda: eng.ICLM2D1(16, 16, 0.001, 10),
                 lambda: eng.ICLM2D2(16, 16, 0.001, 10), lambda: eng.ICGN3D1(8, 8, 8, 0.001, 10), lambda: eng.FFTCC3D(8, 8, 8)):
        e = make()
        with pytest.raises(Exception, match="arith_onepass"):
            e.set_tuning("arith_onepass", 1)
        e.set_tuning("arith_onepass", 0)


@pytest.mark.parametrize("dof", [6, 12])
def test_unsupported_call_paths_raise(eng, case2d, dof):
    """Centre offsets and self-adaptive radii are refused under the contract -- they never silently run another one -- and work again
    once the key is back at 0."""
    import oracle
    ref, tar, pois, prep = case2d
    icgn = _engine(eng, dof, 12, 12, ref, tar)
    off = np.random.default_rng(5).uniform(-2, 2, (len(pois), 2)).astype(np.float32)
    q = pois.copy()
    with pytest.raises(Exception, match="arith_onepass"):
        icgn.compute_with_offsets(q, off)
    assert np.array_equal(_bits(q), _bits(pois))          # nothing was computed
    icgn.set_self_adaptive(True)
    sa = pois.copy()
    sa[:, oracle.P2["srx"]] = 9
    sa[:, oracle.P2["sry"]] = 8
    q = sa.copy()
    with pytest.raises(Exception, match="arith_onepass"):
        icgn.compute(q)
    assert np.array_equal(_bits(q), _bits(sa))
    icgn.set_self_adaptive(False)
    _assert_same_bits(icgn.compute(pois.copy()), twin.icgn2d(dof, prep, 12, 12, 0.001, 10, pois.copy()))
    icgn.set_tuning("arith_onepass", 0)
    fn = oracle.icgn2d1 if dof == 6 else oracle.icgn2d2
    want = pois.copy()
    fn(prep, 12, 12, 0.001, 10, want, order=oracle.ORDER_LANES, lanes=64, center_offsets=off)
    _assert_same_bits(icgn.compute_with_offsets(pois.copy(), off), want)


def test_chain_and_single_poi_front_end(eng, case2d, speckle_small):
    import oracle
    ref, tar, pois, prep = case2d
    want = twin.icgn2d1(prep, 16, 16, 0.001, 10, pois.copy())
    icgn = _engine(eng, 6, 16, 16, ref, tar)
    # compute_one through the combining front end == compute
    for k in (0, 1, 2, 5, 100, len(pois) - 1):
        one = pois[k].copy()
        icgn.compute_one(one)
        _assert_same_bits(one, want[k], k)
    # compute_chain([fftcc, icgn]) == the two calls
    fftcc = eng.FFTCC2D(16, 16)
    fftcc.set_images(ref, tar)
    icgn.share_images(fftcc)
    icgn.prepare()
    fresh = oracle.make_pois2d(pois[2:-2, 0], pois[2:-2, 1])
    two = fresh.copy()
    fftcc.compute(two)
    icgn.compute(two)
    chained = eng.compute_chain([fftcc, icgn], fresh.copy())
    _assert_same_bits(chained, two)
    _assert_same_bits(two, twin.icgn2d1(prep, 16, 16, 0.001, 10, fftcc.compute(fresh.copy())))

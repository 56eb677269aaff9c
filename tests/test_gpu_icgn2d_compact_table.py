"""ICGN2D variants 10 and 11 (icgn2d.hip MODE 6): the lockstep sweeps of variants 5 / 4 in 4-WAVE workgroups, six / four per CU,
on a coordinate table of 6 bytes per sample slot (byte offset + 8-bit column and row) instead of 12.

Bar everywhere: BIT-IDENTICAL (uint32 view) to the CPU oracle in OC_ORDER_LANES (OC_ORDER_LANES_FMA under "arith_fma" = 1) and
to variant 2 -- 4-wave workgroups without table, barriers or cache -- on the same engine.  The variant is named through
set_tuning("icgn2d_variant", 10 | 11); a named variant runs at any queue length, so the queues here stay small.  The path a
call took through the set-up cache is asserted through setup_cache_last().

One CPU-only test (no `gpu` mark) restates the LDS arithmetic of the two shapes and checks the library's limits against it.
"""
import ctypes

import numpy as np
import pytest

gpu = pytest.mark.gpu

# (rx, ry): 18 passes with the lone 1 089th sample | 3 passes, partial tail | 9 samples, no full pass | 19 passes, the largest
# that six workgroups admit | 301 rows: a row index above 255, the engine must fall back by itself
SHAPES = [(16, 16), (4, 7), (1, 1), (17, 16), (1, 150)]
VARIANT_OF = {6: 10, 12: 11}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_but_nan_sign(a, b):
    """bit-identical, except that a field which is NaN in both may carry either default NaN: x86 produces 0xffc00000 for an invalid
    operation, gfx950 0x7fc00000"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(_bits(a)[~both_nan], _bits(b)[~both_nan])


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    assert opencorr_amd.capi.device_count() >= 1
    return opencorr_amd


@pytest.fixture(scope="module")
def tall_pair():
    """340 x 96 speckle pair: the only fixture here that is not speckle_small -- a subset of 301 rows does not fit its 300"""
    from opencorr_amd import synth
    return synth.speckle_pair_2d(340, 96, seed=20261019)


class _Ref:
    """Oracle results, computed once per case and handed out as copies"""

    def __init__(self):
        self.prep, self.memo = {}, {}

    def prepared(self, ref, tar):
        import oracle
        if id(ref) not in self.prep:
            self.prep[id(ref)] = (oracle.Prepared2D(ref, tar), ref)   # (ref kept alive: its id is the key)
        return self.prep[id(ref)][0]

    def solve(self, key, ref, tar, dof, rx, ry, q, fma=0, **kw):
        import oracle
        if key not in self.memo:
            want = q.copy()
            fn = oracle.icgn2d1 if dof == 6 else oracle.icgn2d2
            fn(self.prepared(ref, tar), rx, ry, 0.001, 10, want, order=oracle.ORDER_LANES_FMA if fma else oracle.ORDER_LANES, lanes=64, **kw)
            self.memo[key] = want
        return self.memo[key].copy()


@pytest.fixture(scope="module")
def refs():
    return _Ref()


def _start(eng, ref, tar, nx, ny, margin, r=16, grid=None):
    """an FFTCC2D-initialised queue (integral u, v: the first sweep of every POI is the integer-translation one)"""
    from opencorr_amd import synth
    h, w = ref.shape
    xs, ys = synth.poi_grid_2d(h, w, nx, ny, margin) if grid is None else grid
    q = eng.make_pois2d(np.float32(xs), np.float32(ys))
    f = eng.FFTCC2D(r, r)
    f.set_images(ref, tar)
    f.compute(q)
    f.close()
    return q


def _engine(eng, dof, rx, ry, ref, tar, variant, **tuning):
    e = (eng.ICGN2D1 if dof == 6 else eng.ICGN2D2)(rx, ry, 0.001, 10)
    e.set_images(ref, tar)
    e.prepare()
    e.set_tuning("icgn2d_variant", variant)
    for k, v in tuning.items():
        e.set_tuning(k, v)
    return e


@pytest.fixture(scope="module")
def big(eng, speckle_small):
    """4 097 FFTCC guesses at r = 16 (4 096 grid POIs + one that trips the geometric guard): the last workgroup holds one
    wave, and with "icgn2d_xcd" = 1 whole workgroups of the grid are empty"""
    ref, tar = speckle_small
    q = _start(eng, ref, tar, 64, 64, 20)
    assert len(q) == 4096
    tripper = eng.make_pois2d(np.float32([5.0]), np.float32([150.0]))
    return np.concatenate([q, tripper]).astype(np.float32)


# ---- subset shapes -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rx,ry", SHAPES)
@pytest.mark.parametrize("dof", [6, 12])
def test_subset_shapes_match_oracle_and_variant_2(eng, speckle_small, tall_pair, refs, dof, rx, ry):
    """Both new variants on every shape, at both DoF: a queue of 103 POIs (the last workgroup holds three waves; 19 on the tall
    pair) with guard trippers, a rejected and a NaN POI spread over the workgroups.
    One case cannot be bit-identical to the oracle in any variant, old or new: 9 samples do not determine 12 parameters, the
    Hessian of a 3 x 3 subset at 12 DoF is singular, and the records fill with NaN -- the same fields on both sides, but the
    host's default NaN has the sign bit set and the GPU's has not (measured: 160 fields of this queue, identical in variants 2, 3,
    10 and 11).  There, and only there, a field that is NaN on both sides counts as equal to the oracle; against variant 2 the
    bar stays bit for bit."""
    import oracle
    ref, tar = tall_pair if ry > 140 else speckle_small
    h, w = ref.shape
    P = oracle.P2
    if ry > 140:
        gx, gy = np.meshgrid([20.0, 34.0, 48.0, 61.0, 75.0], [152.0, 165.0, 187.0])      # 15 POIs whose 301 rows fit 340
        q = _start(eng, ref, tar, 0, 0, 0, r=8, grid=(gx.ravel(), gy.ravel()))
    else:
        q = _start(eng, ref, tar, 11, 9, max(rx, ry) + 8, r=12)                          # 99 POIs
    extra = oracle.make_pois2d([0.0, w / 2.0, w / 2.0, w / 2.0], [h / 2.0, h / 2.0, h / 2.0, h / 2.0])
    extra[1, P["u"]] = float(w) - 4.0          # in range for the guard, outside for the table: abort after the first sweep
    extra[2, P["zncc"]] = -1.0
    extra[3, P["v"]] = np.nan
    q = np.concatenate([extra[:2], q, extra[2:]]).astype(np.float32)
    want = refs.solve(("shape", dof, rx, ry), ref, tar, dof, rx, ry, q)
    # the queue is solved, not rejected wholesale (a 3 x 301 subset holds on to two POIs in three; 9 x 15 and 3 x 3 subsets are
    # there for their pass counts, whatever becomes of the POIs)
    if min(rx, ry) >= 16:
        assert (want[:, P["zncc"]] > 0.9).sum() >= (len(q) - 4) * 0.9
    elif ry > 140:
        assert (want[:, P["zncc"]] > 0.9).sum() >= 8
    singular = (2 * rx + 1) * (2 * ry + 1) < dof
    plain = None
    for variant in (2, 10, 11):
        e = _engine(eng, dof, rx, ry, ref, tar, variant)
        got = e.compute(q.copy())
        e.close()
        assert (_same_but_nan_sign if singular else _same)(got, want), "variant %d" % variant
        plain = got if variant == 2 else plain
        assert _same(got, plain), "variant %d against variant 2" % variant


# ---- queue lengths, with and without the XCD mapping -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_queue_lengths_that_fill_neither_workgroup_nor_table_share(eng, speckle_small, refs, big, dof, xcd):
    ref, tar = speckle_small
    want = refs.solve(("big", dof), ref, tar, dof, 16, 16, big)
    e = _engine(eng, dof, 16, 16, ref, tar, VARIANT_OF[dof], icgn2d_xcd=xcd)
    plain = _engine(eng, dof, 16, 16, ref, tar, 2, icgn2d_xcd=xcd)
    for n in (1, 3, 5, 4097):
        # (POIs are solved independently: the oracle's records of a prefix are the prefix of its records)
        q = big[-n:] if n == 1 else big[:n]
        w = want[-n:] if n == 1 else want[:n]
        got = e.compute(q.copy())
        assert _same(got, w), "n = %d" % n
        assert _same(plain.compute(q.copy()), w), "variant 2, n = %d" % n
    e.close()
    plain.close()


# ---- waves of one workgroup that live for different numbers of iterations --------------------------------------------------
@gpu
@pytest.mark.parametrize("rotate", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_lockstep_barriers_in_4_wave_groups_with_mixed_wave_lifetimes(eng, speckle_small, refs, dof, rotate):
    """tests/test_gpu_parity_2d.py::test_icgn2d_lockstep_barriers_with_mixed_wave_lifetimes in 4-wave workgroups.  Six kinds of
    POI -- a guard reject (zncc < 0), a first-sweep abort (-3), a NaN guess, a POI that starts converged (one iteration), a far-off
    guess that runs to the stop limit (-4), a normal one -- do not fit four waves, so the kinds repeat with period 6 along the
    queue (queue order: below the tile-schedule threshold): workgroups see the windows of four consecutive kinds that start at
    kind 0, 4, 2 (`rotate` = 0) and 1, 5, 3 (`rotate` = 1), i.e. every one of them; each window mixes waves that leave before
    or after their first sweep with waves that iterate.  Must terminate and match, three times in a row."""
    import oracle
    ref, tar = speckle_small
    r, P = 16, oracle.P2
    h, w = ref.shape
    start = _start(eng, ref, tar, 30, 24, 26)            # 720 POIs = 180 workgroups of 4
    solved = refs.solve(("mixed-solved", dof), ref, tar, dof, r, r, start)
    q = start.copy()
    kind = (np.arange(len(q)) + rotate) % 6
    q[kind == 0, P["zncc"]] = -2.0
    q[kind == 1, P["u"]] = w - 30.0
    q[kind == 2, P["v"]] = np.nan
    one = kind == 3
    q[one, 2:14] = solved[one, 2:14]
    q[kind == 4, P["u"]] += 6.5
    q[kind == 4, P["v"]] -= 5.5
    want = refs.solve(("mixed", dof, rotate), ref, tar, dof, r, r, q)
    it = want[:, P["iteration"]]
    assert (want[kind == 0, P["zncc"]] == -2.0).all() and (want[kind == 1, P["zncc"]] == -3.0).all()
    assert (it[one & (want[:, P["zncc"]] > 0)] <= (1 if dof == 6 else 3)).mean() > 0.9
    assert ((want[kind == 4, P["zncc"]] == -4.0) | (it[kind == 4] >= 6)).mean() > 0.5
    assert (want[kind == 5, P["zncc"]] > 0.9).mean() > 0.9
    e = _engine(eng, dof, r, r, ref, tar, VARIANT_OF[dof])
    for _ in range(3):
        assert _same(e.compute(q.copy()), want)
    e.close()
    plain = _engine(eng, dof, r, r, ref, tar, 2)
    assert _same(plain.compute(q.copy()), want)
    plain.close()


# ---- set-up cache ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_setup_cache_fill_use_use(eng, speckle_small, refs, big, dof, fma):
    ref, tar = speckle_small
    want = refs.solve(("big", dof, fma) if fma else ("big", dof), ref, tar, dof, 16, 16, big, fma=fma)
    off = _engine(eng, dof, 16, 16, ref, tar, VARIANT_OF[dof], icgn2d_setup_cache=0, arith_fma=fma)
    got = off.compute(big.copy())
    assert off.setup_cache_last() == "none" and _same(got, want)
    off.close()
    on = _engine(eng, dof, 16, 16, ref, tar, VARIANT_OF[dof], icgn2d_setup_cache=1, arith_fma=fma)
    states = []
    for _ in range(3):
        got = on.compute(big.copy())
        states.append(on.setup_cache_last())
        assert _same(got, want)
    assert states == ["fill", "use", "use"]
    on.close()


@gpu
@pytest.mark.parametrize("dof", [6, 12])
def test_setup_cache_other_guesses_are_served_and_a_moved_poi_fills(eng, speckle_small, refs, big, dof):
    """The records depend on the reference and on (x, y) alone, exactly as for variants 5 / 4: a use call may bring other
    guesses -- POIs that the fill call's data guard rejected are solved from their records, others are rejected now -- while
    one POI moved by a pixel makes the call a fill.  Bits: those of "icgn2d_setup_cache" = 0 and of the oracle."""
    import oracle
    ref, tar = speckle_small
    P = oracle.P2
    slot = np.arange(len(big)) % 4
    qa, qb = big.copy(), big.copy()
    qa[slot == 0, P["zncc"]] = -2.0
    qa[slot == 1, P["u"]] = np.nan
    qb[slot == 2, P["zncc"]] = -2.0
    qb[slot == 3, P["u"]] += 0.4
    qb[slot == 3, P["ux"]] = 0.01
    moved = big.copy()
    moved[1234, P["x"]] += 1.0
    want = {k: refs.solve(("cache", dof, k), ref, tar, dof, 16, 16, q) for k, q in (("a", qa), ("b", qb), ("moved", moved))}
    assert (want["b"][slot == 0, P["zncc"]] > 0.9).mean() > 0.9           # rejected by A, solved by B
    on = _engine(eng, dof, 16, 16, ref, tar, VARIANT_OF[dof])
    off = _engine(eng, dof, 16, 16, ref, tar, VARIANT_OF[dof], icgn2d_setup_cache=0)
    for k, q, expect in (("a", qa, "fill"), ("b", qb, "use"), ("a", qa, "use"), ("moved", moved, "fill"), ("moved", moved, "use")):
        got = on.compute(q.copy())
        assert on.setup_cache_last() == expect, (k, expect)
        assert _same(got, want[k]), k
        assert _same(off.compute(q.copy()), want[k]) and off.setup_cache_last() == "none"
    on.close()
    off.close()


# ---- the other paths -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("int_first", [0, 1])
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_int_first_and_both_arithmetic_contracts(eng, speckle_small, refs, dof, fma, int_first):
    """An FFTCC queue (first sweep: the value plane with "icgn2d_int_first" = 1) whose every third POI carries a non-integral
    guess, so workgroups mix the two sweep bodies behind the shared barrier."""
    import oracle
    ref, tar = speckle_small
    P = oracle.P2
    q = _start(eng, ref, tar, 19, 11, 24)               # 209 POIs
    q[::3, P["u"]] += 0.3
    q[::3, P["vy"]] = 0.004
    want = refs.solve(("arith", dof, fma), ref, tar, dof, 16, 16, q, fma=fma)
    for variant in (VARIANT_OF[dof], 2):
        e = _engine(eng, dof, 16, 16, ref, tar, variant, arith_fma=fma, icgn2d_int_first=int_first)
        # prepare() after the key, so that the value plane exists / does not exist as the key says
        e.prepare()
        got = e.compute(q.copy())
        e.close()
        assert _same(got, want), "variant %d" % variant


@gpu
@pytest.mark.parametrize("dof", [6, 12])
def test_centre_offsets_go_around_the_cache(eng, speckle_small, refs, dof):
    ref, tar = speckle_small
    rx, ry = 13, 9
    q = _start(eng, ref, tar, 13, 9, 24, r=12)[:-2]       # 115 POIs
    off = np.random.default_rng(dof).uniform(-2, 2, (len(q), 2)).astype(np.float32)
    want = refs.solve(("offs", dof), ref, tar, dof, rx, ry, q, center_offsets=off)
    for variant in (VARIANT_OF[dof], 2):
        e = _engine(eng, dof, rx, ry, ref, tar, variant)
        for _ in range(2):
            got = e.compute_with_offsets(q.copy(), off)
            assert e.setup_cache_last() == "none"
            assert _same(got, want), "variant %d" % variant
        e.close()


@gpu
@pytest.mark.parametrize("dof", [6, 12])
def test_self_adaptive_radii_take_the_table_free_fallback(eng, speckle_small, refs, dof):
    import oracle
    ref, tar = speckle_small
    P = oracle.P2
    rx, ry = 13, 9
    q = _start(eng, ref, tar, 13, 9, 24, r=12)
    q[:, P["srx"]] = np.random.default_rng(1).integers(6, rx + 1, len(q))
    q[:, P["sry"]] = np.random.default_rng(2).integers(6, ry + 1, len(q))
    want = refs.solve(("sa", dof), ref, tar, dof, rx, ry, q, self_adaptive=True)
    e = _engine(eng, dof, rx, ry, ref, tar, VARIANT_OF[dof])
    e.set_self_adaptive(True)
    for _ in range(2):
        got = e.compute(q.copy())
        assert e.setup_cache_last() == "none"
        assert _same(got, want)
    e.close()


# ---- CPU only: the limits against the LDS arithmetic -----------------------------------------------------------------------
def _limits(variant, rx, ry, count):
    from opencorr_amd import capi
    ms, adm = ctypes.c_int(-1), ctypes.c_int(-1)
    capi.check(capi.lib().oc_hip_icgn2d_variant_limits(variant, rx, ry, count, ctypes.byref(ms), ctypes.byref(adm)))
    return ms.value, adm.value


def test_max_samples_and_admissibility_follow_the_lds_arithmetic():
    """A 4-wave workgroup of the compact-table shape holds, per pass of 64 samples, four target arrays (4 x 256 B) and the table
    (64 x 6 B): 1 408 B.  A CU offers 160 KiB less 2 KiB: six such workgroups fit up to 19 passes, four up to 28, one up to 114."""
    budget = 160 * 1024 - 2048
    per_pass = 4 * 64 * 4 + 64 * 6
    assert per_pass == 1408 and 18 * per_pass == 25344 and 6 * 25344 == 152064 <= budget      # r = 16
    assert 27 * per_pass == 38016 and 28 * per_pass == 39424 and 4 * 39424 <= budget          # r = 20, and the last that fits
    for variant in (10, 11):
        assert _limits(variant, 16, 16, 1 << 16)[0] == budget // per_pass * 64 == 114 * 64
    # the float table of variants 6 (four waves) and 5 (eight), for comparison: 12 B per slot
    assert _limits(6, 16, 16, 0)[0] == budget // (4 * 256 + 768) * 64
    assert _limits(5, 16, 16, 0)[0] == budget // (8 * 256 + 768) * 64
    assert _limits(2, 16, 16, 0)[0] == budget // (2 * 4 * 256) * 64

    def passes(rx, ry):
        return ((2 * rx + 1) * (2 * ry + 1) + 63) // 64

    def rule(variant, rx, ry):
        return 2 * rx + 1 <= 256 and 2 * ry + 1 <= 256 and (6 if variant == 10 else 4) * passes(rx, ry) * per_pass <= budget

    big = 1 << 16
    for variant in (10, 11):
        for rx, ry in SHAPES + [(17, 17), (20, 20), (20, 21), (21, 21), (127, 1), (128, 1), (1, 127), (1, 128), (0, 0), (40, 40)]:
            adm = _limits(variant, rx, ry, big)[1]
            assert adm == (2 if rule(variant, rx, ry) else 0), (variant, rx, ry)
            # below 32 768 POIs the automatic choice does not take them; a named variant still runs
            assert _limits(variant, rx, ry, 32767)[1] == (1 if rule(variant, rx, ry) else 0)
            assert _limits(variant, rx, ry, 32768)[1] == adm
    assert passes(17, 16) == 19 and _limits(10, 17, 16, big)[1] == 2 and _limits(10, 17, 17, big)[1] == 0
    assert passes(20, 20) == 27 and _limits(11, 20, 20, big)[1] == 2 and _limits(10, 20, 20, big)[1] == 0
    assert _limits(11, 20, 21, big)[1] == 2 and passes(20, 21) == 28 and _limits(11, 21, 21, big)[1] == 0
    assert _limits(10, 1, 150, big)[1] == 0 and _limits(11, 1, 150, big)[1] == 0            # 301 rows
    for variant in (2, 4, 5):
        assert _limits(variant, 16, 16, big)[1] == 0

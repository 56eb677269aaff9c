"""The HIP engines on images that are not 8-bit speckle (tests/image_domains.py), against the oracle.

Every other GPU parity test feeds the kernels integer grey levels 0 ... 255 on a background of 20: window sums are exact in every
association, the gradient numerator is exact however it is bracketed, no interpolated sample comes near zero, nothing is flat.
Here the same bars are asked on six other intensity domains -- `u16`, `unit`, `pedestal` (float32 sums round: a reduction in the
wrong order shows in the bits), `dark` (the reference's "any target sample < 0 -> -3" rule decides on the sign of a rounded sum),
`flat` (zero norm, NaN ZNCC, singular Hessian) and `signed` (negative intensities):

  * prepare: gradients, coefficient table / volume and the value plane bit for bit;
  * FFTCC2D / FFTCC3D, every kernel family: integers identical, NaN ZNCC on the same records, ZNCC within the domain's bar
    (image_domains.fftcc_bar: the 8-bit bar, or 4 x the oracle's measured distance from float64 where that is larger), every
    other field untouched;
  * ICGN2D1 / ICGN2D2 under the three arithmetic contracts, ICLM2D1 / ICLM2D2, NR2D1, ICGN3D1 under its three contracts: EVERY
    float of EVERY record (NaN meets NaN, tests/test_gpu_fuzz.py::_same), on a queue of integer FFTCC guesses (the value-plane
    sweep) and on its noisy copy, and again on a second compute() -- through the set-up cache where the launch has one;
  * ICGN2D2 / ICGN3D1 against the float64 model within the domain's bars (image_domains.model_bars).
tests/test_oracle_domains.py asserts, without a GPU, that none of these passes emptily.
"""
import numpy as np
import pytest

import image_domains as dom

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    return opencorr_amd


def _bit_equal(a, b, what):
    assert np.array_equal(dom.bits(a), dom.bits(b)), (what, int((dom.bits(a) != dom.bits(b)).sum()), "floats differ")


# ---- prepare ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dom.NAMES)
def test_prepare2d_fields(eng, name):
    import oracle
    ref, tar = dom.images2d(name)
    prep, _ = dom.prepared2d(name)
    e = eng.ICGN2D1(dom.R2D[0], dom.R2D[1], dom.CONV, dom.STOP2D)
    e.set_images(ref, tar)
    e.prepare()
    _bit_equal(e.read_field("gx"), prep.gx, "gx")
    _bit_equal(e.read_field("gy"), prep.gy, "gy")
    lut, val = e.read_field("lut"), e.read_field("lut_val")
    _bit_equal(lut, prep.lut, "lut")
    # the value plane: what the interpolator returns at every interior integer point, the leading coefficient everywhere
    h, w = tar.shape
    inner = (slice(1, h - 2), slice(1, w - 2))
    ev = np.array([[oracle.bspline2d_eval(prep.lut, x, y) for x in range(1, w - 2)] for y in range(1, h - 2)], dtype=np.float32)
    _bit_equal(val[inner], ev, "lut_val against the evaluator")
    _bit_equal(val, lut[..., 0], "lut_val against the table")
    e.close()


@pytest.mark.parametrize("name", dom.NAMES)
def test_prepare3d_fields(eng, name):
    ref, tar = dom.images3d(name)
    prep = dom.prepared3d(name)
    e = eng.ICGN3D1(dom.R3D[0], dom.R3D[1], dom.R3D[2], dom.CONV, dom.STOP3D)
    e.set_images(ref, tar)
    e.prepare()
    for f in ("gx", "gy", "gz", "coef"):
        _bit_equal(e.read_field(f), getattr(prep, f), f)
    e.close()


# ---- FFTCC -----------------------------------------------------------------------------------------------------------------
# (radii, tuning "fftcc2d_fused", shape class): the fused square kernel (fftcc2d_fusedn.hip), the dedicated 32 x 32 kernel
# (fftcc2d_fused.hip), the 40 x 40 instance (a window of `u16` whose sums pass 2^24), the two rectangular kernels, the rocFFT pipeline
FFTCC2D_CASES = [((12, 12), 1, "2d_square"), ((16, 16), 1, "2d_square"), ((20, 20), 1, "2d_square"), ((9, 11), 1, "2d_rect"),
                 ((4, 32), 1, "2d_rect"), ((12, 12), 0, "2d_square")]


@pytest.mark.parametrize("r,fused,cls", FFTCC2D_CASES, ids=["r12", "r16", "r20", "9x11", "4x32", "r12-rocfft"])
@pytest.mark.parametrize("name", dom.NAMES)
def test_fftcc2d(eng, name, r, fused, cls):
    import oracle
    ref, tar = dom.images2d(name)
    q = dom.fftcc_queue2d(*r)
    want = q.copy()
    oracle.fftcc2d(ref, tar, r[0], r[1], want)
    f = eng.FFTCC2D(*r)
    f.set_images(ref, tar)
    if not fused:
        f.set_tuning("fftcc2d_fused", 0)
    got = f.compute(q.copy())
    bar = dom.fftcc_bar(name, cls)
    with np.errstate(invalid="ignore"):
        print(name, r, fused, "ZNCC distance %.3e, bar %.3e, NaN records %d" % (
            float(np.nanmax(np.abs(got[:, 16].astype(np.float64) - want[:, 16]))), bar, int(np.isnan(want[:, 16]).sum())))
    dom.check_fftcc(got, want, oracle.P2, ("u", "v", "u0", "v0"), bar, (name, r, fused))
    assert np.array_equal(dom.bits(got[-3:]), dom.bits(q[-3:]))     # the guarded records stay untouched
    f.close()


@pytest.mark.parametrize("r,fused", [((6, 6, 6), 1), ((5, 6, 4), 1), ((6, 6, 6), 0)], ids=["r6-lds", "5x6x4-box", "r6-rocfft"])
@pytest.mark.parametrize("name", dom.NAMES)
def test_fftcc3d(eng, name, r, fused):
    import oracle
    ref, tar = dom.images3d(name)
    q = dom.fftcc_queue3d()
    want = q.copy()
    oracle.fftcc3d(ref, tar, r[0], r[1], r[2], want)
    f = eng.FFTCC3D(*r)
    f.set_images(ref, tar)
    if not fused:
        f.set_tuning("fftcc3d_fused", 0)
    got = f.compute(q.copy())
    bar = dom.fftcc_bar(name, "3d")
    with np.errstate(invalid="ignore"):
        print(name, r, fused, "ZNCC distance %.3e, bar %.3e, NaN records %d" % (
            float(np.nanmax(np.abs(got[:, 18].astype(np.float64) - want[:, 18]))), bar, int(np.isnan(want[:, 18]).sum())))
    dom.check_fftcc(got, want, oracle.P3, ("u", "v", "w", "u0", "v0", "w0"), bar, (name, r, fused))
    f.close()


@pytest.mark.parametrize("name", dom.NAMES)
def test_fftcc3d_register_kernel_on_clamped_windows(eng, name):
    """r = 16 (fftcc3d_fused.hip): on the 44 x 46 x 48 volumes most windows are clamped at a face, where the oracle does not
    reach -- against the rocFFT pipeline of the same engine (same clamping: integers identical, ZNCC within 5e-6, the bar of
    tests/test_gpu_fuzz.py::test_fuzz_fftcc3d_32_cubed_windows_anywhere: by the rule of image_domains.fftcc_bar every domain keeps
    the 8-bit bar in 3D, so this one carries over as well), and against the oracle, at the domain's bar, on the windows inside both
    volumes.  The box of `flat` holds no 32^3 window: test_fftcc3d_one_constant_window asks that on a wider one."""
    import oracle
    P = oracle.P3
    ref, tar = dom.images3d(name)
    q = dom.fftcc_queue3d()
    f = eng.FFTCC3D(16, 16, 16)
    f.set_images(ref, tar)
    got = f.compute(q.copy())
    f.set_tuning("fftcc3d_fused", 0)
    base = f.compute(q.copy())
    for k in ("u", "v", "w", "u0", "v0", "w0"):
        assert np.array_equal(got[:, P[k]], base[:, P[k]]), (name, k)
    d = dom.zncc_distance(got, base, P["zncc"])
    print(name, "r = 16 against the pipeline: ZNCC distance %.3e" % d)
    assert d <= 5e-6
    inner = dom.inner16(q)
    assert inner.sum() >= 2
    want = q[inner].copy()
    oracle.fftcc3d(ref, tar, 16, 16, 16, want)
    dom.check_fftcc(got[inner], want, P, ("u", "v", "w", "u0", "v0", "w0"), dom.fftcc_bar(name, "3d"), (name, "r = 16, inner windows"))
    f.close()


# `flat` on the border of its block: exactly one window constant, in both directions (image_domains.flat_border_queue2d / 3d;
# tests/test_oracle_domains.py asserts that the queues hold such records for every shape below).  (32, 4) stands for (4, 32),
# whose 64 rows no 60-row block can hold; r = 14 is the plane-wise kernel, r = 16 the register kernel, both on the widened box.
@pytest.mark.parametrize("r,fused,cls", [c for c in FFTCC2D_CASES if c[0] != (4, 32)] + [((32, 4), 1, "2d_rect")],
                         ids=["r12", "r16", "r20", "9x11", "r12-rocfft", "32x4"])
def test_fftcc2d_one_constant_window(eng, r, fused, cls):
    import oracle
    ref, tar = dom.images2d("flat")
    q = dom.flat_border_queue2d(*r)
    want = q.copy()
    oracle.fftcc2d(ref, tar, r[0], r[1], want)
    f = eng.FFTCC2D(*r)
    f.set_images(ref, tar)
    if not fused:
        f.set_tuning("fftcc2d_fused", 0)
    got = f.compute(q.copy())
    f.close()
    dom.check_flat_border(got, *dom.constant_windows(ref, tar, r, q[:5]), oracle.P2["zncc"])
    dom.check_fftcc(got, want, oracle.P2, ("u", "v", "u0", "v0"), dom.fftcc_bar("flat", cls), ("flat border", r, fused))


@pytest.mark.parametrize("r,fused,wide", [((6, 6, 6), 1, False), ((5, 6, 4), 1, False), ((6, 6, 6), 0, False), ((14, 14, 14), 1, True),
                                          ((16, 16, 16), 1, True), ((16, 16, 16), 0, True)],
                         ids=["r6-lds", "5x6x4-box", "r6-rocfft", "r14-planes", "r16-registers", "r16-rocfft"])
def test_fftcc3d_one_constant_window(eng, r, fused, wide):
    import oracle
    ref, tar = dom.flat_wide3d() if wide else dom.images3d("flat")
    q = dom.flat_border_queue3d(r, dom.FLAT_WIDE3D if wide else dom.FLAT3D)
    want = q.copy()
    oracle.fftcc3d(ref, tar, r[0], r[1], r[2], want)
    f = eng.FFTCC3D(*r)
    f.set_images(ref, tar)
    if not fused:
        f.set_tuning("fftcc3d_fused", 0)
    got = f.compute(q.copy())
    f.close()
    dom.check_flat_border(got, *dom.constant_windows(ref, tar, r, q), oracle.P3["zncc"])
    dom.check_fftcc(got, want, oracle.P3, ("u", "v", "w", "u0", "v0", "w0"), dom.fftcc_bar("flat", "3d"), ("flat border", r, fused))


# ---- 2D solvers ------------------------------------------------------------------------------------------------------------
def _icgn2d(eng, name, dof, r=None, variant=None):
    r = r or dom.R2D
    e = (eng.ICGN2D1 if dof == 6 else eng.ICGN2D2)(r[0], r[1], dom.CONV, dom.STOP2D)
    if variant is not None:
        e.set_tuning("icgn2d_variant", variant)
    e.set_images(*dom.images2d(name))
    e.prepare()
    return e


@pytest.mark.parametrize("dof", [6, 12])
@pytest.mark.parametrize("name", dom.NAMES)
def test_icgn2d_three_contracts(eng, name, dof):
    """Default against ORDER_LANES, arith_fma against ORDER_LANES_FMA, arith_onepass against its CPU twin; each twice."""
    import oracle
    import onepass_twin as twin
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    prep, _ = dom.prepared2d(name)
    e = _icgn2d(eng, name, dof)
    for k, q in enumerate(dom.queues2d(name)):
        e.set_tuning("arith_onepass", 0)
        e.set_tuning("arith_fma", 0)
        want = dom.oracle2d(name, solver, q, oracle.ORDER_LANES)
        for call in (1, 2):
            dom.assert_same(e.compute(q.copy()), want, (name, solver, "default", "queue %d call %d" % (k, call)))
        e.set_tuning("arith_fma", 1)
        want = dom.oracle2d(name, solver, q, oracle.ORDER_LANES_FMA)
        for call in (1, 2):
            dom.assert_same(e.compute(q.copy()), want, (name, solver, "arith_fma", "queue %d call %d" % (k, call)))
        e.set_tuning("arith_onepass", 1)
        want = twin.icgn2d(dof, prep, dom.R2D[0], dom.R2D[1], dom.CONV, dom.STOP2D, q.copy())
        for call in (1, 2):
            dom.assert_same(e.compute(q.copy()), want, (name, solver, "arith_onepass", "queue %d call %d" % (k, call)))
    e.close()


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
@pytest.mark.parametrize("name", dom.NAMES)
def test_icgn2d_through_the_setup_cache(eng, name, dof, fma):
    """The coordinate-table launch shape (variant 5 / 4, named because these queues are below its automatic threshold) keeps
    { reference mean, norm, H^-1 } per POI: the first compute() fills the records, the second starts from them -- same bits."""
    import oracle
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    e = _icgn2d(eng, name, dof, variant=5 if dof == 6 else 4)
    e.set_tuning("arith_fma", fma)
    q, _ = dom.queues2d(name)
    want = dom.oracle2d(name, solver, q, oracle.ORDER_LANES_FMA if fma else oracle.ORDER_LANES)
    states = []
    for call in (1, 2, 3):
        got = e.compute(q.copy())
        states.append(e.setup_cache_last())
        dom.assert_same(got, want, (name, solver, fma, "call %d" % call, states))
    assert states == ["fill", "use", "use"], states
    e.close()


@pytest.mark.parametrize("dof", [6, 12])
@pytest.mark.parametrize("name", dom.NAMES)
def test_iclm2d(eng, name, dof):
    import oracle
    solver = "iclm2d1" if dof == 6 else "iclm2d2"
    e = (eng.ICLM2D1 if dof == 6 else eng.ICLM2D2)(dom.R2D[0], dom.R2D[1], dom.CONV, dom.STOP2D)
    e.set_images(*dom.images2d(name))
    e.prepare()
    for k, q in enumerate(dom.queues2d(name)):
        for fma, order in ((0, oracle.ORDER_LANES), (1, oracle.ORDER_LANES_FMA)):
            e.set_tuning("arith_fma", fma)
            want = dom.oracle2d(name, solver, q, order)
            for call in (1, 2):
                dom.assert_same(e.compute(q.copy()), want, (name, solver, "fma %d" % fma, "queue %d call %d" % (k, call)))
    e.close()


@pytest.mark.parametrize("name", dom.NAMES)
def test_nr2d1(eng, name):
    import oracle
    e = eng.NR2D1(dom.R2D[0], dom.R2D[1], dom.CONV, dom.STOP2D)
    e.set_images(*dom.images2d(name))
    e.prepare()
    for k, q in enumerate(dom.queues2d(name)):
        want = dom.oracle2d(name, "nr2d1", q, oracle.ORDER_LANES)
        for call in (1, 2):
            dom.assert_same(e.compute(q.copy()), want, (name, "nr2d1", "queue %d call %d" % (k, call)))
    e.close()


@pytest.mark.parametrize("dof", [6, 12])
@pytest.mark.parametrize("name", ["u16", "dark"])
def test_icgn2d_center_offsets_and_self_adaptive(eng, name, dof):
    import oracle
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    e = _icgn2d(eng, name, dof)
    _, q = dom.queues2d(name)
    off = dom.center_offsets2d(len(q))
    dom.assert_same(e.compute_with_offsets(q.copy(), off), dom.oracle2d(name, solver, q, oracle.ORDER_LANES, center_offsets=off),
                    (name, solver, "offsets"))
    e.set_self_adaptive(True)
    sa = dom.with_radii(q)
    dom.assert_same(e.compute(sa.copy()), dom.oracle2d(name, solver, sa, oracle.ORDER_LANES, self_adaptive=True),
                    (name, solver, "self-adaptive"))
    e.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_u16_wide_subsets(eng, dof):
    """41 x 41 samples of `u16`: the reference-mean sum passes 2^24 and rounds (image_domains.R_WIDE2D) -- its association shows."""
    import oracle
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    q = dom.wide_queue2d(*dom.images2d("u16"))
    for variant in (None, 5 if dof == 6 else 4):
        e = _icgn2d(eng, "u16", dof, r=dom.R_WIDE2D, variant=variant)
        for fma, order in ((0, oracle.ORDER_LANES), (1, oracle.ORDER_LANES_FMA)):
            e.set_tuning("arith_fma", fma)
            want = dom.oracle2d("u16", solver, q, order, r=dom.R_WIDE2D)
            for call in (1, 2):
                dom.assert_same(e.compute(q.copy()), want, (solver, "variant %s fma %d call %d" % (variant, fma, call)))
        e.close()


# ---- ICGN3D1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dom.NAMES)
def test_icgn3d1_three_contracts(eng, name):
    """Default against GPU_ORDER_3D, arith_fma against ORDER_LANES_FMA, arith_onepass3d against its CPU twin."""
    import oracle
    import onepass3d_twin as twin
    prep = dom.prepared3d(name)
    e = eng.ICGN3D1(dom.R3D[0], dom.R3D[1], dom.R3D[2], dom.CONV, dom.STOP3D)
    e.set_images(*dom.images3d(name))
    e.prepare()
    for k, q in enumerate(dom.queues3d(name)):
        e.set_tuning("arith_onepass3d", 0)
        e.set_tuning("arith_fma", 0)
        dom.assert_same(e.compute(q.copy()), dom.oracle3d(name, q, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D), (name, "default", k))
        e.set_tuning("arith_fma", 1)
        dom.assert_same(e.compute(q.copy()), dom.oracle3d(name, q, oracle.ORDER_LANES_FMA, oracle.GPU_LANES_3D), (name, "arith_fma", k))
        e.set_tuning("arith_onepass3d", 1)
        want = twin.icgn3d1(prep, dom.R3D[0], dom.R3D[1], dom.R3D[2], dom.CONV, dom.STOP3D, q.copy())
        dom.assert_same(e.compute(q.copy()), want, (name, "arith_onepass3d", k))
    e.close()


# ---- float64 model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["2D2", "3D"])
@pytest.mark.parametrize("name", dom.ROUNDING)
def test_default_contract_within_the_bars_of_the_float64_model(eng, name, family):
    """ICGN2D2 / ICGN3D1, ordinary run, against tests/icgn_model64.py: flags and iteration counts identical (with the one
    exception of image_domains.model_distance), every field group within the domain's bar -- 4 x the compiled reference's measured
    distance on `pedestal`, where float32 loses to the offset what the model keeps; the 8-bit bars on `u16` and `unit` except
    where the reference itself is farther than a quarter of them at these smaller radii."""
    r, ref, tar, _, pois, _, _ = dom.model_case(name, family)
    e = eng.ICGN2D2(r[0], r[1], dom.CONV, dom.STOP2D) if family == "2D2" else eng.ICGN3D1(r[0], r[1], r[2], dom.CONV, dom.STOP3D)
    e.set_images(ref, tar)
    e.prepare()
    got = e.compute(pois.copy())
    e.close()
    used, dist = dom.model_distance(name, family, got)
    bars = dom.model_bars(name, family)
    print(name, family, "exceptions used %d of %d;" % (used, len(pois)), {g: "%.3e (bar %.3e)" % (dist[g], bars[g]) for g in dist})
    assert all(dist[g] <= bars[g] for g in dist), (dist, bars)
    assert used <= dom.MODEL_EXCEPTIONS[name][family] + dom.MODEL_EXCEPTION_MARGIN

"""The intensity domains of tests/image_domains.py on the oracle alone (CPU, runs everywhere).

What tests/test_gpu_domains.py relies on is asserted here, where no GPU and no reference tree is needed: the images are what the
table says, and no domain passes emptily -- the rounding domains converge and SEE an association (ORDER_SEQ and ORDER_LANES differ
in their bits), `dark` has the -3 rule decide in both directions, `flat` produces NaN ZNCC and failed solver records, `signed` is
rejected by ICGN and solved by NR2D1 / IC-LM.  tests/test_oracle_vs_ref_domains.py asserts the same on the compiled reference.
"""
import numpy as np
import pytest

import image_domains as dom
import oracle

Z2, Z3 = oracle.P2["zncc"], oracle.P3["zncc"]


def test_images_are_what_the_table_says():
    for images, flat, shape in ((dom.images2d, dom.FLAT2D, dom.SHAPE2D), (dom.images3d, dom.FLAT3D, dom.SHAPE3D)):
        for name in dom.NAMES:
            for a in images(name):
                assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape and np.isfinite(a).all(), name
        for a in images("u16"):
            assert (a == np.round(a)).all() and a.min() >= 0 and a.max() <= 65535 and a.max() > 30000
        for a in images("unit"):
            assert 0 < a.max() <= 1.01
            assert (np.ascontiguousarray(a).view(np.uint32) & 0xFF != 0).mean() > 0.9      # full mantissas
        for a in images("pedestal"):
            assert a.min() > 2.9e7
        for a in images("dark"):
            assert a.min() == 0 and (a < 4).mean() > 0.1 and (a == np.round(a * 2) / 2).all()
        for a in images("flat"):
            assert (a[flat] == dom.FLAT_VALUE).all()
        for a in images("signed"):
            assert (a < 0).mean() > 0.3 and abs(float(a.mean(dtype=np.float64))) < 1e-3
    # u16: where the sum of a subset or a window passes 2^24 -- float32 rounds it -- and where it does not (image_domains.R_WIDE2D)
    ref, _ = dom.images2d("u16")
    xs, ys = dom.grid2d()
    sums = lambda r: np.array([ref[int(y) - r[1]:int(y) + r[1] + 1, int(x) - r[0]:int(x) + r[0] + 1].sum(dtype=np.float64)
                               for x, y in zip(xs, ys) if min(x, y) >= 26 and x < 150 and y < 134])
    assert (sums(dom.R2D) < 2 ** 24).all() and (sums(dom.R_WIDE2D) > 2 ** 24).all()
    ref, _ = dom.images3d("u16")
    assert float(ref.mean(dtype=np.float64)) * (2 * dom.R_GUESS3D) ** 3 > 2 ** 24


@pytest.mark.parametrize("name", dom.ROUNDING)
def test_rounding_domains_converge_and_see_an_association(name):
    for q in dom.queues2d(name):
        for solver in ("icgn2d1", "icgn2d2", "iclm2d1", "nr2d1"):
            seq = dom.oracle2d(name, solver, q, oracle.ORDER_SEQ)
            dom.check_converges(name, seq, Z2, dom.N_CLEAN2D, solver)
            dom.check_orders_differ(seq, dom.oracle2d(name, solver, q, oracle.ORDER_LANES), dom.N_CLEAN2D, (name, solver))
        # the planted records do what they were planted for
        seq = dom.oracle2d(name, "icgn2d1", q, oracle.ORDER_SEQ)
        assert seq[-4:, Z2].tolist()[:3] == [-3.0, -1.0, -4.0] and seq[-1, Z2] > 0.9
    if name == "u16":
        q = dom.wide_queue2d(*dom.images2d(name))
        for solver in ("icgn2d1", "icgn2d2"):
            seq = dom.oracle2d(name, solver, q, oracle.ORDER_SEQ, r=dom.R_WIDE2D)
            dom.check_converges(name, seq, Z2, len(q), solver)
            dom.check_orders_differ(seq, dom.oracle2d(name, solver, q, oracle.ORDER_LANES, r=dom.R_WIDE2D), len(q), (name, solver, "wide"))
    for q in dom.queues3d(name):
        seq = dom.oracle3d(name, q, oracle.ORDER_SEQ)
        dom.check_converges(name, seq, Z3, dom.N_CLEAN3D, "icgn3d1")
        dom.check_orders_differ(seq, dom.oracle3d(name, q, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D), dom.N_CLEAN3D, (name, "icgn3d1"))
        assert seq[-4:, Z3].tolist()[:3] == [-3.0, -1.0, -3.0] and seq[-1, Z3] > 0.9


def test_dark_has_the_minus_3_rule_decide_both_ways():
    for solver in ("icgn2d1", "icgn2d2"):
        both = np.concatenate([dom.oracle2d("dark", solver, q, oracle.ORDER_SEQ)[:dom.N_CLEAN2D] for q in dom.queues2d("dark")])
        dom.check_dark(both, Z2, len(both), solver)
    both = np.concatenate([dom.oracle3d("dark", q, oracle.ORDER_SEQ)[:dom.N_CLEAN3D] for q in dom.queues3d("dark")])
    dom.check_dark(both, Z3, len(both), "icgn3d1")
    # NR2D1 and IC-LM do not apply the rule
    for solver in ("iclm2d1", "nr2d1"):
        for q in dom.queues2d("dark"):
            got = dom.oracle2d("dark", solver, q, oracle.ORDER_SEQ)
            assert not (got[:dom.N_CLEAN2D, Z2] == -3).any()
            dom.check_converges("dark", got, Z2, dom.N_CLEAN2D, solver)


def test_flat_gives_nan_zncc_and_failed_records():
    ref, tar = dom.images2d("flat")
    f = dom.fftcc_queue2d(12, 12)
    oracle.fftcc2d(ref, tar, 12, 12, f)
    qi, _ = dom.queues2d("flat")
    dom.check_flat(f, dom.oracle2d("flat", "icgn2d1", qi, oracle.ORDER_SEQ))
    assert int(np.isnan(qi[:, Z2]).sum()) >= 5          # the solver queue's guesses carry them too
    f3 = dom.fftcc_queue3d()
    oracle.fftcc3d(*dom.images3d("flat"), 6, 6, 6, f3)
    assert np.isnan(f3[:, Z3]).any()


# every FFTCC shape tests/test_gpu_domains.py asks on the border of the flat block: (radii, wide box)
FLAT_BORDER2D = [(12, 12), (16, 16), (20, 20), (9, 11), (32, 4)]
FLAT_BORDER3D = [((6, 6, 6), False), ((5, 6, 4), False), ((14, 14, 14), True), ((16, 16, 16), True)]


def test_flat_border_queues_hold_one_constant_window_and_two():
    """Per shape: at least one record with both windows constant and, in each direction, one with exactly one (the case the
    kernels' `norm == 0` branch exists for), all with NaN ZNCC, the peak at index 0 (u = the truncated guess)."""
    ref, tar = dom.images2d("flat")
    for r in FLAT_BORDER2D:
        q = dom.flat_border_queue2d(*r)
        got = q.copy()
        oracle.fftcc2d(ref, tar, r[0], r[1], got)
        dom.check_flat_border(got, *dom.constant_windows(ref, tar, r, q[:5]), Z2)
        assert np.array_equal(got[:5, oracle.P2["u"]], q[:5, oracle.P2["u"]]) and np.array_equal(got[:5, oracle.P2["v"]], q[:5, oracle.P2["v"]])
        assert np.array_equal(dom.bits(got[5]), dom.bits(q[5]))
    for r, wide in FLAT_BORDER3D:
        ref, tar = dom.flat_wide3d() if wide else dom.images3d("flat")
        q = dom.flat_border_queue3d(r, dom.FLAT_WIDE3D if wide else dom.FLAT3D)
        got = q.copy()
        oracle.fftcc3d(ref, tar, r[0], r[1], r[2], got)
        dom.check_flat_border(got, *dom.constant_windows(ref, tar, r, q), Z3)
        for k in ("u", "v", "w"):
            assert np.array_equal(got[:, oracle.P3[k]], q[:, oracle.P3[k]])
        assert r != (16, 16, 16) or dom.inner16(q).all()
    # (4, 32): a window 64 rows tall, the block has 60 -- no window of that shape is constant, whatever the POI
    assert 2 * 32 > dom.FLAT2D[0].stop - dom.FLAT2D[0].start


def test_signed_is_rejected_by_icgn_and_solved_by_nr_and_iclm():
    for q in dom.queues2d("signed"):
        for solver in ("icgn2d1", "icgn2d2"):
            dom.check_signed_rejected(dom.oracle2d("signed", solver, q, oracle.ORDER_SEQ), Z2, dom.N_CLEAN2D, solver)
        for solver in ("nr2d1", "iclm2d1"):
            dom.check_converges("signed", dom.oracle2d("signed", solver, q, oracle.ORDER_SEQ), Z2, dom.N_CLEAN2D, solver)
    for q in dom.queues3d("signed"):
        dom.check_signed_rejected(dom.oracle3d("signed", q, oracle.ORDER_SEQ), Z3, dom.N_CLEAN3D, "icgn3d1")


def test_bar_tables_are_complete_and_follow_the_rule():
    for name in dom.NAMES:
        for cls, existing in dom.FFTCC_EXISTING_BAR.items():
            d = dom.FFTCC_DISTANCE[name][cls]
            assert dom.fftcc_bar(name, cls) == (existing if d <= existing / 4 else 4 * d)
    for name in dom.ROUNDING:
        for family in ("2D2", "3D"):
            bars = dom.model_bars(name, family)
            assert set(bars) == set(dom.MODEL_DISTANCE[name][family])
            assert all(b >= 4 * dom.MODEL_DISTANCE[name][family][g] * 0.999 for g, b in bars.items())


@pytest.mark.parametrize("name", dom.NAMES)
def test_fftcc_distances_are_the_recorded_ones(name):
    """The oracle's ZNCC against the float64 NumPy restatement stays within the recorded distance (+ 2e-7: a few float32 ulps of a
    quotient near 1, for another libm / BLAS-free NumPy build)."""
    got = dom.measure_fftcc(only=name)[name]
    print(name, got, dom.FFTCC_DISTANCE[name])
    for cls, d in got.items():
        assert d <= dom.FFTCC_DISTANCE[name][cls] + 2e-7, (cls, d)


@pytest.mark.parametrize("family", ["2D2", "3D"])
@pytest.mark.parametrize("name", dom.ROUNDING)
def test_gpu_order_of_the_oracle_within_the_model_bars(name, family):
    """The oracle in the kernels' summation order against the float64 model, within the domain's bars: what
    tests/test_gpu_domains.py asserts of the kernels holds for the order they claim."""
    _, _, _, _, pois, _, _ = dom.model_case(name, family)
    if family == "2D2":
        got = dom.oracle2d(name, "icgn2d2", pois, oracle.GPU_ORDER_2D)
    else:
        got = dom.oracle3d(name, pois, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D)
    used, dist = dom.model_distance(name, family, got)
    bars = dom.model_bars(name, family)
    print(name, family, "exceptions", used, {g: "%.3e / %.3e" % (dist[g], bars[g]) for g in dist})
    assert all(dist[g] <= bars[g] for g in dist), (dist, bars)
    assert used <= dom.MODEL_EXCEPTIONS[name][family] + dom.MODEL_EXCEPTION_MARGIN

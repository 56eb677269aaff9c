"""The oracle against the compiled reference (oracle/_ref/liboc_ref.so) on the intensity domains of tests/image_domains.py.

tests/test_oracle_vs_ref.py pins the oracle on 8-bit speckle only -- where window sums are exact, no interpolated sample comes
near zero and nothing is flat.  Here, per domain, with the bars of that file: gradients and the bicubic / tricubic evaluators bit
for bit; ICGN2D1, ICGN2D2 (plain, with centre offsets, self-adaptive), ICLM2D1 / ICLM2D2 (at most one POI may fork on the powf
ulp), NR2D1 and ICGN3D1: oracle(ORDER_SEQ) == reference in every float of every record, on the integer-guess queue and on the
noisy one; FFTCC2D / FFTCC3D: integers identical, ZNCC within 1e-5 / 1e-4, NaN where the reference has NaN.  The conditions that
keep a domain from passing emptily are asserted on the REFERENCE's results; the reference's distance from the float64 model
(image_domains.MODEL_DISTANCE, from which the GPU bars derive) is re-measured.  Skipped where the reference tree is not mounted.
"""
import numpy as np
import pytest

import image_domains as dom
import oracle
from oracle import ref as oref

pytestmark = pytest.mark.skipif(not oref.available(), reason="reference tree not mounted: oracle/_ref cannot be built")

Z2, Z3 = oracle.P2["zncc"], oracle.P3["zncc"]
ENGINE = {"icgn2d1": 0, "icgn2d2": 1, "iclm2d1": 2, "iclm2d2": 3, "nr2d1": 4}   # oref.ICGN2D1 ... oref.NR2D1


# (domain, solver) whose failed records may differ in the SIGN of a NaN: a zero norm makes 0 / 0, and which operand's NaN an x86
# addition or multiplication hands on depends on the operand order the compiler chose for that expression -- nothing reads it.
NAN_SIGN_FREE = {("flat", "iclm2d1"), ("flat", "iclm2d2"), ("flat", "icgn3d1")}


def _same(got, want, nan_sign_free):
    return dom.same(got, want) if nan_sign_free else dom.bits(got) == dom.bits(want)


def _same_bits(got, want, what="", nan_sign_free=False):
    """The bar of tests/test_oracle_vs_ref.py: the same bits, NaN included.  `nan_sign_free` (the cases of NAN_SIGN_FREE alone):
    where BOTH sides hold NaN the sign bit is not compared."""
    mism = np.argwhere(~_same(got, want, nan_sign_free))
    assert mism.size == 0, (what, "first mismatches (poi, field): %s" % mism[:10].tolist())


def _ref2d(name, solver, q, r=None, **kw):
    ref, tar = dom.images2d(name)
    r = r or dom.R2D
    out = q.copy()
    if solver.startswith("iclm"):
        kw["damping"] = oracle.DEFAULT_DAMPING
    oref.solve2d(ENGINE[solver], ref, tar, r[0], r[1], dom.CONV, dom.STOP2D, out, **kw)
    return out


def _ref3d(name, q):
    ref, tar = dom.images3d(name)
    out = q.copy()
    oref.icgn3d1(ref, tar, dom.R3D[0], dom.R3D[1], dom.R3D[2], dom.CONV, dom.STOP3D, out)
    return out


@pytest.fixture(scope="module")
def solved():
    """{(domain, solver, queue index): the reference's records}: computed once, shared by the tests below, never written to."""
    out = {}
    for name in dom.NAMES:
        for k, q in enumerate(dom.queues2d(name)):
            for solver in dom.SOLVERS2D:
                out[name, solver, k] = _ref2d(name, solver, q)
        for k, q in enumerate(dom.queues3d(name)):
            out[name, "icgn3d1", k] = _ref3d(name, q)
    return out


@pytest.mark.parametrize("name", dom.NAMES)
def test_gradients_and_interpolators(name):
    ref, tar = dom.images2d(name)
    prep, _ = dom.prepared2d(name)
    gx, gy = oref.gradient2d(ref)
    _same_bits(prep.gx, gx, "gx")
    _same_bits(prep.gy, gy, "gy")
    rng = np.random.default_rng(1)
    h, w = tar.shape
    xy = np.stack([rng.uniform(-2, w + 2, 3000), rng.uniform(-2, h + 2, 3000)], 1).astype(np.float32)
    xy[:6] = [[1, 1], [w - 2, 5], [w - 2.0001, 5], [0.9999, 5], [np.nan, 5], [1, h - 2.001]]
    xy[6:1000] = np.round(xy[6:1000])                                   # integer positions: what the value plane holds
    want = oref.bspline2d_eval(tar, xy)
    got = np.array([oracle.bspline2d_eval(prep.lut, x, y) for x, y in xy], dtype=np.float32)
    _same_bits(got, want, "bicubic")
    if name == "signed":               # negative samples other than the out-of-range -1
        assert ((want < 0) & (want != -1)).sum() > 10
    ref, tar = dom.images3d(name)
    prep3 = dom.prepared3d(name)
    dz, dy, dx = tar.shape
    xyz = np.stack([rng.uniform(-1, dx + 1, 2000), rng.uniform(-1, dy + 1, 2000), rng.uniform(-1, dz + 1, 2000)], 1).astype(np.float32)
    xyz[:4] = [[1, 1, 1], [dx - 2, 5, 5], [5, 5, dz - 2.001], [np.nan, 3, 3]]
    xyz[4:700] = np.round(xyz[4:700])
    gx, gy, gz, want = oref.prepare3d(ref, tar, xyz)
    _same_bits(prep3.gx, gx, "gx3")
    _same_bits(prep3.gy, gy, "gy3")
    _same_bits(prep3.gz, gz, "gz3")
    got = np.array([oracle.bspline3d_eval(prep3.coef, *p) for p in xyz], dtype=np.float32)
    _same_bits(got, want, "tricubic")
    if name == "signed":
        assert ((want < 0) & (want != -1)).sum() > 10


@pytest.mark.parametrize("name", dom.NAMES)
def test_fftcc(name):
    ref, tar = dom.images2d(name)
    P = oracle.P2
    for shapes in dom.FFTCC2D_SHAPES.values():
        for rx, ry in shapes:
            q = dom.fftcc_queue2d(rx, ry)
            want, got = q.copy(), q.copy()
            oref.fftcc2d(ref, tar, rx, ry, want)
            oracle.fftcc2d(ref, tar, rx, ry, got)
            dom.check_fftcc(got, want, P, ("u", "v", "u0", "v0"), 1e-5, (name, rx, ry))
            _same_bits(got[-3:], q[-3:], "guarded records stay untouched")
            if name == "flat" and (rx, ry) == (12, 12):
                assert int(np.isnan(want[:, Z2]).sum()) >= 5
    ref, tar = dom.images3d(name)
    P = oracle.P3
    for r in dom.FFTCC3D_SHAPES["3d"]:
        q = dom.fftcc_queue3d()
        want, got = q.copy(), q.copy()
        oref.fftcc3d(ref, tar, r[0], r[1], r[2], want)
        oracle.fftcc3d(ref, tar, r[0], r[1], r[2], got)
        dom.check_fftcc(got, want, P, ("u", "v", "w", "u0", "v0", "w0"), 1e-4, (name, r))


@pytest.mark.parametrize("solver", dom.SOLVERS2D)
@pytest.mark.parametrize("name", dom.NAMES)
def test_2d_solvers_bit_exact(solved, name, solver):
    for k, q in enumerate(dom.queues2d(name)):
        want = solved[name, solver, k]
        got = dom.oracle2d(name, solver, q, oracle.ORDER_SEQ)
        if solver.startswith("iclm"):
            bad = np.unique(np.argwhere(~_same(got, want, (name, solver) in NAN_SIGN_FREE))[:, 0])
            assert len(bad) <= 1, (name, solver, k, "POIs that differ: %s" % bad.tolist())
        else:
            _same_bits(got, want, (name, solver, k))


@pytest.mark.parametrize("solver", ["icgn2d1", "icgn2d2"])
@pytest.mark.parametrize("name", dom.NAMES)
def test_center_offsets_and_self_adaptive_bit_exact(name, solver):
    for k, q in enumerate(dom.queues2d(name)):
        off = dom.center_offsets2d(len(q))
        _same_bits(dom.oracle2d(name, solver, q, oracle.ORDER_SEQ, center_offsets=off), _ref2d(name, solver, q, center_offsets=off),
                   (name, solver, k, "offsets"))
        sa = dom.with_radii(q)
        _same_bits(dom.oracle2d(name, solver, sa, oracle.ORDER_SEQ, self_adaptive=True), _ref2d(name, solver, sa, self_adaptive=True),
                   (name, solver, k, "self-adaptive"))


@pytest.mark.parametrize("solver", ["icgn2d1", "icgn2d2"])
def test_u16_wide_subsets_bit_exact(solver):
    """r = (20, 20): the subset's sum passes 2^24 (image_domains.R_WIDE2D)."""
    q = dom.wide_queue2d(*dom.images2d("u16"))
    want = _ref2d("u16", solver, q, r=dom.R_WIDE2D)
    _same_bits(dom.oracle2d("u16", solver, q, oracle.ORDER_SEQ, r=dom.R_WIDE2D), want, solver)
    dom.check_converges("u16", want, Z2, len(q), solver)
    dom.check_orders_differ(want, dom.oracle2d("u16", solver, q, oracle.ORDER_LANES, r=dom.R_WIDE2D), len(q), solver)


@pytest.mark.parametrize("name", dom.NAMES)
def test_icgn3d1_bit_exact(solved, name):
    for k, q in enumerate(dom.queues3d(name)):
        _same_bits(dom.oracle3d(name, q, oracle.ORDER_SEQ), solved[name, "icgn3d1", k], (name, k), (name, "icgn3d1") in NAN_SIGN_FREE)


def test_fftcc_on_the_border_of_the_flat_block():
    """One window constant, the other textured, per FFTCC shape (image_domains.flat_border_queue2d / 3d): the oracle returns the
    reference's integers and NaN where it has NaN -- the reference's two transforms give an all-zero surface there."""
    from test_oracle_domains import FLAT_BORDER2D, FLAT_BORDER3D
    ref, tar = dom.images2d("flat")
    for r in FLAT_BORDER2D:
        q = dom.flat_border_queue2d(*r)
        want, got = q.copy(), q.copy()
        oref.fftcc2d(ref, tar, r[0], r[1], want)
        oracle.fftcc2d(ref, tar, r[0], r[1], got)
        dom.check_fftcc(got, want, oracle.P2, ("u", "v", "u0", "v0"), 1e-5, ("flat border", r))
        dom.check_flat_border(want, *dom.constant_windows(ref, tar, r, q[:5]), Z2)
    for r, wide in FLAT_BORDER3D:
        ref, tar = dom.flat_wide3d() if wide else dom.images3d("flat")
        q = dom.flat_border_queue3d(r, dom.FLAT_WIDE3D if wide else dom.FLAT3D)
        want, got = q.copy(), q.copy()
        oref.fftcc3d(ref, tar, r[0], r[1], r[2], want)
        oracle.fftcc3d(ref, tar, r[0], r[1], r[2], got)
        dom.check_fftcc(got, want, oracle.P3, ("u", "v", "w", "u0", "v0", "w0"), 1e-4, ("flat border", r))
        dom.check_flat_border(want, *dom.constant_windows(ref, tar, r, q), Z3)


# ---- no domain passes emptily: the conditions on the reference's own results -------------------------------------------------
@pytest.mark.parametrize("name", dom.ROUNDING)
def test_rounding_domains_converge_and_see_an_association(solved, name):
    for k, q in enumerate(dom.queues2d(name)):
        for solver in ("icgn2d1", "icgn2d2", "iclm2d1", "nr2d1"):
            dom.check_converges(name, solved[name, solver, k], Z2, dom.N_CLEAN2D, solver)
            dom.check_orders_differ(solved[name, solver, k], dom.oracle2d(name, solver, q, oracle.ORDER_LANES), dom.N_CLEAN2D, (name, solver))
    for k, q in enumerate(dom.queues3d(name)):
        dom.check_converges(name, solved[name, "icgn3d1", k], Z3, dom.N_CLEAN3D, "icgn3d1")
        dom.check_orders_differ(solved[name, "icgn3d1", k], dom.oracle3d(name, q, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D), dom.N_CLEAN3D,
                                (name, "icgn3d1"))


def test_dark_flat_signed_on_the_reference(solved):
    for solver in ("icgn2d1", "icgn2d2"):
        both = np.concatenate([solved["dark", solver, k][:dom.N_CLEAN2D] for k in (0, 1)])
        dom.check_dark(both, Z2, len(both), solver)
    both = np.concatenate([solved["dark", "icgn3d1", k][:dom.N_CLEAN3D] for k in (0, 1)])
    dom.check_dark(both, Z3, len(both), "icgn3d1")
    ref, tar = dom.images2d("flat")
    f = dom.fftcc_queue2d(12, 12)
    oref.fftcc2d(ref, tar, 12, 12, f)
    dom.check_flat(f, solved["flat", "icgn2d1", 0])
    for k in (0, 1):
        for solver in ("icgn2d1", "icgn2d2"):
            dom.check_signed_rejected(solved["signed", solver, k], Z2, dom.N_CLEAN2D, solver)
        for solver in ("nr2d1", "iclm2d1"):
            dom.check_converges("signed", solved["signed", solver, k], Z2, dom.N_CLEAN2D, solver)
            dom.check_converges("dark", solved["dark", solver, k], Z2, dom.N_CLEAN2D, solver)
            assert not (solved["dark", solver, k][:dom.N_CLEAN2D, Z2] == -3).any()
        dom.check_signed_rejected(solved["signed", "icgn3d1", k], Z3, dom.N_CLEAN3D, "icgn3d1")


@pytest.mark.parametrize("family", ["2D2", "3D"])
@pytest.mark.parametrize("name", dom.ROUNDING)
def test_reference_at_the_recorded_distance_from_the_model(name, family):
    """image_domains.MODEL_DISTANCE was measured from exactly this comparison (the exception is judged with the domain's bar
    here, with no bar while measuring)."""
    used, dist = dom.model_distance(name, family, dom.reference_model_run(name, family))
    print(name, family, "exceptions", used, dist)
    for g, d in dist.items():
        assert d <= dom.MODEL_DISTANCE[name][family][g] * 1.001, (g, d)
    assert used == dom.MODEL_EXCEPTIONS[name][family]

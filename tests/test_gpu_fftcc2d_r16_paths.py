"""The two paths of the 32 x 32 FFTCC2D kernel (fftcc2d_fused.hip) on one queue, and its new body against its old one.

A wave of fftcc2d_fused32x2_kernel serves two POIs.  When every live lane of the wave holds integral x, y, u, v the window rows
are fetched from one per-lane offset plus a scalar row offset; a wave with any fractional value keeps the per-row float
expressions, whose truncations are reference behaviour (src/oc_fftcc.cpp:190-216).  The last inverse pass is a real-output
transform of the rows 0 ... 16 of a Hermitian array.  Tuning "fftcc2d_fused" = 3 launches the body without either change, 4 / 5 the
body with the first / the second alone.

The queue (101 POIs, r = 16) puts every mix into the two halves of one wave: integral next to integral, integral next to a
fractional position whose float sums round (x = 40.5, y = the float below 41; y = 40.99999 elsewhere), an integral position with a fractional guess, integral
guesses of both signs, a POI the guard rejects in either half next to a live one, windows that touch the image border, a POI over
an exactly constant block planted in the reference image, two fractional POIs, and the lone last half-wave.  Asserted, on an 8-bit
speckle pair and on the `u16` pair of tests/image_domains.py:

  * u, v, u0, v0 equal the oracle's exactly; ZNCC within 1.5e-5 of the oracle and 2e-6 of the rocFFT pipeline (the bars of
    tests/test_gpu_parity_2d.py), NaN on the same records; guarded POIs untouched bit for bit; the constant window gives index 0;
  * new body against old body: identical integers; the row stepping moves no bit (3 against 4 and 5 against the default: every
    float of every record, ZNCC included, on the mixed queue and on a queue of integral POIs only).
"""
import numpy as np
import pytest

import image_domains as dom

pytestmark = pytest.mark.gpu

R = 16
N = 101
INTS = ("u", "v", "u0", "v0")
BLOCK = 40          # side of the constant block; its centre is (w - 50, h - 50)
# the float below 41: y + 31 rounds UP to 72, so the last window row is row 56, not trunc(y) - 16 + 31 = 55 (reference behaviour)
Y_ROUNDS = float(np.nextafter(np.float32(41.0), np.float32(0.0)))
I_FRACTIONAL_POS, I_FRACTIONAL_GUESS, I_GUARDED, I_BORDER, I_CONSTANT = 3, 6, (10, 13, 14), (16, 17, 18, 19), 20


def _queue(h, w, integral_only=False):
    """The mixed queue for an h x w pair (records 2i and 2i + 1 are the two halves of one wave), or its integral-only variant."""
    import oracle
    P = oracle.P2
    rows = [
        (60, 60, 0, 0), (100, 70, 0, 0),                                # integral | integral
        (80, 90, 0, 0), (40.5, Y_ROUNDS, 0, 0),                         # integral | fractional position (sums round up)
        (120.25, 57.75, 0, 0), (130, 60, 0, 0),                         # fractional | integral
        (70, 100, 1.5, -0.7), (90, 110, 0, 0),                          # integral position, fractional guess | integral
        (64, 80, 3, -2), (96, 72, -4, 5),                               # integral guesses of both signs
        (3, 80, 0, 0), (110, 64, 0, 0),                                 # guarded in the first half | live
        (72, 66, 0, 0), (88, h - 2, 0, 0),                              # live | guarded in the second half
        (100, 100, 4000, 0), (76, 92, 0, 0),                            # guarded by its guess | live
        (20, 20, -4, -4), (w - 20, h - 20, 3, 3),                       # target windows on the border: pixel 0, pixel w - 2 / h - 2
        (16, 16, 0, 0), (w - 17, h - 17, 0, 0),                         # both windows on the border
        (w - 50, h - 50, 0, 0), (66, 58, 0, 0),                         # the constant reference window | live
        (50.75, 40.99999, 0.25, 2.5), (71.125, 83.9, -1.5, 0.99999),    # fractional | fractional
    ]
    rng = np.random.default_rng(1600 + h)
    while len(rows) < N:
        x, y = float(rng.integers(40, w - 40)), float(rng.integers(40, h - 40))
        u, v = (float(rng.integers(-3, 4)), float(rng.integers(-3, 4))) if len(rows) % 3 == 0 else (0.0, 0.0)
        if len(rows) % 8 == 5:
            x += 0.375
            v += 0.5
        rows.append((x, y, u, v))
    a = np.asarray(rows, dtype=np.float32)
    if integral_only:
        a = np.trunc(a)
    q = oracle.make_pois2d(a[:, 0], a[:, 1])
    q[:, P["u"]], q[:, P["v"]] = a[:, 2], a[:, 3]
    return np.ascontiguousarray(q, dtype=np.float32)


def _pair(name, speckle_small):
    ref, tar = speckle_small if name == "speckle" else dom.images2d("u16")
    ref = ref.copy()
    h, w = ref.shape
    ref[h - 50 - BLOCK // 2:h - 50 + BLOCK // 2, w - 50 - BLOCK // 2:w - 50 + BLOCK // 2] = ref[h - 50, w - 50]
    return ref, np.ascontiguousarray(tar)


@pytest.fixture(scope="module", params=["speckle", "u16"])
def case(request, speckle_small):
    """Images, both queues, the oracle's records and one compute() per kernel body -- made once, shared, never written to."""
    import opencorr_amd
    import oracle
    ref, tar = _pair(request.param, speckle_small)
    h, w = ref.shape
    out = {"name": request.param, "ref": ref, "tar": tar}
    f = opencorr_amd.FFTCC2D(R, R)
    f.set_images(ref, tar)
    for key, q in (("mixed", _queue(h, w)), ("integral", _queue(h, w, integral_only=True))):
        want = q.copy()
        oracle.fftcc2d(ref, tar, R, R, want)
        got = {}
        for body in (1, 0, 3, 4, 5):
            f.set_tuning("fftcc2d_fused", body)
            got[body] = f.compute(q.copy())
        out[key] = dict(base=q, want=want, got=got)
    f.close()
    for d in (out["mixed"], out["integral"]):
        for a in [d["base"], d["want"]] + list(d["got"].values()):
            a.flags.writeable = False
    return out


def _assert_same(a, b, what):
    ok = dom.same(a, b)
    assert ok.all(), (what, "%d floats differ; first (record, field): %s" % (int((~ok).sum()), np.argwhere(~ok)[:8].tolist()))


def test_queue_holds_what_it_claims(case):
    """The planted records are what their comments say (no GPU result is read here)."""
    import oracle
    P = oracle.P2
    q, ref, tar = case["mixed"]["base"], case["ref"], case["tar"]
    h, w = ref.shape
    assert len(q) == N and N % 2 == 1
    x, y, u, v = q[:, P["x"]], q[:, P["y"]], q[:, P["u"]], q[:, P["v"]]
    integral = (x == np.trunc(x)) & (y == np.trunc(y)) & (u == np.trunc(u)) & (v == np.trunc(v))
    halves = {(bool(integral[i]), bool(integral[i + 1])) for i in range(0, N - 1, 2)}
    assert halves == {(True, True), (True, False), (False, True), (False, False)}
    k = np.arange(2 * R, dtype=np.float32)
    assert ((y[I_FRACTIONAL_POS] + k - np.float32(R)).astype(np.int32) != int(y[I_FRACTIONAL_POS]) - R + np.arange(2 * R)).any()
    assert not integral[I_FRACTIONAL_POS] and not integral[I_FRACTIONAL_GUESS] and x[I_FRACTIONAL_GUESS] == np.trunc(x[I_FRACTIONAL_GUESS])
    assert int(x[16] + u[16]) - R == 0 and int(y[16] + v[16]) - R == 0 and int(x[17] + u[17]) + R - 1 == w - 2
    rc, tc = dom.constant_windows(ref, tar, (R, R), q[[I_CONSTANT]])
    assert rc[0] and not tc[0]
    live = np.ones(N, bool)
    live[list(I_GUARDED)] = False
    rc, tc = dom.constant_windows(ref, tar, (R, R), q[live & (np.arange(N) != I_CONSTANT)])
    assert not rc.any() and not tc.any()
    qi = case["integral"]["base"][:, [P["x"], P["y"], P["u"], P["v"]]]
    assert np.array_equal(qi, np.trunc(qi)) and len(qi) == N


@pytest.mark.parametrize("body", [1, 3, 4, 5])
def test_every_body_matches_oracle_and_pipeline(case, body):
    import oracle
    P = oracle.P2
    d = case["mixed"]
    base, want, got, piped = d["base"], d["want"], d["got"][body], d["got"][0]
    for k in INTS:
        assert np.array_equal(got[:, P[k]], want[:, P[k]]), (k, np.flatnonzero(got[:, P[k]] != want[:, P[k]])[:8].tolist())
        assert np.array_equal(got[:, P[k]], piped[:, P[k]]), (k, np.flatnonzero(got[:, P[k]] != piped[:, P[k]])[:8].tolist())
    to_oracle, to_pipeline = dom.zncc_distance(got, want, P["zncc"]), dom.zncc_distance(got, piped, P["zncc"])
    print(case["name"], "body", body, "ZNCC distance: oracle %.3e (bar 1.5e-5), rocFFT pipeline %.3e (bar 2e-6)" % (to_oracle, to_pipeline))
    assert to_oracle <= 1.5e-5
    assert to_pipeline <= 2e-6
    other = [c for c in range(base.shape[1]) if c not in [P[k] for k in INTS] + [P["zncc"]]]
    _assert_same(got[:, other], base[:, other], "fields FFTCC never writes")
    assert np.array_equal(dom.bits(got[list(I_GUARDED)]), dom.bits(base[list(I_GUARDED)]))
    assert np.array_equal(dom.bits(want[list(I_GUARDED)]), dom.bits(base[list(I_GUARDED)]))
    # the constant window: the reference's all-zero surface, arg-max index 0, ZNCC 0 / 0
    assert got[I_CONSTANT, P["u"]] == base[I_CONSTANT, P["u"]] and got[I_CONSTANT, P["v"]] == base[I_CONSTANT, P["v"]]
    assert np.isnan(got[I_CONSTANT, P["zncc"]]) and np.isnan(want[I_CONSTANT, P["zncc"]])
    live = np.ones(N, bool)
    live[list(I_GUARDED) + [I_CONSTANT]] = False
    assert (got[live, P["zncc"]] > 0.5).mean() > 0.8      # most live records correlate: the queue does not pass emptily


@pytest.mark.parametrize("queue", ["mixed", "integral"])
def test_new_body_against_old_body(case, queue):
    """Identical integers; the row stepping (3 -> 4, 5 -> default) moves no bit of any record, ZNCC included."""
    import oracle
    P = oracle.P2
    got = case[queue]["got"]
    for body in (1, 4, 5):
        for k in INTS:
            assert np.array_equal(got[body][:, P[k]], got[3][:, P[k]]), (body, k)
        other = [c for c in range(got[3].shape[1]) if c != P["zncc"]]
        _assert_same(got[body][:, other], got[3][:, other], ("body", body, "everything except ZNCC"))
    _assert_same(got[4], got[3], "row stepping alone against the old body")
    _assert_same(got[1], got[5], "row stepping on top of the real-output last pass")
    print(case["name"], queue, "ZNCC, new body against old body: max |difference| %.3e"
          % dom.zncc_distance(got[1], got[3], P["zncc"]))
    assert dom.zncc_distance(got[1], got[3], P["zncc"]) <= 2e-6

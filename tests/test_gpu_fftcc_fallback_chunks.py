"""The rocFFT fallback of FFTCC2D / FFTCC3D (run_fftcc_rocfft, capi.hip) on queues longer than one of its chunks -- 32 768 POIs
in 2D, 1 024 in 3D -- and on a window no single-kernel path takes.

A queue of two full chunks and 37 POIs cycles 97 distinct POIs (97 is coprime to both chunk sizes: a chunk-offset error lands
on another POI).  The last chunk is a partial one: its windows' tail is cleared and the plans run their full batch.  Every
queue entry must equal what the same engine, with the same tuning, computes for that POI in a call of the 97 alone, and that
call must agree with the oracle under the bars of tests/test_gpu_parity_2d.py::test_fftcc2d_matches_oracle and
tests/test_gpu_parity_3d.py::test_fftcc3d_every_fused_cube.

The POIs of a cycle are chosen by the oracle alone: out of 100 candidates (every third with an integer initial guess) those
whose oracle peak has ZNCC > 0.5, in candidate order; at most one candidate in a hundred may have to be discarded.  The 2D cycle
is 95 of them and two POIs that trip the bounds guard, the 3D cycle (FFTCC3D clamps, it has no guard) 97.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK_2D, CHUNK_3D, CYCLE, CANDIDATES = 32768, 1024, 97, 100
R = 8
SHAPE_3D = (72, 76, 80)  # dz, dy, dx: the volumes of tests/test_gpu_parity_3d.py


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _chosen(cands, done, zncc_col, wanted):
    """The first `wanted` candidates whose oracle peak (`done`: the candidates after the oracle's FFTCC) has ZNCC > 0.5."""
    good = np.flatnonzero(done[:, zncc_col] > 0.5)
    assert len(cands) - len(good) <= len(cands) // 100, ("discarded", len(cands) - len(good), done[:, zncc_col].min())
    assert len(good) >= wanted
    return cands[good[:wanted]].copy()


def _long_queue(cycle, n, mark_col):
    """cycle[k % 97] at queue position k; a field FFTCC never writes carries k itself (exact in float32)."""
    queue = cycle[np.arange(n) % len(cycle)].copy()
    queue[:, mark_col] = np.arange(n, dtype=np.float32)
    return queue


@pytest.fixture(scope="module")
def cycle2d(speckle_small):
    import oracle
    ref, tar = speckle_small
    h, w = ref.shape
    P = oracle.P2
    rng = np.random.default_rng(9701)
    xs = rng.uniform(R + 4, w - R - 4, CANDIDATES).astype(np.float32)
    ys = rng.uniform(R + 4, h - R - 4, CANDIDATES).astype(np.float32)
    xs[::2], ys[::2] = np.floor(xs[::2]), np.floor(ys[::2])
    cands = oracle.make_pois2d(xs, ys)
    # integer initial guesses displace the target window: within a pixel of the pair's displacement (2.3, -1.7), so that a 16 x 16
    # window keeps its overlap (a guess AWAY from it leaves too little of five speckles: 2 - 3 % of such candidates fall below 0.5)
    cands[::3, P["u"]] = rng.integers(1, 4, len(cands[::3]))
    cands[::3, P["v"]] = rng.integers(-3, 0, len(cands[::3]))
    done = cands.copy()
    oracle.fftcc2d(ref, tar, R, R, done)
    guarded = oracle.make_pois2d([3.0, 150.0], [100.0, 2.0])
    cycle = np.concatenate([_chosen(cands, done, P["zncc"], CYCLE - 2), guarded]).astype(np.float32)
    want = cycle.copy()
    oracle.fftcc2d(ref, tar, R, R, want)
    assert np.array_equal(_bits(want[-2:]), _bits(cycle[-2:]))  # the oracle's guard leaves them alone
    return cycle, want


@pytest.fixture(scope="module")
def volumes():
    from opencorr_amd import synth
    return synth.speckle_pair_3d(*SHAPE_3D, seed=21)


@pytest.fixture(scope="module")
def cycle3d(volumes):
    import oracle
    ref, tar = volumes
    dz, dy, dx = ref.shape
    P = oracle.P3
    rng = np.random.default_rng(9703)
    m = R + 4
    xs = rng.uniform(m, dx - m, CANDIDATES).astype(np.float32)
    ys = rng.uniform(m, dy - m, CANDIDATES).astype(np.float32)
    zs = rng.uniform(m, dz - m, CANDIDATES).astype(np.float32)
    xs[::2], ys[::2], zs[::2] = np.floor(xs[::2]), np.floor(ys[::2]), np.floor(zs[::2])
    cands = oracle.make_pois3d(xs, ys, zs)
    cands[::3, P["u"]] = rng.integers(-2, 3, len(cands[::3]))
    cands[::3, P["w"]] = rng.integers(-2, 3, len(cands[::3]))
    done = cands.copy()
    oracle.fftcc3d(ref, tar, R, R, R, done)
    cycle = _chosen(cands, done, P["zncc"], CYCLE)
    want, exact = cycle.copy(), cycle.copy()
    oracle.fftcc3d(ref, tar, R, R, R, want)
    oracle.fftcc3d(ref, tar, R, R, R, exact, exact_sums=True)
    return cycle, want, exact


def _assert_2d_matches_oracle(got, want, base, guarded):
    """The bars of test_fftcc2d_matches_oracle."""
    import oracle
    P = oracle.P2
    for key in ("u", "v", "u0", "v0"):
        assert np.array_equal(got[:, P[key]], want[:, P[key]]), key
    dz = float(np.abs(got[:, P["zncc"]] - want[:, P["zncc"]]).max())
    print("2D ZNCC against the oracle: max |d| = %.3g" % dz)
    assert dz <= 1e-5, dz
    if guarded:
        assert np.array_equal(_bits(got[-guarded:]), _bits(base[-guarded:]))
    untouched = [c for c in range(25) if c not in (P["u"], P["v"], P["u0"], P["v0"], P["zncc"])]
    assert np.array_equal(_bits(got[:, untouched]), _bits(base[:, untouched]))


def test_fftcc2d_fallback_across_chunks(speckle_small, cycle2d):
    import opencorr_amd
    import oracle
    ref, tar = speckle_small
    cycle, want = cycle2d
    P = oracle.P2
    f = opencorr_amd.FFTCC2D(R, R)
    f.set_images(ref, tar)
    f.set_tuning("fftcc2d_fused", 0)
    short = f.compute(cycle.copy())
    _assert_2d_matches_oracle(short, want, cycle, guarded=2)
    n = 2 * CHUNK_2D + 37
    queue = _long_queue(cycle, n, P["feature"])
    got = f.compute(queue.copy())
    k = np.arange(n) % CYCLE
    for key in ("u", "v", "u0", "v0"):
        assert np.array_equal(got[:, P[key]], short[k, P[key]]), key
    dz = float(np.abs(got[:, P["zncc"]] - short[k, P["zncc"]]).max())
    print("2D ZNCC, long queue against the 97-POI call: max |d| = %.3g" % dz)
    assert dz <= 1e-5, dz
    is_guarded = k >= CYCLE - 2
    assert is_guarded.sum() >= 2 * (n // CYCLE) and np.array_equal(_bits(got[is_guarded]), _bits(queue[is_guarded]))
    untouched = [c for c in range(25) if c not in (P["u"], P["v"], P["u0"], P["v0"], P["zncc"])]
    assert np.array_equal(_bits(got[:, untouched]), _bits(queue[:, untouched]))


def test_fftcc3d_fallback_across_chunks(volumes, cycle3d):
    import opencorr_amd
    import oracle
    ref, tar = volumes
    cycle, want, exact = cycle3d
    P = oracle.P3
    keys = ("u", "v", "w", "u0", "v0", "w0")
    untouched = [c for c in range(31) if c not in [P[key] for key in keys + ("zncc",)]]
    f = opencorr_amd.FFTCC3D(R, R, R)
    f.set_images(ref, tar)
    f.set_tuning("fftcc3d_fused", 0)
    short = f.compute(cycle.copy())
    # the bars of test_fftcc3d_every_fused_cube at r <= 12
    for key in keys:
        assert np.array_equal(short[:, P[key]], want[:, P[key]]), key
    dz_exact = float(np.abs(short[:, P["zncc"]] - exact[:, P["zncc"]]).max())
    dz_oracle = float(np.abs(short[:, P["zncc"]] - want[:, P["zncc"]]).max())
    print("3D ZNCC against the oracle: exact sums %.3g, running sums %.3g" % (dz_exact, dz_oracle))
    assert dz_exact <= 1e-4, dz_exact
    assert dz_oracle <= 1e-4, dz_oracle
    assert np.array_equal(_bits(short[:, untouched]), _bits(cycle[:, untouched]))
    n = 2 * CHUNK_3D + 37
    queue = _long_queue(cycle, n, P["feature"])
    got = f.compute(queue.copy())
    k = np.arange(n) % CYCLE
    for key in keys:
        assert np.array_equal(got[:, P[key]], short[k, P[key]]), key
    dz = float(np.abs(got[:, P["zncc"]] - short[k, P["zncc"]]).max())
    print("3D ZNCC, long queue against the 97-POI call: max |d| = %.3g" % dz)
    assert dz <= 2e-5, dz
    assert np.array_equal(_bits(got[:, untouched]), _bits(queue[:, untouched]))


def test_fftcc2d_radius_33_takes_the_fallback_by_default():
    """66 x 66 windows are beyond every single-kernel path: default tuning, and the rocFFT pipeline serves the call.  11 POIs, two
    of them guarded; the pair is the smallest that leaves distinct windows and their integer guesses of up to two pixels inside
    the bounds guard."""
    import opencorr_amd
    import oracle
    from opencorr_amd import synth
    r = 33
    ref, tar = synth.speckle_pair_2d(76, 80, seed=9733)
    h, w = ref.shape
    P = oracle.P2
    rng = np.random.default_rng(9733)
    xs = rng.uniform(r + 2, w - r - 3, 9).astype(np.float32)   # int(x) in 35 ... 44, int(x + u) in 33 ... 46 = width - r - 1
    ys = rng.uniform(r + 2, h - r - 3, 9).astype(np.float32)
    xs[::2], ys[::2] = np.floor(xs[::2]), np.floor(ys[::2])
    inner = oracle.make_pois2d(xs, ys)
    inner[::3, P["u"]] = rng.integers(-2, 3, len(inner[::3]))
    inner[::3, P["v"]] = rng.integers(-2, 3, len(inner[::3]))
    pois = np.concatenate([inner, oracle.make_pois2d([32.0, 40.0], [40.0, 43.0])]).astype(np.float32)   # two guarded ones
    want = pois.copy()
    oracle.fftcc2d(ref, tar, r, r, want)
    assert np.array_equal(_bits(want[-2:]), _bits(pois[-2:])) and (want[:-2, P["zncc"]] > 0.5).all()
    f = opencorr_amd.FFTCC2D(r, r)
    f.set_images(ref, tar)
    got = f.compute(pois.copy())
    _assert_2d_matches_oracle(got, want, pois, guarded=2)

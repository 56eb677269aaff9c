"""The integer-translation sweep of icgn2d.hip (tuning key "icgn2d_int_first"): while a POI's warp is an integer translation --
the first Gauss-Newton iteration of every FFTCC guess -- a sample's interpolated value is read from the VALUE PLANE that
prepare() stores behind the coefficient table (one 4-byte load) instead of four 16-byte gathers and the 16-term polynomial.

Bar everywhere: records BIT-IDENTICAL (uint32 view) between "icgn2d_int_first" = 1 and 0 -- 0 is the kernel's behaviour
before the plane existed -- and, where the oracle reaches, identical to the oracle as well.  The CPU half of the claim is
tests/test_int_first_oracle.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

H, W, R = 640, 720, 16
X, Y, U, UX, V, ZNCC, ITER = 0, 1, 2, 3, 8, 16, 17


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _make_case():
    """Device-resident speckle pair and an FFTCC-initialised queue of 34 000 POIs (>= 32 768: variants 5 / 4 are taken by
    themselves)."""
    import torch
    import opencorr_amd
    from opencorr_amd import synth
    dev = torch.device("cuda", 0)
    ref, tar = synth.speckle_pair_2d(H, W, seed=20260925, device=dev)
    xs, ys = synth.poi_grid_2d(H, W, 200, 170, 26)
    start = opencorr_amd.make_pois2d(xs, ys)
    assert len(start) == 34000
    f = opencorr_amd.FFTCC2D(R, R)
    f.set_images(ref, tar)
    q = torch.from_numpy(start).to(dev)
    f.compute(q)
    torch.cuda.synchronize()
    start = q.cpu().numpy()
    f.close()
    # what makes every POI of this queue eligible: integral coordinates, an integral guess, zero gradients
    ok = start[:, ZNCC] >= 0
    assert ok.mean() > 0.95
    assert (start[:, [X, Y, U, V]] == np.trunc(start[:, [X, Y, U, V]])).all()
    assert (start[:, [3, 4, 9, 10]] == 0).all()
    return dict(dev=dev, ref=ref, tar=tar, start=start)


@pytest.fixture(scope="module")
def case():
    return _make_case()


def _engine(case, dof, int_first, fma=0, cache=1, variant=-1, tar=None, tile_px=None):
    import opencorr_amd
    e = (opencorr_amd.ICGN2D1 if dof == 6 else opencorr_amd.ICGN2D2)(R, R, 0.001, 10)
    e.set_tuning("icgn2d_int_first", int_first)
    e.set_tuning("icgn2d_setup_cache", cache)
    e.set_tuning("arith_fma", fma)
    e.set_tuning("icgn2d_variant", variant)
    if tile_px is not None:
        e.set_tuning("icgn2d_tile_px", tile_px)
    e.set_images(case["ref"], case["tar"] if tar is None else tar)
    e.prepare()
    return e


def _run(case, e, q):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(q)).to(case["dev"])
    e.compute(t)
    state = e.setup_cache_last()
    torch.cuda.synchronize()
    return t.cpu().numpy(), state


def _oracle(case, dof, fma, q, tar=None):
    import oracle
    prep = oracle.Prepared2D(case["ref"].cpu().numpy(), (case["tar"] if tar is None else tar).cpu().numpy())
    want = np.ascontiguousarray(q).copy()
    fn = oracle.icgn2d1 if dof == 6 else oracle.icgn2d2
    fn(prep, R, R, 0.001, 10, want, order=oracle.ORDER_LANES_FMA if fma else oracle.ORDER_LANES, lanes=64)
    return want


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_big_queue_fill_and_use_calls_same_bits_key_on_and_off(case, dof, fma):
    on, off = _engine(case, dof, 1, fma), _engine(case, dof, 0, fma)
    start = case["start"]
    states = []
    for _ in range(3):
        want, s0 = _run(case, off, start)
        got, s1 = _run(case, on, start)
        states.append((s0, s1))
        assert _same(got, want)
    assert states == [("fill", "fill"), ("use", "use"), ("use", "use")]
    assert (want[:, ZNCC] > 0.9).mean() > 0.95
    # ... and with the cache off (every call computes its set-up in front of the sweeps)
    on.set_tuning("icgn2d_setup_cache", 0)
    got, s = _run(case, on, start)
    assert s == "none" and _same(got, want)
    # the oracle on every 23rd POI
    pick = start[::23]
    assert _same(got[::23], _oracle(case, dof, fma, pick))
    on.close()
    off.close()


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("variant", [1, 2, 3, 7])
@pytest.mark.parametrize("dof", [6, 12])
def test_small_queue_variants_same_bits_key_on_and_off(case, dof, variant, fma):
    """The walking variants (no coordinate table) take the same branch with the offset formed from the sample walk."""
    q = case["start"][5000:8000]
    on, off = _engine(case, dof, 1, fma, variant=variant), _engine(case, dof, 0, fma, variant=variant)
    want, _ = _run(case, off, q)
    got, _ = _run(case, on, q)
    assert _same(got, want)
    assert _same(got[::7], _oracle(case, dof, fma, q[::7]))
    on.close()
    off.close()


def _mixed_queue(start, solved):
    """Every eight consecutive POIs mix what takes the short body with what must not, and every kind of early leaver."""
    q = start.copy()
    slot = np.arange(len(q)) % 8
    # 0, 7: FFTCC guesses as they are
    q[slot == 1, U] += 0.25                                # non-integer u
    q[slot == 2, UX] = 0.01                                # non-zero ux
    q[slot == 3, X] += 0.5                                 # non-integral x
    g = slot == 4                                          # guard failures: zncc < 0, NaN u, |v| >= height
    q[g & (np.arange(len(q)) % 24 == 4), ZNCC] = -2.0
    q[g & (np.arange(len(q)) % 24 == 12), U] = np.nan
    q[g & (np.arange(len(q)) % 24 == 20), V] = float(H)
    q[slot == 5, U] = float(W - 30)                        # an integer translation whose corners leave the image: abort after the test
    one = slot == 6                                        # starts converged: stops after one iteration (full sweep)
    q[one, 2:14] = solved[one, 2:14]
    return q, slot


def _mixed_main(dof, fma):
    """Body of test_mixed_workgroups (run in a child process under a time limit of its own)."""
    case = _make_case()
    start = case["start"]
    solver = _engine(case, dof, 0, fma)
    solved, _ = _run(case, solver, start)
    solver.close()
    q, slot = _mixed_queue(start, solved)
    # tile_px = 0: queue order, so eight consecutive POIs ARE one workgroup; the default schedule is run as well
    for tile_px in (0, None):
        on, off = _engine(case, dof, 1, fma, tile_px=tile_px), _engine(case, dof, 0, fma, tile_px=tile_px)
        want, s = _run(case, off, q)
        assert s == "fill"
        assert (want[slot == 5, ZNCC] == -3.0).all()
        assert (want[slot == 4, ZNCC] < 0).all()
        ok = (slot == 6) & (want[:, ZNCC] > 0)
        assert (want[ok, ITER] <= (1 if dof == 6 else 3)).mean() > 0.9
        for k in (0, 1, 2, 7):
            assert (want[slot == k, ZNCC] > 0.9).mean() > 0.9, k
        for expect in ("fill", "use", "use"):
            got, s = _run(case, on, q)
            assert s == expect and _same(got, want), (tile_px, expect)
        # the plain queue right behind it: every wave on the short body.  Its coordinates differ from the mixed queue's (slot 3
        # was moved by half a pixel), so the first call rebuilds the set-up records and the second starts from them
        want2, _ = _run(case, off, start)
        for expect in ("fill", "use"):
            got2, s = _run(case, on, start)
            assert s == expect, (tile_px, s, expect)
            assert _same(got2, want2), (tile_px, expect)
        on.close()
        off.close()
    # a queue the oracle reaches, in 8-wave table workgroups by name (960 POIs: queue order)
    small, sslot = q[:960], slot[:960]
    want = _oracle(case, dof, fma, small)
    assert (want[sslot == 5, ZNCC] == -3.0).all()
    variant = 5 if dof == 6 else 4
    for key in (1, 0):
        e = _engine(case, dof, key, fma, variant=variant)
        for _ in range(3):
            got, _ = _run(case, e, small)
            assert _same(got, want), key
        e.close()
    print("mixed ok")


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_mixed_workgroups_keep_the_barrier_sequence(dof, fma):
    """The lockstep test of test_icgn2d_lockstep_barriers_with_mixed_wave_lifetimes with the new axis: waves on the short body
    and waves on the full sweep share workgroups with every kind of early leaver.  Both bodies sit inside ONE group loop, so
    the sweep barriers pair as before; a mismatch would hang, hence the child process and its time limit."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "mixed", str(dof), str(fma)], cwd=ROOT, capture_output=True,
                         text=True, timeout=420)
    assert out.returncode == 0 and "mixed ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def _special_target(case):
    """The target with a NaN, an Inf, a -0.0 and a block of 3e38 pixels (their coefficients overflow) inside subsets."""
    tar = case["tar"].clone()
    tar[100, 120] = float("nan")
    tar[100, 300] = float("inf")
    tar[200, 150] = -0.0
    tar[200:203, 400:403] = 3e38
    tar[300, 500] = -0.0
    tar[299:302, 499] = 0.0
    return tar


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_special_values_same_bits_key_on_and_off(case, dof, fma):
    import torch
    tar = _special_target(case)
    torch.cuda.synchronize()
    start = case["start"]
    on, off = _engine(case, dof, 1, fma, tar=tar), _engine(case, dof, 0, fma, tar=tar)
    for expect in ("fill", "use"):
        want, _ = _run(case, off, start)
        got, s = _run(case, on, start)
        assert s == expect and _same(got, want)
    # the special pixels did reach subsets: some POIs end differently than on the clean target
    clean = _engine(case, dof, 0, fma)
    base, _ = _run(case, clean, start)
    assert 4 <= (_bits(base) != _bits(want)).any(axis=1).sum() < 2000
    clean.close()
    # the small-queue shape, and the oracle, on the POIs around the special pixels
    near = np.zeros(len(start), dtype=bool)
    for (py, px) in ((100, 120), (100, 300), (200, 150), (201, 401), (300, 500)):
        near |= (np.abs(start[:, X] - px) <= R + 8) & (np.abs(start[:, Y] - py) <= R + 8)
    q = start[near]
    assert len(q) >= 20
    w2, _ = _run(case, off, q)
    g2, _ = _run(case, on, q)
    assert _same(g2, w2) and _same(g2, want[near])
    on.close()
    off.close()


def _poly_at_zero(lut):
    """The 16-term left-to-right polynomial of lut_poly at dx = dy = 0, separately rounded, in float32."""
    z = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        v = lut[..., 0].copy()
        for k in range(4):
            for l in range(4):
                if k == 0 and l == 0:
                    continue
                c = lut[..., 4 * k + l]
                term = c * z if (k == 0 or l == 0) else (c * z) * z
                v = v + term
    return v


def test_value_plane_equals_the_polynomial_at_zero_fractions(case):
    """Special values included: NaN where the polynomial is NaN, the same bits everywhere else."""
    import torch
    tar = _special_target(case)
    torch.cuda.synchronize()
    e = _engine(case, 6, 1, tar=tar)
    lut, val = e.read_field("lut"), e.read_field("lut_val")
    assert val.shape == (H, W)
    want = _poly_at_zero(lut)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(val))
    assert nan.sum() >= 16 + 16              # the 4 x 4 neighbourhoods of the NaN and of the Inf pixel (0 * Inf), at least
    assert np.isnan(val[199:204, 399:404]).any()   # ... and overflowing coefficients (Inf * 0) around the 3e38 block
    assert np.array_equal(_bits(val)[~nan], _bits(want)[~nan])
    # -0.0 pixels come out as +0.0 (the sum that forms a coefficient starts from +0): what reading the image instead would miss
    assert _bits(val)[200, 150] == 0 and _bits(val)[300, 500] == 0
    t = tar.cpu().numpy()
    assert _bits(t)[300, 500] == 0x80000000
    # a finite pixel whose neighbourhood holds an Inf: the coefficient is NaN although the pixel is finite
    assert np.isfinite(t[101, 301]) and np.isnan(val[101, 301])
    e.close()


def test_value_plane_of_a_small_image():
    """The new field against the oracle at every interior integer point, against the table, the image and the zero border."""
    import oracle
    import opencorr_amd
    h, w = 41, 52
    rng = np.random.default_rng(11)
    ref = rng.uniform(0, 255, (h, w)).astype(np.float32)
    tar = rng.uniform(0, 255, (h, w)).astype(np.float32)
    for cls in (opencorr_amd.ICGN2D1, opencorr_amd.ICGN2D2):
        e = cls(4, 4, 0.001, 10)
        e.set_images(ref, tar)
        e.prepare()
        lut, val = e.read_field("lut"), e.read_field("lut_val")
        assert lut.shape == (h, w, 16) and val.shape == (h, w)
        olut = oracle.bspline2d_lut(tar)
        assert np.array_equal(_bits(lut), _bits(olut))
        inner = (slice(1, h - 2), slice(1, w - 2))
        ev = np.array([[oracle.bspline2d_eval(olut, x, y) for x in range(1, w - 2)] for y in range(1, h - 2)], dtype=np.float32)
        assert np.array_equal(_bits(val[inner]), _bits(ev))
        assert np.array_equal(_bits(val), _bits(lut[..., 0]))
        assert np.array_equal(_bits(val[inner]), _bits(tar[inner]))
        border = np.ones((h, w), dtype=bool)
        border[inner] = False
        assert (_bits(val)[border] == 0).all()
        e.close()


def test_engines_without_a_plane_refuse_the_field():
    import opencorr_amd
    rng = np.random.default_rng(5)
    ref = rng.uniform(0, 255, (64, 64)).astype(np.float32)
    e = opencorr_amd.NR2D1(8, 8, 0.001, 10)
    e.set_images(ref, ref)
    e.prepare()
    assert e.read_field("lut").shape == (64, 64, 16)
    with pytest.raises(Exception):
        e.read_field("lut_val")
    e.close()


if __name__ == "__main__":
    assert sys.argv[1] == "mixed"
    _mixed_main(int(sys.argv[2]), int(sys.argv[3]))

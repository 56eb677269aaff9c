"""The planted-peak queues of tests/fftcc_peak_cases.py on the CPU: are the closed-form expectations right, do the queues reach every
branch of the decode, does the oracle find every planted peak, and would the slips these queues are for show?

(a) the closed form against an independent float64 model (numpy's FFT over the reshaped buffer, first maximum, the reference's decode):
    same integers, peak height 1 to 1e-9, runner-up at most half the peak -- the margin that makes the integers a fair demand on a
    float32 transform;  (b) every seam value of every axis is planted in every shape;  (c) the oracle gives the expected integers on
    every record of every shape the GPU test runs;  (d) five slips planted in a NumPy restatement of the tail, counted on these queues
    and on the speckle inputs of test_fftcc2d_every_fused_shape / test_fftcc3d_every_fused_cube (DESIGN.md section 3 keeps the table).
"""
import numpy as np
import pytest

import fftcc_peak_cases as pc
import oracle
from test_oracle_fftcc_numpy import fftcc2d_numpy

CPU2D = [(4, 4), (5, 5), (7, 7), (8, 8), (16, 16), (4, 32), (32, 4), (7, 15), (12, 20), (8, 10)]
CPU3D = [(4, 4, 4), (5, 5, 5), (8, 8, 8), (4, 6, 8), (8, 5, 4), (14, 14, 14), (16, 16, 16)]
RUNNER_UP_CAP = 0.5


def fftcc3d_numpy(ref, tar, radii, x, y, z, g):
    """tests/test_oracle_fftcc_numpy.py's model with three radii: the window's floats, filled x-fastest, transformed as the array
    [2rx][2ry][2rz] (src/oc_fftcc.cpp:68-70, 349-360) and the peak's buffer index decoded as a window position (:401-416)."""
    idx = [(np.float32(p) + np.arange(2 * r, dtype=np.float32) - np.float32(r)).astype(np.int64) for p, r in zip((x, y, z), radii)]
    tdx = [(np.float32(p) + np.arange(2 * r, dtype=np.float32) - np.float32(r) + np.float32(gg)).astype(np.int64)
           for p, r, gg in zip((x, y, z), radii, g)]
    rwin = ref[np.ix_(idx[2], idx[1], idx[0])].astype(np.float64)
    twin = tar[np.ix_(tdx[2], tdx[1], tdx[0])].astype(np.float64)
    rwin -= rwin.mean()
    twin -= twin.mean()
    shape = tuple(2 * r for r in radii)
    a, b = rwin.reshape(-1).reshape(shape), twin.reshape(-1).reshape(shape)
    surf = np.fft.irfftn(np.conj(np.fft.rfftn(a)) * np.fft.rfftn(b), s=shape, axes=(0, 1, 2)).reshape(-1)
    k = int(np.argmax(surf))
    d = [int(v) for v in pc.decode3d(k, *radii)]
    zncc = surf[k] / np.sqrt((rwin ** 2).sum() * (twin ** 2).sum())
    return [d[a] + g[a] for a in range(3)], zncc, surf


def _runner_up(surf):
    top = np.partition(surf, -2)[-2:]
    return top[0] / top[1]


# every shape plain; guesses and fractional positions (the generator's window offsets) on a square and a rectangular one
CASES2D = [(r, (0, 0), 0.0) for r in CPU2D] + [(r, g, f) for r in [(16, 16), (7, 15)] for g, f in [((3, -2), 0.5), ((-1.75, 2.25), 0.0)]]
CASES3D = [(r, (0, 0, 0), 0.0) for r in CPU3D] + [(r, (2, -1, 1.5), 0.25) for r in [(5, 5, 5), (4, 6, 8)]]


@pytest.mark.parametrize("radii,guess,frac", CASES2D)
def test_closed_form_2d_against_the_float64_model(radii, guess, frac):
    rx, ry = radii
    ref, tar, queue, expected = pc.queue2d(rx, ry, guess, frac)
    assert ref.nbytes <= pc.MAX_BYTES and len(queue) == min(4 * rx * ry, pc.LIMIT2D)
    P = pc.P2
    worst = 0.0
    for i in range(len(queue)):
        u, v, zncc, surf = fftcc2d_numpy(ref, tar, rx, ry, queue[i, P["x"]], queue[i, P["y"]], queue[i, P["u"]], queue[i, P["v"]])
        assert (np.float32(u), np.float32(v)) == (expected[i, P["u"]], expected[i, P["v"]]), (i, u, v, expected[i])
        assert abs(zncc - 1.0) <= 1e-9
        worst = max(worst, _runner_up(surf))
    assert worst <= RUNNER_UP_CAP, worst


@pytest.mark.parametrize("radii,guess,frac", CASES3D)
def test_closed_form_3d_against_the_float64_model(radii, guess, frac):
    ref, tar, queue, expected = pc.queue3d(*radii, guess, frac)
    m = 8 * radii[0] * radii[1] * radii[2]
    assert ref.nbytes <= pc.MAX_BYTES and len(queue) == (m if m <= 1024 else min(pc.LIMIT3D, pc.records_that_fit([2 * r for r in radii])))
    P = pc.P3
    worst = 0.0
    for i in (range(len(queue)) if m <= 1024 else pc.sample(len(queue), 96)):
        g = [queue[i, P[k]] for k in "uvw"]
        d, zncc, surf = fftcc3d_numpy(ref, tar, radii, queue[i, P["x"]], queue[i, P["y"]], queue[i, P["z"]], g)
        assert [np.float32(v) for v in d] == [expected[i, P[k]] for k in "uvw"], (i, d, expected[i])
        assert abs(zncc - 1.0) <= 1e-9
        worst = max(worst, _runner_up(surf))
    assert worst <= RUNNER_UP_CAP, worst


def test_every_seam_value_is_planted_on_every_axis_of_every_shape():
    """Per shape: the six seam values on each axis of the plan's array (where the transforms' rows and columns are) AND on each
    component of the decode (raw, before the wrap: r stays, r + 1 wraps).  On cubes and squares the two are the same thing."""
    shapes = {r for fam in pc.FAMILIES2D.values() for r in fam} | {r for fam in pc.FAMILIES3D.values() for r in fam}
    shapes |= set(CPU2D) | set(CPU3D)
    for radii in sorted(shapes):
        shape = tuple(2 * r for r in radii)
        ks = pc.positions(shape, pc.SEED)
        assert len(set(ks.tolist())) == len(ks)
        for raw, n in zip(np.unravel_index(ks, shape), shape):
            assert set(pc.seam(n)) <= set(raw.tolist()), (radii, "plan", n)
        for raw, n in zip(np.unravel_index(ks, shape[::-1]), shape[::-1]):
            assert set(pc.seam(n)) <= set(raw.tolist()), (radii, "decode", n)
        local = pc.decode2d(ks, *radii) if len(radii) == 2 else pc.decode3d(ks, *radii)
        for d, r in zip(local, radii):      # the decoded values on both sides of the wrap
            assert {r, -r + 1, 0, 1, -1, r - 1} <= set(d.tolist()), (radii, r)


def test_every_family_has_a_bar_and_the_2d_bars_catch_one_wrong_bin():
    """A rolled copy puts 1 / M of the peak into every frequency bin: the 2D bars lie below that at each family's largest window.
    (In 3D the share of one bin falls below float32 rounding of the sums from about 22^3 on: the integers carry that check there.)"""
    for nd, fams in ((2, pc.FAMILIES2D), (3, pc.FAMILIES3D)):
        for family, shapes in fams.items():
            largest = max(int(np.prod([2 * r for r in radii])) for radii in shapes)
            assert 0.0 < pc.bar(nd, family) <= pc.EXACT_BAR[nd]
            assert nd == 3 or pc.bar(nd, family) < 1.0 / largest, (family, pc.bar(nd, family), largest)


def _check_oracle(nd, radii):
    ref, tar, queue, expected = (pc.queue2d if nd == 2 else pc.queue3d)(*radii)
    got = queue.copy()
    (oracle.fftcc2d if nd == 2 else oracle.fftcc3d)(ref, tar, *radii, got)
    P = pc.P2 if nd == 2 else pc.P3
    out = pc.OUT2D if nd == 2 else pc.OUT3D
    ints = [c for c in out if c != P["zncc"]]
    assert np.array_equal(got[:, ints], expected[:, ints]), (radii, np.flatnonzero((got[:, ints] != expected[:, ints]).any(axis=1))[:8])
    rest = [c for c in range(queue.shape[1]) if c not in out]
    assert np.array_equal(got[:, rest].view(np.uint32), queue[:, rest].view(np.uint32))
    return float(np.abs(got[:, P["zncc"]].astype(np.float64) - 1.0).max())


@pytest.mark.parametrize("family", sorted(pc.FAMILIES2D))
def test_oracle_finds_every_planted_peak_2d(family):
    worst = max(_check_oracle(2, radii) for radii in pc.FAMILIES2D[family])
    assert worst <= 1e-4, worst          # (its float32 running sums over up to 5 760 grey levels: no bar of the pull request, the integers are)


@pytest.mark.parametrize("family", sorted(pc.FAMILIES3D))
def test_oracle_finds_every_planted_peak_3d(family):
    worst = max(_check_oracle(3, radii) for radii in pc.FAMILIES3D[family])
    assert worst <= (5e-4 if family == "planes" else 2e-4), worst     # the reference's running float32 sums: test_fftcc3d_every_fused_cube (ii)


# ---- (d) planted slips -------------------------------------------------------------------------------------------------------------
def surfaces(ref, tar, radii, queue):
    """The float64 correlation surfaces of a queue, (n, M), divided by the norms: what the tail scans."""
    nd = len(radii)
    P = pc.P2 if nd == 2 else pc.P3
    out = []
    for first in range(0, len(queue), 64):
        q = queue[first:first + 64]
        n = len(q)
        wins = []
        for img, with_guess in ((ref, False), (tar, True)):
            idx = []
            for name, gname, r in zip("xyz", "uvw", radii):
                c = q[:, P[name]].astype(np.float32)[:, None] + np.arange(2 * r, dtype=np.float32)[None, :] - np.float32(r)
                if with_guess:
                    c = c + q[:, P[gname]].astype(np.float32)[:, None]
                idx.append(c.astype(np.int64))
            if nd == 2:
                w = img[idx[1][:, :, None], idx[0][:, None, :]]
            else:
                w = img[idx[2][:, :, None, None], idx[1][:, None, :, None], idx[0][:, None, None, :]]
            w = w.reshape(n, -1).astype(np.float64)
            wins.append(w - w.mean(axis=1, keepdims=True))
        shape = tuple(2 * r for r in radii)
        axes = tuple(range(1, nd + 1))
        a, b = (w.reshape((n,) + shape) for w in wins)
        s = np.fft.irfftn(np.conj(np.fft.rfftn(a, axes=axes)) * np.fft.rfftn(b, axes=axes), s=shape, axes=axes).reshape(n, -1)
        out.append(s / np.sqrt((wins[0] ** 2).sum(axis=1) * (wins[1] ** 2).sum(axis=1))[:, None])
    return np.concatenate(out)


SLIPS = ("ge", "side", "swap", "conj", "half")


def tail(surf, radii, slip=None):
    """The reference's tail (src/oc_fftcc.cpp:246-266, 391-416) on surfaces (n, M), with one slip planted:
    "ge": `>=` for `>` in the decode;  "side": the window's second side for its first in the decode (sh for sw, ny for nx);
    "swap": row and column exchanged when the winner's position is put back into a linear index;  "conj": the conjugate on the wrong
    factor (the surface of the exchanged pair: the peak at -s);  "half": the upper half of the rows never merged into the result."""
    nd = len(radii)
    sides = [2 * r for r in radii]                  # x, y[, z]
    shape = tuple(sides)                            # the plan's array
    n, m = surf.shape
    if slip == "conj":
        s = surf.reshape((n,) + shape)
        for ax in range(1, nd + 1):
            s = np.roll(np.flip(s, axis=ax), 1, axis=ax)
        surf = s.reshape(n, m)
    idx = np.argmax(surf[:, :m // 2] if slip == "half" else surf, axis=1)     # the first maximum, like the strict '>' scan
    if slip == "swap":
        col, row, rest = idx % sides[0], (idx // sides[0]) % sides[1], idx // (sides[0] * sides[1])
        idx = (rest * sides[0] + col) * sides[1] + row
    n0, n1 = (sides[1], sides[0]) if slip == "side" else (sides[0], sides[1])
    raw = [idx % n0, idx // n0] if nd == 2 else [idx % n0, (idx // n0) % n1, idx // (n0 * n1)]
    out = []
    for d, r, side in zip(raw, radii, sides):
        out.append(np.where(d >= r if slip == "ge" else d > r, d - side, d))
    return np.stack(out, axis=1)


def _changed(surf, radii):
    right = tail(surf, radii)
    return right, {slip: int((tail(surf, radii, slip) != right).any(axis=1).sum()) for slip in SLIPS}


def _closed_form_counts(ks, radii):
    """What each slip does to a delta at K, without a surface."""
    shape = tuple(2 * r for r in radii)
    m = int(np.prod(shape))
    raw = np.stack(np.unravel_index(ks, shape[::-1])[::-1], axis=1)          # x, y[, z] components of the decode
    s = np.stack(np.unravel_index(ks, shape), axis=1)
    counts = {"ge": int((raw == np.array(radii)).any(axis=1).sum()),
              "conj": int(((s != 0) & (2 * s != np.array(shape))).any(axis=1).sum()),
              "half": int((ks >= m // 2).sum())}
    onehot = np.zeros((len(ks), m), dtype=np.uint8)
    onehot[np.arange(len(ks)), ks] = 1
    for slip in ("side", "swap"):
        counts[slip] = int((tail(onehot, radii, slip) != tail(onehot, radii)).any(axis=1).sum())
    return counts


def _old_inputs_2d():
    """The live records of test_fftcc2d_every_fused_shape (tests/test_gpu_parity_2d.py), shape by shape."""
    from opencorr_amd import synth
    ref, tar = synth.speckle_pair_2d(300, 320, seed=20260925)        # conftest's speckle_small
    h, w = ref.shape
    P = oracle.P2
    sides = [16, 20, 24, 32, 40, 48, 64]
    for rx, ry in [(r, r) for r in range(4, 33)] + [(a // 2, b // 2) for a in sides for b in sides if a != b]:
        rng = np.random.default_rng(rx * 100 + ry)
        n = 75
        m = max(rx, ry) + 6
        xs = rng.uniform(m, w - m, n).astype(np.float32)
        ys = rng.uniform(m, h - m, n).astype(np.float32)
        xs[::2] = np.floor(xs[::2])
        ys[::2] = np.floor(ys[::2])
        base = oracle.make_pois2d(xs, ys)
        base[:, P["u"]] = rng.integers(-3, 4, n).astype(np.float32)
        base[:, P["v"]] = rng.integers(-3, 4, n).astype(np.float32)
        yield (rx, ry), ref, tar, np.delete(base, [7, 40, n - 1], axis=0)       # (the three guard trippers)


def _old_inputs_3d():
    """The inner records of test_fftcc3d_every_fused_cube (tests/test_gpu_parity_3d.py)."""
    from opencorr_amd import synth
    ref, tar = synth.speckle_pair_3d(96, 100, 104, seed=23)
    dz, dy, dx = ref.shape
    P = oracle.P3
    for r in range(4, 33):
        rng = np.random.default_rng(100 + r)
        n = 11
        m = r + 4
        xs = rng.uniform(m, dx - m, n).astype(np.float32)
        ys = rng.uniform(m, dy - m, n).astype(np.float32)
        zs = rng.uniform(m, dz - m, n).astype(np.float32)
        xs[::2], ys[::2], zs[::2] = np.floor(xs[::2]), np.floor(ys[::2]), np.floor(zs[::2])
        pois = oracle.make_pois3d(xs, ys, zs)
        pois[::3, P["u"]] = rng.integers(-2, 3, len(pois[::3]))
        pois[1::3, P["w"]] = rng.integers(-2, 3, len(pois[1::3]))
        yield (r, r, r), ref, tar, pois


def _total(counts_list):
    return {slip: sum(c[slip] for c in counts_list) for slip in SLIPS}


SLIP_CUBES = (4, 5, 8, 13, 16, 32)        # the planted 3D queues counted: fftcc3d_fusedn, _fused32, _planes at both ends of each
SLIP_BOXES = [(4, 6, 8), (8, 5, 4), (14, 4, 15)]
# The table of DESIGN.md section 3: records, records each slip changes, records on the seam / beyond +-5 -- (planted queues, speckle
# inputs of the existing every-shape tests).  The planted counts follow from the positions; the speckle counts are measured.
TOTALS = {
    2: (dict(records=57256, ge=3647, side=34084, swap=56494, conj=56972, half=28674, far=50476),
        dict(records=5112, ge=38, side=1967, swap=4672, conj=4758, half=3021, seam=84, far=534)),
    3: (dict(records=4554, ge=1312, side=1409, swap=4187, conj=4489, half=2276, far=2117),
        dict(records=319, ge=1, side=0, swap=318, conj=319, half=25, seam=2, far=0)),
}


@pytest.mark.parametrize("nd", [2, 3])
def test_planted_slips_on_the_new_queues_and_on_the_old_inputs(nd):
    """Each slip changes exactly the records the closed form says it must -- at least one in every shape --; the same count on the
    speckle inputs of the existing every-shape tests (all 71 2D shapes, all 29 cubes), and how far from index 0 their peaks ever
    lie, are pinned in TOTALS, the table of DESIGN.md section 3.  Asserted of the old inputs: the `>=` slip touches a far smaller share of them."""
    if nd == 2:
        shapes = pc.FAMILIES2D["fusedn"] + pc.FAMILIES2D["fusedr"]
        old = _old_inputs_2d()
    else:
        shapes = [(r, r, r) for r in SLIP_CUBES] + SLIP_BOXES
        old = _old_inputs_3d()
    new_counts, new_records, new_far = [], 0, 0
    for radii in shapes:
        ref, tar, queue, expected = (pc.queue2d if nd == 2 else pc.queue3d)(*radii)
        ks = pc.positions([2 * r for r in radii], pc.SEED)
        right, counts = _changed(surfaces(ref, tar, radii, queue), radii)
        assert np.array_equal(right, np.stack(pc.decode2d(ks, *radii) if nd == 2 else pc.decode3d(ks, *radii), axis=1)), radii
        assert counts == _closed_form_counts(ks, radii), (radii, counts, _closed_form_counts(ks, radii))
        assert min(counts[s] for s in ("ge", "swap", "conj", "half")) > 0 and (counts["side"] > 0) == (radii[0] != radii[1]), (radii, counts)
        new_counts.append(counts)
        new_records += len(queue)
        new_far += int((np.abs(right) > 5).any(axis=1).sum())
    old_counts, old_records, old_seam, old_far = [], 0, 0, 0
    for radii, ref, tar, queue in old:
        right, counts = _changed(surfaces(ref, tar, radii, queue), radii)
        old_seam += int(((right == np.array(radii)) | (right == 1 - np.array(radii))).any(axis=1).sum())
        old_far += int((np.abs(right) > 5).any(axis=1).sum())
        old_counts.append(counts)
        old_records += len(queue)
    new, was = _total(new_counts), _total(old_counts)
    print("\n%dD slips: new queues %d records %s, %d with |d| > 5 | old inputs %d records %s, %d on the seam, %d with |d| > 5"
          % (nd, new_records, new, new_far, old_records, was, old_seam, old_far))
    assert (dict(new, records=new_records, far=new_far), dict(was, records=old_records, seam=old_seam, far=old_far)) == TOTALS[nd]
    assert new["ge"] / new_records > 5 * was["ge"] / old_records and was["ge"] <= old_seam

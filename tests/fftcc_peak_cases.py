"""Planted correlation peaks: FFTCC queues whose answer lies at a CHOSEN position of the correlation surface (no GPU).

Every FFTCC kernel ends in the reference's tail (src/oc_fftcc.cpp:246-266, 391-416): a strict-'>' scan for the first maximum of the
surface, then `du = idx % sw; if (du > rx) du -= sw; ...`.  On speckle with a displacement of a few pixels that tail only ever sees
indices next to 0.  Here each record owns a pair of windows of integer grey levels 0 ... 255:

  * the reference window is random;
  * the target window is the reference window's M floats, read as the array the reference really transforms -- the plan's
    (n0, n1[, n2]) = (2rx, 2ry[, 2rz]) over the buffer filled x-fastest (src/oc_fftcc.cpp:40-42, 68-70), i.e. the RESHAPED window
    when the sides differ --, rolled cyclically by (s0, s1[, s2]) and written back in fill order.

The circular cross-correlation of an array with its own roll is its autocorrelation, rolled: the surface has its maximum at flat
buffer index K = s0 * n1 + s1 (3D: (s0 * n1 + s1) * n2 + s2), of height exactly ZNCC = 1 (a roll keeps mean and norm), and the record
the reference writes is decode(K) + guess, in closed form.  Nothing here is taken from the oracle, the reference or a kernel.

A planted peak is also the hardest input for the transforms: a rolled copy differs from the original by a pure phase, so every
frequency bin contributes its share of the peak height and a single wrong twiddle or mirror bin costs about 1/M of ZNCC (1e-3 at
32 x 32), where speckle keeps its energy in the low bins.

MEASURED holds, per kernel family, the largest |ZNCC - 1| of the COMPILED REFERENCE over every record of these queues (`python
tests/fftcc_peak_cases.py --measure`; tests/test_oracle_vs_ref_fftcc_peaks.py repeats a sample of every shape against it).  The GPU bars are BAR_FACTOR times that -- never a GPU figure.
"""
import itertools
import math

import numpy as np

P2 = dict(x=0, y=1, u=2, v=8, u0=14, v0=15, zncc=16)
P3 = dict(x=0, y=1, z=2, u=3, v=7, w=11, u0=15, v0=16, w0=17, zncc=18)
POI2D_FLOATS, POI3D_FLOATS = 25, 31
OUT2D = tuple(P2[k] for k in ("u", "v", "u0", "v0", "zncc"))
OUT3D = tuple(P3[k] for k in ("u", "v", "w", "u0", "v0", "w0", "zncc"))

LIMIT2D, LIMIT3D = 1024, 512        # records per queue where the surface has more than 1 024 positions
MAX_BYTES = 64 << 20                # of one image or volume
RIM = 2


# ---- where the peaks go ----------------------------------------------------------------------------------------------------------
def seam(n):
    """The values of one index around which the decode changes branch: 0, 1, r - 1, r, r + 1 (`> r` wraps, `r` does not), N - 1."""
    r = n // 2
    return sorted({0, 1, r - 1, r, r + 1, n - 1})


GUESS_ROOM = 3                      # |floor(frac + guess)| the generator leaves room for when it sizes a queue


def volume_dims(sides, n, offsets):
    """Dimensions (slowest first) of the image that holds n windows of `sides` (x, y[, z]) on the generator's grid: per axis a rim
    of RIM + |offset| on both ends, the cells, and the spare row / column of the guard."""
    box = list(sides)[::-1]
    rim = [RIM + abs(o) for o in offsets][::-1]
    return [2 * rm + c * b + 1 for rm, c, b in zip(rim, _grid(n, len(box)), box)]


def records_that_fit(shape, limit=LIMIT3D):
    """The largest record count up to `limit` whose volume, laid out by the generator with room for GUESS_ROOM voxels of guess on
    every axis, stays within MAX_BYTES."""
    for n in range(limit, 0, -1):
        if int(np.prod(volume_dims(shape, n, [GUESS_ROOM] * len(shape)))) * 4 <= MAX_BYTES:
            return n
    raise ValueError(shape)


def positions(shape, seed=0):
    """Flat buffer indices K to plant, for a plan of dimensions `shape` = (2rx, 2ry[, 2rz]).

    Every K where the surface has at most 1 024 positions.  Otherwise the full product of the per-axis seam sets -- of the plan's axes
    and, where the sides differ, of the decode's axes too (the decode cuts K by the window's width, not by the plan's n1) -- plus
    seeded random positions up to LIMIT2D / LIMIT3D records (fewer where the volume would pass 64 MB).  3D sides above 32: the six
    seam values on one axis at a time (18 records, the other two indices random), the 8 corners of {r, r + 1}^3 and 8 random ones."""
    shape = tuple(int(n) for n in shape)
    m = int(np.prod(shape))
    if m <= 1024:
        return np.arange(m, dtype=np.int64)
    rng = np.random.default_rng([seed, len(shape), *shape])
    ks = []
    if len(shape) == 3 and max(shape) > 32:
        for ax in range(3):
            for v in seam(shape[ax]):
                s = [int(rng.integers(0, n)) for n in shape]
                s[ax] = v
                ks.append(np.ravel_multi_index(s, shape))
        ks += [np.ravel_multi_index(s, shape) for s in itertools.product(*[(n // 2, n // 2 + 1) for n in shape])]
        limit = len(ks) + 8
    else:
        ks += [np.ravel_multi_index(s, shape) for s in itertools.product(*[seam(n) for n in shape])]
        if len(set(shape)) > 1:
            ks += [np.ravel_multi_index(s, shape[::-1]) for s in itertools.product(*[seam(n) for n in shape[::-1]])]
        limit = LIMIT2D if len(shape) == 2 else min(LIMIT3D, records_that_fit(shape))
    ks = list(dict.fromkeys(int(k) for k in ks))
    assert len(ks) <= limit, (shape, len(ks), limit)
    taken = set(ks)
    for k in rng.permutation(m):
        if len(ks) >= limit:
            break
        if int(k) not in taken:
            ks.append(int(k))
    return np.array(ks, dtype=np.int64)


# ---- the closed form -------------------------------------------------------------------------------------------------------------
def decode2d(k, rx, ry):
    """src/oc_fftcc.cpp:256-266 on integer arrays."""
    k = np.asarray(k, dtype=np.int64)
    du, dv = k % (2 * rx), k // (2 * rx)
    return np.where(du > rx, du - 2 * rx, du), np.where(dv > ry, dv - 2 * ry, dv)


def decode3d(k, rx, ry, rz):
    """src/oc_fftcc.cpp:401-416."""
    k = np.asarray(k, dtype=np.int64)
    du, dv, dw = k % (2 * rx), (k // (2 * rx)) % (2 * ry), k // (4 * rx * ry)
    return np.where(du > rx, du - 2 * rx, du), np.where(dv > ry, dv - 2 * ry, dv), np.where(dw > rz, dw - 2 * rz, dw)


def _rolled(win, shape, ks):
    """win[i] (M floats each) read as `shape`, rolled by unravel(ks[i]), flat again."""
    n = len(ks)
    a = win.reshape((n,) + shape)
    shifts = np.unravel_index(ks, shape)
    index = [np.arange(n).reshape((n,) + (1,) * len(shape))]
    for ax, (dim, s) in enumerate(zip(shape, shifts)):
        i = (np.arange(dim)[None, :] - s[:, None]) % dim          # b[i] = a[i - s]: the correlation peaks at +s
        index.append(i.reshape((n,) + tuple(dim if d == ax else 1 for d in range(len(shape)))))
    return a[tuple(index)].reshape(n, -1)


def _window_offset(frac, guess):
    """Where the truncating fill puts the target window, relative to the reference window: the reference forms
    (int)((x + c - rx) + u) in float32 (src/oc_fftcc.cpp:209-216); with x = c0 + rx + frac that is c0 + c + floor(frac + u), exactly,
    as long as frac and u are multiples of 1/8 (asserted) and the coordinates stay below 2^20."""
    assert 0.0 <= frac < 1.0 and (frac * 8).is_integer() and all((float(g) * 8).is_integer() for g in guess), (frac, guess)
    return [int(math.floor(frac + float(g))) for g in guess]


def _grid(n, nd):
    """Cells per axis (slowest first) of a nearly cubic grid with room for n windows."""
    cells = []
    left = n
    for d in range(nd, 0, -1):
        c = int(math.ceil(left ** (1.0 / d) - 1e-9))
        cells.append(c)
        left = -(-left // c)
    assert np.prod(cells) >= n
    return cells


def _plant(radii, ks, seed, guess, frac):
    nd = len(radii)
    sides = [2 * r for r in radii]                       # x, y[, z]
    shape = tuple(sides)                                 # the plan's (n0, n1[, n2])
    m = int(np.prod(sides))
    ks = np.asarray(ks, dtype=np.int64)
    n = len(ks)
    assert n > 0 and ks.min() >= 0 and ks.max() < m
    rng = np.random.default_rng([seed, nd, *radii])
    off = _window_offset(frac, guess)                    # x, y[, z]
    cells = _grid(n, nd)                                 # slowest (z or y) ... x
    box = sides[::-1]                                    # a window as it lies in the image: [z][y][x]
    rim = [RIM + abs(o) for o in off][::-1]
    dims = volume_dims(sides, n, off)
    assert int(np.prod(dims)) * 4 <= MAX_BYTES, (radii, n, dims)
    total = int(np.prod(cells))
    rwin = rng.integers(0, 256, (total, m)).astype(np.float32)
    twin = rng.integers(0, 256, (total, m)).astype(np.float32)
    twin[:n] = _rolled(rwin[:n], shape, ks)
    ref = rng.integers(0, 256, dims).astype(np.float32)
    tar = rng.integers(0, 256, dims).astype(np.float32)
    # cell (a, b[, c]) x window [z][y][x]  ->  image block
    order = [i for pair in zip(range(nd), range(nd, 2 * nd)) for i in pair]
    for img, win, shift in ((ref, rwin, [0] * nd), (tar, twin, off[::-1])):
        block = win.reshape(cells + box).transpose(order).reshape([c * b for c, b in zip(cells, box)])
        img[tuple(slice(rm + s, rm + s + c * b) for rm, s, c, b in zip(rim, shift, cells, box))] = block
    cell = np.unravel_index(np.arange(n), cells)         # slowest ... x
    coords = [(rm + c * b + b // 2 + frac).astype(np.float32) for rm, c, b in zip(rim, cell, box)][::-1]     # x, y[, z]
    floats = POI2D_FLOATS if nd == 2 else POI3D_FLOATS
    P = P2 if nd == 2 else P3
    queue = rng.uniform(-1.0, 1.0, (n, floats)).astype(np.float32)        # FFTCC reads x, y, u, v only: the rest must come back as it is
    for name, c in zip("xyz", coords):
        queue[:, P[name]] = c
    for name, g in zip("uvw", guess):
        queue[:, P[name]] = np.float32(g)
    expected = queue.copy()
    local = decode2d(ks, *radii) if nd == 2 else decode3d(ks, *radii)
    for name, d, g in zip("uvw", local, guess):
        expected[:, P[name]] = d.astype(np.float32) + np.float32(g)
        expected[:, P[name + "0"]] = np.float32(g)
    expected[:, P["zncc"]] = 1.0
    return ref, tar, queue, expected


def plant2d(rx, ry, ks, seed, guess=(0, 0), frac=0.0):
    """(ref, tar, queue, expected): one record per planted index.  `guess` (u, v) displaces the target windows (the rim grows with
    it); `frac` < 1 is added to the POI coordinates -- the truncating fill leaves the windows where they are."""
    return _plant((rx, ry), ks, seed, tuple(guess), frac)


def plant3d(rx, ry, rz, ks, seed, guess=(0, 0, 0), frac=0.0):
    return _plant((rx, ry, rz), ks, seed, tuple(guess), frac)


# ---- the window shapes of every kernel family (radii) ------------------------------------------------------------------------------
_SIDES_R = [16, 20, 24, 32, 40, 48, 64]
FUSEDR_2D = [(a // 2, b // 2) for a in _SIDES_R for b in _SIDES_R if a != b]                    # the 42 instantiated pairs
RECT_2D = [(r, 4 + ((r - 4) + 11) % 29) for r in range(4, 33)] + [(4, 32), (32, 4), (31, 32), (5, 4)]   # run-time sides
FAMILIES2D = {
    "fused32x2": [(16, 16)],
    "fusedn": [(r, r) for r in range(4, 33)],             # r = 16 takes fftcc2d_fused.hip unless "fftcc2d_fused" = 2
    "fusedr": FUSEDR_2D,
    "rect": RECT_2D,
    "pipeline": [(33, 33), (40, 36)],
}
# one shape per line length 8 ... 32 on each axis (out of the box test's 30), and two whose three sides all differ
BOX_3D = [(4, 5, 6), (6, 4, 5), (5, 6, 4), (7, 8, 9), (9, 7, 8), (8, 9, 7), (10, 11, 12), (12, 10, 11), (11, 12, 10),
          (11, 12, 13), (13, 11, 12), (12, 13, 11), (14, 4, 15), (15, 14, 4), (4, 15, 14), (16, 4, 4), (4, 16, 4), (4, 4, 16),
          (4, 6, 8), (8, 5, 4)]
FAMILIES3D = {
    "fusedn": [(r, r, r) for r in range(4, 14)],
    "fused32": [(16, 16, 16)],
    "planes": [(r, r, r) for r in range(14, 33) if r != 16],
    "box": BOX_3D,
    "pipeline": [(9, 9, 9), (6, 8, 5)],                   # through "fftcc3d_fused" = 0
}
assert len(FUSEDR_2D) == 42 and len(RECT_2D) == 33 and not set(FUSEDR_2D) & set(RECT_2D)
for _ax in range(3):
    assert {r[_ax] for r in BOX_3D} >= set(range(4, 17))

SEED = 20261019


def queue2d(rx, ry, guess=(0, 0), frac=0.0, seed=SEED):
    return plant2d(rx, ry, positions((2 * rx, 2 * ry), seed), seed, guess, frac)


def queue3d(rx, ry, rz, guess=(0, 0, 0), frac=0.0, seed=SEED):
    return plant3d(rx, ry, rz, positions((2 * rx, 2 * ry, 2 * rz), seed), seed, guess, frac)


# ---- the reference's own distance from ZNCC = 1 on these queues ----------------------------------------------------------------------
# Largest |ZNCC - 1| of the compiled reference (its float32 running sums of means and norms, src/oc_fftcc.cpp:198-231, 340-376, over
# the stand-in FFTW's double transforms) per family, over every record of every shape of the family.  Paste from `--measure`.
MEASURED = {
    "2D": {"fused32x2": 9.418e-06, "fusedn": 3.564e-05, "fusedr": 3.421e-05, "rect": 2.801e-05, "pipeline": 3.350e-05},
    "3D": {"fusedn": 9.394e-05, "fused32": 1.026e-04, "planes": 1.751e-04, "box": 6.241e-05, "pipeline": 3.386e-05},
}
BAR_FACTOR = 4.0                    # the project's margin for another float32 realisation of the same sums (tests/icgn_model64.py)
EXACT_BAR = {2: 1e-5, 3: 1e-4}      # the project's FFTCC bars; here against the exact value, 1


def bar(nd, family):
    """On |ZNCC - 1| of a kernel: 4 x the reference's own distance, and never above the project's bar."""
    return min(BAR_FACTOR * MEASURED["%dD" % nd][family], EXACT_BAR[nd])


QUICK_WORK = 1.5e8                  # complex multiply-adds of the stand-in DFT per shape in the quick run: a fraction of a second


def reference_runs(nd, family, quick):
    """(radii, records) the reference runs: every shape of the family, and every record of its queue (None) -- what MEASURED is
    taken from.  `quick` (what tests/test_oracle_vs_ref_fftcc_peaks.py repeats on every run): still every shape of every family, a
    strided sample of each queue sized by the stand-in DFT's work per record, 3 transforms x M x (sum of the sides) multiply-adds,
    never fewer than 8 records."""
    runs = []
    for radii in (FAMILIES2D if nd == 2 else FAMILIES3D)[family]:
        sides = [2 * r for r in radii]
        per_record = 3.0 * np.prod(sides) * sum(sides)
        runs.append((radii, max(8, int(QUICK_WORK / per_record)) if quick else None))
    return runs


def sample(n, want):
    """About `want` record indices out of n, strided from 0 (all if want is None)."""
    return np.arange(n) if want is None or want >= n else np.arange(0, n, -(-n // want))


def reference_distance(nd, family, quick, run):
    """max |ZNCC - 1| over reference_runs; `run(ref, tar, radii, queue)` computes in place.  Asserts the closed-form integers."""
    worst = 0.0
    P = P2 if nd == 2 else P3
    for radii, want in reference_runs(nd, family, quick):
        ref, tar, queue, expected = (queue2d if nd == 2 else queue3d)(*radii)
        pick = sample(len(queue), want)
        got = np.ascontiguousarray(queue[pick])
        run(ref, tar, radii, got)
        for name in "uvw"[:nd]:
            for key in (name, name + "0"):
                assert np.array_equal(got[:, P[key]], expected[pick, P[key]]), (family, radii, key)
        worst = max(worst, float(np.abs(got[:, P["zncc"]].astype(np.float64) - 1.0).max()))
    return worst


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    if "--measure" in sys.argv:
        from oracle import ref as oref

        def run(ref, tar, radii, q):
            (oref.fftcc2d if len(radii) == 2 else oref.fftcc3d)(ref, tar, *radii, q)

        print("MEASURED = {")
        for nd, fams in ((2, FAMILIES2D), (3, FAMILIES3D)):
            print('    "%dD": {%s},' % (nd, ", ".join('"%s": %.3e' % (f, reference_distance(nd, f, False, run)) for f in fams)))
        print("}")

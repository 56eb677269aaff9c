"""Volumes where voxel offsets pass 2^31 and 2^32: the shapes, what is pasted into them and what is asked there, without HIP.

The 3D engines form voxel addresses in size_t (prepare3d.hip, the fftcc3d* gathers, the base pointers and the coefficient staging of
icgn3d*.hip) -- except the streaming sweeps of ICGN3D1, which walk the box of a subvolume with a 32-bit voxel offset (Walk3 in
icgn3d_device.h, RowWalk in icgn3d_rows.hip).  None of that is exercised by a volume of 512^3 voxels.  The CPU oracle cannot prepare
a volume of 2 * 10^9 voxels, so the reference for a far BLOCK of a huge zero volume is the oracle on the CROP of that block
(the method of tests/large_image_cases.py, whose helpers are used here).  Two properties make that valid:

  1. the prepare fields are local: gx, gy, gz read +-2 voxels along their axis; coef is three separable 15-tap passes, +-7 with
     clamp-to-edge (prepare3d.hip, src/oc_cubic_bspline.cpp:214-351).  The fields of a crop therefore equal those of the volume at a
     margin of 2 (gradients) or 7 (coefficients) from the crop's artificial faces -- and right up to a face that IS a volume face.
     (The clamp rule and the zero gradient of the two outermost planes apply at volume faces only, so a crop's artificial face must not
     be compared, a true one must.)
  2. one ICGN3D1 iteration is origin-invariant for integer POI coordinates, zero displacement gradients and guesses in multiples of
     1/2: `centre + W(p) * (x, y, z, 1)` is then exact in float32 while the coordinates stay below 2^22, so a solve with
     stop_condition = 1 writes the same bits at any origin.  FFTCC3D is origin-invariant outright for integer coordinates and integer
     guesses (truncated integer windows).

tests/test_oracle_large_volume_cases.py proves both on a CPU before tests/test_gpu_large_volumes.py relies on them.

Everything outside the blocks is zero, so a fetch that wraps reads 0 against a pedestal of 30.  A block is seeded speckle (3D Gaussian
blobs on that pedestal, so that no interpolated value of a valid sample is negative: a negative sample ends a solve with -3); the
target is the reference translated by (TX, TY, TZ) = (2.5, -1.5, -1.5).  TZ is negative so that the POIs hard against a far z face are
SOLVED: their target samples stay below the interpolation range's end, and their reference samples are the volume's last plane -- in
INDEX31 the plane that holds voxel index 2^31.  CONV = 2 with STOP = 1 for the reason given in tests/large_image_cases.py.

FFTCC3D has no bounds guard in the reference (src/oc_fftcc.cpp:340-376 indexes unclamped; the HIP kernels clamp): its queues keep every
window inside the volume, up to the last voxel of a true face, and hold nothing that "trips".
"""
import collections
import functools

import numpy as np

import fftcc_plan_model as plan
import large_image_cases as lic
import oracle

P = oracle.P3
CONV, STOP = lic.CONV, lic.STOP
bits = lic.bits
GRAD_MARGIN, COEF_MARGIN = 2, 7
# What a POI keeps beyond its radius from an artificial face.  FFTCC3D reads the volumes themselves: 8 as in 2D.  ICGN3D1 reads
# coefficients, which are the volume's only 7 voxels inside; a sample moved by a guess of up to 3 takes coefficients up to 2 further:
# 7 + 3 + 2 = 12 (the 8 of the 2D file, whose table entries reach 2 pixels, would let the crop's clamped face show).
MARGIN, ICGN_MARGIN = lic.MARGIN, 12
TX, TY, TZ = 2.5, -1.5, -1.5
THREADS = 512                      # kBlock3d, icgn3d_device.h


# ---- the rule, restated from opencorr_amd/csrc/host/volume_limits.h with exact integers -------------------------------------------
MAX_SPAN = (1 << 32) - 1


def box_span(rx, ry, rz, dy, dx):
    """offset of a subvolume's last sample from its first one, in voxels of a volume with rows of dx and planes of dy rows"""
    return 2 * rz * dy * dx + 2 * ry * dx + 2 * rx


def accepted(rx, ry, rz, dy, dx):
    return box_span(rx, ry, rz, dy, dx) <= MAX_SPAN


# ---- shapes (dz, dy, dx) -------------------------------------------------------------------------------------------------------------
# 1290 * 1290 * 1291 = 2 148 353 100 voxels, 864 452 past 2^31; dx odd: the scalar prepare kernels.  A plane holds 1 665 390 voxels:
# voxel index 2^30 (byte offset 2^32) is (z, y, x) = (644, 953, 341), voxel index 2^31 is (1289, 616, 682) -- in the LAST plane.
INDEX31 = (1290, 1290, 1291)
# 68 * 5984 * 5984 = 2 434 961 408 voxels; dx % 4 == 0: the float4 prepare kernels.  A plane holds 35 808 256 voxels, so the box of a
# subset with rz = 30 spans 60 * 35 808 256 + 6 * 5984 + 6 = 2 148 531 270 voxels: past 2^31 = 2 147 483 648, below 2^32 -- the range in
# which the int products Walk3 used to form overflowed.  The far corner's voxels of planes 59 ... 67 lie past voxel index 2^31 (2^31 / 35 808 256 = 59.97).
SLAB = (68, 5984, 5984)
R_SLAB = (3, 3, 30)
# A volume has 15 planes or more (set_images3d), so the cheapest subset that spans 2^32 voxels is 15 planes deep: radii (3, 3, 7).  The
# smallest dy at dx = 17 517 for which the rule fires: 14 * 17 514 * 17 517 + 6 * 17 517 + 6 = 4 295 203 440 >= 2^32 = 4 294 967 296, and
# one row per plane less (dy = 17 513) gives 4 294 958 202 < 2^32.  4 601 891 070 voxels are one allocation of 18.4 GB (the target IS
# the reference).  Every sample of the subset's last plane lies 14 * 17 514 * 17 517 = 4 295 098 332 > 2^32 voxels behind the first.
REFUSED = (15, 17514, 17517)
R_REFUSED = (3, 3, 7)
SHAPES = {"INDEX31": INDEX31, "SLAB": SLAB, "REFUSED": REFUSED}
RADII = {"INDEX31": [(5, 7, 6), (8, 8, 8)], "SLAB": [R_SLAB]}
# The row mapping (icgn3d_rows.hip, A/B build) hands subsets with fewer than 28 samples per row to the kernel of icgn3d.hip: its own walk
# (RowWalk) runs from rx = 14 on.  29 x 7 x 61 samples, the box spans 2 148 531 292 voxels of SLAB: past 2^31 as well.
# On INDEX31 the same width with a shallow subset, (14, 5, 5), fits the blocks: there the row kernel's own base addresses (the box's
# first voxel) lie past byte offset 2^32 and past voxel index 2^31.  (A cross-section of 7 x 7 holds too little texture: the single
# iteration from an integer guess, half a voxel off on every axis, leaves one POI of the grid at a ZNCC of 0.87, below the 0.9 that
# tests/test_oracle_large_volume_cases.py asks of every grid POI; 11 x 11 gives 0.91 and more.)
ROWS_RADII = {"INDEX31": [(14, 5, 5)], "SLAB": [(14, 3, 30)]}

BZ, BY, BX = 56, 56, 64            # a block: holds a 32^3 window 8 and a 17^3 subset 12 voxels inside its artificial faces


def voxel_index(shape, z, y, x):
    return (z * shape[1] + y) * shape[2] + x


def voxel_at(shape, index):
    z, rem = divmod(index, shape[1] * shape[2])
    return (z,) + divmod(rem, shape[2])


SEAM30, SEAM31 = voxel_at(INDEX31, 1 << 30), voxel_at(INDEX31, 1 << 31)


class Block(collections.namedtuple("Block", "name shape z0 y0 x0 bz by bx seed same")):
    """bz x by x bx voxels of speckle at (z0, y0, x0) of a zero volume of `shape`; same: the target is the reference"""
    __slots__ = ()

    @property
    def origin(self):
        return (self.z0, self.y0, self.x0)

    @property
    def size(self):
        return (self.bz, self.by, self.bx)

    @property
    def lo(self):
        """per axis (z, y, x): the crop's near face is the volume's"""
        return tuple(o == 0 for o in self.origin)

    @property
    def hi(self):
        return tuple(o + n == s for o, n, s in zip(self.origin, self.size, self.shape))

    @property
    def slices(self):
        return tuple(slice(o, o + n) for o, n in zip(self.origin, self.size))

    def at(self, shape, z0, y0, x0):
        """the same speckle somewhere else (the CPU embeddings)"""
        return self._replace(shape=tuple(shape), z0=z0, y0=y0, x0=x0)


def _block(name, shape, origin, seed, size=(BZ, BY, BX), same=False):
    size = tuple(min(n, s) for n, s in zip(size, shape))
    origin = tuple(min(max(o, 0), s - n) for o, n, s in zip(origin, size, shape))
    return Block(name, tuple(shape), *origin, *size, seed, same)


def centred(name, shape, voxel, seed):
    """the block whose middle voxel is `voxel`, moved inside the volume where it would leave it"""
    return _block(name, shape, tuple(v - n // 2 for v, n in zip(voxel, (BZ, BY, BX))), seed)


def corner(name, shape, seed, far=True, size=(BZ, BY, BX), same=False):
    return _block(name, shape, tuple(s if far else 0 for s in shape), seed, size, same)


BLOCKS = {
    "INDEX31": [centred("seam30", INDEX31, SEAM30, 61), centred("seam31", INDEX31, SEAM31, 62), corner("corner", INDEX31, 63)],
    "SLAB": [corner("near", SLAB, 71, far=False, size=(68, BY, BX)), corner("far", SLAB, 72, size=(68, BY, BX))],
    "REFUSED": [corner("corner", REFUSED, 81, size=(15, BY, BX), same=True)],
}

# window (rx, ry, rz) -> family of fftcc_plan.h, tuning "fftcc3d_fused", and the bar tests/test_gpu_parity_3d.py holds that kernel's
# ZNCC to against the oracle in the reference's own arithmetic (sequential float32 sums of means and norms):
#   fused32  test_fftcc3d_fused_kernel_matches_oracle_and_rocfft_pipeline: 1e-4
#   cube     test_fftcc3d_matches_oracle[r0] (r = 8): 1e-5
#   planes   test_fftcc3d_every_fused_cube[14]: 2e-4 (12 < r <= 16)
#   box      test_fftcc3d_matches_oracle[r1] ((6, 8, 10)): 1e-5
#   rocfft   test_fftcc3d_fused_kernel_matches_oracle_and_rocfft_pipeline: the pipeline lies within 2e-6 of the fused kernel, which lies
#            within 1e-4 of the oracle; the docstring there states that the pipeline differs from the oracle by the same 8e-5: 1e-4
FFTCC_FAMILIES = [((16, 16, 16), "fused32", 1, 1e-4), ((8, 8, 8), "cube", 1, 1e-5), ((14, 14, 14), "planes", 1, 2e-4),
                  ((6, 8, 10), "box", 1, 1e-5), ((16, 16, 16), "rocfft", 0, 1e-4)]
# REFUSED holds 15 planes: no 32-plane window fits, and with no guard in the reference the oracle cannot be asked about a window that
# leaves the volume.  The families there are the cube and the box whose 8-plane windows fit, at both ends of the 15 planes.
FFTCC_REFUSED = [((4, 4, 4), "cube", 1, 1e-5), ((6, 8, 4), "box", 1, 1e-5)]
assert all(plan.kernel3d(*r, key, False) == family for r, family, key, _ in FFTCC_FAMILIES + FFTCC_REFUSED)


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def _blobs(size, seed):
    rng = np.random.default_rng(9100 + seed)
    bz, by, bx = size
    n = (bz + 16) * (by + 16) * (bx + 16) // 40
    return (rng.uniform(-8, bx + 8, n), rng.uniform(-8, by + 8, n), rng.uniform(-8, bz + 8, n), rng.uniform(1.3, 2.1, n), rng.uniform(40.0, 110.0, n))


def _render(size, blobs, tx, ty, tz):
    """pedestal + sum of Gaussian blobs whose centres are moved by (tx, ty, tz), float64, then one rounding to float32"""
    vol = np.full(size, 30.0)
    for cx, cy, cz, s, a in zip(*blobs):
        span = []
        for c, n in ((cz + tz, size[0]), (cy + ty, size[1]), (cx + tx, size[2])):
            lo, hi = max(0, int(c - 5 * s)), min(n, int(c + 5 * s) + 2)
            span.append((lo, hi, np.exp(-((np.arange(lo, hi) - c) ** 2) / (2 * s * s))))
        if any(lo >= hi for lo, hi, _ in span):
            continue
        (z0, z1, gz), (y0, y1, gy), (x0, x1, gx) = span
        vol[z0:z1, y0:y1, x0:x1] += a * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    return vol.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _crop(size, seed, same):
    blobs = _blobs(size, seed)
    ref = _render(size, blobs, 0.0, 0.0, 0.0)
    tar = ref if same else _render(size, blobs, TX, TY, TZ)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


def crop(block):
    """(ref, tar) of the block as host arrays: what the oracle is run on"""
    return _crop(block.size, block.seed, block.same)


def embed(block):
    """(ref, tar): the zero volume of block.shape with the block pasted in -- host arrays, for shapes a CPU can hold"""
    out = []
    for a in crop(block):
        vol = np.zeros(block.shape, dtype=np.float32)
        vol[block.slices] = a
        out.append(vol)
    return out


def inside(block, margin):
    """slices (z, y, x) of the crop where its fields are the volume's: `margin` away from artificial faces, up to true ones"""
    return tuple(slice(0 if lo else margin, n if hi else n - margin) for lo, hi, n in zip(block.lo, block.hi, block.size))


@functools.lru_cache(maxsize=None)
def _prepared(size, seed, same):
    return oracle.Prepared3D(*_crop(size, seed, same))


def prepared(block):
    return _prepared(block.size, block.seed, block.same)


def crop_fields(block):
    """name as read_field names it -> (the oracle's field of the crop, its margin)"""
    p = prepared(block)
    return dict(gx=(p.gx, GRAD_MARGIN), gy=(p.gy, GRAD_MARGIN), gz=(p.gz, GRAD_MARGIN), coef=(p.coef, COEF_MARGIN))


# ---- queues (crop coordinates) ----------------------------------------------------------------------------------------------------------
# per axis (z, y, x): what a guess adds to a sample's coordinate
REACH = ((-2.0, -1.0), (-2.0, -1.0), (2.0, 3.0))
GUESSES = {"int": [(2.0, -1.0, -1.0), (3.0, -2.0, -2.0), (3.0, -1.0, -2.0), (2.0, -2.0, -1.0)], "half": [(TX, TY, TZ)]}   # (u, v, w)


def _solved_range(n, r, lo_true, hi_true, reach):
    """integer positions along one axis whose subset, moved by any guess in `reach`, stays ICGN_MARGIN inside an artificial face and
    inside the interpolatable range [1, n - 2) at a true one"""
    g_lo, g_hi = reach
    lo = r + int(np.ceil(1 - g_lo)) if lo_true else r + ICGN_MARGIN
    hi = int(np.ceil(n - 2 - r - g_hi)) - 1 if hi_true else n - 1 - r - ICGN_MARGIN
    return max(lo, r), min(hi, n - 1 - r)


def solver_queue(block, guesses, radii):
    """A grid of integer POIs inside the block (the block's middle voxel, which a seam block puts on its seam, among them), then per
    true face: the position one beyond the last the guard admits (it trips: -3, record untouched) and the last the guard admits --
    hard against the face, its reference samples are the volume's outermost plane, row or column -- at two places of the face; and
    the POI hard against every true face at once.  A POI hard against the far z face is given w = -2 among the "int" guesses (with
    w = -1 its last plane of samples sits at dz - 2, where the interpolatable range ends).  Returns (queue, number of grid POIs)."""
    rx, ry, rz = radii
    r = (rz, ry, rx)
    ranges = [_solved_range(n, rr, lo, hi, reach) for n, rr, lo, hi, reach in zip(block.size, r, block.lo, block.hi, REACH)]
    axes = [lic._spread(lo, hi, most) for (lo, hi), most in zip(ranges, (2, 2, 3))]
    mid = tuple(n // 2 for n in block.size)
    grid = [(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]]
    if all(lo <= m <= hi for m, (lo, hi) in zip(mid, ranges)):
        grid.append(mid)
    else:    # the middle voxel's row and column at the nearest plane that can be solved (seam31: the seam lies in the last plane)
        grid.append(tuple(min(max(m, lo), hi) for m, (lo, hi) in zip(mid, ranges)))
    edge = []
    hard_all = list(grid[0])
    for axis in range(3):
        n, rr = block.size[axis], r[axis]
        others = [grid[-1], grid[1]]     # (the middle voxel's row and column first: a seam block's seam)
        for true, last, beyond in ((block.lo[axis], rr, rr - 1), (block.hi[axis], n - 1 - rr, n - rr)):
            if not true:
                continue
            for pos, base in ((beyond, others[0]), (last, others[0]), (last, others[1])):
                p = list(base)
                p[axis] = pos
                edge.append(tuple(p))
            hard_all[axis] = last
    if any(block.lo) or any(block.hi):
        edge.append(tuple(hard_all))
    pts = np.array(grid + edge)
    q = oracle.make_pois3d(pts[:, 2], pts[:, 1], pts[:, 0])
    g = GUESSES[guesses]
    for i in range(len(q)):
        q[i, P["u"]], q[i, P["v"]], q[i, P["w"]] = g[i % len(g)]
        if guesses == "int" and block.hi[0] and q[i, P["z"]] == block.size[0] - 1 - rz:
            q[i, P["w"]] = -2.0
    return q, len(grid)


# every guess leaves a residual of +1/2 or +3/2 per axis (u - TX etc. negative would put the peak in the wrapped half of a window)
FFTCC_GUESSES = [(2.0, -2.0, -2.0), (1.0, -3.0, -3.0), (2.0, -3.0, -2.0), (1.0, -2.0, -3.0)]


def fftcc_queue(block, radii):
    """Integer POIs and integer guesses whose reference and target windows [p - r, p + r) (+ guess) lie inside the volume -- at a true
    face up to its last voxel -- and MARGIN inside artificial faces.  A block whose target is its reference gets zero guesses."""
    rx, ry, rz = radii
    guesses = [(0.0, 0.0, 0.0)] if block.same else FFTCC_GUESSES
    axes = []
    for axis, rr in enumerate((rz, ry, rx)):
        g = [gs[2 - axis] for gs in guesses] + [0.0]
        n = block.size[axis]
        lo = rr - int(min(g)) if block.lo[axis] else rr + MARGIN
        hi = n - rr - int(max(g)) if block.hi[axis] else n - rr - MARGIN
        axes.append(lic._spread(lo, hi, 2))
    pts = [(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]]
    pts.append(tuple(min(max(n // 2, a[0]), a[-1]) for n, a in zip(block.size, axes)))
    pts = np.array(pts)
    q = oracle.make_pois3d(pts[:, 2], pts[:, 1], pts[:, 0])
    for i in range(len(q)):
        q[i, P["u"]], q[i, P["v"]], q[i, P["w"]] = guesses[i % len(guesses)]
    return q


def shift(queue, block):
    """the queue in volume coordinates"""
    out = queue.copy()
    for c, o in zip("zyx", block.origin):
        out[:, P[c]] += np.float32(o)
    assert (out[:, :3] == np.round(out[:, :3])).all() and out[:, :3].max() < 1 << 22
    return out


def padded(queue, count=2048):
    """the queue repeated up to `count` records: the locality schedule (tile_order3d, capi.hip) starts at 2048 POIs"""
    return np.ascontiguousarray(np.resize(queue, (count, queue.shape[1])))


def differing(got, want):
    """(poi, float) pairs outside x, y, z whose bits differ (NaN meeting NaN is equal)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    bad[:, :3] = False
    return np.argwhere(bad)


def assert_same_but_xyz(got, want, what=""):
    bad = differing(got, want)
    assert len(bad) == 0, "%s: %d floats differ, first (poi, float) %s" % (what, len(bad), bad[:6].tolist())


# ---- the oracle on a crop (or on any host pair) ---------------------------------------------------------------------------------------
CONTRACTS = ("lanes", "fma", "onepass", "rows")


def solve(contract, prep, queue, radii, stop=STOP, conv=CONV):
    """a copy of the queue solved by the oracle.  contract: "lanes" (the default kernel), "fma" (arith_fma = 1), "onepass"
    (arith_onepass3d = 1: tests/onepass3d_twin.py) or "rows" (icgn3d_mapping = 1, A/B build)"""
    q = np.ascontiguousarray(queue, dtype=np.float32).copy()
    rx, ry, rz = radii
    if contract == "onepass":
        import onepass3d_twin
        onepass3d_twin.icgn3d1(prep, rx, ry, rz, conv, stop, q)
    else:
        order = {"lanes": oracle.GPU_ORDER_3D, "fma": oracle.GPU_ORDER_3D | oracle.ARITH_FMA, "rows": oracle.ORDER_ROWS}[contract]
        oracle.icgn3d1(prep, rx, ry, rz, conv, stop, q, order=order, lanes=oracle.GPU_LANES_3D)
    return q


def fftcc(ref, tar, radii, queue):
    q = np.ascontiguousarray(queue, dtype=np.float32).copy()
    oracle.fftcc3d(ref, tar, radii[0], radii[1], radii[2], q)
    return q


def fftcc_surface(ref, tar, radii, poi):
    """The correlation surface the reference forms for one POI, in float64: the windows are filled x fastest and transformed as
    (2rx, 2ry, 2rz) arrays (src/oc_fftcc.cpp:68-70, 349-360: the RESHAPED window when the sides differ), flat as the peak scan
    reads it.  Not normalised."""
    rx, ry, rz = radii
    x, y, z = (int(poi[P[c]]) for c in "xyz")
    u, v, w = (int(poi[P[c]]) for c in "uvw")
    a = np.asarray(ref[z - rz:z + rz, y - ry:y + ry, x - rx:x + rx], dtype=np.float64)
    b = np.asarray(tar[z - rz + w:z + rz + w, y - ry + v:y + ry + v, x - rx + u:x + rx + u], dtype=np.float64)
    assert a.shape == b.shape == (2 * rz, 2 * ry, 2 * rx), (a.shape, b.shape, poi[:3])
    a, b = (a - a.mean()).reshape(2 * rx, 2 * ry, 2 * rz), (b - b.mean()).reshape(2 * rx, 2 * ry, 2 * rz)
    return np.fft.ifftn(np.conj(np.fft.fftn(a)) * np.fft.fftn(b)).real.ravel()


# ---- Walk3 and RowWalk, restated in wrapping 32-bit arithmetic ----------------------------------------------------------------------
M32 = (1 << 32) - 1


def walk_offsets(rx, ry, rz, dy, dx, tid, threads=THREADS):
    """[(sample index s, 32-bit offset)] of the samples thread `tid` owns, as Walk3 (icgn3d_device.h) forms them: the constructor's
    products and next()'s increments modulo 2^32 (unsigned wrapping; int products that wrap and are cast give the same words)."""
    SX, SY, SZ = 2 * rx + 1, 2 * ry + 1, 2 * rz + 1
    plane, N = SX * SY, SX * SY * SZ
    s = tid
    i, rem = divmod(s, plane)
    j, k = divmod(rem, SX)
    di, rem = divmod(threads, plane)
    dj, dk = divmod(rem, SX)
    off = ((i * dy + j) * dx + k) & M32
    doff = ((di * dy + dj) * dx + dk) & M32
    coff_k = (dx - SX) & M32
    coff_j = ((dy - SY) * dx) & M32
    out = []
    while s < N:
        out.append((s, off))
        s += threads
        k += dk
        off = (off + doff) & M32
        ck = k >= SX
        if ck:
            k -= SX
            off = (off + coff_k) & M32
        j += dj + (1 if ck else 0)
        cj = j >= SY
        if cj:
            j -= SY
            off = (off + coff_j) & M32
        i += di + (1 if cj else 0)
    return out


def row_walk_offsets(ry, rz, dy, dx, h, halves=THREADS // 32):
    """[(row = i * SY + j, 32-bit offset of the row's first sample)] of the rows half-wave `h` owns, as RowWalk (icgn3d_rows.hip)"""
    SY, SZ = 2 * ry + 1, 2 * rz + 1
    row = h
    i, j = divmod(row, SY)
    di, dj = divmod(halves, SY)
    off = ((i * dy + j) * dx) & M32
    doff = ((di * dy + dj) * dx) & M32
    coff = ((dy - SY) * dx) & M32
    out = []
    while row < SY * SZ:
        out.append((row, off))
        row += halves
        j += dj
        off = (off + doff) & M32
        c = j >= SY
        if c:
            j -= SY
            off = (off + coff) & M32
        i += di + (1 if c else 0)
    return out


def exact_offset(rx, ry, s, dy, dx):
    """the offset of sample s of a subset, in exact integers"""
    SX, SY = 2 * rx + 1, 2 * ry + 1
    i, rem = divmod(s, SX * SY)
    j, k = divmod(rem, SX)
    return (i * dy + j) * dx + k

"""Images at the size limits of the 2D engines: the shapes, what is pasted into them and what is asked there, without HIP.

The 2D hot path addresses image-sized arrays with 32-bit byte offsets (dic2d_device.h: buffer resources, `(int)voff`,
`(__umul24(yi, width) + xi) << 4`; fftcc2d_fused*.hip: `(__umul24(row, width) + col) << 2`; icgn2d.hip / nr2d.hip:
`__umul24(row, width * 4)`), and the prepare kernels launch one row of workgroups per image row.  None of that is exercised by
an image of a thousand pixels on a side.  The CPU oracle cannot prepare a 2^28-pixel image in a few seconds (its table alone is
17 GB), so the reference for a far BLOCK of a huge image is the oracle on the CROP of that block:

  1. the prepare fields are local (gradient: rows and columns +-2; table entry: a 4 x 4 neighbourhood; NR2D1's gradient
     tables: both, a margin of 4), so the fields of a crop equal those of the image away from the crop's artificial edges, and
     up to the edge where a crop edge IS an image edge;
  2. the first iteration is origin-invariant for integer POI coordinates, zero gradients and a guess (u, v) in multiples of 1/2:
     `center + W(p) * (x_local, y_local, 1)` is then exact in float32 while the coordinate stays below 2^22, so a solve with
     stop_condition = 1 writes the same bits at any image origin.  From the second iteration on the rounding of
     `center + warped` depends on the magnitude of the coordinate.  FFTCC2D is origin-invariant outright for integer coordinates
     and integer guesses (truncated integer windows).

tests/test_oracle_large_image_cases.py proves both on a CPU before tests/test_gpu_large_images.py relies on them.

Everything outside the blocks is zero.  A block is seeded speckle (Gaussian blobs on a pedestal, so that no interpolated value
of a valid sample is negative: a negative sample ends an ICGN solve with -3); the target is the reference translated by
(TX, TY) = (2.5, -1.5).  CONV = 2 on purpose: with stop_condition = 1 a POI whose first step is not below the criterion comes
back as -4 in place of its ZNCC, and a ZNCC is what tells a wrong fetch from a right one most plainly.
"""
import collections
import functools

import numpy as np

import fftcc_plan_model as plan
import oracle

P = oracle.P2

# ---- limits, restated from capi.hip (check_image2d_limits, check_fftcc2d_limits) -----------------------------------------------
ICGN_PIXELS = 1 << 28      # ICGN2D1 / ICGN2D2 / ICLM2D1 / ICLM2D2: one descriptor per table plane, 16 B per pixel
NR_PIXELS = 1 << 26        # NR2D1: one descriptor per table, the plane in the scalar offset
SOLVER_SIDE = 1 << 22      # all of those: row * (width * 4) through a 24-bit multiply
FFTCC_PIXELS = 1 << 30     # FFTCC2D: the images alone, 4 B per pixel
FFTCC_SIDE = 1 << 24       # FFTCC2D: row * width through a 24-bit multiply


def accepted(kind, h, w):
    """kind: "icgn" (also IC-LM), "nr" or "fftcc" """
    pixels, side = {"icgn": (ICGN_PIXELS, SOLVER_SIDE), "nr": (NR_PIXELS, SOLVER_SIDE), "fftcc": (FFTCC_PIXELS, FFTCC_SIDE)}[kind]
    return h * w <= pixels and h < side and w < side


# ---- shapes (h, w) --------------------------------------------------------------------------------------------------------------
ICGN_LIMIT = (16384, 16384)       # exactly 2^28 pixels: the last table offset of plane k is 2^32 - 16
NR_LIMIT = (8192, 8192)           # NR2D1's limit: vector offset + 3 * plane just under 2^32
WIDE = [(32, 4194300), (33, 4194299)]   # the second factor of the 24-bit multiply near 2^22, vector and scalar prepare kernels
TALL = (4194300, 32)              # the first factor near 2^22, grid.y in the millions
ROWS = [(65535, 8), (65536, 8), (65537, 9), (70001, 12)]   # around 65 535 rows, small enough for the oracle to take whole
FFTCC_LIMIT = (32768, 32768)      # 2^30 pixels: the `<< 2` offsets reach 2^32
REFUSED_FFTCC = [(5, 1 << 24), (32769, 32768)]

BH, BW = 160, 192                 # a block: holds 32 x 32 windows and 13 x 17 subsets 8 pixels inside its artificial edges
TX, TY = 2.5, -1.5                # target = reference translated by an integer plus one half
CONV, STOP = 2.0, 1
R_ICGN = (6, 8)                   # (rx, ry) of every solver on the blocks
R_THIN = [(16, 16), (12, 12)]     # FFTCC2D on WIDE and TALL: a window as long as a thin side of 32 fits nowhere (the guard), on
                                  # 33 in one row; 24 x 24 windows fit all three
MARGIN = 8                        # what a POI keeps beyond its radius from an artificial edge
FIELD_MARGIN, NR_MARGIN = 2, 4    # where a crop's fields are the image's: gradient / table, NR2D1's gradient tables

# window (rx, ry) -> family of fftcc_plan.h, tuning "fftcc2d_fused", ZNCC bar of tests/test_gpu_parity_2d.py for that family
FFTCC_FAMILIES = [((16, 16), "fused32", 1, 1.5e-5), ((12, 12), "smooth", 1, 1.5e-5), ((11, 11), "prime", 1, 1.5e-5),
                  ((8, 10), "pair", 1, 3e-5), ((9, 11), "rect", 1, 3e-5), ((16, 16), "rocfft", 0, 1.5e-5)]
assert all(plan.kernel2d(rx, ry, key) == family for (rx, ry), family, key, _ in FFTCC_FAMILIES)


class Block(collections.namedtuple("Block", "name shape y0 x0 bh bw seed")):
    """bh x bw pixels of speckle at (y0, x0) of a zero image of `shape`"""
    __slots__ = ()

    @property
    def top(self):
        return self.y0 == 0

    @property
    def left(self):
        return self.x0 == 0

    @property
    def bottom(self):
        return self.y0 + self.bh == self.shape[0]

    @property
    def right(self):
        return self.x0 + self.bw == self.shape[1]

    def at(self, shape, y0, x0):
        """the same speckle somewhere else (the CPU embeddings)"""
        return self._replace(shape=tuple(shape), y0=y0, x0=x0)


def corner(name, shape, seed, bh=BH, bw=BW):
    """flush with the bottom-right corner: both true borders and their +0 rule lie inside"""
    h, w = shape
    bh, bw = min(bh, h), min(bw, w)
    return Block(name, tuple(shape), h - bh, w - bw, bh, bw, seed)


def table_offset(shape, row, col=0, plane=0):
    """byte offset of a table entry from the start of the table (planar: [k][y][x] float4)"""
    h, w = shape
    return plane * h * w * 16 + (row * w + col) * 16


def image_offset(shape, row, col=0):
    return (row * shape[1] + col) * 4


def seam_row(shape, bytes_per_pixel, bound, base=0):
    """the first row whose first pixel lies at or beyond `bound` bytes when the array starts `base` bytes in"""
    return max(0, -(-(bound - base) // (shape[1] * bytes_per_pixel)))


ICGN_SEAM = seam_row(ICGN_LIMIT, 16, 1 << 31)
FFTCC_SEAM = seam_row(FFTCC_LIMIT, 4, 1 << 31)
# NR2D1 at its limit: a plane is exactly 2^30 bytes, so plane k of a table starts AT k * 2^30 -- `e + 3 * plane` is at 2^32 - 2^30
# from row 0 on and `e + 2 * plane` at 2^31 from row 0 on; no row inside a plane crosses either.  The rows the sums "pass" those
# values are therefore both row 0, and the block that holds them is flush with the TOP-LEFT corner (true top and left borders).
NR_PLANE = NR_LIMIT[0] * NR_LIMIT[1] * 16
NR_SEAMS = (seam_row(NR_LIMIT, 16, 1 << 31, 3 * NR_PLANE), seam_row(NR_LIMIT, 16, (1 << 32) - (1 << 30), 3 * NR_PLANE))

BLOCKS = {
    "ICGN_LIMIT": [corner("corner", ICGN_LIMIT, 11), Block("seam", ICGN_LIMIT, ICGN_SEAM - BH // 2, 5003, BH, BW, 12)],
    "NR_LIMIT": [corner("corner", NR_LIMIT, 21), Block("seam", NR_LIMIT, NR_SEAMS[0], 0, BH, BW, 22)],
    "FFTCC_LIMIT": [corner("corner", FFTCC_LIMIT, 31), Block("seam", FFTCC_LIMIT, FFTCC_SEAM - BH // 2, 20011, BH, BW, 32)],
    "WIDE0": [corner("corner", WIDE[0], 41)],
    "WIDE1": [corner("corner", WIDE[1], 42)],
    "TALL": [corner("corner", TALL, 151)],      # (seed 51 leaves an FFTCC peak 3e-5 above its neighbour: a near tie)
}
SHAPES = {"ICGN_LIMIT": ICGN_LIMIT, "NR_LIMIT": NR_LIMIT, "FFTCC_LIMIT": FFTCC_LIMIT, "WIDE0": WIDE[0], "WIDE1": WIDE[1], "TALL": TALL}


# ---- data -----------------------------------------------------------------------------------------------------------------------
def _blobs(bh, bw, seed):
    rng = np.random.default_rng(9000 + seed)
    n = bh * bw // 9
    return (rng.uniform(-8, bw + 8, n), rng.uniform(-8, bh + 8, n), rng.uniform(1.3, 2.1, n), rng.uniform(40.0, 110.0, n))


def _render(bh, bw, blobs, tx, ty):
    """pedestal + sum of Gaussian blobs whose centres are moved by (tx, ty), float64, then one rounding to float32"""
    img = np.full((bh, bw), 30.0)
    for cx, cy, s, a in zip(*blobs):
        cx, cy = cx + tx, cy + ty
        x0, x1 = max(0, int(cx - 5 * s)), min(bw, int(cx + 5 * s) + 2)
        y0, y1 = max(0, int(cy - 5 * s)), min(bh, int(cy + 5 * s) + 2)
        if x0 >= x1 or y0 >= y1:
            continue
        gx = np.exp(-((np.arange(x0, x1) - cx) ** 2) / (2 * s * s))
        gy = np.exp(-((np.arange(y0, y1) - cy) ** 2) / (2 * s * s))
        img[y0:y1, x0:x1] += a * gy[:, None] * gx[None, :]
    return img.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _crop(bh, bw, seed):
    blobs = _blobs(bh, bw, seed)
    ref, tar = _render(bh, bw, blobs, 0.0, 0.0), _render(bh, bw, blobs, TX, TY)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


def crop(block):
    """(ref, tar) of the block as host arrays: what the oracle is run on"""
    return _crop(block.bh, block.bw, block.seed)


def embed(block):
    """(ref, tar): the zero image of block.shape with the block pasted in -- host arrays, for shapes a CPU can hold"""
    out = []
    for a in crop(block):
        img = np.zeros(block.shape, dtype=np.float32)
        img[block.y0:block.y0 + block.bh, block.x0:block.x0 + block.bw] = a
        out.append(img)
    return out


def inside(block, margin):
    """(rows, columns) of the crop where its fields are the image's: `margin` away from artificial edges, up to true ones"""
    ys = slice(0 if block.top else margin, block.bh if block.bottom else block.bh - margin)
    xs = slice(0 if block.left else margin, block.bw if block.right else block.bw - margin)
    return ys, xs


# ---- queues (crop coordinates) --------------------------------------------------------------------------------------------------
def _spread(lo, hi, most):
    assert lo <= hi, (lo, hi)
    return np.unique(np.linspace(lo, hi, min(most, hi - lo + 1)).round().astype(int))


def _interior(block, rx, ry, u_reach, v_reach, most=6):
    """integer positions whose subset, moved by a guess u in [u_lo, u_hi] and v in [v_lo, v_hi], stays MARGIN inside artificial
    edges and inside the interpolatable range [1, side - 2) at true ones; the block's middle row (a seam block's seam) is one of
    the rows"""
    (ul, uh), (vl, vh) = u_reach, v_reach
    x_lo = rx + max(0, 1 - int(np.floor(ul))) if block.left else rx + MARGIN
    x_hi = block.bw - 1 - (rx + 2 + int(np.ceil(uh)) if block.right else rx + MARGIN)
    y_lo = ry + max(0, 1 - int(np.floor(vl))) if block.top else ry + MARGIN
    y_hi = block.bh - 1 - (ry + 2 + int(np.ceil(vh)) if block.bottom else ry + MARGIN)
    ys = _spread(y_lo, y_hi, most)
    if y_lo <= block.bh // 2 <= y_hi:
        ys = np.unique(np.append(ys, block.bh // 2))
    return _spread(x_lo, x_hi, most), ys


GUESSES = {"int": [(2.0, -1.0), (3.0, -2.0), (3.0, -1.0), (2.0, -2.0)], "half": [(2.5, -1.5)]}
U_REACH, V_REACH = (2.0, 3.0), (-2.0, -1.0)


def solver_queue(block, guesses, rx=R_ICGN[0], ry=R_ICGN[1]):
    """A grid of integer POIs inside the block, then rows at every true edge: two positions that trip the guard (the subset leaves
    the image by one and by two pixels) and the two nearest that pass it (their subsets reach the rows and columns the table
    holds as +0 border).  guesses: "int" (warps that are integer translations: the value
    plane, icgn2d_int_first) or "half" (all four table planes carry weight)."""
    xs, ys = _interior(block, rx, ry, U_REACH, V_REACH)
    gx, gy = np.meshgrid(xs, ys)
    px, py = list(gx.ravel()), list(gy.ravel())
    # per true edge: the subset leaves the image by two pixels and by one (the guard trips), and the nearest position that passes
    # the guard, whose samples reach the table's +0 border; the nearest position that is solved is the grid's own last row or column
    few = 1 if (block.top and block.bottom) or (block.left and block.right) else 2
    edge = []
    if block.right:
        edge += [(block.bw - rx + d, y) for d in (1, 0) for y in ys[::2]] + [(block.bw - rx - 1, y) for y in ys[1::2][:few]]
    if block.bottom:
        edge += [(x, block.bh - ry + d) for d in (1, 0) for x in xs[::2]] + [(x, block.bh - ry - 1) for x in xs[1::2][:few]]
    if block.left:
        edge += [(rx + d, y) for d in (-2, -1) for y in ys[::2]]
    if block.top:
        edge += [(x, ry + d) for d in (-2, -1) for x in xs[::2]] + [(x, ry) for x in xs[1::2][:few]]
    q = oracle.make_pois2d(px + [e[0] for e in edge], py + [e[1] for e in edge])
    g = GUESSES[guesses]
    for i in range(len(q)):
        q[i, P["u"]], q[i, P["v"]] = g[i % len(g)]
    return q, len(px)


def fftcc_queue(block, rx, ry, thin=False):
    """Integer POIs and integer guesses; at true edges two positions that trip the guard and the nearest that passes.  thin: the
    block spans the image's thin side, so the guess along it is zero.  Where the window is as long as that side (32 on 32) the
    reference's guard `x >= width - rx` leaves no position at all: the queue is then trippers only, and they must come back
    untouched."""
    gu = [2.0, 3.0, 0.0, 2.0]
    gv = [-1.0, -2.0, 0.0, -2.0]
    if thin and block.top and block.bottom:
        gv = [0.0] * 4
    if thin and block.left and block.right:
        gu = [0.0] * 4

    def axis(n, r, lo_true, hi_true, g):
        lo = r - int(min(g + [0])) if lo_true else r + MARGIN
        hi = n - r - 1 - int(max(g + [0])) if hi_true else n - r - 1 - MARGIN
        return _spread(lo, hi, 12 if thin else 5) if lo <= hi else np.zeros(0, dtype=int)

    xs = axis(block.bw, rx, block.left, block.right, gu)
    ys = axis(block.bh, ry, block.top, block.bottom, gv)
    mx, my = np.meshgrid(xs, ys)
    px, py = list(mx.ravel()), list(my.ravel())
    xm = xs[len(xs) // 2] if len(xs) else block.bw // 2
    ym = ys[len(ys) // 2] if len(ys) else block.bh // 2
    edge = []
    if block.right:
        edge += [(block.bw - rx + d, ym) for d in (1, 0, -1)]
    if block.bottom:
        edge += [(xm, block.bh - ry + d) for d in (1, 0, -1)]
    if block.left:
        edge += [(rx - 1, ym)]
    if block.top:
        edge += [(xm, ry - 1)]
    q = oracle.make_pois2d(px + [e[0] for e in edge], py + [e[1] for e in edge])
    for i in range(len(q)):
        q[i, P["u"]], q[i, P["v"]] = gu[i % 4], gv[i % 4]
    return q, len(px)


def shift(queue, block):
    """the queue in image coordinates"""
    out = queue.copy()
    out[:, P["x"]] += np.float32(block.x0)
    out[:, P["y"]] += np.float32(block.y0)
    assert (out[:, :2] == np.round(out[:, :2])).all() and out[:, :2].max() < SOLVER_SIDE
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def differing(got, want):
    """(poi, float) pairs outside x, y whose bits differ (NaN meeting NaN is equal)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    bad[:, :2] = False
    return np.argwhere(bad)


def same_but_xy(got, want):
    return len(differing(got, want)) == 0


def assert_same_but_xy(got, want, what=""):
    bad = differing(got, want)
    assert len(bad) == 0, "%s: %d floats differ, first (poi, float) %s" % (what, len(bad), bad[:6].tolist())


# ---- the oracle on a crop (or on any host pair) -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prepared(bh, bw, seed):
    ref, tar = _crop(bh, bw, seed)
    return oracle.Prepared2D(ref, tar), oracle.PreparedNR2D(ref, tar)


def prepared(block):
    """(Prepared2D, PreparedNR2D) of the crop, computed once"""
    return _prepared(block.bh, block.bw, block.seed)


def crop_fields(block):
    """name as read_field names it -> the oracle's field of the crop; the ICGN engines' and NR2D1's"""
    p2, nr = prepared(block)
    tgx, tgy = oracle.gradient2d(nr.tar)
    icgn = dict(gx=p2.gx, gy=p2.gy, lut=p2.lut)
    nr2d = dict(gx=tgx, gy=tgy, lut=nr.lut, lut_gx=nr.lut_gx, lut_gy=nr.lut_gy)
    return icgn, nr2d


SOLVERS = ("icgn2d1", "icgn2d2", "iclm2d1", "iclm2d2", "nr2d1")


def solve(solver, prep2d, prepnr, queue, order=oracle.ORDER_LANES, stop=STOP, conv=CONV, rx=R_ICGN[0], ry=R_ICGN[1]):
    """a copy of the queue solved by the oracle; solver: one of SOLVERS, or "onepass1" / "onepass2" (the one-pass contract's twin)"""
    q = np.ascontiguousarray(queue, dtype=np.float32).copy()
    if solver == "nr2d1":
        oracle.nr2d1(prepnr, rx, ry, conv, stop, q, order=order, lanes=64)
    elif solver in ("onepass1", "onepass2"):
        import onepass_twin
        onepass_twin.icgn2d(6 if solver == "onepass1" else 12, prep2d, rx, ry, conv, stop, q)
    else:
        getattr(oracle, solver)(prep2d, rx, ry, conv, stop, q, order=order, lanes=64)
    return q


def fftcc(ref, tar, rx, ry, queue):
    q = np.ascontiguousarray(queue, dtype=np.float32).copy()
    oracle.fftcc2d(ref, tar, rx, ry, q)
    return q


# ---- ROWS: whole images ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_pair(shape):
    """(ref, tar): a smooth texture over the whole image and the same texture moved by (0.3, -0.2)"""
    h, w = shape
    rng = np.random.default_rng(700 + h + w)
    k = rng.uniform(0.5, 1.3, (6, 2)) * rng.choice([-1.0, 1.0], (6, 2))
    ph, amp = rng.uniform(0, 2 * np.pi, 6), rng.uniform(8.0, 20.0, 6)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")

    def tex(x, y):
        return 130.0 + sum(a * np.cos(kx * x + ky * y + p) for (kx, ky), p, a in zip(k, ph, amp))

    ref, tar = tex(x, y).astype(np.float32), tex(x - 0.3, y + 0.2).astype(np.float32)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


ROWS_CONV, ROWS_STOP = 0.01, 10    # (subsets of 25 or 49 samples do not all settle below 0.001)


def rows_radius(shape):
    return 2 if shape[1] < 12 else 3


def rows_queue(shape):
    """POIs on rows 65 530 ... 65 539 (as far as the image has them) and at the bottom edge (the last that passes the guard, the
    first that trips it), in every column a subset of the radius fits with its interpolation range"""
    h, w = shape
    r = rows_radius(shape)
    xs = [x for x in range(r, w - r) if x - r >= 1 and x + r <= w - 3]       # (0 <= u < 1 stays inside [1, w - 2))
    assert xs, shape
    ys = sorted(set([y for y in range(65530, 65540) if y + r <= h - 1] + [h - 3 - r, h - 2 - r, h - 1 - r, h - r]))
    mx, my = np.meshgrid(xs, ys)
    q = oracle.make_pois2d(mx.ravel(), my.ravel())
    # (a start near the translation: in the one or two columns such a narrow image leaves, a step from zero leaves the range)
    q[:, P["u"]], q[:, P["v"]] = 0.25, -0.25
    return q


# ---- 3D: the prepare launches alone ---------------------------------------------------------------------------------------------
VOLUMES = [(65537, 15, 16), (15, 262145, 16)]     # (dz, dy, dx): grid.z = dz, or dy / 4 rows of workgroups in grid.y


@functools.lru_cache(maxsize=None)
def volume_pair(shape):
    """(ref, tar): noise with full mantissas, and nine parts of it moved by one voxel along x plus one part of other noise"""
    rng = np.random.default_rng(sum(shape))
    ref = rng.uniform(0, 255, shape).astype(np.float32)
    tar = np.roll(ref, 1, axis=2) * np.float32(0.9) + rng.uniform(0, 25.5, shape).astype(np.float32)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


def volume_queue(shape):
    """a dozen POIs along the long axis: at its far end (the last position the 8^3 window fits), around 65 535, near the start"""
    axis = int(np.argmax(shape))
    n = shape[axis]
    along = sorted(set([n - 5, n - 6, n - 7, n - 9, n - 12, n - 20, 65529, 65526, n // 2, 40, 6, 5]))
    assert len(along) >= 11 and all(5 <= a <= n - 5 for a in along)
    centre = [s // 2 for s in shape]          # (dz, dy, dx)
    zyx = np.tile(centre, (len(along), 1))
    zyx[:, axis] = along
    return oracle.make_pois3d(zyx[:, 2], zyx[:, 1], zyx[:, 0])

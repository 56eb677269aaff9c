"""Edge image shapes, 4-byte aligned in-place buffers and engine re-use: the cases and what is expected of them, without HIP.

Every other parity test hands the kernels images whose widths are multiples of 4 at 16-byte aligned addresses, one image size per
engine.  Here the DATA is ordinary (seeded float32 with fractional values, so that an operation order shows in the bits) and what
varies is how it reaches the kernels:

  * SHAPES2D / SHAPES3D_MIN: the sizes at which the prepare kernels (prepare2d.hip, prepare3d.hip) take another path -- the
    launchers' predicates are restated below (grad2d_kernel_of, transposer_tiles, rows_of_float4) and every shape carries the
    edges it is there for (edges2d);
  * ALIGN2D / ALIGN3D: a pair whose width is a multiple of 4, so that the ADDRESS alone decides between the 16-byte kernels and
    the scalar ones (carve);
  * SEQUENCE2D / SEQUENCE3D: what one long-lived engine is walked through, step by step.

tests/test_oracle_shape_cases.py asserts on a CPU that the lists hit what they claim and that the expected fields are sharp;
tests/test_gpu_shape_cases.py runs them.
"""
import functools

import numpy as np

import oracle

# ---- the launchers' predicates (prepare2d.hip launch_grad2d / launch_colmajor_to_rowmajor, prepare3d.hip rows_of_float4) -------
GRAD_ROWS = 16        # kGradRows: rows a thread of grad2d4_kernel walks down
GRAD_BLOCK = 256      # threads per workgroup of both gradient kernels, one row (scalar) or 16 rows (vector) per blockIdx.y
TILE = 32             # colmajor_to_rowmajor_kernel: 32 x 32 tiles
MIN2D, MIN3D = 5, 15  # what set_images accepts


def rows_of_float4(width, *addresses):
    """the 16-byte kernels: rows of whole float4s at 16-byte aligned addresses"""
    return width % 4 == 0 and all(a % 16 == 0 for a in addresses)


def grad2d_kernel_of(width, *addresses):
    return "grad2d4_kernel" if rows_of_float4(width, *addresses) else "grad2d_kernel"


def grad3d_kernel_of(dx, *addresses):
    return "grad3d4_kernel" if rows_of_float4(dx, *addresses) else "grad3d_kernel"


def prefilter3d_kernels_of(dx, *addresses):
    return "x4 + walk4" if rows_of_float4(dx, *addresses) else "x + walk"


def grad2d_grid(h, w, *addresses):
    """(threads that pass `c < width` in the last workgroup of a row, workgroups per row, row blocks)"""
    if rows_of_float4(w, *addresses):
        threads, rows = w // 4, (h + GRAD_ROWS - 1) // GRAD_ROWS
    else:
        threads, rows = w, h
    groups = (threads + GRAD_BLOCK - 1) // GRAD_BLOCK
    return threads - (groups - 1) * GRAD_BLOCK, groups, rows


def transposer_tiles(h, w):
    """(tiles along x, tiles along y, columns in the last tile, rows in the last tile)"""
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE, w - (w - 1) // TILE * TILE, h - (h - 1) // TILE * TILE


# ---- 2D shapes (h, w) -----------------------------------------------------------------------------------------------------------
MINIMUM = [(5, 5), (5, 8), (6, 7), (8, 5)]
WALK = [(h, w) for w in (12, 13) for h in (15, 16, 17, 18, 31, 33)]
THREADS = [(5, 1020), (6, 1024), (7, 1028), (5, 255), (6, 257), (7, 513)]
TRANSPOSER = [(31, 33), (32, 32), (33, 31), (5, 70), (70, 5), (64, 96)]
SHAPES2D = MINIMUM + WALK + THREADS + TRANSPOSER

# edge -> what it means; edges2d() says which of them a shape (at 16-byte aligned addresses) has
EDGES2D = {
    "minimum": "a side of 5 pixels, the least set_images accepts: one interior row or column of the gradient, two of the table",
    "vector, two threads": "width 8: the first thread has no left pair (c >= 4 fails), the other no right pair (c + 8 <= width fails)",
    "vector, below the walk": "fewer rows than one walk of 16: the loop ends on `height`",
    "vector, one walk": "exactly 16 rows",
    "vector, just past the walk": "17 or 18 rows: the second row block starts with rows r0 - 2, r0 - 1 of the first in its window "
                                  "and holds only rows of the zero border (17) or one row that is not (18: height - 2 = 16)",
    "vector, two walks": "31 or 33 rows: the second block one row short, a third block of one row",
    "vector, workgroup one thread short": "width 1020: 255 threads",
    "vector, workgroup full": "width 1024: 256 threads",
    "vector, one thread spills": "width 1028: a second workgroup whose first thread alone passes `c < width`",
    "scalar, walk heights": "the scalar kernel at the heights the vector kernel is asked at",
    "scalar, workgroup one thread short": "width 255",
    "scalar, one thread spills": "width 257",
    "scalar, three workgroups": "width 513: two full workgroups and one thread",
    "transposer, exact tile": "32 x 32",
    "transposer, partial tiles": "a last tile with fewer than 32 rows or columns, in both directions",
    "transposer, one row of tiles": "5 x 70 and 70 x 5: three tiles in a line, 5 rows or columns each",
    "transposer, whole tiles": "64 x 96: 2 x 3 whole tiles",
}


def edges2d(h, w):
    vec = rows_of_float4(w)
    last, groups, _ = grad2d_grid(h, w)
    tx, ty, lc, lr = transposer_tiles(h, w)
    out = set()
    if min(h, w) == MIN2D:
        out.add("minimum")
    if vec:
        if w == 8:
            out.add("vector, two threads")
        if h < GRAD_ROWS:
            out.add("vector, below the walk")
        if h == GRAD_ROWS:
            out.add("vector, one walk")
        if h in (GRAD_ROWS + 1, GRAD_ROWS + 2):
            out.add("vector, just past the walk")
        if h in (2 * GRAD_ROWS - 1, 2 * GRAD_ROWS + 1):
            out.add("vector, two walks")
        if groups == 1 and last == GRAD_BLOCK - 1:
            out.add("vector, workgroup one thread short")
        if groups == 1 and last == GRAD_BLOCK:
            out.add("vector, workgroup full")
        if groups == 2 and last == 1:
            out.add("vector, one thread spills")
    else:
        if h in (15, 16, 17, 18, 31, 33) and w == 13:
            out.add("scalar, walk heights")
        if groups == 1 and last == GRAD_BLOCK - 1:
            out.add("scalar, workgroup one thread short")
        if groups == 2 and last == 1:
            out.add("scalar, one thread spills")
        if groups == 3 and last == 1:
            out.add("scalar, three workgroups")
    if (h, w) == (TILE, TILE):
        out.add("transposer, exact tile")
    if tx * ty > 1 and lc < TILE and lr < TILE:
        out.add("transposer, partial tiles")
    if (tx == 3 and ty == 1 and h == 5) or (ty == 3 and tx == 1 and w == 5):
        out.add("transposer, one row of tiles")
    if tx * ty > 1 and lc == TILE and lr == TILE:
        out.add("transposer, whole tiles")
    return out


# ---- 3D shapes (dz, dy, dx): what test_gpu_parity_3d.py::test_prepare3d_odd_shapes_bit_exact asks in addition -------------------
SHAPES3D_MIN = [(15, 15, 15), (15, 16, 20), (16, 15, 17)]


# ---- images ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """bit equality, NaN meeting NaN (tests/test_gpu_fuzz.py::_same)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(nan, np.isnan(got)) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def assert_same(got, want, what=""):
    if not same(got, want):
        got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
        bad = np.argwhere(bits(got) != bits(want)) if got.shape == want.shape else "shapes %r / %r" % (got.shape, want.shape)
        raise AssertionError("%s: %s floats differ, first at %s" % (what, len(bad), bad[:6].tolist() if not isinstance(bad, str) else bad))


@functools.lru_cache(maxsize=None)
def _noise(shape):
    rng = np.random.default_rng(20261020 + 1009 * sum(shape) + 31 * shape[-1])
    ref = rng.uniform(0, 255, shape).astype(np.float32)
    tar = rng.uniform(0, 255, shape).astype(np.float32)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


def noise(shape):
    """(ref, tar) of the field tests: uniform in [0, 255), full mantissas"""
    return _noise(tuple(shape))


def _waves(rng, n, ndim):
    lam = rng.uniform(4.0, 10.0, n)
    d = rng.normal(size=(n, ndim))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return 2 * np.pi * d / lam[:, None], rng.uniform(0, 2 * np.pi, n), rng.uniform(3.0, 9.0, n)


def _texture(k, phase, amp, coords):
    """120 + sum of plane waves at (possibly displaced) float64 coordinates"""
    arg = sum(k[:, i].reshape((-1,) + (1,) * coords[i].ndim) * coords[i][None] for i in range(len(coords)))
    return 120.0 + (amp.reshape((-1,) + (1,) * coords[0].ndim) * np.cos(arg + phase.reshape((-1,) + (1,) * coords[0].ndim))).sum(axis=0)


@functools.lru_cache(maxsize=None)
def _pair(shape):
    rng = np.random.default_rng(977 + 13 * sum(shape) + shape[-1])
    ndim = len(shape)
    k, phase, amp = _waves(rng, 28, ndim)
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")   # slowest axis first
    coords = grid[::-1]                                                                  # x, y[, z]
    ref = _texture(k, phase, amp, coords)
    shift = (0.62, -0.41, 0.27)[:ndim]
    grad = (0.004, 0.003, -0.002)[:ndim]
    moved = [c - (s + g * (c - shape[::-1][i] / 2.0)) for i, (c, s, g) in enumerate(zip(coords, shift, grad))]
    tar = _texture(k, phase, amp, moved)
    ref, tar = np.ascontiguousarray(ref, dtype=np.float32), np.ascontiguousarray(tar, dtype=np.float32)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


def pair(shape):
    """(ref, tar) of the solver tests: a smooth texture (a sum of 28 plane waves of 4 ... 10 pixels) and the same texture moved by
    about (0.62, -0.41[, 0.27]) with a small stretch -- float32 with fractional values, a target the solvers converge on"""
    return _pair(tuple(shape))


# ---- expected fields ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected2d(shape, kind="noise"):
    """What prepare() builds for a shape, from the oracle: ICGN2D1 / ICGN2D2 (`gx`, `gy` of the reference; `lut` and the value
    plane `val` of the target, the latter from the evaluator at the interior integer points and +0 on the border) and NR2D1
    (`nr_gx`, `nr_gy` of the TARGET and the tables `lut_gx`, `lut_gy` of those)."""
    ref, tar = noise(shape) if kind == "noise" else pair(shape)
    h, w = shape
    gx, gy = oracle.gradient2d(ref)
    lut = oracle.bspline2d_lut(tar)
    val = np.zeros((h, w), dtype=np.float32)
    for y in range(1, h - 2):
        for x in range(1, w - 2):
            val[y, x] = oracle.bspline2d_eval(lut, x, y)
    nr = oracle.PreparedNR2D(ref, tar)
    tgx, tgy = oracle.gradient2d(tar)
    return dict(ref=ref, tar=tar, gx=gx, gy=gy, lut=lut, val=val, nr_gx=tgx, nr_gy=tgy, lut_gx=nr.lut_gx, lut_gy=nr.lut_gy)


@functools.lru_cache(maxsize=None)
def expected3d(shape, kind="noise"):
    ref, tar = noise(shape) if kind == "noise" else pair(shape)
    gx, gy, gz = oracle.gradient3d(ref)
    return dict(ref=ref, tar=tar, gx=gx, gy=gy, gz=gz, coef=oracle.bspline3d_prefilter(tar))


def gradient_border(shape):
    """True on the two-pixel / two-voxel border of a gradient field, per axis: (x mask, y mask[, z mask])"""
    masks = []
    for axis in range(len(shape) - 1, -1, -1):
        m = np.ones(shape, dtype=bool)
        sl = [slice(None)] * len(shape)
        sl[axis] = slice(2, shape[axis] - 2)
        m[tuple(sl)] = False
        masks.append(m)
    return masks


def lut_border(shape):
    """True where the table holds zeros: row 0, the last two rows, column 0, the last two columns"""
    h, w = shape
    m = np.ones(shape, dtype=bool)
    m[1:h - 2, 1:w - 2] = False
    return m


# ---- the same fields in plain float32 NumPy, in the reference's order and in another one ----------------------------------------
_F = np.float32
_FIRST, _SECOND = _F(1) / _F(12), _F(2) / _F(3)


def gradient2d_numpy(img, reverse=False):
    """result = 0; -= f[+2] / 12; += f[+1] * 2/3; -= f[-1] * 2/3; += f[-2] / 12 (prepare2d.hip), or the four terms last to first"""
    img = np.asarray(img, dtype=np.float32)
    h, w = img.shape
    gx, gy = np.zeros_like(img), np.zeros_like(img)

    def four(p2, p1, m1, m2):
        terms = [(-1, p2 * _FIRST), (1, p1 * _SECOND), (-1, m1 * _SECOND), (1, m2 * _FIRST)]
        acc = np.zeros_like(p2)
        for sign, t in (terms[::-1] if reverse else terms):
            acc = acc + t if sign > 0 else acc - t
        return acc

    gx[:, 2:w - 2] = four(img[:, 4:], img[:, 3:w - 1], img[:, 1:w - 3], img[:, :w - 4])
    gy[2:h - 2, :] = four(img[4:, :], img[3:h - 1, :], img[1:h - 3, :], img[:h - 4, :])
    return gx, gy


_BC = np.array([[-144, 384, -384, 144], [342, -702, 450, -90], [-198, -18, 270, -54], [0, 336, 0, 0]], dtype=np.float32) / _F(336)


def bspline2d_lut_numpy(img, n_outer=False):
    """acc += BC[l][m] * BC[k][n] * q[n][m] over m (outer), n (inner) as prepare2d.hip and the reference do, or with n outside"""
    img = np.asarray(img, dtype=np.float32)
    h, w = img.shape
    lut = np.zeros((h, w, 16), dtype=np.float32)
    if h < 4 or w < 4:
        return lut
    q = [[img[n:h - 3 + n, m:w - 3 + m] for m in range(4)] for n in range(4)]   # q[n][m]: row offset n - 1, column offset m - 1
    order = [(m, n) for n in range(4) for m in range(4)] if n_outer else [(m, n) for m in range(4) for n in range(4)]
    pm = {}
    for k in range(4):
        for l in range(4):
            acc = np.zeros((h - 3, w - 3), dtype=np.float32)
            for m, n in order:
                acc = acc + (_BC[l][m] * _BC[k][n]) * q[n][m]
            pm[k, l] = acc
    for k in range(4):
        for l in range(4):
            lut[1:h - 2, 1:w - 2, 4 * k + l] = pm[3 - k, 3 - l]
    return lut


# ---- alignment ------------------------------------------------------------------------------------------------------------------
ALIGN2D = (40, 48)         # width % 4 == 0
ALIGN3D = (16, 18, 20)     # dx % 4 == 0
ALIGN_R2D = 4              # the smallest radius with a fused FFTCC2D kernel (8 x 8 windows); 9 x 9 subsets
ALIGN_R3D = 4              # the smallest cube kernel of FFTCC3D (8^3 windows)
ALIGN_R3D_ICGN = 3
OFFSETS = (1, 2, 3)        # floats
CONV, STOP = 0.001, 20     # convergence criterion and stop condition of every solver run on these pairs


def carve(flat, k, shape):
    """the contiguous view flat[k : k + n].view(shape) of a 1-d buffer"""
    n = int(np.prod(shape))
    return flat[k:k + n].reshape(shape) if isinstance(flat, np.ndarray) else flat[k:k + n].view(shape)


def _axis(n, margin, step, most):
    """margin, margin + step, ... below n - margin; step None: the smallest step that leaves at most `most` positions"""
    if step is None:
        step = max(1, -(-(n - 2 * margin) // most))
    return np.arange(margin, n - margin, step)


def grid2d(shape, margin, step=None, most=10):
    h, w = shape
    ys, xs = np.meshgrid(_axis(h, margin, step, most), _axis(w, margin, step, most), indexing="ij")
    return oracle.make_pois2d(xs.ravel(), ys.ravel())


def grid3d(shape, margin, step=None, most=5):
    dz, dy, dx = shape
    zs, ys, xs = np.meshgrid(_axis(dz, margin, step, most), _axis(dy, margin, step, most), _axis(dx, margin, step, most), indexing="ij")
    return oracle.make_pois3d(xs.ravel(), ys.ravel(), zs.ravel())


def align_queue2d():
    """48 POIs, 4 pixels apart, whose 8 x 8 windows and 9 x 9 subsets stay inside 40 x 48 also after a shift by two pixels"""
    return grid2d(ALIGN2D, ALIGN_R2D + 4, 4)


def align_queue3d():
    """24 POIs whose 8^3 windows and 7^3 subvolumes stay inside 16 x 18 x 20 after a shift by one voxel"""
    return grid3d(ALIGN3D, ALIGN_R3D + 2, 2)


# ---- re-use ---------------------------------------------------------------------------------------------------------------------
# (shape, how the pair is handed over, subset radius -- a change means set_subset() before the step)
SEQUENCE2D = [((96, 128), "host", 6), ((24, 20), "host", 4), ((37, 53), "col-major", 4), ((128, 24), "device", 5), ((96, 128), "host", 5)]
SEQUENCE3D = [((24, 26, 28), "host", 5), ((15, 16, 20), "host", 4), ((20, 33, 17), "host", 4), ((24, 26, 28), "host", 5)]
SEQUENCE_R3D_ICGN = {5: 4, 4: 3}     # ICGN3D1 runs one voxel tighter than the FFTCC3D that starts it


def sequence_queue2d(shape, r):
    """at most 10 x 10 POIs, three pixels inside what an r-window needs"""
    return grid2d(shape, r + 3)


def sequence_queue3d(shape, r):
    """at most 5 x 5 x 5 POIs, two voxels inside what an r-window needs"""
    return grid3d(shape, r + 2)

"""Queues that put warped samples ON the limits of the interpolatable range (plain NumPy, no GPU).

Every solver abandons a POI (ZNCC = -3) as soon as one warped sample leaves [1, size - 2) (src/oc_cubic_bspline.cpp:137-142 and
:356-358; the abandon: src/oc_icgn.cpp:251-255, :1396-1400).  The kernels restate that rule in several places, each in another
form (an unsigned compare on floor(x), a test of the subset's four corner samples, the `inside` test of the integer-translation
sweep, the clipping of the staged coefficient box in 3D, per-sample tests elsewhere).  The queues built here decide between `<` and
`<=`, `size - 2` and `size - 3`, a box clipped at `D - 1` and at `D - 2`:

A LADDER is a set of records at one position whose guess steps across the value at which the extreme sample crosses a limit.  The
step is the float32 spacing of the LIMIT coordinate, `np.spacing(np.float32(limit))`, not of the guess: the sample coordinate is
`centre + (local + guess)`, rounded at the magnitude of the coordinate -- near a high limit of 110 that is 7.6e-6, and one ulp of a
guess near -1 (6e-8) would leave every rung on one side (and where `local + guess` rounds coarser still, see _rungs).  A plain ladder
has 13 rungs, `thr + k * step` for k = -6 .. 6; where the threshold is only known to a few ulp (sheared guesses, centre offsets) it has
33, k = -16 .. 16.  At a low limit the ladder is coarser than it looks: `local + guess` (about -9 for r = 10) is rounded in units of
9.5e-7 before the centre is added, so over the 13 rungs the extreme coordinate takes two or three values -- the float below 1, 1 itself
and the float pair above; the arithmetic offers nothing between them at these positions, and it is `<` against `<=` AT 1 that the
ladder decides.  At a high limit every rung is another float.  The positions along a side were chosen where the ORACLE's in-range rungs converge (some stretches of a border
hold too little texture for a subset half outside its own truth); tests/test_oracle_border.py asserts that they do.

Pairs: `speckle_pair_2d` / `speckle_pair_3d` with the default gradients and a translation of +-(1.2, 1.3) / +-(1.2, 1.3, 1.1), keyed
by the signs of the translation.  At a low face the limit is 1 and the threshold guess +1, at a high face size - 2 and -1: the pair
whose translation has the sign of the threshold puts the truth INWARD of the limit (an in-range rung converges), the other one
OUTWARD (an in-range rung starts inside and leaves in a later iteration: the walk-out ladders).

`first_sweep(ladder)` restates the warp of the first iteration and the range rule in float32 NumPy; `tests/test_oracle_border.py`
asserts that it predicts the oracle's records, uses it to say which abandoned record started inside, and plants the slips in it.
"""
import functools

import numpy as np

SHAPE2D = (96, 112)          # height, width
R2D = (10, 8)                # rx, ry
CONV, STOP2D = 1e-3, 10
T2D = (1.2, 1.3)
SHAPE3D = (40, 44, 48)       # dz, dy, dx
R3D = (5, 6, 4)              # rx, ry, rz
STOP3D = 10
T3D = (1.2, 1.3, 1.1)
LARGE_R = (16, 21, 25, 30)   # six staging passes; icgn3d1_kernel<48>, <64>, <0>
STOP_LARGE = 6
N_PLAIN, N_WIDE = 6, 16      # rungs on each side of the threshold


@functools.lru_cache(maxsize=None)
def pair2d(su, sv):
    """(ref, tar) whose translation is (su * 1.2, sv * 1.3); read-only."""
    from opencorr_amd import synth
    warp = dict(synth.DEFAULT_WARP_2D, u=su * T2D[0], v=sv * T2D[1])
    ref, tar = synth.speckle_pair_2d(*SHAPE2D, seed=20261018, warp=warp)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


@functools.lru_cache(maxsize=None)
def pair3d(su, sv, sw, shape=SHAPE3D):
    from opencorr_amd import synth
    warp = dict(synth.DEFAULT_WARP_3D, u=su * T3D[0], v=sv * T3D[1], w=sw * T3D[2])
    ref, tar = synth.speckle_pair_3d(*shape, seed=20261019, warp=warp)
    ref.setflags(write=False)
    tar.setflags(write=False)
    return ref, tar


@functools.lru_cache(maxsize=None)
def prepared2d(su, sv):
    import oracle
    return oracle.Prepared2D(*pair2d(su, sv))


@functools.lru_cache(maxsize=None)
def prepared2d_nr(su, sv):
    import oracle
    return oracle.PreparedNR2D(*pair2d(su, sv))


@functools.lru_cache(maxsize=None)
def prepared3d(su, sv, sw, shape=SHAPE3D):
    import oracle
    return oracle.Prepared3D(*pair3d(su, sv, sw, shape))


class Ladder:
    """name; dim; pair (sign key of pair2d / pair3d); shape; r (engine radii); queue (n x 25 / 31 float32); offsets (n x 2 or None);
    adaptive (per-POI radii in the records); kind: 'inward' (in-range rungs converge), 'walkout' (they leave later), 'integer'
    (whole-pixel rungs, they decide the integer-translation sweep); limits: [(axis, side)] of the limits the ladder crosses; stop."""

    def __init__(self, **kw):
        self.offsets, self.adaptive, self.stop = None, False, None
        self.__dict__.update(kw)
        self.queue.setflags(write=False)
        if self.offsets is not None:
            self.offsets.setflags(write=False)

    @property
    def mode(self):
        return {(False, False): "plain", (True, False): "offsets", (False, True): "adaptive", (True, True): "both"}[
            (self.offsets is not None, self.adaptive)]

    def __repr__(self):
        return "Ladder(%s)" % self.name


# ---- thresholds ------------------------------------------------------------------------------------------------------------------
_G2 = {"u": ("ux", "uy"), "v": ("vx", "vy")}
_G3 = {"u": ("ux", "uy", "uz"), "v": ("vx", "vy", "vz"), "w": ("wx", "wy", "wz")}


def _threshold(axis, side, size, centre, r, grads, off):
    """The guess (float64) at which the extreme sample of the subset sits on the limit of `axis`: low side -> coordinate 1, high side
    -> size - 2.  `axis`: index of the coordinate (0 = x); centre, r, off: per coordinate; grads: the row of the guess's gradient
    belonging to this coordinate (d/dx, d/dy[, d/dz])."""
    lin = float(centre[axis] + off[axis])
    for a in range(len(r)):
        w = grads[a] + (1.0 if a == axis else 0.0)
        lo, hi = (-r[a] - off[a]) * w, (r[a] - off[a]) * w
        lin += min(lo, hi) if side == "low" else max(lo, hi)
    limit = 1.0 if side == "low" else float(size - 2)
    return limit - lin, limit, limit - float(centre[axis] + off[axis])


def _rungs(thr, limit, inner, n):
    """thr + k * step, k = -n .. n.  step: the spacing of the limit coordinate -- or, where that is finer, an eighth of the spacing of
    `inner` = local + guess, the sum that is rounded before the centre is added: the crossing lies within half a spacing of that sum,
    i.e. four steps, of the threshold (r = 21 at a low face: 1 - 21 rounds in units of 1.9e-6, sixteen spacings of 1)."""
    step = max(float(np.spacing(np.float32(limit))), float(np.spacing(np.float32(abs(inner)))) / 8)
    return (np.float32(thr).astype(np.float64) + np.arange(-n, n + 1) * step).astype(np.float32)


def _ladder2d(name, pair, x, y, steps, kind, base=None, n=N_PLAIN, off=(0.0, 0.0), radii=None, fixed=None):
    """steps: [(field 'u' / 'v', side)]: the fields that walk (together) across their thresholds; `fixed`: [(field, side, k)] fields
    held k steps from their threshold.  base: the guess's gradients.  radii: per-POI radii (self-adaptive) or None."""
    import oracle
    P = oracle.P2
    h, w = SHAPE2D
    base = dict(base or {})
    r = radii or R2D
    m = 2 * n + 1
    q = oracle.make_pois2d([x] * m, [y] * m)
    for k, v in base.items():
        q[:, P[k]] = v
    # a field that crosses no limit starts on the pair's translation
    q[:, P["u"]], q[:, P["v"]] = pair[0] * T2D[0], pair[1] * T2D[1]
    limits = []
    for field, side, k in [(f, s, None) for f, s in steps] + list(fixed or []):
        axis = "uv".index(field)
        grads = [base.get(g, 0.0) for g in _G2[field]]
        thr, limit, inner = _threshold(axis, side, (w, h)[axis], (x, y), r, grads, off)
        rungs = _rungs(thr, limit, inner, n)
        q[:, P[field]] = rungs if k is None else rungs[n + k]
        limits.append((axis, side))
    if radii:
        q[:, P["srx"]], q[:, P["sry"]] = radii
    offsets = np.tile(np.float32(off), (m, 1)) if tuple(off) != (0.0, 0.0) else None
    return Ladder(name=name, dim=2, pair=pair, shape=SHAPE2D, r=R2D, queue=q.astype(np.float32), offsets=offsets,
                  adaptive=radii is not None, kind=kind, limits=limits, stop=STOP2D)


def _side2d(side):
    """-> (x, y, field, low / high, sign) of the plain ladder on a side of the image"""
    h, w = SHAPE2D
    rx, ry = R2D
    return {"left": (rx, 54, "u", "low", 1), "right": (w - 1 - rx, 54, "u", "high", -1),
            "top": (74, ry, "v", "low", 1), "bottom": (78, h - 1 - ry, "v", "high", -1)}[side]


def _inward2d(field, sign):
    return (sign, 1) if field == "u" else (1, sign)


@functools.lru_cache(maxsize=None)
def ladders2d():
    h, w = SHAPE2D
    rx, ry = R2D
    out = []
    # the four sides, truth inward ...
    for side in ("left", "right", "top", "bottom"):
        x, y, field, lohi, sign = _side2d(side)
        out.append(_ladder2d(side, _inward2d(field, sign), x, y, [(field, lohi)], "inward"))
    # ... and outward: the in-range rungs start inside and walk out in a later iteration
    for side in ("right", "bottom"):
        x, y, field, lohi, sign = _side2d(side)
        pair = _inward2d(field, -sign)
        out.append(_ladder2d("walkout-" + side, pair, x, y, [(field, lohi)], "walkout"))
    # corners: one field walks, the other one is held on the last value inside (k = 0 at a low limit, k = -1 at a high one)
    for cx, sx, lx in ((rx, 1, "low"), (w - 1 - rx, -1, "high")):
        for cy, sy, ly in ((ry, 1, "low"), (h - 1 - ry, -1, "high")):
            tag = "corner-%s%s" % ("T" if ly == "low" else "B", "L" if lx == "low" else "R")
            out.append(_ladder2d(tag + "-u", (sx, sy), cx, cy, [("u", lx)], "inward", fixed=[("v", ly, 0 if ly == "low" else -1)]))
            out.append(_ladder2d(tag + "-v", (sx, sy), cx, cy, [("v", ly)], "inward", fixed=[("u", lx, 0 if lx == "low" else -1)]))
    # sheared guesses, both signs: exactly one corner sample is the extreme
    for side in ("left", "right", "top", "bottom"):
        x, y, field, lohi, sign = _side2d(side)
        for s in (1, -1):
            base = dict(ux=0.02 * s, uy=-0.03 * s, vx=0.025 * s, vy=-0.015 * s)
            out.append(_ladder2d("shear%+d-%s" % (s, side), _inward2d(field, sign), x, y, [(field, lohi)], "inward", base=base, n=N_WIDE))
    # non-integer POI positions
    out.append(_ladder2d("fraction-left", (1, 1), rx + 0.375, 54.5, [("u", "low")], "inward"))
    out.append(_ladder2d("fraction-right", (-1, 1), w - 1 - rx - 0.375, 54.5, [("u", "high")], "inward"))
    out.append(_ladder2d("fraction-top", (1, 1), 74.25, ry + 0.625, [("v", "low")], "inward"))
    out.append(_ladder2d("fraction-bottom", (1, -1), 78.25, h - 1 - ry - 0.625, [("v", "high")], "inward"))
    # fractional centre offsets (the corner is +-rx - offx), per-POI radii, both
    for side in ("left", "right", "top", "bottom"):
        x, y, field, lohi, sign = _side2d(side)
        pair = _inward2d(field, sign)
        base = dict(ux=0.01, uy=0.02, vx=-0.02, vy=0.01)
        out.append(_ladder2d("offset-" + side, pair, x, y, [(field, lohi)], "inward", off=(0.375, -0.25), n=N_WIDE))
        out.append(_ladder2d("offset-shear-" + side, pair, x, y, [(field, lohi)], "inward", base=base, off=(-0.3, 0.7), n=N_WIDE))
        # per-POI radii: a smaller subset one pixel inside of what ITS guard accepts (the threshold moves by that pixel), one on the
        # border of its guard, and one with centre offsets and gradients as well
        def at(rr, inset):
            return ({"left": rr[0] + inset, "right": w - 1 - rr[0] - inset}.get(side, x),
                    {"top": rr[1] + inset, "bottom": h - 1 - rr[1] - inset}.get(side, y))
        out.append(_ladder2d("adaptive-" + side, pair, *at((8, 7), 1), [(field, lohi)], "inward", radii=(8, 7)))
        out.append(_ladder2d("adaptive-edge-" + side, pair, *at((9, 6), 0), [(field, lohi)], "inward", radii=(9, 6)))
        out.append(_ladder2d("both-" + side, pair, *at((9, 7), 0), [(field, lohi)], "inward", base=base, off=(0.375, -0.25), radii=(9, 7),
                             n=N_WIDE))
    out.append(integer_rungs2d())
    names = [l.name for l in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def integer_rungs2d():
    """Whole-pixel guesses thr - 1, thr, thr + 1 with zero gradients at integer positions on the four sides and in the four corners
    (all nine combinations there): what the `inside` test of the integer-translation sweep decides.  One ladder; pair (+, +)."""
    import oracle
    P = oracle.P2
    h, w = SHAPE2D
    rx, ry = R2D
    rec = []
    for x, tu in ((rx, 1), (50, None), (w - 1 - rx, -1)):
        for y, tv in ((ry, 1), (40, None), (h - 1 - ry, -1)):
            if tu is None and tv is None:
                continue
            for du in ((-1, 0, 1) if tu is not None else (None,)):
                for dv in ((-1, 0, 1) if tv is not None else (None,)):
                    rec.append((x, y, 1.0 if du is None else tu + du, 1.0 if dv is None else tv + dv))
    rec = np.float32(rec)
    q = oracle.make_pois2d(rec[:, 0], rec[:, 1])
    q[:, P["u"]], q[:, P["v"]] = rec[:, 2], rec[:, 3]
    return Ladder(name="integer", dim=2, pair=(1, 1), shape=SHAPE2D, r=R2D, queue=q, kind="integer",
                  limits=[(0, "low"), (0, "high"), (1, "low"), (1, "high")], stop=STOP2D)


# ---- 3D --------------------------------------------------------------------------------------------------------------------------
def _ladder3d(name, pair, shape, r, pos, steps, kind, fixed=None, stop=STOP3D, n=N_PLAIN):
    import oracle
    P = oracle.P3
    dz, dy, dx = shape
    m = 2 * n + 1
    q = oracle.make_pois3d([pos[0]] * m, [pos[1]] * m, [pos[2]] * m)
    for a, field in enumerate("uvw"):
        q[:, P[field]] = pair[a] * T3D[a]
    limits = []
    for field, side, k in [(f, s, None) for f, s in steps] + list(fixed or []):
        axis = "uvw".index(field)
        thr, limit, inner = _threshold(axis, side, (dx, dy, dz)[axis], pos, r, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        rungs = _rungs(thr, limit, inner, n)
        q[:, P[field]] = rungs if k is None else rungs[n + k]
        limits.append((axis, side))
    return Ladder(name=name, dim=3, pair=pair, shape=shape, r=r, queue=q.astype(np.float32), kind=kind, limits=limits, stop=stop)


@functools.lru_cache(maxsize=None)
def ladders3d():
    """One ladder per face and three per corner, one per field, at r = (5, 6, 4): an in-range rung at a
    low face uses tap index 0, at a high face tap index D - 1."""
    dz, dy, dx = SHAPE3D
    size = (dx, dy, dz)
    c = (30, 16, 22)
    out = []
    for axis, field in enumerate("uvw"):
        for side, sign in (("low", 1), ("high", -1)):
            pos = list(c)
            pos[axis] = R3D[axis] if side == "low" else size[axis] - 1 - R3D[axis]
            pair = tuple(sign if a == axis else 1 for a in range(3))
            out.append(_ladder3d("%s-%s" % (side, "xyz"[axis]), pair, SHAPE3D, R3D, pos, [(field, side)], "inward"))
    # corners: low-low-low and two that between them visit the three high faces.  (high-high-high, the diagonal opposite, was tried:
    # the 11 x 13 x 9 subvolume there holds too little texture, its in-range rungs leave the volume in the second iteration.)
    for tag, sides in (("lll", ("low", "low", "low")), ("hhl", ("high", "high", "low")), ("lhh", ("low", "high", "high"))):
        pos = [R3D[a] if sides[a] == "low" else size[a] - 1 - R3D[a] for a in range(3)]
        pair = tuple(1 if s == "low" else -1 for s in sides)
        for axis, field in enumerate("uvw"):
            # (the other two fields start on the translation, 0.1 - 0.3 voxels inside: their samples read tap 0 / D - 1 as well)
            out.append(_ladder3d("corner-%s-%s" % (tag, field), pair, SHAPE3D, R3D, pos, [(field, sides[axis])], "inward"))
    return tuple(out)


def large_shape(r):
    return (2 * r + 14,) * 3


@functools.lru_cache(maxsize=None)
def ladders3d_large(r):
    """r = 16 / 21 / 25 / 30 in a volume just large enough (2 r + 14 per side): a low-face ladder on x and a high-face ladder on y, on
    the pair (+, -, +) whose truth lies inward of both; stop = 6."""
    shape = large_shape(r)
    d = shape[0]
    mid = r + 7
    rr = (r, r, r)
    return (_ladder3d("r%d-low-x" % r, (1, -1, 1), shape, rr, (r, mid, mid), [("u", "low")], "inward", stop=STOP_LARGE),
            _ladder3d("r%d-high-y" % r, (1, -1, 1), shape, rr, (mid, d - 1 - r, mid), [("v", "high")], "inward", stop=STOP_LARGE))


# ---- queues: the ladders that share images, radii and overload, concatenated -------------------------------------------------------
def group(ladders):
    """{(pair, mode): (queue, offsets or None, [(ladder, slice)])} -- one compute() call per key."""
    keys = {}
    for l in ladders:
        keys.setdefault((l.pair, l.mode), []).append(l)
    out = {}
    for key, ls in keys.items():
        q = np.concatenate([l.queue for l in ls])
        off = np.concatenate([l.offsets for l in ls]) if ls[0].offsets is not None else None
        at, n = [], 0
        for l in ls:
            at.append((l, slice(n, n + len(l.queue))))
            n += len(l.queue)
        out[key] = (np.ascontiguousarray(q), off, at)
    return out


SOLVERS2D = ("icgn2d1", "icgn2d2", "iclm2d1", "iclm2d2", "nr2d1")


def oracle2d(solver, pair, queue, order, offsets=None, adaptive=False, stop=STOP2D):
    """A copy of `queue` solved by the oracle on pair2d(*pair) with R2D, CONV and `stop`."""
    import oracle
    out = np.ascontiguousarray(queue, dtype=np.float32).copy()
    if solver == "nr2d1":
        assert offsets is None and not adaptive
        oracle.nr2d1(prepared2d_nr(*pair), R2D[0], R2D[1], CONV, stop, out, order=order, lanes=64)
    elif solver.startswith("iclm"):
        assert offsets is None
        getattr(oracle, solver)(prepared2d(*pair), R2D[0], R2D[1], CONV, stop, out, order=order, lanes=64, self_adaptive=adaptive)
    else:
        getattr(oracle, solver)(prepared2d(*pair), R2D[0], R2D[1], CONV, stop, out, order=order, lanes=64, center_offsets=offsets,
                                self_adaptive=adaptive)
    return out


def oracle3d(ladder_or_key, queue, order, lanes, stop=None):
    """A copy of `queue` solved by the oracle; `ladder_or_key`: a Ladder, or (pair, shape, r, stop); `stop` overrides the ladder's."""
    import oracle
    pair, shape, r, stop_ = ((ladder_or_key.pair, ladder_or_key.shape, ladder_or_key.r, ladder_or_key.stop)
                            if isinstance(ladder_or_key, Ladder) else ladder_or_key)
    stop = stop_ if stop is None else stop
    out = np.ascontiguousarray(queue, dtype=np.float32).copy()
    oracle.icgn3d1(prepared3d(*pair, shape), r[0], r[1], r[2], CONV, stop, out, order=order, lanes=lanes)
    return out


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------
def first_sweep(ladder):
    """Per record and axis, the extremes of the sample coordinates of the FIRST iteration, computed per sample in float32 as the
    reference does (src/oc_deformation.cpp:94-105, :518-530; the quadratic warp of ICGN2D2 with zero second-order terms adds exact
    zeros and gives the same numbers): (lo, hi), each n x dim float32.  Not fused: the default arithmetic."""
    q = ladder.queue
    f32 = np.float32
    if ladder.dim == 2:
        import oracle
        P = oracle.P2
        lo, hi = np.empty((len(q), 2), f32), np.empty((len(q), 2), f32)
        for i, rec in enumerate(q):
            rx, ry = (int(rec[P["srx"]]), int(rec[P["sry"]])) if ladder.adaptive else ladder.r
            off = ladder.offsets[i] if ladder.offsets is not None else None
            xl, yl = np.meshgrid(np.arange(-rx, rx + 1, dtype=f32), np.arange(-ry, ry + 1, dtype=f32))
            cx, cy = rec[P["x"]], rec[P["y"]]
            if off is not None:
                xl, yl = xl - off[0], yl - off[1]
                cx, cy = cx + off[0], cy + off[1]
            wx = ((f32(1) + rec[P["ux"]]) * xl + rec[P["uy"]] * yl) + rec[P["u"]]
            wy = (rec[P["vx"]] * xl + (f32(1) + rec[P["vy"]]) * yl) + rec[P["v"]]
            x, y = cx + wx, cy + wy
            assert x.dtype == f32 and y.dtype == f32
            lo[i], hi[i] = (x.min(), y.min()), (x.max(), y.max())
        return lo, hi
    import oracle
    P = oracle.P3
    rx, ry, rz = ladder.r
    lo, hi = np.empty((len(q), 3), f32), np.empty((len(q), 3), f32)
    # zero gradients: the warp is 1 * xl + 0 * yl + 0 * zl + u, and the extremes are at xl = -+r
    for i, rec in enumerate(q):
        for a, (r, c, g) in enumerate(((rx, "x", "u"), (ry, "y", "v"), (rz, "z", "w"))):
            assert all(rec[P[k]] == 0 for k in _G3[g])
            lo[i, a] = rec[P[c]] + (f32(-r) + rec[P[g]])
            hi[i, a] = rec[P[c]] + (f32(r) + rec[P[g]])
    return lo, hi


def outside(ladder, lo, hi, low=1.0, high_offset=2, high_closed=True):
    """The range rule `x < 1 || x >= size - 2` on the extremes of first_sweep(); the keywords plant a slip."""
    size = np.float32((ladder.shape[1], ladder.shape[0]) if ladder.dim == 2 else (ladder.shape[2], ladder.shape[1], ladder.shape[0]))
    top = size - np.float32(high_offset)
    return ((lo < np.float32(low)) | ((hi >= top) if high_closed else (hi > top))).any(axis=1)


def integer_inside(ladder, x_low=1):
    """The `inside` test of the integer-translation sweep (icgn2d.hip) for the records of a 2D ladder: the subset's rectangle under an
    integral translation at an integral position lies in the range -> the sweep reads the value plane.  -> (applies, inside)"""
    import oracle
    P = oracle.P2
    q = ladder.queue
    h, w = ladder.shape
    rx, ry = ladder.r
    grads = np.stack([q[:, P[k]] for k in ("ux", "uy", "vx", "vy")], 1)
    whole = lambda a: np.trunc(a) == a
    applies = (grads == 0).all(axis=1) & whole(q[:, P["u"]]) & whole(q[:, P["v"]]) & whole(q[:, P["x"]]) & whole(q[:, P["y"]])
    applies &= (ladder.offsets is None) & (not ladder.adaptive)
    x0 = q[:, P["x"]].astype(np.int64) + np.where(applies, q[:, P["u"]], 0).astype(np.int64) - rx
    y0 = q[:, P["y"]].astype(np.int64) + np.where(applies, q[:, P["v"]], 0).astype(np.int64) - ry
    inside = (x0 >= x_low) & (y0 >= x_low) & (x0 + 2 * rx <= w - 3) & (y0 + 2 * ry <= h - 3)
    return applies, inside


def uses_last_tap(ladder, lo, hi):
    """3D: records whose first sweep is in range and reads coefficient index D - 1 on some axis (a sample with floor(x) = D - 3):
    what a staged box clipped at D - 2 would leave out."""
    size = np.float32((ladder.shape[2], ladder.shape[1], ladder.shape[0]))
    return ~outside(ladder, lo, hi) & (np.floor(hi) == size - 3).any(axis=1)


def uses_first_tap(ladder, lo, hi):
    return ~outside(ladder, lo, hi) & (np.floor(lo) == 1).any(axis=1)

"""Queues that carry non-finite POI records among clean ones (plain NumPy, no GPU, no fixtures).

The solvers restate the reference's entry guard (src/oc_icgn.cpp:160-167, :1279-1286; src/oc_nr.cpp:165-171;
src/oc_iclm.cpp:166-172) as a chain of `<` / `>` comparisons.  Every comparison with a NaN is false, so a record whose OWN
coordinate is NaN passes that chain, and the reference then indexes the images with (int)NaN, which is undefined.  This project
writes the geometric part of the guard negated, `!(py - ry >= 0 && ...)`: the same decision for every other input, and a NaN
coordinate is rejected like a subset that leaves the image, before any address is formed from it.  The contract:

    ICGN2D1 / ICGN2D2 / ICLM2D1 / ICLM2D2 / ICGN3D1 (every arithmetic contract, every variant)
        zncc = zncc_in >= 0 ? -3 : zncc_in; no other float of the record is written
    NR2D1       its own guard branch: -1, then the -4 and -5 rules, on the fields the record came in with
    FFTCC2D     the record stays untouched
    FFTCC3D     no guard (the reference has none): indices are clamped per element, the record is that of an all-voxel(0, 0, 0) window

A queue built here holds
    CLEAN    records that converge in the oracle (tests/test_oracle_nonfinite.py asserts it),
    COORD    NaN in x, in y (in z), in every combination; the finite coordinates mid-image, on the low guard edge and on the high
             one; the four NaN encodings NAN_BITS; each with incoming ZNCC 0, -2.5 and NaN,
    CONTROL  +-inf and +-3e38 in each coordinate, which the guard as the reference writes it rejects already,
    WARP     NaN and +-inf in the gradient terms of the guess (and, in a queue with centre offsets, in the offsets): the oracle is
             defined there (the range rule of the interpolation rejects a NaN sample) and gives the expected record,
    GUESS    (FFTCC2D only) NaN and +-inf in the guess u, v,
with planted records at index 0, at the last index, at 63 and 64, at even and odd indices and next to each other.  `expected()`
gives COORD and CONTROL records from the contract alone and takes every other record from the oracle.
"""
import functools

import numpy as np

import border_cases as bc

NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)     # quiet, negative quiet, signalling, all ones
ZNCC_IN = (0.0, -2.5, float("nan"))
HUGE = (float("inf"), float("-inf"), 3e38, -3e38)
BAD = (float("nan"), float("inf"), float("-inf"))
CLEAN, COORD, CONTROL, WARP, GUESS = 0, 1, 2, 3, 4
PAIR2D, PAIR3D = (1, 1), (1, 1, 1)
RADII_ADAPTIVE = ((9, 8), (10, 8))       # per-POI radii of the clean records (even / odd); planted records carry R2D
OFFSET = (0.375, -0.25)
SEED = 20261019
# 21 x 17 samples are few for the twelve parameters of the second-order solvers: ten iterations (bc.STOP2D) leave some clean records
# short of the criterion, forty none
STOP2D = 40


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """The suite's rule: the same bits, or NaN on both sides."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


class Planted:
    """queue (n x 25 / 31 float32), offsets (n x 2 or None), kind (n; CLEAN ... GUESS), names (n strings), dim, r."""

    def __init__(self, queue, kind, names, dim, r, offsets=None):
        self.queue, self.kind, self.names, self.dim, self.r, self.offsets = queue, kind, tuple(names), dim, r, offsets
        for a in (queue, kind, offsets):
            if a is not None:
                a.setflags(write=False)

    @property
    def clean(self):
        return self.kind == CLEAN

    @property
    def by_contract(self):
        return (self.kind == COORD) | (self.kind == CONTROL)

    def without_planted(self):
        """The clean records alone, in queue order."""
        m = self.clean
        return Planted(self.queue[m].copy(), self.kind[m].copy(), [n for n, k in zip(self.names, m) if k], self.dim, self.r,
                       None if self.offsets is None else self.offsets[m].copy())

    def with_offsets(self, offsets):
        return Planted(self.queue.copy(), self.kind.copy(), self.names, self.dim, self.r, np.ascontiguousarray(offsets, np.float32))

    def __repr__(self):
        return "Planted(%dD, %d records, %d clean)" % (self.dim, len(self.queue), int(self.clean.sum()))


def _P(dim):
    import oracle
    return oracle.P2 if dim == 2 else oracle.P3


def _set_bits(rec, col, word):
    rec.view(np.uint32)[col] = np.uint32(word)


def _coord_records(dim, blank, mid, low, high):
    """COORD and CONTROL records.  blank(): a zero record with the radii fields filled; mid / low / high: per axis, a finite value
    mid-image, exactly on the low guard edge (x == rx) and on the high one (x + rx == width - 1)."""
    P = _P(dim)
    axes = "xyz"[:dim]
    recs, kinds, names = [], [], []

    def emit(kind, name, rec):
        for z in ZNCC_IN:
            r = rec.copy()
            r[P["zncc"]] = np.float32(z)
            recs.append(r)
            kinds.append(kind)
            names.append("%s zncc_in=%s" % (name, z))

    subsets = [s for s in range(1, 2 ** dim)]
    for word in NAN_BITS:
        for s in subsets:
            places = (("mid", mid),) if s == 2 ** dim - 1 else (("mid", mid), ("low", low), ("high", high))
            for tag, at in places:
                if word != NAN_BITS[0] and tag != "mid" and dim == 3:
                    continue        # 3D: the edge positions once, with the first encoding
                rec = blank()
                for a, ax in enumerate(axes):
                    if s >> a & 1:
                        _set_bits(rec, P[ax], word)
                    else:
                        rec[P[ax]] = at[a]
                emit(COORD, "NaN %08x in %s, rest %s" % (word, "".join(ax for a, ax in enumerate(axes) if s >> a & 1), tag), rec)
    for a, ax in enumerate(axes):
        for v in HUGE:
            rec = blank()
            for b, bx in enumerate(axes):
                rec[P[bx]] = v if a == b else mid[b]
            emit(CONTROL, "%s in %s" % (v, ax), rec)
    # what NR2D1's branch looks at besides the ZNCC: a record that comes in "converged at the stop" (-4), and one with a NaN guess
    # whose u0, v0 the -5 rule copies back
    rec = blank()
    _set_bits(rec, P["x"], NAN_BITS[0])
    for b, bx in enumerate(axes[1:], 1):
        rec[P[bx]] = mid[b]
    rec[P["iteration"]], rec[P["convergence"]] = 1000.0, 1.0
    emit(COORD, "NaN in x, came in at the stop", rec)
    rec = blank()
    rec[P["x"]] = mid[0]
    _set_bits(rec, P["y"], NAN_BITS[1])
    if dim == 3:
        rec[P["z"]] = mid[2]
    rec[P["u"]], rec[P["u0"]], rec[P["v0"]] = np.float32("nan"), 3.0, 4.0
    emit(COORD, "NaN in y and in the guess u", rec)
    return recs, kinds, names


def _arrange(clean, planted, kinds, names):
    """One queue: planted records at 0, 63, 64 and the last index, the others at random (seeded) places, so that they sit at even and
    odd indices, next to each other and between clean records; both groups keep their order."""
    n = len(clean) + len(planted)
    assert n >= 66 and len(planted) >= 4
    forced = [0, 63, 64, n - 1]
    rng = np.random.default_rng(SEED)
    rest = np.setdiff1d(np.arange(n), forced)
    slots = np.zeros(n, bool)
    slots[forced] = True
    slots[rng.choice(rest, len(planted) - len(forced), replace=False)] = True
    width = len(clean[0])
    q = np.empty((n, width), np.float32)
    q.view(np.uint32)[slots] = np.stack(planted).view(np.uint32)
    q[~slots] = np.stack(clean)
    kind = np.zeros(n, np.int8)
    kind[slots] = kinds
    out_names = np.empty(n, object)
    out_names[slots] = names
    out_names[~slots] = ["clean %d" % i for i in range(len(clean))]
    return q, kind, list(out_names), slots


def _warp_records(dim, fields, blank_at):
    """A clean record with NaN / +inf / -inf in one field of the guess."""
    P = _P(dim)
    recs, names = [], []
    for f in fields:
        for v in BAD:
            rec = blank_at()
            rec[P[f]] = np.float32(v)
            recs.append(rec)
            names.append("%s = %s" % (f, v))
    return recs, names


# ---- 2D solvers ------------------------------------------------------------------------------------------------------------------
def _clean2d():
    import oracle
    P = oracle.P2
    xs, ys = np.meshgrid(np.arange(20, 93, 12, dtype=np.float32), np.arange(16, 77, 10, dtype=np.float32))
    q = oracle.make_pois2d(xs.ravel(), ys.ravel())
    # every other record at a fractional position with the pair's translation as its guess; the others whole-pixel (the
    # integer-translation sweep of icgn2d.hip)
    odd = np.arange(len(q)) % 2 == 1
    q[odd, P["x"]] += 0.375
    q[odd, P["y"]] += 0.625
    q[:, P["u"]] = np.where(odd, np.float32(bc.T2D[0]), np.float32(1))
    q[:, P["v"]] = np.where(odd, np.float32(bc.T2D[1]), np.float32(1))
    for k, (rx, ry) in enumerate(RADII_ADAPTIVE):
        q[k::2, P["srx"]], q[k::2, P["sry"]] = rx, ry
    return q


@functools.lru_cache(maxsize=None)
def queue2d(offsets=False):
    """The queue of the 2D solvers on bc.pair2d(*PAIR2D) with bc.R2D.  Every record carries per-POI radii (read only under
    set_self_adaptive: the clean ones RADII_ADAPTIVE, the planted ones R2D, so that the edge positions are edges in both modes).
    offsets: with a centre-offset queue -- OFFSET for every record, and six more WARP records with a bad offset."""
    import oracle
    P = oracle.P2
    h, w = bc.SHAPE2D
    rx, ry = bc.R2D

    def blank():
        rec = np.zeros(oracle.POI2D_FLOATS, np.float32)
        rec[P["srx"]], rec[P["sry"]] = rx, ry
        return rec

    def blank_at():
        rec = blank()
        rec[P["x"]], rec[P["y"]], rec[P["u"]], rec[P["v"]] = 56.0, 48.0, bc.T2D[0], bc.T2D[1]
        return rec

    planted, kinds, names = _coord_records(2, blank, (56.0, 48.0), (float(rx), float(ry)), (float(w - 1 - rx), float(h - 1 - ry)))
    warp, wnames = _warp_records(2, ("ux", "uy", "vx", "vy", "uxx", "uxy", "uyy", "vxx", "vxy", "vyy"), blank_at)
    n_bad_off = 0
    if offsets:
        for axis in (0, 1):
            for v in BAD:
                warp.append(blank_at())
                wnames.append("offset %s = %s" % ("xy"[axis], v))
                n_bad_off += 1
    planted, kinds, names = planted + warp, kinds + [WARP] * len(warp), names + wnames
    q, kind, names, slots = _arrange(list(_clean2d()), planted, kinds, names)
    off = None
    if offsets:
        off = np.tile(np.float32(OFFSET), (len(q), 1))
        at = np.flatnonzero(slots)[len(planted) - n_bad_off:]
        for k, i in enumerate(at):
            off[i, k // len(BAD)] = np.float32(BAD[k % len(BAD)])
    return Planted(q, kind, names, 2, bc.R2D, off)


def contract2d(queue, solver, conv=bc.CONV, stop=STOP2D):
    """What the contract table says about records rejected at the guard: `queue` with the ZNCC rewritten (NR2D1: its branch)."""
    import oracle
    P = oracle.P2
    out = np.array(queue, dtype=np.float32, copy=True)
    z = queue[:, P["zncc"]]
    with np.errstate(invalid="ignore"):
        if solver != "nr2d1":
            out[:, P["zncc"]] = np.where(z >= 0, np.float32(-3), z)
            return out
        zn = np.where(z < -1, z, np.float32(-1))                                                    # src/oc_nr.cpp:165-171
        zn = np.where((queue[:, P["convergence"]] >= np.float32(conv)) & (queue[:, P["iteration"]] >= np.float32(stop)), np.float32(-4), zn)
        bad = np.isnan(zn) | np.isnan(queue[:, P["u"]]) | np.isnan(queue[:, P["v"]])               # :304-316
    out[:, P["u"]] = np.where(bad, queue[:, P["u0"]], queue[:, P["u"]])
    out[:, P["v"]] = np.where(bad, queue[:, P["v0"]], queue[:, P["v"]])
    out[:, P["zncc"]] = np.where(bad, np.float32(-5), zn)
    return out


def oracle2d(solver, case, order, adaptive=False):
    """The oracle's records of a Planted 2D queue (a copy)."""
    return bc.oracle2d(solver, PAIR2D, case.queue, order, offsets=case.offsets, adaptive=adaptive, stop=STOP2D)


def expected2d(solver, case, order, adaptive=False, solved=None):
    """COORD and CONTROL records from the contract, every other one from the oracle (`solved`: its records, if already there)."""
    want = oracle2d(solver, case, order, adaptive) if solved is None else solved.copy()
    m = case.by_contract
    want.view(np.uint32)[m] = bits(contract2d(case.queue, solver))[m]
    return want


# ---- ICGN3D1 ---------------------------------------------------------------------------------------------------------------------
def _clean3d():
    import oracle
    P = oracle.P3
    zs, ys, xs = np.meshgrid(np.float32((10, 18, 28)), np.float32((12, 20, 30)), np.float32((12, 20, 28, 36)), indexing="ij")
    q = oracle.make_pois3d(xs.ravel(), ys.ravel(), zs.ravel())
    for a, f in enumerate("uvw"):
        q[:, P[f]] = bc.T3D[a]
    return q


@functools.lru_cache(maxsize=None)
def queue3d():
    """The queue of ICGN3D1 on bc.pair3d(*PAIR3D) with bc.R3D: every subset of axes NaN (all three: the most negative address the
    unguarded kernel would form), the finite axes mid-volume and on the low / high guard edges."""
    import oracle
    P = oracle.P3
    dz, dy, dx = bc.SHAPE3D
    r = bc.R3D
    size = (dx, dy, dz)

    def blank():
        return np.zeros(oracle.POI3D_FLOATS, np.float32)

    def blank_at():
        rec = blank()
        rec[P["x"]], rec[P["y"]], rec[P["z"]] = 20.0, 20.0, 18.0
        for a, f in enumerate("uvw"):
            rec[P[f]] = bc.T3D[a]
        return rec

    planted, kinds, names = _coord_records(3, blank, (20.0, 20.0, 18.0), tuple(float(v) for v in r),
                                           tuple(float(size[a] - 1 - r[a]) for a in range(3)))
    warp, wnames = _warp_records(3, ("ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz"), blank_at)
    planted, kinds, names = planted + warp, kinds + [WARP] * len(warp), names + wnames
    q, kind, names, _ = _arrange(list(_clean3d()), planted, kinds, names)
    return Planted(q, kind, names, 3, bc.R3D)


def contract3d(queue):
    import oracle
    Z = oracle.P3["zncc"]
    out = np.array(queue, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        out[:, Z] = np.where(queue[:, Z] >= 0, np.float32(-3), queue[:, Z])
    return out


def oracle3d(case, order, lanes):
    return bc.oracle3d((PAIR3D, bc.SHAPE3D, bc.R3D, bc.STOP3D), case.queue, order, lanes)


def expected3d(case, order, lanes, solved=None):
    want = oracle3d(case, order, lanes) if solved is None else solved.copy()
    m = case.by_contract
    want.view(np.uint32)[m] = bits(contract3d(case.queue))[m]
    return want


# ---- FFTCC -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fftcc_queue2d(rx, ry):
    """FFTCC2D on bc.pair2d(*PAIR2D): its guard truncates to int (src/oc_fftcc.cpp:190-196), and the planted records -- COORD,
    CONTROL and NaN / +-inf in the guess u, v (GUESS) -- stay untouched."""
    import oracle
    P = oracle.P2
    h, w = bc.SHAPE2D
    mid = (56.0, 48.0)
    nx, ny = 8, 8
    xs, ys = np.meshgrid(np.linspace(rx + 2, w - rx - 4, nx).round().astype(np.float32),
                         np.linspace(ry + 2, h - ry - 4, ny).round().astype(np.float32))
    clean = oracle.make_pois2d(xs.ravel(), ys.ravel())
    odd = np.arange(len(clean)) % 4 == 1          # (one record in four at a fractional position: the r = 16 kernel pairs POIs per wave)
    clean[odd, P["x"]] += 0.5
    clean[:, P["u"]], clean[:, P["v"]] = 1.0, 1.0

    def blank():
        return np.zeros(oracle.POI2D_FLOATS, np.float32)

    def blank_at():
        rec = blank()
        rec[P["x"]], rec[P["y"]] = mid
        return rec

    planted, kinds, names = _coord_records(2, blank, mid, (float(rx), float(ry)), (float(w - rx - 1), float(h - ry - 1)))
    guess, gnames = _warp_records(2, ("u", "v"), blank_at)
    planted, kinds, names = planted + guess, kinds + [GUESS] * len(guess), names + gnames
    q, kind, names, _ = _arrange(list(clean), planted, kinds, names)
    return Planted(q, kind, names, 2, (rx, ry))


@functools.lru_cache(maxsize=None)
def fftcc_queue3d():
    """FFTCC3D on bc.pair3d(*PAIR3D): clean records mid-volume and records with NaN coordinates (every subset of axes, the four
    encodings).  No guard: what is pinned is that every kernel agrees with the rocFFT pipeline on them."""
    import oracle
    P = oracle.P3
    zs, ys, xs = np.meshgrid(np.float32((16, 20, 24)), np.float32((18, 22, 26)), np.float32((18, 22, 26, 30)), indexing="ij")
    clean = oracle.make_pois3d(xs.ravel(), ys.ravel(), zs.ravel())
    clean[:, P["u"]], clean[:, P["v"]], clean[:, P["w"]] = 1.0, 1.0, 1.0
    planted, names = [], []
    for word in NAN_BITS:
        for s in range(1, 8):
            rec = np.zeros(oracle.POI3D_FLOATS, np.float32)
            for a, ax in enumerate("xyz"):
                if s >> a & 1:
                    _set_bits(rec, P[ax], word)
                else:
                    rec[P[ax]] = (22.0, 22.0, 20.0)[a]
            planted.append(rec)
            names.append("NaN %08x in %s" % (word, "".join(ax for a, ax in enumerate("xyz") if s >> a & 1)))
    q, kind, names, _ = _arrange(list(clean) + list(clean), planted, [COORD] * len(planted), names)
    return Planted(q, kind, names, 3, None)


# ---- long queues for the locality schedules -----------------------------------------------------------------------------------------
def long_queue(case, want, at_least, run=64):
    """`case.queue` repeated to `at_least` records, with a run of `run` consecutive COORD records in the middle; -> (queue, expected),
    `want` being the expected records of `case.queue` (per-POI solves do not depend on the position in the queue)."""
    coord = np.flatnonzero(case.kind == COORD)
    pick = coord[np.arange(run) % len(coord)]
    reps = -(-at_least // len(case.queue))
    half = reps // 2
    parts_q = [case.queue] * half + [case.queue[pick]] + [case.queue] * (reps - half)
    parts_w = [want] * half + [want[pick]] + [want] * (reps - half)
    q = np.empty((sum(len(p) for p in parts_q), case.queue.shape[1]), np.float32)
    w = np.empty_like(q)
    q.view(np.uint32)[:] = np.concatenate([bits(p) for p in parts_q])
    w.view(np.uint32)[:] = np.concatenate([bits(p) for p in parts_w])
    return q, w

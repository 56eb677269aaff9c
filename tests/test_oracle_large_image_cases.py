"""tests/large_image_cases.py on a CPU: the method is proved on the oracle before the GPU is trusted with it.

  * arithmetic: the shapes sit at the limits capi.hip states, the seam rows are where the byte offsets pass 2^31;
  * locality: the prepare fields of a crop are those of the image it was cut from, inside the stated margins and up to true edges;
  * origin invariance: stop_condition = 1 (and FFTCC2D outright) writes the same bits on the crop and on an embedding;
  * the restriction is real: with stop_condition = 2 and an origin of 2^20 records differ;
  * sharpness: a swapped table plane, or table entries / pixels missing from the seam row on, change a result;
  * conditions on the data: the oracle alone converges on the blocks, guard trippers keep the reference's codes, and no FFTCC
    peak is a near tie that two correct implementations could decide differently.
"""
import functools

import numpy as np
import pytest

import large_image_cases as lc
import oracle

P = lc.P
EMBED = (900, 1100)
ALL_BLOCKS = [(key, b) for key, blocks in lc.BLOCKS.items() for b in blocks]
IDS = ["%s-%s" % (key, b.name) for key, b in ALL_BLOCKS]
TWINS = ("onepass1", "onepass2")


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------
def test_shapes_sit_at_the_limits():
    h, w = lc.ICGN_LIMIT
    assert h * w == 1 << 28 and lc.accepted("icgn", h, w) and not lc.accepted("icgn", h + 1, w) and not lc.accepted("nr", h, w)
    assert lc.table_offset(lc.ICGN_LIMIT, h - 1, w - 1) == (1 << 32) - 16           # the last entry of a plane
    h, w = lc.NR_LIMIT
    assert h * w == 1 << 26 and lc.accepted("nr", h, w) and not lc.accepted("nr", h + 1, w)
    assert lc.table_offset(lc.NR_LIMIT, h - 1, w - 1, plane=3) == (1 << 32) - 16    # vector part + 3 * plane
    h, w = lc.FFTCC_LIMIT
    assert h * w == 1 << 30 and lc.accepted("fftcc", h, w) and not lc.accepted("fftcc", h + 1, w) and not lc.accepted("icgn", h, w)
    assert lc.image_offset(lc.FFTCC_LIMIT, h - 1, w - 1) == (1 << 32) - 4
    for shape in lc.REFUSED_FFTCC:
        assert not lc.accepted("fftcc", *shape)
    assert lc.accepted("fftcc", 5, (1 << 24) - 1)
    for h, w in lc.WIDE:
        assert lc.accepted("icgn", h, w) and not lc.accepted("nr", h, w) and (1 << 22) - 8 < w < 1 << 22 and 4 * w > 1 << 24 - 1
        assert w - lc.BW >= 1 << 21          # the blocks' x coordinates lie in [2^21, 2^22): an ulp of 0.25
    assert lc.WIDE[0][1] % 4 == 0 and lc.WIDE[1][1] % 4 != 0                        # the 16-byte and the scalar prepare kernels
    h, w = lc.TALL
    assert lc.accepted("icgn", h, w) and not lc.accepted("nr", h, w) and (1 << 22) - 8 < h < 1 << 22
    assert [h for h, _ in lc.ROWS[:3]] == [65535, 65536, 65537] and all(h * w < 1 << 20 for h, w in lc.ROWS)
    assert all(dz > 65535 or dy // 4 > 65535 for dz, dy, _ in lc.VOLUMES)


def test_seam_blocks_straddle_the_rows_where_offsets_pass_2_31():
    assert lc.ICGN_SEAM == 8192 and lc.table_offset(lc.ICGN_LIMIT, 8192) == 1 << 31 and lc.table_offset(lc.ICGN_LIMIT, 8191, 16383) == (1 << 31) - 16
    assert lc.FFTCC_SEAM == 16384 and lc.image_offset(lc.FFTCC_LIMIT, 16384) == 1 << 31 and lc.image_offset(lc.FFTCC_LIMIT, 16383, 32767) == (1 << 31) - 4
    for key, seam in (("ICGN_LIMIT", lc.ICGN_SEAM), ("FFTCC_LIMIT", lc.FFTCC_SEAM)):
        b = lc.BLOCKS[key][1]
        assert b.name == "seam" and b.y0 + lc.BH // 2 == seam and not (b.top or b.left or b.bottom or b.right)
        for guesses in ("int", "half"):
            q, n = lc.solver_queue(b, guesses)
            y = q[:n, P["y"]] + b.y0
            assert (y < seam).sum() >= 6 and (y >= seam).sum() >= 6             # POIs on both sides, subsets across the seam
            assert ((y - lc.R_ICGN[1] < seam) & (y + lc.R_ICGN[1] >= seam)).any()
    # NR2D1: a plane is 2^30 bytes, so the scalar parts ARE the boundaries and both rows the sums pass them at are row 0
    assert lc.NR_PLANE == 1 << 30 and lc.NR_SEAMS == (0, 0)
    assert lc.table_offset(lc.NR_LIMIT, 0, plane=2) == 1 << 31 and lc.table_offset(lc.NR_LIMIT, 0, plane=3) == (1 << 32) - (1 << 30)
    b = lc.BLOCKS["NR_LIMIT"][1]
    assert b.top and b.left and not b.bottom and not b.right
    for key, blocks in lc.BLOCKS.items():
        c = blocks[0]
        assert c.bottom and c.right and c.shape == lc.SHAPES[key]


def test_queues_hold_what_they_claim():
    for key, b in ALL_BLOCKS:
        for guesses in ("int", "half"):
            q, n = lc.solver_queue(b, guesses)
            assert 24 <= n and len(q) <= 120, (key, b.name, len(q))
            assert (q[:, :2] == np.round(q[:, :2])).all() and (2 * q[:, [P["u"], P["v"]]] == np.round(2 * q[:, [P["u"], P["v"]]])).all()
            frac = q[:, P["u"]] != np.round(q[:, P["u"]])
            assert frac.all() if guesses == "half" else not frac.any()
            trip = _trips(b, q, *lc.R_ICGN)
            assert not trip[:n].any()
            for edge in ("right", "bottom", "left", "top"):
                if getattr(b, edge):
                    assert trip[n:].any() and (~trip[n:]).any(), (key, b.name, edge)
            if not (b.top or b.left or b.bottom or b.right):
                assert len(q) == n


def _trips(block, q, rx, ry):
    """the geometric part of the guard, with the crop's edges counted only where they are the image's"""
    x, y = q[:, P["x"]], q[:, P["y"]]
    return ((block.left & (x - rx < 0)) | (block.right & (x + rx > block.bw - 1)) | (block.top & (y - ry < 0)) | (block.bottom & (y + ry > block.bh - 1)))


# ---- embeddings -------------------------------------------------------------------------------------------------------------------
def _placements(block):
    """(somewhere inside a moderate zero image, the crop's true edges kept) -- a thin block keeps its thin side in both"""
    thin_h, thin_w = block.top and block.bottom, block.left and block.right
    shape = (block.bh if thin_h else EMBED[0], block.bw if thin_w else EMBED[1])
    inner = block.at(shape, 0 if thin_h else 333, 0 if thin_w else 401)
    y0 = 0 if block.top else shape[0] - block.bh if block.bottom else 333
    x0 = 0 if block.left else shape[1] - block.bw if block.right else 401
    return inner, block.at(shape, y0, x0)


@functools.lru_cache(maxsize=None)
def _embedded(block):
    ref, tar = lc.embed(block)
    return ref, tar, oracle.Prepared2D(ref, tar), oracle.PreparedNR2D(ref, tar)


def _cut(field, block, ys, xs):
    return field[block.y0:block.y0 + block.bh, block.x0:block.x0 + block.bw][ys, xs]


@pytest.mark.parametrize("key,block", ALL_BLOCKS, ids=IDS)
def test_fields_of_a_crop_are_the_fields_of_the_image(key, block):
    icgn, nr = lc.crop_fields(block)
    inner, flush = _placements(block)
    assert (inner.y0, inner.x0) != (0, 0) or (block.top and block.bottom) or (block.left and block.right)
    assert (flush.top, flush.left, flush.bottom, flush.right) == (block.top, block.left, block.bottom, block.right)
    for e in (inner, flush):
        _, _, p2, pnr = _embedded(e)
        tgx, tgy = oracle.gradient2d(pnr.tar)
        got_icgn = dict(gx=p2.gx, gy=p2.gy, lut=p2.lut)
        got_nr = dict(gx=tgx, gy=tgy, lut=pnr.lut, lut_gx=pnr.lut_gx, lut_gy=pnr.lut_gy)
        for want, got in ((icgn, got_icgn), (nr, got_nr)):
            for name in want:
                ys, xs = lc.inside(e, lc.NR_MARGIN if name in ("lut_gx", "lut_gy") else lc.FIELD_MARGIN)
                a, b = _cut(got[name], e, ys, xs), want[name][ys, xs]
                assert a.size >= 0.8 * want[name].size and np.array_equal(lc.bits(a), lc.bits(b)), (key, block.name, name, (e.y0, e.x0))
                assert np.abs(b).max() > 1.0
        # ... and nothing but +0 outside the block and its two-pixel (NR2D1: four-pixel) skirt
        skirt = np.ones(e.shape, dtype=bool)
        skirt[max(0, e.y0 - 4):e.y0 + e.bh + 4, max(0, e.x0 - 4):e.x0 + e.bw + 4] = False
        for f in (p2.gx, p2.gy, p2.lut, pnr.lut_gx, pnr.lut_gy):
            assert not lc.bits(f)[skirt].any()


# ---- origin invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,block", ALL_BLOCKS, ids=IDS)
def test_stop_1_writes_the_same_bits_at_any_origin(key, block):
    p2, pnr = lc.prepared(block)
    for e in _placements(block):
        _, _, ep2, epnr = _embedded(e)
        for guesses in ("int", "half"):
            q, n = lc.solver_queue(block, guesses)
            for solver in lc.SOLVERS + TWINS:
                for order in ((oracle.ORDER_LANES,) if solver in TWINS or solver == "nr2d1" else (oracle.ORDER_LANES, oracle.ORDER_LANES_FMA)):
                    want = lc.solve(solver, p2, pnr, q, order)
                    keep = _comparable(block, e, q)
                    assert keep.sum() >= 12
                    got = lc.solve(solver, ep2, epnr, lc.shift(q, e)[keep], order)
                    lc.assert_same_but_xy(got, want[keep], "%s %s %s %s order %x at %s" % (key, block.name, guesses, solver, order, (e.y0, e.x0)))
                    assert (got[:, :2] != want[keep][:, :2]).any() or (e.y0, e.x0) == (0, 0)


def _comparable(block, e, q, rx=lc.R_ICGN[0], ry=lc.R_ICGN[1]):
    """the POIs whose results the crop and the embedding share: where an edge of the crop is an edge of the image in one and not in
    the other, only those that keep radius + MARGIN from it"""
    x, y = q[:, P["x"]], q[:, P["y"]]
    keep = np.ones(len(q), dtype=bool)
    for mine, theirs, d, r in ((block.left, e.left, x, rx), (block.right, e.right, block.bw - 1 - x, rx), (block.top, e.top, y, ry),
                               (block.bottom, e.bottom, block.bh - 1 - y, ry)):
        if mine != theirs:
            keep &= d >= r + lc.MARGIN
    return keep


def _fftcc_cases(key, block):
    if key == "FFTCC_LIMIT":
        return [(r, False) for r in sorted(set(r for r, _, _, _ in lc.FFTCC_FAMILIES))]
    if key in ("WIDE0", "WIDE1", "TALL"):
        return [(r, True) for r in lc.R_THIN]
    return []


@pytest.mark.parametrize("key,block", [kb for kb in ALL_BLOCKS if _fftcc_cases(*kb)], ids=[i for i, kb in zip(IDS, ALL_BLOCKS) if _fftcc_cases(*kb)])
def test_fftcc_writes_the_same_bits_at_any_origin_and_has_no_near_ties(key, block):
    ref, tar = lc.crop(block)
    _, flush = _placements(block)
    eref, etar, _, _ = _embedded(flush)
    for (rx, ry), thin in _fftcc_cases(key, block):
        q, n = lc.fftcc_queue(block, rx, ry, thin)
        fits = min(block.bh - 2 * ry, block.bw - 2 * rx) > 0
        assert (n >= (8 if thin else 20)) == fits and (fits or n == 0) and (len(q) > n) == (block.top or block.left or block.bottom or block.right)
        want = lc.fftcc(ref, tar, rx, ry, q)
        got = lc.fftcc(eref, etar, rx, ry, lc.shift(q, flush))
        lc.assert_same_but_xy(got, want, "%s %s FFTCC %dx%d" % (key, block.name, rx, ry))
        untouched = (want[:, P["zncc"]] == 0) & (want[:, P["u0"]] == 0)
        assert not untouched[:n].any() and untouched[n:].any() == (len(q) > n)        # guard trippers come back as they went in
        # the peak: 1e-4 of its height above every other bin, more than three times the widest ZNCC bar (3e-5, a ZNCC being the
        # peak over the norms): two correct implementations cannot decide such a scan differently
        for i in range(n):
            one = q[i:i + 1].copy()
            surf = np.sort(oracle.fftcc2d(ref, tar, rx, ry, one, want_surface=True).ravel())
            assert surf[-1] > 0 and surf[-1] - surf[-2] >= 1e-4 * surf[-1], (key, block.name, rx, ry, i, surf[-3:])
        assert n == 0 or (want[:n, P["zncc"]] > 0.5).mean() > 0.9


# ---- the restriction is real ------------------------------------------------------------------------------------------------------
def _far_embedding(block, x0):
    """A Prepared2D of a (block.bh, x0 + block.bw) zero image with the block at its right end, assembled from the crop's own fields
    (proved equal above) in arrays whose untouched pages cost nothing: right inside the block's left margin, which is all a queue
    of this file reads."""
    shape = (block.bh, x0 + block.bw)
    p2, _ = lc.prepared(block)
    far = oracle.Prepared2D.__new__(oracle.Prepared2D)
    for name in ("ref", "tar", "gx", "gy", "lut"):
        src = getattr(p2, name)
        a = np.zeros(shape + src.shape[2:], dtype=np.float32)
        a[:, x0:] = src
        setattr(far, name, a)
    return far


def test_from_the_second_iteration_on_the_origin_shows():
    block = lc.BLOCKS["WIDE0"][0]                      # top, bottom and right edges true: the crop is the image's right end
    far = _far_embedding(block, 1 << 20)
    p2, pnr = lc.prepared(block)
    e = block.at(far.ref.shape, 0, 1 << 20)
    q, n = lc.solver_queue(block, "half")
    moved = lc.shift(q, e)
    assert moved[:, P["x"]].min() >= 1 << 20
    for solver in ("icgn2d1", "icgn2d2"):
        one = lc.solve(solver, far, None, moved)
        lc.assert_same_but_xy(one, lc.solve(solver, p2, pnr, q), solver + " stop 1 at 2^20")
        two_far, two = lc.solve(solver, far, None, moved, stop=2, conv=1e-7), lc.solve(solver, p2, pnr, q, stop=2, conv=1e-7)
        assert (two[:n, P["iteration"]] == 2).all()
        assert len(lc.differing(two_far, two)) > 0, solver


# ---- sharpness --------------------------------------------------------------------------------------------------------------------
def _changed(a, b, n):
    return len(set(lc.differing(a, b)[:, 0].tolist()) & set(range(n)))


@pytest.mark.parametrize("key", ["ICGN_LIMIT", "NR_LIMIT"])
def test_a_wrong_plane_or_a_fetch_lost_at_the_seam_changes_a_result(key):
    block = lc.BLOCKS[key][1]
    _, e = _placements(block)
    eref, etar, ep2, epnr = _embedded(e)
    seam = e.y0 + lc.BH // 2
    rows, cols = slice(e.y0, e.y0 + e.bh), slice(e.x0, e.x0 + e.bw)
    solvers = ("nr2d1",) if key == "NR_LIMIT" else ("icgn2d1", "icgn2d2", "iclm2d1", "iclm2d2")
    tables = ("lut", "lut_gx", "lut_gy") if key == "NR_LIMIT" else ("lut",)
    half, n = lc.solver_queue(block, "half")
    whole, _ = lc.solver_queue(block, "int")
    half, whole = lc.shift(half, e), lc.shift(whole, e)
    for solver in solvers:
        base = lc.solve(solver, ep2, epnr, half)
        prep = epnr if solver == "nr2d1" else ep2
        for table in tables:
            kept = getattr(prep, table)
            for a, b in ((0, 1), (1, 2), (2, 3), (0, 3)):
                bad = kept.copy()
                bad[rows, cols, 4 * a:4 * a + 4], bad[rows, cols, 4 * b:4 * b + 4] = kept[rows, cols, 4 * b:4 * b + 4], kept[rows, cols, 4 * a:4 * a + 4]
                setattr(prep, table, bad)
                assert _changed(lc.solve(solver, ep2, epnr, half), base, n) > 0, (solver, table, "planes", a, b)
            bad = kept.copy()
            bad[seam:e.y0 + e.bh, cols] = 0
            setattr(prep, table, bad)
            assert _changed(lc.solve(solver, ep2, epnr, half), base, n) > 0, (solver, table, "entries from the seam row on")
            setattr(prep, table, kept)
        # the integer set reads values (the value plane on the GPU): the sampled image zeroed from the seam row on
        cut = etar.copy()
        cut[seam:] = 0
        base = lc.solve(solver, ep2, epnr, whole)
        assert _changed(lc.solve(solver, oracle.Prepared2D(eref, cut), oracle.PreparedNR2D(eref, cut), whole), base, n) > 0, (solver, "pixels")


def test_pixels_lost_at_the_seam_change_an_fftcc_result():
    block = lc.BLOCKS["FFTCC_LIMIT"][1]
    _, e = _placements(block)
    eref, etar, _, _ = _embedded(e)
    seam = e.y0 + lc.BH // 2
    for image in (0, 1):
        pair = [eref.copy(), etar.copy()]
        pair[image][seam:] = 0
        for (rx, ry), _, _, bar in lc.FFTCC_FAMILIES[:-1]:
            q, n = lc.fftcc_queue(block, rx, ry)
            q = lc.shift(q, e)
            base, cut = lc.fftcc(eref, etar, rx, ry, q), lc.fftcc(pair[0], pair[1], rx, ry, q)
            assert (np.abs(cut[:n, P["zncc"]] - base[:n, P["zncc"]]) > 100 * bar).any(), (image, rx, ry)


# ---- conditions on the data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,block", ALL_BLOCKS, ids=IDS)
def test_the_oracle_alone_converges_on_the_blocks(key, block):
    p2, pnr = lc.prepared(block)
    ref, tar = lc.crop(block)
    assert ref.min() >= 30.0 and tar.min() >= 30.0
    for guesses in ("int", "half"):
        q, n = lc.solver_queue(block, guesses)
        trip = _trips(block, q, *lc.R_ICGN)
        for solver in lc.SOLVERS + TWINS:
            want = lc.solve(solver, p2, pnr, q)
            good = (want[:, P["zncc"]] > 0.9) & (want[:, P["iteration"]] == 1)
            assert good[~trip].mean() >= 0.9, (key, block.name, guesses, solver, want[~trip, P["zncc"]])
            assert ((~trip).sum() > n) == (len(q) > n)
            # src/oc_icgn.cpp:160-167 / src/oc_iclm.cpp (-3), src/oc_nr.cpp:165-171 (-1): the record is otherwise left as it came
            code = -1.0 if solver == "nr2d1" else -3.0
            assert (want[trip, P["zncc"]] == code).all(), (key, block.name, solver)
            if solver != "nr2d1":
                assert np.array_equal(lc.bits(want[trip][:, :16]), lc.bits(q[trip][:, :16]))
            if not solver.startswith("iclm") and solver != "nr2d1" and (~trip[n:]).any():
                # ICGN ends a POI whose subset reaches the +0 border of the table with -3 as well (src/oc_icgn.cpp:251-255)
                assert (want[n:][~trip[n:], P["zncc"]] == -3.0).any()


def test_the_rows_images_converge():
    for shape in lc.ROWS:
        ref, tar = lc.rows_pair(shape)
        q, r = lc.rows_queue(shape), lc.rows_radius(shape)
        want = q.copy()
        oracle.icgn2d1(oracle.Prepared2D(ref, tar), r, r, lc.ROWS_CONV, lc.ROWS_STOP, want, order=oracle.ORDER_LANES, lanes=64)
        h = shape[0]
        y = q[:, P["y"]]
        # the subset leaves the image (the guard), or its last row reaches the table's +0 border: -3 both; everything else is solved
        solved = y + r <= h - 2
        assert (y + r > h - 1).any() and (y + r == h - 1).any() and (want[~solved, P["zncc"]] == -3.0).all()
        assert solved.sum() >= 2 and (want[solved, P["zncc"]] > 0.9).all() and (want[solved, P["iteration"]] >= 2).all(), (shape, want[:, P["zncc"]])
        assert np.abs(want[solved, P["u"]] - 0.3).max() < 0.05 and np.abs(want[solved, P["v"]] + 0.2).max() < 0.05
        ys = set(y.astype(int))
        assert {v for v in (65534, 65535, 65536, 65537) if v + r <= h - 1} <= ys and h - 1 - r in ys

"""tests/large_volume_cases.py on a CPU: the method is proved on the oracle before the GPU is trusted with it.

  * arithmetic: the seam blocks hold voxels on both sides of the offsets they are named for, every SLAB subset's box spans between
    2^31 and 2^32 voxels, REFUSED's spans 2^32 or more and one row per plane less does not;
  * the walk: Walk3 and RowWalk restated in wrapping 32-bit arithmetic give every sample's exact offset at INDEX31 and SLAB with their
    radii, and offsets 2^32 too small at REFUSED -- the rule of host/volume_limits.h, checked on both sides;
  * locality: the prepare fields of a crop are those of the volume it was cut from, inside the stated margins and up to true faces;
  * origin invariance: stop_condition = 1 (and FFTCC3D outright) writes the same bits on the crop and on an embedding;
  * sharpness: samples fetched 2^32 voxels too low (zeros, in REFUSED's geometry) change a result in bits and in ZNCC;
  * conditions on the data: the oracle alone converges on the blocks, guard trippers keep their records, and no FFTCC peak is a near
    tie that two correct implementations could decide differently.
"""
import functools

import numpy as np
import pytest

import large_volume_cases as lv
import oracle

P = lv.P
ALL_BLOCKS = [(key, b) for key, blocks in lv.BLOCKS.items() for b in blocks]
SOLVED_BLOCKS = [(key, b) for key, b in ALL_BLOCKS if key != "REFUSED"]
IDS = ["%s-%s" % (key, b.name) for key, b in ALL_BLOCKS]
SOLVED_IDS = ["%s-%s" % (key, b.name) for key, b in SOLVED_BLOCKS]
CPU_CONTRACTS = ("lanes", "fma", "onepass")


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_shapes_and_seams_are_where_the_comments_say():
    dz, dy, dx = lv.INDEX31
    assert dz * dy * dx == 2148353100 and dz * dy * dx > 1 << 31 and dx % 4 != 0
    assert lv.SEAM30 == (644, 953, 341) and lv.SEAM31 == (1289, 616, 682)
    assert lv.voxel_index(lv.INDEX31, *lv.SEAM30) == 1 << 30 and lv.voxel_index(lv.INDEX31, *lv.SEAM31) == 1 << 31
    seam30, seam31, far = lv.BLOCKS["INDEX31"]
    for b, seam, index in ((seam30, lv.SEAM30, 1 << 30), (seam31, lv.SEAM31, 1 << 31)):
        first = lv.voxel_index(b.shape, *b.origin)
        last = lv.voxel_index(b.shape, *(o + n - 1 for o, n in zip(b.origin, b.size)))
        assert first < index - 10 ** 6 and last > index and all(o <= s < o + n for o, s, n in zip(b.origin, seam, b.size))
        # the seam voxel's row holds voxels on both sides, 8 or more inside the block
        assert b.x0 + 8 <= seam[2] < b.x0 + b.bx - 8 and b.y0 + 8 <= seam[1] < b.y0 + b.by - 8
    assert not any(seam30.lo) and not any(seam30.hi)
    assert seam31.hi == (True, False, False) and not any(seam31.lo)          # voxel index 2^31 lies in the last plane
    assert far.hi == (True, True, True) and lv.voxel_index(far.shape, *(o + n - 1 for o, n in zip(far.origin, far.size))) == dz * dy * dx - 1
    dz, dy, dx = lv.SLAB
    assert dz * dy * dx == 2434961408 and dx % 4 == 0 and dy * dx == 35808256
    near, far = lv.BLOCKS["SLAB"]
    assert near.lo == (True, True, True) and near.hi == (True, False, False) and far.lo == (True, False, False) and far.hi == (True, True, True)
    assert lv.voxel_index(lv.SLAB, 59, far.y0, far.x0) > 1 << 31 > lv.voxel_index(lv.SLAB, 58, dy - 1, dx - 1)      # the far block's planes 59 ... 67
    dz, dy, dx = lv.REFUSED
    (b,) = lv.BLOCKS["REFUSED"]
    assert b.same and b.hi == (True, True, True) and b.lo == (True, False, False) and 4 * dz * dy * dx < 19 * 10 ** 9
    assert lv.voxel_index(lv.REFUSED, 14, b.y0, b.x0) > 1 << 32 > lv.voxel_index(lv.REFUSED, 13, b.y0, b.x0)      # the block's last plane (and the end of plane 13)
    for radii, _, _, _ in lv.FFTCC_REFUSED:
        assert (lv.fftcc_queue(b, radii)[:, P["z"]] + radii[2] - 1 >= 14).sum() >= 4     # windows that hold that plane


def test_spans_lie_on_the_stated_side_of_2_31_and_2_32():
    _, dy, dx = lv.SLAB
    assert lv.box_span(*lv.R_SLAB, dy, dx) == 2148531270
    assert 1 << 31 <= lv.box_span(*lv.R_SLAB, dy, dx) < 1 << 32 and lv.accepted(*lv.R_SLAB, dy, dx)
    for r in lv.ROWS_RADII["SLAB"]:
        assert lv.box_span(*r, dy, dx) == 2148531292 and lv.accepted(*r, dy, dx) and 2 * r[0] + 1 >= 28
    _, dy, dx = lv.INDEX31
    for r in lv.RADII["INDEX31"] + lv.ROWS_RADII["INDEX31"]:
        assert lv.box_span(*r, dy, dx) < 1 << 31 and lv.accepted(*r, dy, dx)
    assert all(2 * r[0] + 1 >= 28 for r in lv.ROWS_RADII["INDEX31"])          # wide enough for the row kernel's own walk
    _, dy, dx = lv.REFUSED
    assert lv.box_span(*lv.R_REFUSED, dy, dx) == 4295203440 >= 1 << 32 and not lv.accepted(*lv.R_REFUSED, dy, dx)
    assert lv.box_span(*lv.R_REFUSED, dy - 1, dx) == 4294958202 < 1 << 32 and lv.accepted(*lv.R_REFUSED, dy - 1, dx)
    # a radius triple whose span fits is not refused on the same volume
    assert lv.accepted(16, 16, 6, dy, dx) and not lv.accepted(1, 1, 7, dy, dx)
    assert lv.accepted(0, 0, 1, 65536, 32767) and not lv.accepted(0, 0, 1, 65536, 32768) and lv.accepted(2, 1, 0, 1 << 30, (1 << 31) - 3)


# ---- the walk -----------------------------------------------------------------------------------------------------------------------
def _walk(radii, dy, dx, threads):
    rx, ry, rz = radii
    n = (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1)
    got = {}
    for tid in range(threads):
        for s, off in lv.walk_offsets(rx, ry, rz, dy, dx, tid, threads):
            assert s not in got and s % threads == tid
            got[s] = off
    assert sorted(got) == list(range(n))
    exact = [lv.exact_offset(rx, ry, s, dy, dx) for s in range(n)]
    return [got[s] for s in range(n)], exact


def _row_walk(radii, dy, dx, halves=16):
    rx, ry, rz = radii
    rows = (2 * ry + 1) * (2 * rz + 1)
    got = {}
    for h in range(halves):
        got.update(lv.row_walk_offsets(ry, rz, dy, dx, h, halves))
    assert sorted(got) == list(range(rows))
    return [got[r] for r in range(rows)], [(r // (2 * ry + 1) * dy + r % (2 * ry + 1)) * dx for r in range(rows)]


@pytest.mark.parametrize("threads", [512, 1024])
def test_the_32_bit_walk_is_exact_up_to_the_limit_and_wraps_beyond(threads):
    for key, radii in [(key, r) for key in ("INDEX31", "SLAB") for r in lv.RADII[key] + lv.ROWS_RADII[key]]:
        _, dy, dx = lv.SHAPES[key]
        got, exact = _walk(radii, dy, dx, threads)
        assert got == exact and max(exact) == lv.box_span(*radii, dy, dx), (key, radii)
        got, exact = _row_walk(radii, dy, dx)
        assert got == exact
    assert max(_walk(lv.R_SLAB, *lv.SLAB[1:], threads)[1]) >= 1 << 31                   # (the products of SLAB's walk pass int's range)
    _, dy, dx = lv.REFUSED
    got, exact = _walk(lv.R_REFUSED, dy, dx, threads)
    wrong = [s for s in range(len(exact)) if got[s] != exact[s]]
    # exactly the subset's last plane, every sample of it 2^32 voxels too low
    assert wrong == [s for s in range(len(exact)) if exact[s] >= 1 << 32] and len(wrong) == 7 * 7
    assert all(exact[s] - got[s] == 1 << 32 for s in wrong) and max(exact) == lv.box_span(*lv.R_REFUSED, dy, dx)
    got, exact = _row_walk(lv.R_REFUSED, dy, dx)
    assert [r for r in range(len(exact)) if got[r] != exact[r]] == list(range(14 * 7, 15 * 7))
    # one row per plane less: the same radii are served
    got, exact = _walk(lv.R_REFUSED, dy - 1, dx, threads)
    assert got == exact


# ---- embeddings ---------------------------------------------------------------------------------------------------------------------
EMBED = (96, 100, 110)


def _placements(block):
    """(somewhere inside a moderate zero volume, the crop's true faces kept).  A block that spans the volume along z keeps that in
    both."""
    shape = tuple(n if lo and hi else e for n, e, lo, hi in zip(block.size, EMBED, block.lo, block.hi))
    inner = block.at(shape, *(0 if lo and hi else o for o, lo, hi in zip((21, 23, 27), block.lo, block.hi)))
    flush = block.at(shape, *(0 if lo else s - n if hi else o for o, lo, hi, s, n in zip((21, 23, 27), block.lo, block.hi, shape, block.size)))
    return inner, flush


@functools.lru_cache(maxsize=None)
def _embedded(block):
    ref, tar = lv.embed(block)
    return ref, tar, oracle.Prepared3D(ref, tar)


@pytest.mark.parametrize("key,block", ALL_BLOCKS, ids=IDS)
def test_fields_of_a_crop_are_the_fields_of_the_volume(key, block):
    want = lv.crop_fields(block)
    inner, flush = _placements(block)
    assert (flush.lo, flush.hi) == (block.lo, block.hi) and any(inner.origin)
    for e in (inner, flush):
        _, _, prep = _embedded(e)
        for name, (field, margin) in want.items():
            sl = lv.inside(e, margin)
            a, b = getattr(prep, name)[e.slices][sl], field[sl]
            assert a.size >= (0.3 if name == "coef" else 0.7) * field.size and np.array_equal(lv.bits(a), lv.bits(b)), (key, block.name, name, e.origin)
            assert np.abs(b).max() > 1.0
        # ... and nothing but +0 in the gradients outside the block and its two-voxel skirt
        skirt = np.ones(e.shape, dtype=bool)
        skirt[tuple(slice(max(0, o - 2), o + n + 2) for o, n in zip(e.origin, e.size))] = False
        for f in (prep.gx, prep.gy, prep.gz):
            assert not lv.bits(f)[skirt].any()


def test_the_margins_are_needed():
    """one voxel less and an artificial face shows: the margins are the fields' reach, not slack"""
    block = lv.BLOCKS["INDEX31"][0]
    inner, _ = _placements(block)
    _, _, prep = _embedded(inner)
    for name, (field, margin) in lv.crop_fields(block).items():
        sl = lv.inside(inner, margin - 1)
        assert not np.array_equal(lv.bits(getattr(prep, name)[inner.slices][sl]), lv.bits(field[sl])), name


# ---- origin invariance ----------------------------------------------------------------------------------------------------------------
def _comparable(block, e, q, radii):
    """the POIs whose results the crop and the embedding share: where a face of the crop is a face of the volume in one and not in
    the other, only those that keep radius + MARGIN from it"""
    keep = np.ones(len(q), dtype=bool)
    for axis, (c, r) in enumerate(zip("zyx", radii[::-1])):
        pos, n = q[:, P[c]], block.size[axis]
        for mine, theirs, d in ((block.lo[axis], e.lo[axis], pos), (block.hi[axis], e.hi[axis], n - 1 - pos)):
            if mine != theirs:
                keep &= d >= r + lv.ICGN_MARGIN
    return keep


@pytest.mark.parametrize("key,block", SOLVED_BLOCKS, ids=SOLVED_IDS)
def test_stop_1_writes_the_same_bits_at_any_origin(key, block):
    prep = lv.prepared(block)
    for e in _placements(block):
        _, _, eprep = _embedded(e)
        for radii in lv.RADII[key] + lv.ROWS_RADII.get(key, []):
            for guesses in ("int", "half"):
                q, n = lv.solver_queue(block, guesses, radii)
                keep = _comparable(block, e, q, radii)
                assert keep.all() if (e.lo, e.hi) == (block.lo, block.hi) else keep.sum() >= 3
                for contract in CPU_CONTRACTS + ("rows",):
                    want = lv.solve(contract, prep, q, radii)
                    got = lv.solve(contract, eprep, lv.shift(q, e)[keep], radii)
                    lv.assert_same_but_xyz(got, want[keep], "%s %s %s %s %s at %s" % (key, block.name, radii, guesses, contract, e.origin))
                    assert (got[:, :3] != want[keep][:, :3]).any() or not any(e.origin)


def _fftcc_cases(key):
    return lv.FFTCC_REFUSED if key == "REFUSED" else lv.FFTCC_FAMILIES[:-1]      # (the rocFFT family repeats fused32's window)


@pytest.mark.parametrize("key,block", ALL_BLOCKS, ids=IDS)
def test_fftcc_writes_the_same_bits_at_any_origin_and_has_no_near_ties(key, block):
    ref, tar = lv.crop(block)
    _, flush = _placements(block)
    eref, etar, _ = _embedded(flush)
    for radii, family, _, bar in _fftcc_cases(key):
        q = lv.fftcc_queue(block, radii)
        assert len(q) >= 9
        want = lv.fftcc(ref, tar, radii, q)
        got = lv.fftcc(eref, etar, radii, lv.shift(q, flush))
        lv.assert_same_but_xyz(got, want, "%s %s FFTCC %s" % (key, block.name, radii))
        assert (want[:, P["zncc"]] > 0.5).all(), (key, block.name, radii, want[:, P["zncc"]])
        for c in ("u0", "v0", "w0"):
            assert np.array_equal(want[:, P[c]], q[:, P[c[0]]])
        if block.same:
            assert all(np.array_equal(lv.bits(want[:, P[c]]), lv.bits(np.zeros(len(q), dtype=np.float32))) for c in "uvw")
            assert np.abs(want[:, P["zncc"]] - 1).max() <= bar
        # the peak: 1e-4 of its height above every other bin, where the widest ZNCC bar is 2e-4 of a ZNCC that is the peak over the
        # norms -- but that bar is the noise of the reference's running SUMS of means and norms, which scale the whole surface and move
        # no bin against another; the transforms' own rounding is 1e-6 of the peak.  Two correct implementations decide alike.
        for i in range(len(q)):
            surf = lv.fftcc_surface(ref, tar, radii, q[i])
            order = np.argsort(surf)
            sx, sy = 2 * radii[0], 2 * radii[1]
            idx = int(order[-1])
            d = [idx % sx, idx // sx % sy, idx // (sx * sy)]
            d = [v - 2 * r if v > r else v for v, r in zip(d, radii)]
            assert [want[i, P[c]] - q[i, P[c]] for c in "uvw"] == d, (key, block.name, radii, i)
            assert surf[order[-1]] > 0 and surf[order[-1]] - surf[order[-2]] >= 1e-4 * surf[order[-1]], (key, block.name, radii, i, surf[order[-3:]])


# ---- sharpness ------------------------------------------------------------------------------------------------------------------------
def test_a_fetch_2_32_voxels_too_low_changes_bits_and_zncc():
    """REFUSED's geometry: the walk model puts every sample of the subset's last plane 2^32 voxels too low, which in the huge zero
    volume is a voxel outside the block: a zero in the reference and in its gradients.  The crop oracle tells.  (On a crop 24 planes
    deep: in REFUSED's own 15 planes a subset of 15 has no position inside the interpolatable range, which is why it is cheap.)"""
    (block,) = lv.BLOCKS["REFUSED"]
    dz, dy, dx = lv.REFUSED
    rx, ry, rz = lv.R_REFUSED
    # where the wrapped fetches land: 14 planes lower, outside the block's columns (so: zeros)
    first = lv.voxel_index(lv.REFUSED, *block.origin)
    for s in range(14 * 49, 15 * 49):
        z, y, x = lv.voxel_at(lv.REFUSED, first + lv.exact_offset(rx, ry, s, dy, dx) - (1 << 32))
        assert 0 <= z < dz and not (block.x0 - 8 <= x < dx and block.y0 - 8 <= y < dy)
    prep = oracle.Prepared3D(*lv._crop((24, block.by, block.bx), block.seed, True))
    q = oracle.make_pois3d([block.bx // 2, block.bx // 2 + 5, block.bx - 4 - rx], [block.by // 2, block.by // 2 - 4, block.by - 4 - ry], [10, 12, 9])
    right = lv.solve("lanes", prep, q, lv.R_REFUSED, stop=5, conv=0.001)
    assert (right[:, P["zncc"]] > 0.999).all()                 # (the target is the reference)
    for i in range(len(q)):
        bad = oracle.Prepared3D.__new__(oracle.Prepared3D)
        bad.tar, bad.coef = prep.tar, prep.coef
        last = int(q[i, P["z"]]) + rz
        for name in ("ref", "gx", "gy", "gz"):
            a = getattr(prep, name).copy()
            a[last] = 0
            setattr(bad, name, a)
        for contract in CPU_CONTRACTS:
            base = lv.solve(contract, prep, q[i:i + 1], lv.R_REFUSED, stop=5, conv=0.001)
            wrong = lv.solve(contract, bad, q[i:i + 1], lv.R_REFUSED, stop=5, conv=0.001)
            assert len(lv.differing(wrong, base)) > 0 and abs(float(wrong[0, P["zncc"]]) - float(base[0, P["zncc"]])) > 0.01, (i, contract)


def test_voxels_lost_beyond_the_seam_change_a_result():
    """the seam blocks: zeros from the seam voxel on (what a 31-bit or 32-bit byte offset would leave) change ICGN3D1's and FFTCC3D's
    records"""
    for block, seam in zip(lv.BLOCKS["INDEX31"][:2], (lv.SEAM30, lv.SEAM31)):
        ref, tar = (a.copy() for a in lv.crop(block))
        local = lv.voxel_index(block.size, *(s - o for s, o in zip(seam, block.origin)))
        for a in (ref, tar):
            a.reshape(-1)[local:] = 0
        cut = oracle.Prepared3D(ref, tar)
        for radii in lv.RADII["INDEX31"]:
            q, n = lv.solver_queue(block, "half", radii)
            assert len(lv.differing(lv.solve("lanes", cut, q, radii), lv.solve("lanes", lv.prepared(block), q, radii))) > 0, (block.name, radii)
    block = lv.BLOCKS["INDEX31"][0]
    ref, tar = (a.copy() for a in lv.crop(block))
    local = lv.voxel_index(block.size, *(s - o for s, o in zip(lv.SEAM30, block.origin)))
    tar.reshape(-1)[local:] = 0
    for radii, _, _, bar in lv.FFTCC_FAMILIES[:-1]:
        q = lv.fftcc_queue(block, radii)
        base, cut = lv.fftcc(*lv.crop(block), radii, q), lv.fftcc(ref, tar, radii, q)
        assert (np.abs(cut[:, P["zncc"]] - base[:, P["zncc"]]) > 100 * bar).any(), radii


# ---- conditions on the data -------------------------------------------------------------------------------------------------------------
def _trips(block, q, radii):
    """the geometric part of the guard, with the crop's faces counted only where they are the volume's"""
    trip = np.zeros(len(q), dtype=bool)
    for axis, (c, r) in enumerate(zip("zyx", radii[::-1])):
        pos, n = q[:, P[c]], block.size[axis]
        trip |= (block.lo[axis] & (pos - r < 0)) | (block.hi[axis] & (pos + r > n - 1))
    return trip


@pytest.mark.parametrize("key,block", SOLVED_BLOCKS, ids=SOLVED_IDS)
def test_the_oracle_alone_converges_on_the_blocks(key, block):
    prep = lv.prepared(block)
    ref, tar = lv.crop(block)
    assert ref.min() >= 30.0 and tar.min() >= 30.0
    for radii in lv.RADII[key] + lv.ROWS_RADII.get(key, []):
        for guesses in ("int", "half"):
            q, n = lv.solver_queue(block, guesses, radii)
            assert 9 <= n and 12 <= len(q) <= 40, (key, block.name, len(q))
            assert (q[:, :3] == np.round(q[:, :3])).all() and (2 * q[:, [P["u"], P["v"], P["w"]]] == np.round(2 * q[:, [P["u"], P["v"], P["w"]]])).all()
            frac = q[:, P["u"]] != np.round(q[:, P["u"]])
            assert frac.all() if guesses == "half" else not frac.any()
            trip = _trips(block, q, radii)
            assert not trip[:n].any() and trip[n:].any() == (any(block.lo) or any(block.hi)) and (len(q) > n) == (any(block.lo) or any(block.hi))
            for contract in CPU_CONTRACTS + ("rows",):
                want = lv.solve(contract, prep, q, radii)
                good = (want[:, P["zncc"]] > 0.9) & (want[:, P["iteration"]] == 1)
                assert good[:n].all() and good.sum() >= 10, (key, block.name, radii, guesses, contract, want[:, P["zncc"]])
                # nothing comes back -4, and -3 only where the guard trips or a sample leaves the interpolatable range at a true face
                assert not (want[:, P["zncc"]] == -4.0).any() and not (want[:n, P["zncc"]] < 0).any()
                assert (want[trip, P["zncc"]] == -3.0).all() and np.array_equal(lv.bits(want[trip][:, :18]), lv.bits(q[trip][:, :18]))
                hard = ~trip
                hard[:n] = False
                if hard.any():       # hard against a true face: solved where the guess keeps the samples in range -- the far z face always
                    far_z = hard & block.hi[0] & (q[:, P["z"]] == block.size[0] - 1 - radii[2]) & ~(
                        (block.hi[2] & (q[:, P["x"]] == block.size[2] - 1 - radii[0])) | (block.lo[1] & (q[:, P["y"]] == radii[1])))
                    assert good[far_z].all() and (not block.hi[0] or far_z.any()), (key, block.name, radii, guesses, contract)


def test_the_padded_queue_reaches_the_schedule():
    block = lv.BLOCKS["SLAB"][1]
    q, n = lv.solver_queue(block, "half", lv.R_SLAB)
    big = lv.padded(q)
    assert len(big) == 2048 > len(q) and np.array_equal(lv.bits(big[:len(q)]), lv.bits(q)) and np.array_equal(lv.bits(big[len(q):2 * len(q)]), lv.bits(q))

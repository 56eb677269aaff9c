"""The range rule on the GPU: every restatement of `x < 1 || x >= size - 2` in the kernels against the oracle, on queues whose
samples sit ON the limits (tests/border_cases.py).

The library decides "is this warped sample interpolatable" in at least eight places, each written differently: the unsigned compare
on floor(x) of lut_fetch / lut_locate (dic2d_device.h), the four-corner test hoisted out of the ICGN2D1 sweep (icgn2d.hip,
icgn2d_onepass.hip), the `inside` test of the integer-translation sweep, the global- and LDS-tap rules of icgn3d_device.h, the
clipping of the staged coefficient box at the volume faces (icgn3d.hip, icgn3d_onepass.hip), the per-sample tests of ICGN2D2, IC-LM
(which keeps the -1 sentinel as a VALUE and never abandons) and NR2D1.  An off-by-one in any of them solves a POI from zero table
entries or throws a solvable one away; on these queues it changes a record (tests/test_oracle_border.py plants four such slips in a
NumPy restatement and counts), and the bar is the usual one: every float of every record identical to the oracle's, NaN == NaN.
The A/B partners run the same queues in tests/ab/test_ab_border.py.
"""
import functools

import numpy as np
import pytest

import border_cases as bc
from test_gpu_fuzz import _same

pytestmark = pytest.mark.gpu

VARIANTS = (-1, 1, 2, 3, 4, 5, 7)
# per-POI radii: the library replaces the table variants 4 and 5 -- and the automatic choice -- by variant 2 / 3 (capi.hip, "per-POI
# radii: no shared coordinate table"), so naming them would run the same kernel again
VARIANTS_SELF_ADAPTIVE = (-1, 1, 2, 3, 7)
TILE_QUEUE = 2048     # ICGN3D1 visits a queue in cubic blocks ("icgn3d_tile_vox") from this many records on


def _p2(name):
    import oracle
    return oracle.P2[name]


def _p3(name):
    import oracle
    return oracle.P3[name]


def _check(got, want, at, what):
    same = _same(got, want).all(axis=1)
    if not same.all():
        bad = np.flatnonzero(~same)
        where = [(l.name, int(i - s.start)) for i in bad[:8] for l, s in at if s.start <= i < s.stop]
        raise AssertionError((what, "%d records differ" % len(bad), "(ladder, rung): %s" % where, got[bad[0]].tolist(), want[bad[0]].tolist()))


@functools.lru_cache(maxsize=None)
def _groups2d():
    return bc.group(bc.ladders2d())


@functools.lru_cache(maxsize=None)
def _want2d(solver, order, key):
    """The oracle's records of a group: computed once, shared, read-only."""
    pair, mode = key
    q, off, _ = _groups2d()[key]
    out = bc.oracle2d(solver, pair, q, order, offsets=off, adaptive=mode in ("adaptive", "both"))
    out.setflags(write=False)
    return out


def _engine2d(cls, pair):
    e = cls(bc.R2D[0], bc.R2D[1], bc.CONV, bc.STOP2D)
    e.set_images(*bc.pair2d(*pair))
    e.prepare()
    return e


def _compute2d(e, key):
    pair, mode = key
    q, off, _ = _groups2d()[key]
    e.set_self_adaptive(mode in ("adaptive", "both"))
    return e.compute_with_offsets(q.copy(), off.copy()) if off is not None else e.compute(q.copy())


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_every_variant_plain_offsets_self_adaptive(dof, fma):
    """ICGN2D1 / ICGN2D2, default and fused arithmetic: every product variant, the integer-translation sweep on and off, the plain
    call, centre offsets, per-POI radii and both together.  Under per-POI radii five launch choices are distinct, not seven
    (VARIANTS_SELF_ADAPTIVE)."""
    import opencorr_amd
    import oracle
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    order = oracle.ORDER_LANES_FMA if fma else oracle.ORDER_LANES
    engines = {}
    for key in sorted(_groups2d(), key=str):
        pair, mode = key
        if pair not in engines:
            engines[pair] = _engine2d(opencorr_amd.ICGN2D1 if dof == 6 else opencorr_amd.ICGN2D2, pair)
            engines[pair].set_tuning("arith_fma", fma)
        e = engines[pair]
        want = _want2d(solver, order, key)
        for variant in (VARIANTS_SELF_ADAPTIVE if mode in ("adaptive", "both") else VARIANTS):
            e.set_tuning("icgn2d_variant", variant)
            for int_first in (1, 0):
                e.set_tuning("icgn2d_int_first", int_first)
                _check(_compute2d(e, key), want, _groups2d()[key][2], (solver, fma, key, variant, int_first))
    for e in engines.values():
        e.close()


def _swapped(key):
    """The group's queue with the guesses of every ladder in reverse rung order -- the coordinates stay, abandoned and solved rungs
    change places (the whole-pixel ladder, whose records lie at different positions, stays as it is)."""
    q, _, at = _groups2d()[key]
    out = q.copy()
    for l, s in at:
        if l.kind != "integer":
            out[s, _p2("u"):_p2("vyy") + 1] = q[s, _p2("u"):_p2("vyy") + 1][::-1]
    return out


@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_set_up_cache_fill_and_use(dof):
    """The big-queue variant named (5 / 4), so that the ladder queues run through the set-up cache: the fill call, the use call, and a
    use call whose abandoned and solved rungs have changed places."""
    import torch
    import opencorr_amd
    import oracle
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    dev = torch.device("cuda", 0)
    for key in sorted(k for k in _groups2d() if k[1] == "plain"):
        pair, _ = key
        q, _, at = _groups2d()[key]
        e = _engine2d(opencorr_amd.ICGN2D1 if dof == 6 else opencorr_amd.ICGN2D2, pair)
        e.set_tuning("icgn2d_variant", 5 if dof == 6 else 4)
        want = _want2d(solver, oracle.ORDER_LANES, key)
        swapped = _swapped(key)
        want_swapped = bc.oracle2d(solver, pair, swapped, oracle.ORDER_LANES)
        if len(at) > 1 or at[0][0].kind != "integer":
            assert not np.array_equal(want_swapped[:, _p2("zncc")], want[:, _p2("zncc")])
        for queue, expect, state in ((q, want, "fill"), (q, want, "use"), (swapped, want_swapped, "use"), (q, want, "use")):
            t = torch.from_numpy(queue.copy()).to(dev)
            e.compute(t)
            assert e.setup_cache_last() == state, (key, state)
            torch.cuda.synchronize()
            _check(t.cpu().numpy(), expect, at, (solver, key, state))
        e.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_one_pass_contract(dof):
    """`arith_onepass` (icgn2d_onepass.hip holds the corner test again) against its CPU twin."""
    import opencorr_amd
    import onepass_twin as twin
    for key in sorted(k for k in _groups2d() if k[1] == "plain"):
        pair, _ = key
        q, _, at = _groups2d()[key]
        e = _engine2d(opencorr_amd.ICGN2D1 if dof == 6 else opencorr_amd.ICGN2D2, pair)
        e.set_tuning("arith_onepass", 1)
        want = twin.icgn2d(dof, bc.prepared2d(*pair), bc.R2D[0], bc.R2D[1], bc.CONV, bc.STOP2D, q.copy())
        assert (want[:, _p2("zncc")] == -3).sum() >= 2 * len(at) and (want[:, _p2("zncc")] > 0.9).sum() >= 2
        for int_first in (1, 0):
            e.set_tuning("icgn2d_int_first", int_first)
            _check(e.compute(q.copy()), want, at, ("onepass", dof, key, int_first))
        e.close()


@pytest.mark.parametrize("solver", ["iclm2d1", "iclm2d2", "nr2d1"])
def test_iclm_and_nr2d1(solver):
    """IC-LM never abandons: its out-of-range rungs are solved with the -1 sentinel as data, as the reference does; NR2D1 tests per
    sample."""
    import opencorr_amd
    import oracle
    cls = {"iclm2d1": opencorr_amd.ICLM2D1, "iclm2d2": opencorr_amd.ICLM2D2, "nr2d1": opencorr_amd.NR2D1}[solver]
    for key in sorted(k for k in _groups2d() if k[1] == "plain"):
        pair, _ = key
        q, _, at = _groups2d()[key]
        e = _engine2d(cls, pair)
        _check(e.compute(q.copy()), _want2d(solver, oracle.ORDER_LANES, key), at, (solver, key))
        if solver != "nr2d1":
            assert not (_want2d(solver, oracle.ORDER_LANES, key)[:, _p2("zncc")] == -3).any()
            e.set_tuning("arith_fma", 1)
            _check(e.compute(q.copy()), _want2d(solver, oracle.ORDER_LANES_FMA, key), at, (solver, key, "fma"))
        e.close()


# ---- 3D --------------------------------------------------------------------------------------------------------------------------
def _run3d(ladders, tiles):
    """ICGN3D1 on the ladders that share a pair, one queue: default, fused and one-pass arithmetic, in queue order.  `tiles`: also the
    block schedule ("icgn3d_tile_vox" = 8).  The library builds that visiting order only for queues of TILE_QUEUE records or more, so
    the ladder queue is repeated up to that length for it -- the one exception to the size limit of the 3D queues, and only at
    r = (5, 6, 4), where 2 048 subvolumes of 11 x 13 x 9 cost milliseconds; every repetition must give the records of the first."""
    import opencorr_amd
    import onepass3d_twin as twin
    import oracle
    l0 = ladders[0]
    assert all((l.pair, l.shape, l.r, l.stop) == (l0.pair, l0.shape, l0.r, l0.stop) for l in ladders)
    q = np.concatenate([l.queue for l in ladders])
    at, n = [], 0
    for l in ladders:
        at.append((l, slice(n, n + len(l.queue))))
        n += len(l.queue)
    reps = -(-TILE_QUEUE // len(q))
    at_big = [(l, slice(s.start + k * len(q), s.stop + k * len(q))) for k in range(reps) for l, s in at]
    e = opencorr_amd.ICGN3D1(l0.r[0], l0.r[1], l0.r[2], bc.CONV, l0.stop)
    e.set_images(*bc.pair3d(*l0.pair, l0.shape))
    e.prepare()
    prep = bc.prepared3d(*l0.pair, l0.shape)
    wants = {(0, 0): bc.oracle3d(l0, q, oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D),
             (1, 0): bc.oracle3d(l0, q, oracle.ORDER_LANES_FMA, oracle.GPU_LANES_3D),
             (0, 1): twin.icgn3d1(prep, l0.r[0], l0.r[1], l0.r[2], bc.CONV, l0.stop, q.copy())}
    for (fma, onepass), want in wants.items():
        z = want[:, _p3("zncc")]
        assert (z == -3).sum() >= 2 * len(at) and (z > 0.9).sum() >= 2 * len(at)
        e.set_tuning("arith_fma", fma)
        e.set_tuning("arith_onepass3d", onepass)
        e.set_tuning("icgn3d_tile_vox", 0)
        _check(e.compute(q.copy()), want, at, (l0.pair, l0.r, fma, onepass, "queue order"))
        if tiles:
            big = np.tile(q, (reps, 1))
            assert len(big) >= TILE_QUEUE
            e.set_tuning("icgn3d_tile_vox", 8)
            _check(e.compute(big.copy()), np.tile(want, (reps, 1)), at_big, (l0.pair, l0.r, fma, onepass, "8-voxel blocks"))
            e.set_tuning("icgn3d_tile_vox", 0)       # the same long queue in queue order: the persistent-workgroup launch alone
            _check(e.compute(big.copy()), np.tile(want, (reps, 1)), at_big, (l0.pair, l0.r, fma, onepass, "long queue"))
    e.close()


PAIRS3D = sorted({l.pair for l in bc.ladders3d()})


@pytest.mark.parametrize("pair", PAIRS3D, ids=["%+d%+d%+d" % p for p in PAIRS3D])
def test_icgn3d1_faces_and_corners(pair):
    """Low faces read coefficient index 0, high faces index D - 1: the faces at which the staged box is clipped."""
    ladders = [l for l in bc.ladders3d() if l.pair == pair]
    assert sum(len(l.queue) for l in ladders) <= 117
    _run3d(ladders, tiles=True)


@pytest.mark.parametrize("r", bc.LARGE_R)
def test_icgn3d1_large_radii(r):
    """r = 16 (six staging passes), 21, 25, 30 (icgn3d1_kernel<48>, <64>, <0>): a low-face and a high-face ladder each, in queue
    order only: 26 records never reach the block schedule, and 2 048 subvolumes of 33^3 ... 61^3 are no quick test."""
    _run3d(list(bc.ladders3d_large(r)), tiles=False)

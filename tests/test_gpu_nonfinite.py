"""Non-finite POI records on the GPU: every engine on the queues of tests/nonfinite_cases.py, bit for bit.

A record whose own coordinate is NaN passes the entry guard as the reference writes it (every comparison with a NaN is false), and
the kernels then formed the subset origin from (int)NaN -- 0 on this hardware -- minus the radius: a negative offset, passed as an
unsigned scalar offset to an unbounded buffer descriptor in 2D, a pointer in front of the gradient volumes in 3D.  The guards are
written negated now, and a NaN coordinate is rejected like a subset that leaves the image (nonfinite_cases.py holds the contract
table, tests/test_oracle_nonfinite.py holds the oracle to it).  Here: COORD and CONTROL records exactly as the table says, every
other record exactly the oracle's, and the clean records exactly as from a queue without planted ones -- in every kernel that
restates the guard.  The A/B partners run the same queues in tests/ab/test_ab_nonfinite.py.  At the end of the file, the
best-candidate selection (poi_order.hip) on hand-written ZNCC lists.
"""
import functools

import numpy as np
import pytest

import border_cases as bc
import nonfinite_cases as nf
from test_gpu_border import VARIANTS, VARIANTS_SELF_ADAPTIVE

pytestmark = pytest.mark.gpu

MODES = ("plain", "offsets", "adaptive", "both")


def _check(got, want, case, what):
    ok = nf.same(got, want).all(axis=1)
    if not ok.all():
        bad = np.flatnonzero(~ok)
        i = int(bad[0])
        raise AssertionError((what, "%d records differ" % len(bad), [case.names[int(k) % len(case.names)] for k in bad[:6]], got[i].tolist(),
                              want[i].tolist()))


def _case2d(mode):
    return nf.queue2d(offsets=mode in ("offsets", "both"))


@functools.lru_cache(maxsize=None)
def _want2d(solver, order_name, mode):
    """The expected records of a queue: computed once, shared, read-only."""
    import oracle
    out = nf.expected2d(solver, _case2d(mode), getattr(oracle, order_name), adaptive=mode in ("adaptive", "both"))
    out.setflags(write=False)
    return out


def _engine2d(cls):
    e = cls(bc.R2D[0], bc.R2D[1], bc.CONV, nf.STOP2D)
    e.set_images(*bc.pair2d(*nf.PAIR2D))
    e.prepare()
    return e


def _compute2d(e, case, mode):
    import opencorr_amd
    if not isinstance(e, opencorr_amd.NR2D1):       # (NR2D1 has no per-POI radii, in the reference or here)
        e.set_self_adaptive(mode in ("adaptive", "both"))
    if case.offsets is not None:
        return e.compute_with_offsets(case.queue.copy(), case.offsets.copy())
    return e.compute(case.queue.copy())


def _cls(solver):
    import opencorr_amd
    return {"icgn2d1": opencorr_amd.ICGN2D1, "icgn2d2": opencorr_amd.ICGN2D2, "iclm2d1": opencorr_amd.ICLM2D1, "iclm2d2": opencorr_amd.ICLM2D2,
            "nr2d1": opencorr_amd.NR2D1}[solver]


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_every_variant_and_call_mode(dof, fma):
    """ICGN2D1 / ICGN2D2, default and fused arithmetic: every product variant, the integer-translation sweep on and off, the plain
    call, centre offsets, per-POI radii and both together; and the clean records alone."""
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    order = "ORDER_LANES_FMA" if fma else "ORDER_LANES"
    e = _engine2d(_cls(solver))
    e.set_tuning("arith_fma", fma)
    for mode in MODES:
        case, want = _case2d(mode), _want2d(solver, order, mode)
        for variant in (VARIANTS_SELF_ADAPTIVE if mode in ("adaptive", "both") else VARIANTS):
            e.set_tuning("icgn2d_variant", variant)
            for int_first in (1, 0):
                e.set_tuning("icgn2d_int_first", int_first)
                _check(_compute2d(e, case, mode), want, case, (solver, fma, mode, variant, int_first))
        e.set_tuning("icgn2d_variant", -1)
        alone = case.without_planted()
        _check(_compute2d(e, alone, mode), want[case.clean], alone, (solver, fma, mode, "clean records alone"))
    e.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_one_pass_contract(dof):
    """`arith_onepass` = 1 (icgn2d_onepass.hip restates the guard) against its CPU twin and the table."""
    import onepass_twin as twin
    case = nf.queue2d()
    want = twin.icgn2d(dof, bc.prepared2d(*nf.PAIR2D), bc.R2D[0], bc.R2D[1], bc.CONV, nf.STOP2D, case.queue.copy())
    want = nf.expected2d("icgn2d1", case, None, solved=want)
    e = _engine2d(_cls("icgn2d1" if dof == 6 else "icgn2d2"))
    e.set_tuning("arith_onepass", 1)
    for int_first in (1, 0):
        e.set_tuning("icgn2d_int_first", int_first)
        _check(e.compute(case.queue.copy()), want, case, ("onepass", dof, int_first))
    alone = case.without_planted()
    _check(e.compute(alone.queue.copy()), want[case.clean], alone, ("onepass", dof, "clean records alone"))
    e.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_set_up_cache_when_coordinates_turn_nan_and_back(dof):
    """The big-queue variant named (5 / 4), so that the queue runs through the set-up cache (the geometric part of the guard decides
    whether a POI has a set-up record at all): a fill call, a use call, a call in which clean records' coordinates have turned NaN --
    a coordinate that differs makes it a fill, as for a moved POI --, the same once more (use), and the finite queue again."""
    import torch
    import oracle
    P = oracle.P2
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    case = nf.queue2d()
    want = _want2d(solver, "ORDER_LANES", "plain")
    turned = case.queue.copy()
    rows = np.flatnonzero(case.clean)[::3]
    for k, i in enumerate(rows):
        for col in ((P["x"],), (P["y"],), (P["x"], P["y"]))[k % 3]:
            turned.view(np.uint32)[i, col] = nf.NAN_BITS[k % 4]
    want_turned = want.copy()
    want_turned.view(np.uint32)[rows] = nf.bits(nf.contract2d(turned, solver))[rows]
    assert len(rows) >= 12 and (want[rows, P["zncc"]] > 0.9).all() and (want_turned[rows, P["zncc"]] == -3).all()
    e = _engine2d(_cls(solver))
    e.set_tuning("icgn2d_variant", 5 if dof == 6 else 4)
    dev = torch.device("cuda", 0)
    for queue, expect, state in ((case.queue, want, "fill"), (case.queue, want, "use"), (turned, want_turned, "fill"),
                                 (turned, want_turned, "use"), (case.queue, want, "fill"), (case.queue, want, "use")):
        t = torch.from_numpy(queue.copy()).to(dev)
        e.compute(t)
        assert e.setup_cache_last() == state, (dof, state)
        torch.cuda.synchronize()
        _check(t.cpu().numpy(), expect, case, (solver, "set-up cache", state))
    e.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_icgn2d_locality_schedule(dof):
    """16 384 records and more -- the length from which the library visits a queue tile by tile (poi_order.hip: tile_of only compares
    and clamps a coordinate, a NaN lands in row / column 0) -- with planted records scattered and in a run of 64: tiles of 64 px
    and queue order give the same bits."""
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    case = nf.queue2d()
    big, want = nf.long_queue(case, _want2d(solver, "ORDER_LANES", "plain"), 16384)
    assert len(big) >= 16384
    e = _engine2d(_cls(solver))
    for tile in (64, 0):
        e.set_tuning("icgn2d_tile_px", tile)
        _check(e.compute(big.copy()), want, case, (solver, "tile_px", tile))
    e.close()


@pytest.mark.parametrize("solver", ["iclm2d1", "iclm2d2", "nr2d1"])
def test_iclm_and_nr2d1(solver):
    """IC-LM with its default damping (plain and per-POI radii, default and fused arithmetic), and NR2D1, whose rejected records take
    its own branch: -1, then the -4 and the -5 rule."""
    e = _engine2d(_cls(solver))
    for mode in (("plain",) if solver == "nr2d1" else ("plain", "adaptive")):
        case = _case2d(mode)
        for fma in ((0,) if solver == "nr2d1" else (0, 1)):
            if solver != "nr2d1":
                e.set_tuning("arith_fma", fma)
            want = _want2d(solver, "ORDER_LANES_FMA" if fma else "ORDER_LANES", mode)
            _check(_compute2d(e, case, mode), want, case, (solver, mode, fma))
            alone = case.without_planted()
            _check(_compute2d(e, alone, mode), want[case.clean], alone, (solver, mode, fma, "clean records alone"))
    e.close()


# ---- ICGN3D1 ---------------------------------------------------------------------------------------------------------------------
def _engine3d():
    import opencorr_amd
    e = opencorr_amd.ICGN3D1(bc.R3D[0], bc.R3D[1], bc.R3D[2], bc.CONV, bc.STOP3D)
    e.set_images(*bc.pair3d(*nf.PAIR3D))
    e.prepare()
    return e


@functools.lru_cache(maxsize=None)
def _want3d(which):
    import onepass3d_twin as twin
    import oracle
    case = nf.queue3d()
    if which == "onepass":
        solved = twin.icgn3d1(bc.prepared3d(*nf.PAIR3D), *bc.R3D, bc.CONV, bc.STOP3D, case.queue.copy())
        out = nf.expected3d(case, None, None, solved=solved)
    else:
        out = nf.expected3d(case, oracle.ORDER_LANES_FMA if which == "fma" else oracle.GPU_ORDER_3D, oracle.GPU_LANES_3D)
    out.setflags(write=False)
    return out


def test_icgn3d1_contracts_and_resident_queue():
    """Default, fused and one-pass arithmetic (icgn3d.hip twice, icgn3d_onepass.hip), a device-resident queue, the clean records alone."""
    import torch
    case = nf.queue3d()
    e = _engine3d()
    for which, fma, onepass in (("default", 0, 0), ("fma", 1, 0), ("onepass", 0, 1)):
        e.set_tuning("arith_fma", fma)
        e.set_tuning("arith_onepass3d", onepass)
        want = _want3d(which)
        _check(e.compute(case.queue.copy()), want, case, ("icgn3d1", which))
        alone = case.without_planted()
        _check(e.compute(alone.queue.copy()), want[case.clean], alone, ("icgn3d1", which, "clean records alone"))
    e.set_tuning("arith_fma", 0)
    e.set_tuning("arith_onepass3d", 0)
    t = torch.from_numpy(case.queue.copy()).to(torch.device("cuda", 0))
    e.compute(t)
    torch.cuda.synchronize()
    _check(t.cpu().numpy(), _want3d("default"), case, ("icgn3d1", "device-resident queue"))
    e.close()


def test_icgn3d1_locality_schedule():
    """2 048 records and more, with a run of 64 planted ones: blocks of 8 voxels and queue order give the same bits."""
    case = nf.queue3d()
    big, want = nf.long_queue(case, _want3d("default"), 2048)
    assert len(big) >= 2048
    e = _engine3d()
    for tile in (8, 0):
        e.set_tuning("icgn3d_tile_vox", tile)
        _check(e.compute(big.copy()), want, case, ("icgn3d1", "tile_vox", tile))
    e.close()


# ---- FFTCC -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,fused", [((16, 16), 1), ((12, 12), 1), ((9, 11), 1), ((12, 12), 0)], ids=["r16-registers", "r12-lds", "9x11", "r12-rocfft"])
def test_fftcc2d_leaves_planted_records_untouched(r, fused):
    """The four families: a record with a non-finite coordinate or guess stays untouched bit for bit ((int)NaN is 0 here, below every
    radius); the clean records come out as from a queue without planted ones, with the oracle's integers."""
    import opencorr_amd
    import oracle
    P = oracle.P2
    case = nf.fftcc_queue2d(*r)
    f = opencorr_amd.FFTCC2D(*r)
    f.set_images(*bc.pair2d(*nf.PAIR2D))
    if not fused:
        f.set_tuning("fftcc2d_fused", 0)
    got = f.compute(case.queue.copy())
    planted = ~case.clean
    assert np.array_equal(nf.bits(got)[planted], nf.bits(case.queue)[planted]), [n for n, a, b in zip(case.names, nf.bits(got), nf.bits(case.queue))
                                                                                 if not np.array_equal(a, b)][:6]
    alone = case.without_planted()
    _check(got[case.clean], f.compute(alone.queue.copy()), alone, ("fftcc2d", r, fused, "clean records alone"))
    want = case.queue.copy()
    oracle.fftcc2d(*bc.pair2d(*nf.PAIR2D), r[0], r[1], want)
    for k in ("u", "v", "u0", "v0"):
        assert np.array_equal(got[:, P[k]][case.clean], want[:, P[k]][case.clean]), (r, fused, k)
    assert (got[case.clean, P["zncc"]] > 0.5).all()
    f.close()


@pytest.mark.parametrize("r,fused", [((6, 6, 6), 1), ((14, 14, 14), 1), ((16, 16, 16), 1), ((5, 6, 4), 1), ((6, 6, 6), 0)],
                         ids=["r6-lds", "r14-planes", "r16-registers", "5x6x4-box", "r6-rocfft"])
def test_fftcc3d_agrees_with_the_pipeline_on_nan_coordinates(r, fused):
    """FFTCC3D has no guard (the reference has none) and clamps every index: on a record with NaN coordinates every kernel computes
    what the rocFFT pipeline computes -- the same integers, the same NaN-ness of the ZNCC -- and no other record changes."""
    import opencorr_amd
    import oracle
    P = oracle.P3
    case = nf.fftcc_queue3d()
    f = opencorr_amd.FFTCC3D(*r)
    f.set_images(*bc.pair3d(*nf.PAIR3D))
    f.set_tuning("fftcc3d_fused", fused)
    got = f.compute(case.queue.copy())
    alone = case.without_planted()
    _check(got[case.clean], f.compute(alone.queue.copy()), alone, ("fftcc3d", r, fused, "clean records alone"))
    f.set_tuning("fftcc3d_fused", 0)
    base = f.compute(case.queue.copy())
    planted = ~case.clean
    for k in ("u", "v", "w", "u0", "v0", "w0"):
        assert np.array_equal(nf.bits(got[:, P[k]])[planted], nf.bits(base[:, P[k]])[planted]), (r, fused, k)
        assert np.array_equal(got[:, P[k]][case.clean], base[:, P[k]][case.clean]), (r, fused, k, "clean")
    assert np.array_equal(np.isnan(got[:, P["zncc"]]), np.isnan(base[:, P["zncc"]])), (r, fused)
    untouched = [c for c in range(case.queue.shape[1]) if c not in [P[k] for k in ("u", "v", "w", "u0", "v0", "w0", "zncc")]]
    assert np.array_equal(nf.bits(got)[:, untouched], nf.bits(case.queue)[:, untouched])
    f.close()


# ---- select_best on planted ZNCC lists ---------------------------------------------------------------------------------------------
SEGMENT_LENGTHS = (0, 1, 63, 64, 65, 130, 1000)
PATTERNS = ("random", "tie in one lane", "tie across lanes", "all NaN", "NaN first", "only -inf", "+inf ties", "codes")


def _zncc_list(length, pattern, rng):
    """One segment's ZNCCs.  A wave reads candidate c in lane c % 64: `c` and `c + 64` meet in one lane's loop, the others in the
    cross-lane reduction."""
    z = rng.uniform(0.1, 0.9, length).astype(np.float32)
    if length == 0:
        return z
    if pattern == "tie in one lane":
        z[[k for k in (length - 1 - 64, length - 1) if k >= 0]] = 0.95          # the later one is met second by the same lane
        if length > 133:
            z[[5, 69, 133]] = 0.97
    elif pattern == "tie across lanes":
        z[[k for k in (length // 2, length // 3, length - 1) if k >= 0]] = 0.95
    elif pattern == "all NaN":
        z[:] = np.nan
    elif pattern == "NaN first":
        z[:min(length, 70)] = np.nan
        z[-1] = 0.5
        if length > 2:
            z[-2] = 0.5
    elif pattern == "only -inf":
        z[:] = -np.inf
    elif pattern == "+inf ties":
        z[[k for k in (length - 1, length // 2, min(length - 1, 64))]] = np.inf
    elif pattern == "codes":
        z[:] = rng.choice(np.float32([-3, -4, -5, -1]), length)
        if length > 2:
            z[[length // 2, length - 1]] = np.float32([0.25, 0.25])
    return z


def _select_best_want(cand, starts, pois):
    want = pois.copy()
    for s in range(len(pois)):
        seg = cand[starts[s]:starts[s + 1]]
        z = seg[:, 16]
        if len(seg) == 0 or np.all(np.isnan(z)):
            continue
        k = int(np.nanargmax(z))                  # first maximum
        want[s, 2:20] = seg[k, 2:20]
    return want


@pytest.mark.parametrize("nseg", [1, 4, 5])
def test_select_best_on_planted_zncc_lists(nseg):
    """poi2d_best_of_segments_kernel without a solver: every segment length around the wave size with every planted list, in queues
    of 1, 4 and 5 segments (four waves per workgroup): the highest ZNCC wins, the earliest candidate among equals, NaN never, an
    empty or all-NaN segment leaves its POI untouched.  Host queues, device-resident queues, and a candidate stride of 32 floats."""
    import torch
    import opencorr_amd
    rng = np.random.default_rng(20261019 + nseg)
    specs = [(length, p) for p in PATTERNS for length in SEGMENT_LENGTHS]
    specs = [specs[i] for i in rng.permutation(len(specs))]
    e = opencorr_amd.ICGN2D1(bc.R2D[0], bc.R2D[1], bc.CONV, bc.STOP2D)
    e.set_images(*bc.pair2d(*nf.PAIR2D))
    e.prepare()
    dev = torch.device("cuda", 0)
    for g, first in enumerate(range(0, len(specs), nseg)):
        group = specs[first:first + nseg]
        while len(group) < nseg:
            group.append(specs[len(group)])
        lists = [_zncc_list(length, p, rng) for length, p in group]
        starts = np.concatenate([[0], np.cumsum([len(z) for z in lists])]).astype(np.uint32)
        n = int(starts[-1])
        stride = 32 if g % 2 else 25
        cand = rng.uniform(-1, 1, (n + 1, stride)).astype(np.float32)
        cand[:, 2] = np.arange(n + 1)               # names the winner
        cand[:, 16] = np.concatenate(lists + [np.float32([np.inf])])     # (the last row belongs to no segment: never the winner)
        pois = rng.uniform(-1, 1, (nseg, 25)).astype(np.float32)
        want = _select_best_want(cand, starts, pois)
        got = e.select_best(cand, starts, pois.copy())
        assert np.array_equal(nf.bits(got), nf.bits(want)), (group, "host")
        d = e.select_best(torch.from_numpy(cand).to(dev), torch.from_numpy(starts.astype(np.int32)).to(dev), torch.from_numpy(pois.copy()).to(dev))
        assert np.array_equal(nf.bits(d.cpu().numpy()), nf.bits(want)), (group, "device")
    e.close()

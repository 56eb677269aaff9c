"""The CPU oracle and the two one-pass twins on the queues of tests/nonfinite_cases.py (no GPU).

A record with a NaN coordinate is rejected at the guard like a subset that leaves the image (nonfinite_cases.py holds the contract
table); here the oracle is held to that table, in every order and call mode, so that tests/test_gpu_nonfinite.py may take the other
records from it.  The same queues then go through tests/cpp/oracle_nonfinite_check.cpp, a stand-alone program around the oracle's
and the twins' sources, built once plain and once with -fsanitize=undefined,address,float-cast-overflow: the two builds print the
same records as the in-process runs, and the sanitized one is silent -- float-cast-overflow reports any (int)NaN still reachable.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import border_cases as bc
import nonfinite_cases as nf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ("-O1", "-g", "-fsanitize=undefined,address,float-cast-overflow", "-fno-sanitize-recover=all")
ORDERS = ("SEQ", "LANES", "LANES_FMA")
MODES_BY_SOLVER = {"icgn2d1": ("plain", "offsets", "adaptive", "both"), "icgn2d2": ("plain", "offsets", "adaptive", "both"),
                   "iclm2d1": ("plain", "adaptive"), "iclm2d2": ("plain", "adaptive"), "nr2d1": ("plain",)}
FFTCC_RADII = ((16, 16), (12, 12), (9, 11))
ENGINE_ID = {"icgn2d1": 0, "icgn2d2": 1, "iclm2d1": 2, "iclm2d2": 3, "nr2d1": 4, "icgn3d1": 5, "fftcc2d": 6, "twin2d1": 7, "twin2d2": 8,
             "twin3d": 9}


def _order(name):
    import oracle
    return getattr(oracle, "ORDER_" + name)


def _case2d(mode):
    return nf.queue2d(offsets=mode in ("offsets", "both"))


def _assert_same(got, want, case, what):
    ok = nf.same(got, want).all(axis=1)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError((what, "%d records differ" % int((~ok).sum()), i, case.names[i], got[i].tolist(), want[i].tolist()))


def _converged(rec, P):
    return (rec[:, P["zncc"]] > 0.9) & (rec[:, P["iteration"]] < (nf.STOP2D if rec.shape[1] == 25 else bc.STOP3D))


def _hold_to_the_table(case, solve, contract, P, what):
    """The three assertions every engine gets: the clean records converge, the guarded ones obey the table, and the clean ones come
    out as they do from a queue without any planted record."""
    got = solve(case)
    assert _converged(got[case.clean], P).all(), (what, [n for n, c, k in zip(case.names, _converged(got, P), case.clean) if k and not c])
    m = case.by_contract
    assert m.sum() >= 100 if case.dim == 2 else m.sum() >= 90
    sub = nf.Planted(case.queue[m].copy(), case.kind[m].copy(), [n for n, k in zip(case.names, m) if k], case.dim, case.r)
    _assert_same(got[m], contract(case.queue)[m], sub, what + ("table",))
    alone = case.without_planted()
    _assert_same(got[case.clean], solve(alone), alone, what + ("neighbours",))
    return got


def test_the_queues_put_planted_records_where_the_kernels_differ():
    for case in (nf.queue2d(), nf.queue2d(offsets=True), nf.queue3d(), nf.fftcc_queue3d()) + tuple(nf.fftcc_queue2d(*r) for r in FFTCC_RADII):
        p = ~case.clean
        n = len(p)
        assert p[0] and p[-1] and p[63] and p[64] and n >= 66
        idx = np.flatnonzero(p)
        assert (idx % 2 == 0).any() and (idx % 2 == 1).any()
        assert (p[1:] & p[:-1]).any() and (p[1:-1] & ~p[:-2] & ~p[2:]).any()       # neighbours of each other, and alone between clean ones
        assert case.clean.sum() >= 36
    P = nf._P(2)
    q = nf.queue2d().queue
    x, y = q[:, P["x"]], q[:, P["y"]]
    rx, ry = bc.R2D
    h, w = bc.SHAPE2D
    # one coordinate NaN and the other one exactly on a guard edge, low and high: where the unguarded offset goes negative
    assert (np.isnan(x) & (y == ry)).any() and (np.isnan(y) & (x == rx)).any()
    assert (np.isnan(x) & (y == h - 1 - ry)).any() and (np.isnan(y) & (x == w - 1 - rx)).any() and (np.isnan(x) & np.isnan(y)).any()
    for word in nf.NAN_BITS:
        assert (nf.bits(q)[:, :2] == word).any()
    P3 = nf._P(3)
    q3 = nf.queue3d().queue
    nan3 = np.isnan(q3[:, [P3["x"], P3["y"], P3["z"]]])
    assert {tuple(r) for r in nan3.tolist()} == {tuple(bool(s >> a & 1) for a in range(3)) for s in range(8)}
    low = (q3[:, P3["y"]] == bc.R3D[1]) & (q3[:, P3["z"]] == bc.R3D[2]) & nan3[:, 0]
    assert low.any()        # NaN in x, the two finite axes on the low edges


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("solver", sorted(MODES_BY_SOLVER))
def test_oracle_2d_solvers(solver, order):
    import oracle
    for mode in MODES_BY_SOLVER[solver]:
        case = _case2d(mode)
        adaptive = mode in ("adaptive", "both")
        _hold_to_the_table(case, lambda c: nf.oracle2d(solver, c, _order(order), adaptive), lambda q: nf.contract2d(q, solver), oracle.P2,
                           (solver, order, mode))


def test_nr2d1_branch_is_exercised():
    """The -4 and the -5 rule both fire on planted records, and the -5 rule copies u0, v0 back."""
    import oracle
    P = oracle.P2
    case = nf.queue2d()
    want = nf.contract2d(case.queue, "nr2d1")[case.by_contract]
    z = want[:, P["zncc"]]
    assert (z == -1).any() and (z == -2.5).any() and (z == -4).any() and (z == -5).any()
    assert ((z == -5) & (want[:, P["u"]] == 3) & (want[:, P["v"]] == 4)).sum() == 3


@pytest.mark.parametrize("dof", [6, 12])
def test_one_pass_twin_2d(dof):
    import onepass_twin as twin
    import oracle
    case = nf.queue2d()
    _hold_to_the_table(case, lambda c: twin.icgn2d(dof, bc.prepared2d(*nf.PAIR2D), bc.R2D[0], bc.R2D[1], bc.CONV, nf.STOP2D, c.queue.copy()),
                       lambda q: nf.contract2d(q, "icgn2d1"), oracle.P2, ("one-pass twin", dof))


@pytest.mark.parametrize("order,lanes", [("SEQ", 256), ("LANES", 512), ("LANES_FMA", 512)])
def test_oracle_icgn3d1(order, lanes):
    import oracle
    _hold_to_the_table(nf.queue3d(), lambda c: nf.oracle3d(c, _order(order), lanes), nf.contract3d, oracle.P3, ("icgn3d1", order))


def test_one_pass_twin_3d():
    import onepass3d_twin as twin
    import oracle
    prep = bc.prepared3d(*nf.PAIR3D)
    _hold_to_the_table(nf.queue3d(), lambda c: twin.icgn3d1(prep, *bc.R3D, bc.CONV, bc.STOP3D, c.queue.copy()), nf.contract3d, oracle.P3,
                       ("one-pass twin 3D",))


def _fftcc2d(case):
    import oracle
    out = case.queue.copy()
    oracle.fftcc2d(*bc.pair2d(*nf.PAIR2D), case.r[0], case.r[1], out)
    return out


@pytest.mark.parametrize("r", FFTCC_RADII, ids=["r16", "r12", "9x11"])
def test_oracle_fftcc2d_leaves_planted_records_untouched(r):
    import oracle
    P = oracle.P2
    case = nf.fftcc_queue2d(*r)
    got = _fftcc2d(case)
    assert np.array_equal(nf.bits(got)[~case.clean], nf.bits(case.queue)[~case.clean])
    assert (case.kind == nf.GUESS).sum() == 6 and case.by_contract.sum() >= 100
    clean = got[case.clean]
    assert (clean[:, P["zncc"]] > 0.5).all() and (clean[:, P["u"]] == 1).all() and (clean[:, P["v"]] == 1).all()
    alone = case.without_planted()
    _assert_same(clean, _fftcc2d(alone), alone, ("fftcc2d", r, "neighbours"))


# ---- the stand-alone program --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jobs():
    """(name, engine, order, lanes, adaptive, case, stop): every engine once per order and call mode."""
    import oracle
    jobs = []
    for solver, modes in sorted(MODES_BY_SOLVER.items()):
        for order in ORDERS:
            for mode in modes:
                jobs.append(("%s %s %s" % (solver, order, mode), solver, _order(order), 64, mode in ("adaptive", "both"), _case2d(mode), nf.STOP2D))
    for order, lanes in (("SEQ", 256), ("LANES", 512), ("LANES_FMA", 512)):
        jobs.append(("icgn3d1 %s" % order, "icgn3d1", _order(order), lanes, False, nf.queue3d(), bc.STOP3D))
    for r in FFTCC_RADII:
        jobs.append(("fftcc2d %s" % (r,), "fftcc2d", 0, 64, False, nf.fftcc_queue2d(*r), 0))
    jobs.append(("twin2d1", "twin2d1", 0, 64, False, nf.queue2d(), nf.STOP2D))
    jobs.append(("twin2d2", "twin2d2", 0, 64, False, nf.queue2d(), nf.STOP2D))
    jobs.append(("twin3d", "twin3d", 0, 512, False, nf.queue3d(), bc.STOP3D))
    assert oracle.POI2D_FLOATS == 25
    return tuple(jobs)


def _in_process(job):
    import onepass3d_twin
    import onepass_twin
    name, engine, order, lanes, adaptive, case, stop = job
    if engine == "fftcc2d":
        return _fftcc2d(case)
    if engine == "icgn3d1":
        return nf.oracle3d(case, order, lanes)
    if engine == "twin3d":
        return onepass3d_twin.icgn3d1(bc.prepared3d(*nf.PAIR3D), *bc.R3D, bc.CONV, bc.STOP3D, case.queue.copy())
    if engine.startswith("twin2d"):
        return onepass_twin.icgn2d(6 if engine == "twin2d1" else 12, bc.prepared2d(*nf.PAIR2D), *bc.R2D, bc.CONV, nf.STOP2D, case.queue.copy())
    return nf.oracle2d(engine, case, order, adaptive)


def _write_jobs(path):
    with open(path, "wb") as fh:
        for name, engine, order, lanes, adaptive, case, stop in _jobs():
            ref, tar = bc.pair2d(*nf.PAIR2D) if case.dim == 2 else bc.pair3d(*nf.PAIR3D)
            dims = tuple(ref.shape) + ((0,) if case.dim == 2 else ())
            r = tuple(case.r) + ((0,) if case.dim == 2 else ())
            n, stride = case.queue.shape
            fh.write(struct.pack("=16i", ENGINE_ID[engine], order, lanes, int(adaptive), int(case.offsets is not None), *dims, *r, n, stop,
                                 stride, 0, 0))
            fh.write(struct.pack("=f", bc.CONV))
            for a in (ref, tar, case.queue) + ((case.offsets,) if case.offsets is not None else ()):
                fh.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())


def _build(out_dir, flags, tag):
    exe = str(out_dir / ("oracle_nonfinite_check" + tag))
    src = [os.path.join(ROOT, "tests", "cpp", "oracle_nonfinite_check.cpp"), os.path.join(ROOT, "oracle", "oc_oracle.cpp"),
           os.path.join(ROOT, "tests", "cpp", "icgn2d_onepass_twin.cpp"), os.path.join(ROOT, "tests", "cpp", "icgn3d_onepass_twin.cpp")]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fcx-limited-range", "-fopenmp", "-Wall", *flags, *src, "-o", exe],
                   check=True, timeout=900)
    return exe


def _parse(lines):
    out, cur = [], None
    for line in lines:
        if line.startswith("job "):
            cur = []
            out.append(cur)
        else:
            cur.append([int(w, 16) for w in line.split()])
    return [np.array(j, dtype=np.uint32).view(np.float32) for j in out]


def test_stand_alone_program_plain_and_sanitized(tmp_path):
    path = tmp_path / "jobs.bin"
    _write_jobs(path)
    outs = {}
    for tag, flags in (("plain", ("-O2",)), ("sanitized", SANITIZE)):
        exe = _build(tmp_path, flags, "_" + tag)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and not r.stderr, (tag, r.returncode, r.stderr[-3000:])
        outs[tag] = r.stdout
    # (the same records under the suite's rule, not the same text: the sign of a NaN that the arithmetic produces is the compiler's
    # choice of operand order, and differs between -O1 and -O2)
    plain, sanitized = _parse(outs["plain"].splitlines()), _parse(outs["sanitized"].splitlines())
    assert len(plain) == len(sanitized) == len(_jobs())
    for job, a, b in zip(_jobs(), plain, sanitized):
        _assert_same(a, b, job[5], (job[0], "plain against sanitized"))
        _assert_same(a, _in_process(job), job[5], (job[0], "stand-alone against in-process"))

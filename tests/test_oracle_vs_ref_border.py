"""The oracle against the compiled reference (oracle/_ref/liboc_ref.so) on the ladders of tests/border_cases.py.

tests/test_gpu_border.py pins the kernels' range rule on the oracle; what pins the ORACLE's rule at an exact limit -- `x < 1`,
`x >= size - 2` on a sample that sits on the limit or one float beside it -- is this file: ICGN2D1 and ICGN2D2 (plain, with centre
offsets, self-adaptive, both), ICLM2D1 / ICLM2D2, NR2D1 and ICGN3D1 (r = (5, 6, 4) and the four large radii): oracle(ORDER_SEQ) ==
reference in every bit of every record.  The conditions that keep a ladder from passing emptily are asserted on the oracle in
tests/test_oracle_border.py; identical records meet them too.  Skipped where the reference tree is not mounted.
"""
import numpy as np
import pytest

import border_cases as bc
import oracle
from oracle import ref as oref

pytestmark = pytest.mark.skipif(not oref.available(), reason="reference tree not mounted: oracle/_ref cannot be built")

ENGINE = {"icgn2d1": 0, "icgn2d2": 1, "iclm2d1": 2, "iclm2d2": 3, "nr2d1": 4}   # oref.ICGN2D1 ... oref.NR2D1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    mism = np.argwhere(_bits(got) != _bits(want))
    assert mism.size == 0, (what, len(mism), "first mismatches (record, field): %s" % mism[:10].tolist())


def _ref2d(solver, pair, q, off, adaptive):
    ref, tar = bc.pair2d(*pair)
    out = q.copy()
    kw = dict(damping=oracle.DEFAULT_DAMPING) if solver.startswith("iclm") else {}
    oref.solve2d(ENGINE[solver], ref, tar, bc.R2D[0], bc.R2D[1], bc.CONV, bc.STOP2D, out, center_offsets=off, self_adaptive=adaptive, **kw)
    return out


# centre offsets and per-POI radii: the overloads of ICGN2D1 / ICGN2D2 alone
CASES2D = [(key, solver) for key in sorted(bc.group(bc.ladders2d()), key=str) for solver in bc.SOLVERS2D
           if key[1] == "plain" or solver in ("icgn2d1", "icgn2d2")]


@pytest.mark.parametrize("key,solver", CASES2D, ids=["%+d%+d-%s-%s" % (k[0][0], k[0][1], k[1], s) for k, s in CASES2D])
def test_2d_solvers_bit_exact(key, solver):
    pair, mode = key
    q, off, at = bc.group(bc.ladders2d())[key]
    adaptive = mode in ("adaptive", "both")
    want = _ref2d(solver, pair, q, off, adaptive)
    got = bc.oracle2d(solver, pair, q, oracle.ORDER_SEQ, offsets=off, adaptive=adaptive)
    for l, s in at:
        _same_bits(got[s], want[s], (solver, l.name))
    if solver.startswith("icgn"):
        assert (want[:, oracle.P2["zncc"]] == -3).sum() >= 2 * len(at) and (want[:, oracle.P2["zncc"]] > 0.9).sum() >= 2


@pytest.mark.parametrize("name", [l.name for l in bc.ladders3d()])
def test_icgn3d1_bit_exact(name):
    l = [l for l in bc.ladders3d() if l.name == name][0]
    _check3d(l)


@pytest.mark.parametrize("r", bc.LARGE_R)
def test_icgn3d1_large_radii_bit_exact(r):
    for l in bc.ladders3d_large(r):
        _check3d(l)


def _check3d(l):
    ref, tar = bc.pair3d(*l.pair, l.shape)
    want = l.queue.copy()
    oref.icgn3d1(ref, tar, l.r[0], l.r[1], l.r[2], bc.CONV, l.stop, want)
    _same_bits(bc.oracle3d(l, l.queue, oracle.ORDER_SEQ, 256), want, l.name)
    z = want[:, oracle.P3["zncc"]]
    assert (z == -3).sum() >= 2 and (z > 0.9).sum() >= 2, l.name

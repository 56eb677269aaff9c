"""The ladders of tests/border_cases.py through the A/B partners that restate the range rule themselves: the LDS-band kernel
(icgn2d_variant 9, icgn2d_band.hip: its own corner test and band limits) and the ICGN3D1 row mapping (icgn3d_rows.hip), bit for bit
against their oracle orders -- the queues and the bar of tests/test_gpu_border.py.  Runs inside tests/test_gpu_ab_build.py (the A/B
build + a GPU); collected anywhere else it skips."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.skipif(os.environ.get("OC_AB_RUN") != "1", reason="runs inside tests/test_gpu_ab_build.py (needs the A/B build + a GPU)")


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    assert opencorr_amd.capi.LIB_PATH.endswith("libopencorr_hip_ab.so"), opencorr_amd.capi.LIB_PATH
    return opencorr_amd


@pytest.mark.parametrize("dof", [6, 12])
def test_band_kernel_on_the_2d_ladders(eng, dof):
    import border_cases as bc
    import oracle
    from test_gpu_border import _check
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    groups = bc.group(bc.ladders2d())
    for key in sorted(k for k in groups if k[1] in ("plain", "offsets")):
        pair, mode = key
        q, off, at = groups[key]
        e = (eng.ICGN2D1 if dof == 6 else eng.ICGN2D2)(bc.R2D[0], bc.R2D[1], bc.CONV, bc.STOP2D)
        e.set_images(*bc.pair2d(*pair))
        e.prepare()
        e.set_tuning("icgn2d_variant", 9)
        for fma, order in ((0, oracle.ORDER_LANES), (1, oracle.ORDER_LANES_FMA)):
            e.set_tuning("arith_fma", fma)
            want = bc.oracle2d(solver, pair, q, order, offsets=off)
            for xcd in (1, 0):
                e.set_tuning("icgn2d_xcd", xcd)
                got = e.compute_with_offsets(q.copy(), off.copy()) if off is not None else e.compute(q.copy())
                _check(got, want, at, ("band", dof, key, fma, xcd))
        e.close()


def test_row_mapping_on_the_3d_ladders(eng):
    """Every 3D ladder through the row mapping in queue order; at r = (5, 6, 4) also the queue repeated to 2 048 records, the length
    from which the library visits it in cubic blocks (tests/test_gpu_border.py, TILE_QUEUE)."""
    import border_cases as bc
    import oracle
    from test_gpu_border import TILE_QUEUE, _check
    Z = oracle.P3["zncc"]
    sets = [[l for l in bc.ladders3d() if l.pair == pair] for pair in sorted({l.pair for l in bc.ladders3d()})]
    sets += [list(bc.ladders3d_large(r)) for r in bc.LARGE_R]
    for ladders in sets:
        l0 = ladders[0]
        q = np.concatenate([l.queue for l in ladders])
        at = [(l, slice(13 * i, 13 * i + 13)) for i, l in enumerate(ladders)]
        e = eng.ICGN3D1(l0.r[0], l0.r[1], l0.r[2], bc.CONV, l0.stop)
        e.set_images(*bc.pair3d(*l0.pair, l0.shape))
        e.prepare()
        e.set_tuning("icgn3d_mapping", 1)
        want = bc.oracle3d(l0, q, oracle.ORDER_ROWS, 512)      # (the row association has no fused-arithmetic form)
        assert (want[:, Z] == -3).sum() >= 2 * len(at) and (want[:, Z] > 0.9).sum() >= 2 * len(at)
        e.set_tuning("icgn3d_tile_vox", 0)
        _check(e.compute(q.copy()), want, at, ("rows", l0.pair, l0.r, "queue order"))
        if l0.r == bc.R3D:
            reps = -(-TILE_QUEUE // len(q))
            at_big = [(l, slice(s.start + k * len(q), s.stop + k * len(q))) for k in range(reps) for l, s in at]
            e.set_tuning("icgn3d_tile_vox", 8)
            _check(e.compute(np.tile(q, (reps, 1))), np.tile(want, (reps, 1)), at_big, ("rows", l0.pair, l0.r, "8-voxel blocks"))
        e.close()

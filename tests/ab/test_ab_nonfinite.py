"""The queues of tests/nonfinite_cases.py through the A/B partners that restate the entry guard themselves: the LDS-band kernel
(icgn2d_variant 9, icgn2d_band.hip, whose rejected waves stay in the workgroup's loop) and the ICGN3D1 row mapping
(icgn3d_rows.hip) -- the expected records and the bar of tests/test_gpu_nonfinite.py.  Runs inside tests/test_gpu_ab_build.py (the
A/B build + a GPU); collected anywhere else it skips."""
import os

import pytest

pytestmark = pytest.mark.skipif(os.environ.get("OC_AB_RUN") != "1", reason="runs inside tests/test_gpu_ab_build.py (needs the A/B build + a GPU)")


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    assert opencorr_amd.capi.LIB_PATH.endswith("libopencorr_hip_ab.so"), opencorr_amd.capi.LIB_PATH
    return opencorr_amd


@pytest.mark.parametrize("dof", [6, 12])
def test_band_kernel_rejects_nan_coordinates(eng, dof):
    import border_cases as bc
    import nonfinite_cases as nf
    import oracle
    from test_gpu_nonfinite import _check
    solver = "icgn2d1" if dof == 6 else "icgn2d2"
    e = (eng.ICGN2D1 if dof == 6 else eng.ICGN2D2)(bc.R2D[0], bc.R2D[1], bc.CONV, nf.STOP2D)
    e.set_images(*bc.pair2d(*nf.PAIR2D))
    e.prepare()
    e.set_tuning("icgn2d_variant", 9)
    for offsets in (False, True):
        case = nf.queue2d(offsets=offsets)
        for fma, order in ((0, oracle.ORDER_LANES), (1, oracle.ORDER_LANES_FMA)):
            e.set_tuning("arith_fma", fma)
            want = nf.expected2d(solver, case, order)
            got = e.compute_with_offsets(case.queue.copy(), case.offsets.copy()) if offsets else e.compute(case.queue.copy())
            _check(got, want, case, ("band", dof, offsets, fma))
            alone = case.without_planted()
            got = e.compute_with_offsets(alone.queue.copy(), alone.offsets.copy()) if offsets else e.compute(alone.queue.copy())
            _check(got, want[case.clean], alone, ("band", dof, offsets, fma, "clean records alone"))
    e.close()


def test_row_mapping_rejects_nan_coordinates(eng):
    """In queue order, and the queue repeated to 2 048 records with a run of 64 planted ones in 8-voxel blocks."""
    import border_cases as bc
    import nonfinite_cases as nf
    import oracle
    from test_gpu_nonfinite import _check
    case = nf.queue3d()
    want = nf.expected3d(case, oracle.ORDER_ROWS, 512)      # (the row association has no fused-arithmetic form)
    e = eng.ICGN3D1(bc.R3D[0], bc.R3D[1], bc.R3D[2], bc.CONV, bc.STOP3D)
    e.set_images(*bc.pair3d(*nf.PAIR3D))
    e.prepare()
    e.set_tuning("icgn3d_mapping", 1)
    e.set_tuning("icgn3d_tile_vox", 0)
    _check(e.compute(case.queue.copy()), want, case, ("rows", "queue order"))
    big, want_big = nf.long_queue(case, want, 2048)
    e.set_tuning("icgn3d_tile_vox", 8)
    _check(e.compute(big.copy()), want_big, case, ("rows", "8-voxel blocks"))
    e.close()

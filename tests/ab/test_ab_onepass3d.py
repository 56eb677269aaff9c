"""The one-pass contract of ICGN3D1 (`arith_onepass3d`) has one mapping.  In the A/B build, which also contains the row mapping
(`icgn3d_mapping` = 1, icgn3d_rows.hip), the two keys together are refused when compute() is called: a call never silently runs
another contract.  Runs inside tests/test_gpu_ab_build.py (the A/B build + a GPU); collected anywhere else it skips."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.skipif(os.environ.get("OC_AB_RUN") != "1", reason="runs inside tests/test_gpu_ab_build.py (needs the A/B build + a GPU)")


def test_row_mapping_together_with_the_one_pass_contract_is_refused():
    import opencorr_amd
    import onepass3d_twin as twin
    import oracle
    assert opencorr_amd.capi.LIB_PATH.endswith("libopencorr_hip_ab.so"), opencorr_amd.capi.LIB_PATH
    ref, tar = twin.small_pair()
    pois = twin.grid_queue(ref, tar)
    icgn = opencorr_amd.ICGN3D1(8, 8, 8, 0.001, 20)
    icgn.set_images(ref, tar)
    icgn.prepare()
    icgn.set_tuning("arith_onepass3d", 1)
    icgn.set_tuning("icgn3d_mapping", 1)
    q = pois.copy()
    with pytest.raises(Exception, match="arith_onepass3d"):
        icgn.compute(q)
    assert np.array_equal(q.view(np.uint32), pois.view(np.uint32))      # nothing was computed
    icgn.set_tuning("icgn3d_mapping", 0)                                   # the contract alone: the twin's bits, in this build too
    want = twin.icgn3d1(oracle.Prepared3D(ref, tar), 8, 8, 8, 0.001, 20, pois.copy())
    assert np.array_equal(icgn.compute(pois.copy()).view(np.uint32), want.view(np.uint32))
    icgn.set_tuning("arith_onepass3d", 0)                                  # and the row mapping alone still runs
    icgn.set_tuning("icgn3d_mapping", 1)
    rows = pois.copy()
    oracle.icgn3d1(oracle.Prepared3D(ref, tar), 8, 8, 8, 0.001, 20, rows, order=oracle.ORDER_ROWS, lanes=512)
    assert np.array_equal(icgn.compute(pois.copy()).view(np.uint32), rows.view(np.uint32))

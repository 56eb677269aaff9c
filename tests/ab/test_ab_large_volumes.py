"""The row mapping of ICGN3D1 (`icgn3d_mapping` = 1, icgn3d_rows.hip) on INDEX31 and SLAB of tests/large_volume_cases.py, every block,
against the oracle in ORDER_ROWS on the crops.  Subsets with fewer than 28 samples per row are served by the kernel of icgn3d.hip under
this key, so the radii that reach the row kernel's own walk (RowWalk) and its own base addresses are lv.ROWS_RADII, rx = 14: on INDEX31
the box's first voxel lies past byte offset 2^32 (seam30) and past voxel index 2^31 (seam31, corner), on SLAB the box spans more than
2^31 voxels.  The shapes' own radii run too.  Runs inside tests/test_gpu_ab_build.py (the A/B build + a GPU); collected anywhere else
it skips."""
import gc
import os

import pytest

pytestmark = pytest.mark.skipif(os.environ.get("OC_AB_RUN") != "1", reason="runs inside tests/test_gpu_ab_build.py (needs the A/B build + a GPU)")


@pytest.mark.parametrize("key", ["INDEX31", "SLAB"])
def test_row_mapping_where_voxel_offsets_pass_2_31(key):
    import opencorr_amd
    import torch
    import large_volume_cases as lv
    import large_volume_engines as lve
    assert opencorr_amd.capi.LIB_PATH.endswith("libopencorr_hip_ab.so"), opencorr_amd.capi.LIB_PATH
    need = lve.CASES[key][1]
    total = torch.cuda.get_device_properties(0).total_memory
    if total < need:
        pytest.skip("%s needs %.1f GB, the device has %.1f GB in total" % (key, need / lve.GB, total / lve.GB))
    huge = lve.Huge(torch, key)
    try:
        e = huge.get("ICGN3D1", lve.icgn3d1(opencorr_amd, key))
        for radii in lv.ROWS_RADII[key] + lv.RADII[key]:
            for mapping, contract in ((1, "rows"), (0, "lanes")):
                e.set_tuning("icgn3d_mapping", mapping)
                lve.solve_and_compare(e, key, contract, radii, "mapping %d" % mapping)
    finally:
        huge.close()
        del huge
        gc.collect()
        torch.cuda.empty_cache()

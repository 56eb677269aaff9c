"""The planted peaks of tests/fftcc_peak_cases.py through the A/B partner that restates the FFTCC tail itself: the earlier fused 32^3
kernel ("fftcc3d_fused" = 2, fftcc3d_fused_r5.hip) on the r = 16 queue -- every seam combination of the three axes and random
positions, in queue order and repeated to the length of the block schedule; the closed-form expectations and the bars of
tests/test_gpu_fftcc_peaks.py.  Runs inside tests/test_gpu_ab_build.py (the A/B build + a GPU); collected anywhere else it skips."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.skipif(os.environ.get("OC_AB_RUN") != "1", reason="runs inside tests/test_gpu_ab_build.py (needs the A/B build + a GPU)")


def test_fused32_r5_kernel_on_the_planted_r16_queue():
    import opencorr_amd
    import fftcc_peak_cases as pc
    from test_gpu_fftcc_peaks import TILE_QUEUE, _check
    assert opencorr_amd.capi.LIB_PATH.endswith("libopencorr_hip_ab.so"), opencorr_amd.capi.LIB_PATH
    ref, tar, queue, expected = pc.queue3d(16, 16, 16)
    f = opencorr_amd.FFTCC3D(16, 16, 16)
    f.set_images(ref, tar)
    f.set_tuning("fftcc3d_fused", 2)
    _check(f.compute(queue.copy()), queue, expected, 3, "fused32", "fused32 r5 kernel")
    reps = -(-TILE_QUEUE // len(queue))
    big, want = np.tile(queue, (reps, 1)), np.tile(expected, (reps, 1))
    for tile_vox in (64, 0):
        f.set_tuning("fftcc3d_tile_vox", tile_vox)
        _check(f.compute(big.copy()), big, want, 3, "fused32", "fused32 r5 kernel x%d tile_vox=%d" % (reps, tile_vox))
    f.close()

"""The ICGN3D1 launch-shape sweep covers the kernel as it is tuned today (no GPU needed).

tests/icgn3d_launch_shape.py restates how launch_icgn3d1 picks the row pitch and samples_per_pass from the radii.  Retuning
the kernel (another LDS window, workgroup size or candidate list) changes which radii reach which shape: these tests then
fail, and say that the sweep's radius list has to be recomputed.
"""
import collections
import os
import re

import icgn3d_launch_shape as shape

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "opencorr_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_helper_uses_the_kernels_constants():
    dev = _read("icgn3d_device.h")
    assert int(re.search(r"constexpr\s+int\s+kWinCap\s*=\s*(\d+)\s*;", dev).group(1)) == shape.WIN_CAP
    assert int(re.search(r"constexpr\s+int\s+kBlock3d\s*=\s*(\d+)\s*;", dev).group(1)) == shape.BLOCK
    hip = _read("icgn3d.hip")
    launcher = hip[hip.index("hipError_t launch_icgn3d1(const Icgn3dParams& p, float* pois, int stride_f, size_t count, hipStream_t stream) {\n    if (count"):]
    tries = re.search(r"const\s+int\s+tries\[\]\s*=\s*\{([^}]*)\}", launcher).group(1)
    assert tuple(int(v) for v in tries.split(",")) == shape.TRIES
    # the pitch rule and the instantiations it switches over
    assert re.search(r"want\s*<=\s*40\s*\?\s*40\s*:\s*want\s*<=\s*48\s*\?\s*48\s*:\s*want\s*<=\s*64\s*\?\s*64\s*:\s*0", launcher)
    assert sorted(int(v) for v in re.findall(r"icgn3d1_kernel<(\d+)>", launcher)) == [0, 40, 48, 64]


def test_helper_on_known_radii():
    assert shape.launch_shape(16, 16, 16) == (40, 12, True)      # config E: six passes of 12 x 512 samples per sweep
    assert shape.launch_shape(21, 21, 21)[0] == 48 and shape.launch_shape(25, 25, 25)[0] == 64
    assert shape.launch_shape(30, 30, 30) == (0, 1, False)
    assert shape.launch_shape(3, 16, 8) == (40, 2, True) and shape.launch_shape(32, 8, 8) == (0, 10, True)
    assert shape.launch_shape(3, 30, 3) == (40, 1, False)


def test_sweep_reaches_every_launch_shape():
    hit = collections.defaultdict(list)
    for r in shape.SWEEP_RADII:
        assert all(v in shape.RADIUS_RANGE for v in r) and len(set(shape.SWEEP_RADII)) == len(shape.SWEEP_RADII)
        hit[shape.launch_shape(*r)].append(r)
    reach = shape.reachable()
    assert len(reach) == 35 and {s[0] for s in reach} == {0, 40, 48, 64}
    missing = sorted(reach - set(hit))
    assert not missing, "launch shapes (pitch, samples_per_pass, fits) that no radius of SWEEP_RADII reaches: %s" % missing
    # the 15-record queue of the sweep needs room on the 96 x 100 x 104 pair (tests/test_gpu_parity_3d.py BIG)
    for rx, ry, rz in shape.SWEEP_RADII:
        assert 104 - 2 * (rx + 5) >= 8 and 100 - 2 * (ry + 5) >= 8 and 96 - 2 * (rz + 5) >= 8
        assert 104 // 2 - 1.5 - 1.3 * rx - 2 >= 1 and 104 // 2 + 1.3 * rx + 3 < 104 - 2   # the stretched subvolumes stay inside

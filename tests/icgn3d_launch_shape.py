"""The launch shape ICGN3D1 picks from the subvolume radii, restated for the tests (TEST INFRASTRUCTURE ONLY).

``launch_icgn3d1`` (opencorr_amd/csrc/icgn3d.hip) chooses a row pitch of the staged coefficient box in LDS -- a compile-time
40, 48 or 64 floats, or the run-time width (0) -- and ``samples_per_pass``, the samples per thread between two stagings: the
largest of TRIES whose nominal box fits the LDS window of WIN_CAP floats.  Each (pitch, samples_per_pass, fits) is a
different geometry of the staged box and a different split between staged and global taps.
tests/test_icgn3d_launch_shapes.py reads the three constants out of the kernel sources and asserts that SWEEP_RADII reaches
every combination that radii 3 ... 32 can reach; tests/test_gpu_parity_3d.py runs SWEEP_RADII on the GPU.
"""
import itertools

WIN_CAP = 16768                          # kWinCap, icgn3d_device.h
BLOCK = 512                              # kBlock3d, icgn3d_device.h
TRIES = (16, 12, 10, 8, 6, 4, 3, 2, 1)   # tries[], launch_icgn3d1
RADIUS_RANGE = range(3, 33)


def launch_shape(rx, ry, rz):
    """(pitch, samples_per_pass, fits): ``fits`` is False when not even one sample per pass keeps the nominal box inside
    the window (samples_per_pass stays 1 and passes whose box overflows take global taps)."""
    sx, sy, sz = 2 * rx + 1, 2 * ry + 1, 2 * rz + 1
    want = sx + 5
    pitch = 40 if want <= 40 else 48 if want <= 48 else 64 if want <= 64 else 0
    for m in TRIES:
        length = m * BLOCK
        planes = (length + sx * sy - 1) // (sx * sy) + 1
        nz = min(planes, sz) + 3 + 1
        rows = sy if planes > 1 else (length + sx - 1) // sx + 1
        ny = min(rows, sy) + 3 + 2
        nx = pitch if pitch else sx + 3 + 2
        if nx * ny * nz <= WIN_CAP:
            return pitch, m, True
    return pitch, 1, False


def reachable():
    """Every (pitch, samples_per_pass, fits) that radii in RADIUS_RANGE reach."""
    return {launch_shape(*r) for r in itertools.product(RADIUS_RANGE, repeat=3)}


# cubes: the classes no other test runs (r = 3 ... 8, 16, 21, 25, 30 are run elsewhere; 13 and 17 share a shape, both are
# kept: 17 is the largest cube of pitch 40); slabs and rods: one or two large radii, which reach what no cube does
SWEEP_RADII = [
    (10, 10, 10), (13, 13, 13), (17, 17, 17), (18, 18, 18), (19, 19, 19), (20, 20, 20),
    (3, 3, 3), (6, 8, 8), (13, 5, 11),
    (3, 16, 8), (3, 8, 8), (4, 8, 8), (4, 30, 8), (3, 30, 3), (19, 16, 8), (18, 3, 16), (18, 3, 3), (18, 22, 3),
    (22, 16, 8), (23, 16, 8), (22, 8, 8), (23, 3, 16), (27, 3, 16), (22, 3, 3), (22, 12, 3), (22, 14, 3),
    (30, 16, 8), (31, 16, 8), (32, 8, 8), (30, 3, 16), (30, 3, 3), (30, 12, 3), (30, 13, 3), (30, 19, 3),
    (18, 30, 8), (22, 30, 8),
]

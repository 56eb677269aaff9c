"""Which kernel serves an FFTCC2D / FFTCC3D window, restated in Python from the documentation of "fftcc2d_fused", "fftcc3d_fused" and
"fftcc3d_planes_blocks" in include/opencorr_hip.h, DESIGN.md 4.2 / 4.3 / 4.6 and the file headers of the kernels -- NOT from
opencorr_amd/csrc/host/fftcc_plan.h, which tests/test_fftcc_plan_cpu.py compares against this file row by row.  The header keeps the
instantiated window sides as lists; here they are ranges and arithmetic.

plan2d() / plan3d() / planes() return the line tests/cpp/fftcc_plan_check.cpp prints for the request.
"""
LDS_LIMIT = 160 * 1024      # dynamic LDS a workgroup of the box kernel may ask for
ROCFFT_CHUNK_2D, ROCFFT_CHUNK_3D = 32768, 1024
MAX_LAUNCH = 1 << 30


def largest_prime_factor(n):
    p, largest = 2, 1
    while n > 1:
        while n % p == 0:
            n, largest = n // p, p
        p += 1
    return largest


def odd_part(n):
    while n % 2 == 0:
        n //= 2
    return n


def pair_side(n):
    """The sides of the rectangular instantiations: multiples of four from 16 to 64 that are a power of two times 1, 3 or 5."""
    return 16 <= n <= 64 and n % 4 == 0 and odd_part(n) in (1, 3, 5)


def kernel2d(rx, ry, key):
    if key == 0:
        return "rocfft"
    if not (4 <= rx <= 32 and 4 <= ry <= 32):      # window sides 8 ... 64
        return "rocfft"
    if rx != ry:
        return "pair" if pair_side(2 * rx) and pair_side(2 * ry) else "rect"
    if rx == 16 and key != 2:                      # 2: the generic N x N kernel also at 32 x 32
        return "fused32"
    return "smooth" if largest_prime_factor(2 * rx) <= 5 else "prime"


def rect_maxn(rx, ry):
    """The rect kernel's instantiation: the longer side within 32, 48 or 64."""
    longer = 2 * max(rx, ry)
    return 32 if longer <= 32 else 48 if longer <= 48 else 64


def box_lds_bytes(rx, ry, rz):
    """The complex volume [2rx][2ry][2rz + 1] (8 B per element), six index tables of 32 ints, and per wave of the largest workgroup
    (32 x 32 threads = 16 waves) two floats and an int of reduction space."""
    return 2 * rx * 2 * ry * (2 * rz + 1) * 8 + 6 * 32 * 4 + 3 * 16 * 4


def box_kernel_takes(rx, ry, rz):
    """Non-cubic windows with every radius in 4 ... 16 whose volume and tables fit the LDS."""
    return all(4 <= r <= 16 for r in (rx, ry, rz)) and not rx == ry == rz and box_lds_bytes(rx, ry, rz) <= LDS_LIMIT


def kernel3d(rx, ry, rz, key, ab_build):
    if key == 0:
        return "rocfft"
    if rx == ry == rz:
        if rx == 16:
            return "fused32_r5" if key == 2 and ab_build else "fused32"
        return "cube" if 4 <= rx <= 13 else "planes" if 14 <= rx <= 32 else "rocfft"
    return "box" if box_kernel_takes(rx, ry, rz) else "rocfft"


def window_floats(rx, ry, rz=0):
    return 2 * rx * 2 * ry * (2 * rz if rz else 1)


def spectrum_bins(rx, ry, rz=0):
    """Half spectrum of the real transform: the fastest dimension (2ry in 2D, 2rz in 3D) keeps n / 2 + 1 bins."""
    return 2 * rx * 2 * ry * (rz + 1) if rz else 2 * rx * (ry + 1)


def plan2d(rx, ry, key):
    return "%s %d %d %d" % (kernel2d(rx, ry, key), rect_maxn(rx, ry), window_floats(rx, ry), spectrum_bins(rx, ry))


def plan3d(rx, ry, rz, key, ab_build):
    return "%s %d %d %d" % (kernel3d(rx, ry, rz, key, ab_build), box_lds_bytes(rx, ry, rz), window_floats(rx, ry, rz), spectrum_bins(rx, ry, rz))


def planes(tuned, count, radius):
    """Workgroups of the plane-wise kernel: 256 unless tuned, in whole multiples of 8, no more than the queue rounded up to 8;
    each owns (2r)^3 complex values of scratch."""
    blocks = min(-(-(tuned if tuned > 0 else 256) // 8) * 8, -(-count // 8) * 8)
    return "%d %d" % (blocks, (2 * radius) ** 3 * 8 * blocks)

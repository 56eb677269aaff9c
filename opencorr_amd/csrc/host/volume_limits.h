// volume_limits.h -- which volumes ICGN3D1 takes, without the engine.  The streaming sweeps of icgn3d.hip, icgn3d_onepass.hip and
// icgn3d_rows.hip form one 64-bit base address per POI (the first voxel of the subvolume's box) and walk the box with a 32-bit
// voxel offset (Walk3 / RowWalk, icgn3d_device.h and icgn3d_rows.hip): `(i * DY + j) * DX + k`, advanced in wrapping unsigned
// arithmetic.  The offset of the box's last sample -- the box span -- must therefore fit 32 bits; a larger box would read a voxel
// 2^32 below the right one, in bounds and silently.  prepare() and compute() (capi.hip) refuse such a volume for the engine's
// radii.  FFTCC3D and the prepare kernels address with size_t and have no such limit.  Standard headers only
// (tests/cpp/volume_limits_check.cpp runs the rule on a CPU; tests/large_volume_cases.py restates it with exact integers).
#pragma once

namespace ochip_host {

constexpr unsigned long long kIcgn3dMaxBoxSpan = 0xffffffffull;

// (saturating: radii and sides are ints, the product of four of them need not fit 64 bits)
constexpr unsigned long long limits_mul(unsigned long long a, unsigned long long b) { return b != 0 && a > ~0ull / b ? ~0ull : a * b; }
constexpr unsigned long long limits_add(unsigned long long a, unsigned long long b) { return a > ~0ull - b ? ~0ull : a + b; }

// offset, in voxels, of the last sample of a (2rx+1) x (2ry+1) x (2rz+1) subvolume from its first one inside a volume whose rows
// hold dx voxels and whose planes hold dy rows: 2rz * dy * dx + 2ry * dx + 2rx (negative arguments count as 0)
constexpr unsigned long long icgn3d_box_span(int rx, int ry, int rz, int dy, int dx) {
    const unsigned long long x = dx > 0 ? (unsigned long long)dx : 0, y = dy > 0 ? (unsigned long long)dy : 0;
    const unsigned long long a = rx > 0 ? 2ull * (unsigned long long)rx : 0, b = ry > 0 ? 2ull * (unsigned long long)ry : 0,
                             c = rz > 0 ? 2ull * (unsigned long long)rz : 0;
    return limits_add(limits_add(limits_mul(c, limits_mul(y, x)), limits_mul(b, x)), a);
}

constexpr bool icgn3d_volume_accepted(int rx, int ry, int rz, int dy, int dx) {
    return icgn3d_box_span(rx, ry, rz, dy, dx) <= kIcgn3dMaxBoxSpan;
}

}  // namespace ochip_host

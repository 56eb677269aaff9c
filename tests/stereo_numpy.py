"""NumPy restatement of the reference's stereo chain -- the CPU twin of opencorr_amd/csrc/stereo.hip and of the POI2DS mode of
strain.hip, used by tests/test_stereo_host.py and tests/test_gpu_stereo.py only.

    Calibration::prepare / undistort   src/oc_calibration.cpp:117-264   float32, every operation rounded on its own, in the
                                                                         source's operand order (NumPy float32 arrays do that)
    Stereovision::reconstruct          src/oc_stereovision.cpp:70-124   the 4 x 3 system in float32 as written; solved in
                                                                         float64 (or float32) by least squares
    Strain::compute(POI2DS*)           src/oc_strain.cpp:250-370        float64 plane fit over the reference's neighbour sets

The control flow of the per-pixel fixed-point loop (including the `isinf` reset and the "either axis" test as written) is kept
with masks: a pixel that has stopped is not touched again.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt4_stereo_r16.npz")
F32 = np.float32

# columns of the 26-column table (IO2D::saveTable2DS) and of the 28-float POI2DS record
T = {n: i for i, n in enumerate(["x", "y", "u", "v", "w", "r1r2_zncc", "r1t1_zncc", "r1t2_zncc", "r2_x", "r2_y", "t1_x", "t1_y",
                                 "t2_x", "t2_y", "ref_x", "ref_y", "ref_z", "tar_x", "tar_y", "tar_z", "exx", "eyy", "ezz", "exy",
                                 "eyz", "ezx"])}


def load_fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


class Camera:
    def __init__(self, intrinsics, extrinsics):
        c = np.asarray(intrinsics, dtype=F32)
        (self.fx, self.fy, self.fs, self.cx, self.cy, self.k1, self.k2, self.k3, self.k4, self.k5, self.k6, self.p1, self.p2) = [F32(v) for v in c]
        self.intrinsics = c
        self.extrinsics = np.asarray(extrinsics, dtype=F32)

    # src/oc_calibration.cpp:126-133
    def sensor_to_image(self, sx, sy):
        iy = (sy - self.cy) / self.fy
        ix = (sx - self.cx - self.fs * iy) / self.fx
        return ix, iy

    # :117-124
    def image_to_sensor(self, ix, iy):
        sy = iy * self.fy + self.cy
        sx = ix * self.fx + iy * self.fs + self.cx
        return sx, sy

    # :136-159
    def distort(self, x, y):
        one, two = F32(1), F32(2)
        xx = x * x
        yy = y * y
        xy = x * y
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r2 * r4
        radial = (one + self.k1 * r2 + self.k2 * r4 + self.k3 * r6) / (one + self.k4 * r2 + self.k5 * r4 + self.k6 * r6)
        dy = y * radial
        dx = x * radial
        dy = dy + (self.p1 * (r2 + two * yy) + two * self.p2 * xy)
        dx = dx + (two * self.p1 * xy + self.p2 * (r2 + two * xx))
        return dx, dy

    # :161-219.  Returns (map_x, map_y, iterations used per pixel)
    def undistortion_map(self, height, width, convergence=0.001, iteration=40):
        conv = F32(convergence)
        with np.errstate(all="ignore"):
            c, r = np.meshgrid(np.arange(width, dtype=F32), np.arange(height, dtype=F32))
            x0, y0 = self.sensor_to_image(c, r)
            x, y = x0.copy(), y0.copy()
            live = np.ones((height, width), dtype=bool)
            used = np.zeros((height, width), dtype=np.int32)
            for _ in range(int(iteration)):
                if not live.any():
                    break
                idx = np.nonzero(live)
                xi, yi = x[idx], y[idx]
                used[idx] += 1
                dx, dy = self.distort(xi, yi)
                sx, sy = self.image_to_sensor(dx, dy)
                dev_y = r[idx] - sy
                dev_x = c[idx] - sx
                inf = np.isinf(dev_x) | np.isinf(dev_y)
                stop = inf.copy()
                xi = np.where(inf, x0[idx], xi)
                yi = np.where(inf, y0[idx], yi)
                move = (np.abs(dev_x) > conv) | (np.abs(dev_y) > conv)
                dev_y2 = dev_y / self.fy
                yn = yi + dev_y2
                xn = xi + (dev_x - dev_y2 * self.fs) / self.fx
                yi = np.where(move, yn, yi)
                xi = np.where(move, xn, xi)
                stop |= ~move
                x[idx], y[idx] = xi, yi
                live[idx] = ~stop
        return x, y, used

    # :221-264 (NaN coordinates are the caller's to keep away)
    def undistort(self, map_x, map_y, px, py):
        h, w = map_x.shape
        px = np.array(px, dtype=F32)
        py = np.array(py, dtype=F32)
        px[px < 0] = 0
        py[py < 0] = 0
        px[px > F32(w - 2)] = F32(w) - F32(2)
        py[py > F32(h - 2)] = F32(h) - F32(2)
        yi = np.floor(py).astype(np.int64)
        xi = np.floor(px).astype(np.int64)
        yd = py - yi.astype(F32)
        xd = px - xi.astype(F32)
        one = F32(1)

        def look(m):
            v = m[yi, xi] * (one - yd) * (one - xd)
            v = v + m[yi + 1, xi] * yd * (one - xd)
            v = v + m[yi, xi + 1] * (one - yd) * xd
            v = v + m[yi + 1, xi + 1] * yd * xd
            return v

        cy = look(map_y)
        cx = look(map_x)
        return self.image_to_sensor(cx, cy)


def rotation_matrix64(rvec):
    """Rodrigues' formula in float64."""
    r = np.asarray(rvec, dtype=np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def matrices64(intrinsics, extrinsics):
    """(K, R, t, P) of a camera in float64 from its float32 parameters."""
    c = np.asarray(intrinsics, dtype=np.float64)
    e = np.asarray(extrinsics, dtype=np.float64)
    K = np.array([[c[0], c[2], c[3]], [0, c[1], c[4]], [0, 0, 1]])
    R = rotation_matrix64(e[3:6])
    t = e[0:3].copy()
    P = K @ np.hstack([R, t[:, None]])
    return K, R, t, P


def system32(P1, P2, x1, y1, x2, y2):
    """The 4 x 3 system of src/oc_stereovision.cpp:88-112 in float32: (n, 4, 3), (n, 4)."""
    P1 = np.asarray(P1, dtype=F32)
    P2 = np.asarray(P2, dtype=F32)
    n = len(x1)
    A = np.empty((n, 4, 3), dtype=F32)
    b = np.empty((n, 4), dtype=F32)
    for j in range(3):
        A[:, 0, j] = x1 * P1[2, j] - P1[0, j]
        A[:, 1, j] = y1 * P1[2, j] - P1[1, j]
        A[:, 2, j] = x2 * P2[2, j] - P2[0, j]
        A[:, 3, j] = y2 * P2[2, j] - P2[1, j]
    b[:, 0] = P1[0, 3] - x1 * P1[2, 3]
    b[:, 1] = P1[1, 3] - y1 * P1[2, 3]
    b[:, 2] = P2[0, 3] - x2 * P2[2, 3]
    b[:, 3] = P2[1, 3] - y2 * P2[2, 3]
    return A, b


def solve_lstsq(A, b, dtype=np.float64):
    """Least-squares solution of every system by Householder QR (LAPACK) in `dtype` (not rounded)."""
    A = A.astype(dtype)
    b = b.astype(dtype)
    q, r = np.linalg.qr(A)
    x = np.linalg.solve(r, np.einsum("nij,ni->nj", q, b)[..., None])[..., 0]
    return x


def reconstruct(cam1, maps1, P1, cam2, maps2, P2, p1, p2, dtype=np.float64, rounded=True):
    """Stereovision::reconstruct for (n, 2) point pairs; NaN among the inputs -> (0, 0, 0).  rounded=False: the solution in
    `dtype` as solved, before its rounding to float32."""
    p1 = np.asarray(p1, dtype=F32)
    p2 = np.asarray(p2, dtype=F32)
    out = np.zeros((len(p1), 3), dtype=F32 if rounded else dtype)
    ok = ~(np.isnan(p1).any(axis=1) | np.isnan(p2).any(axis=1))
    if ok.any():
        x1, y1 = cam1.undistort(maps1[0], maps1[1], p1[ok, 0], p1[ok, 1])
        x2, y2 = cam2.undistort(maps2[0], maps2[1], p2[ok, 0], p2[ok, 1])
        A, b = system32(P1, P2, x1, y1, x2, y2)
        out[ok] = solve_lstsq(A, b, dtype)
    return out


def strain_neighbours(xy, gate, radius, nmin):
    """Per POI the indices Strain::compute(POI2DS*) fits over (src/oc_strain.cpp:262-294): the POIs within `radius` of (x, y)
    when there are at least nmin of them, else the nmin nearest (distance, then index); of those, the ones whose gate holds.
    Distances in float32 as nanoflann's L2_Simple accumulates them."""
    xy = np.asarray(xy, dtype=F32)
    n = len(xy)
    r2 = F32(radius) * F32(radius)
    order = np.argsort(xy[:, 0], kind="stable")
    xs = xy[order, 0]
    out = []
    knn = np.zeros(n, dtype=bool)
    for i in range(n):
        lo = np.searchsorted(xs, xy[i, 0] - F32(radius) - F32(1), side="left")
        hi = np.searchsorted(xs, xy[i, 0] + F32(radius) + F32(1), side="right")
        cand = np.sort(order[lo:hi])
        dx = xy[i, 0] - xy[cand, 0]
        dy = xy[i, 1] - xy[cand, 1]
        d = dx * dx + dy * dy
        inside = cand[d < r2]
        if len(inside) < nmin:
            dx = xy[i, 0] - xy[:, 0]
            dy = xy[i, 1] - xy[:, 1]
            d = dx * dx + dy * dy
            d = np.where(np.isnan(d), np.inf, d)
            inside = np.lexsort((np.arange(n), d))[:nmin]
            knn[i] = True
        out.append(inside[gate[inside]])
    return out, knn


def strain_poi2ds(xy, ref, uvw, zncc3, radius, nmin, threshold, approximation):
    """Strain::compute(std::vector<POI2DS>&) in float64.  Returns a dict: `strain` (n, 6) float32, `fitted` mask, `grad` (n, 9)
    float64 gradients ux uy uz vx vy vz wx wy wz, `cond` the 2-norm condition number of every fit's matrix, `knn` the POIs that
    took the K-nearest path."""
    xy = np.asarray(xy, dtype=F32)
    ref = np.asarray(ref, dtype=F32)
    uvw = np.asarray(uvw, dtype=F32)
    gate = (np.asarray(zncc3, dtype=F32) >= F32(threshold)).all(axis=1)
    n = len(xy)
    out = np.zeros((n, 6), dtype=F32)
    done = np.zeros(n, dtype=bool)
    grad = np.zeros((n, 9))
    cond = np.zeros(n)
    nb, knn = strain_neighbours(xy, gate, radius, nmin)
    h = F32(0.5)
    for i in range(n):
        if not gate[i] or len(nb[i]) < nmin:
            continue
        k = nb[i]
        d = (ref[k] - ref[i]).astype(np.float64)  # Point3D subtraction in float32, :310
        A = np.hstack([np.ones((len(k), 1)), d])
        g64, _, _, sv = np.linalg.lstsq(A, uvw[k].astype(np.float64), rcond=None)  # (4, 3): column = u, v, w
        grad[i] = g64[1:4].T.reshape(9)
        cond[i] = sv[0] / sv[-1]
        g = g64.astype(F32)
        ux, uy, uz = g[1, 0], g[2, 0], g[3, 0]
        vx, vy, vz = g[1, 1], g[2, 1], g[3, 1]
        wx, wy, wz = g[1, 2], g[2, 2], g[3, 2]
        if approximation == 1:
            e = [ux, vy, wz, h * (uy + vx), h * (vz + wy), h * (wx + uz)]
        else:
            e = [ux + h * (ux * ux + vx * vx + wx * wx), vy + h * (uy * uy + vy * vy + wy * wy), wz + h * (uz * uz + vz * vz + wz * wz),
                 h * (uy + vx + uy * ux + vy * vx + wy * wx), h * (vz + wy + uz * uy + vz * vy + wz * wy),
                 h * (wx + uz + ux * uz + vx * vz + wx * wz)]
        out[i] = e
        done[i] = True
    return dict(strain=out, fitted=done, grad=grad, cond=cond, knn=knn)


def table_to_pois(table):
    """(n, 28) POI2DS records from the 26-column table (subset_radius = 0)."""
    q = np.zeros((len(table), 28), dtype=F32)
    q[:, :26] = table
    return q

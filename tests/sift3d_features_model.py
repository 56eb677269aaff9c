"""float64 NumPy model of SIFT3D's orientation and descriptor stages (assignOrientation, constructDescriptor; src/oc_sift.cpp:849-1249):
the same rules as the contract -- window bounds as written (:870 included), IMG_BORDER, the sphere test, central differences, the
first tile that meets the ray, (int) against floor -- with plain float64 sums, ``numpy.linalg.eigh`` and no float32 rounding anywhere.
It reads the Gaussian layers the scale-space twin made (tests/sift3d_model.py pins those).  It shares nothing with the library or the
twin but the icosahedron's 12 directions, which are data."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)

_V = {0: (0.0, 0.525731, 0.850651), 1: (0.0, -0.525731, 0.850651), 2: (0.0, 0.525731, -0.850651), 3: (0.0, -0.525731, -0.850651),
      4: (0.525731, 0.850651, 0.0), 5: (-0.525731, 0.850651, 0.0), 6: (0.525731, -0.850651, 0.0), 7: (-0.525731, -0.850651, 0.0),
      8: (0.850651, 0.0, 0.525731), 9: (-0.850651, 0.0, 0.525731), 10: (0.850651, 0.0, -0.525731), 11: (-0.850651, 0.0, -0.525731)}
TILES = [(1, 0, 8), (8, 0, 4), (4, 0, 5), (5, 0, 9), (9, 0, 1), (6, 1, 8), (6, 8, 10), (10, 8, 4), (10, 4, 2), (2, 4, 5), (2, 5, 11), (11, 5, 9),
         (11, 9, 7), (7, 9, 1), (7, 1, 6), (6, 3, 7), (7, 3, 11), (11, 3, 2), (2, 3, 10), (10, 3, 6)]
# the constants as the reference holds them: float32
VERT = np.array([[np.float32(c) for c in _V[i]] for i in range(12)], np.float64)


def _window(c, below, above, dim):
    lo = max(int(np.floor(c - below)), 1)
    hi = min(int(np.ceil(c + above)), dim - 1)
    return np.arange(lo, max(hi, lo))


def _grid(vol, centre, units, below, above):
    """voxel indices (k, j, i), physical offsets and gradients over the clamped window; vol is (z, y, x) float64"""
    nz, ny, nx = vol.shape
    ks = _window(centre[0], below[0], above[0], nx)
    js = _window(centre[1], below[1], above[1], ny)
    is_ = _window(centre[2], below[2], above[2], nz)
    i, j, k = np.meshgrid(is_, js, ks, indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    phys = np.stack([(k - centre[0]) * units[0], (j - centre[1]) * units[1], (i - centre[2]) * units[2]], 1)
    if len(i) == 0:
        return phys, np.zeros((0, 3))
    grad = np.stack([0.5 * (vol[i, j, k + 1] - vol[i, j, k - 1]) / units[0], 0.5 * (vol[i, j + 1, k] - vol[i, j - 1, k]) / units[1],
                     0.5 * (vol[i + 1, j, k] - vol[i - 1, j, k]) / units[2]], 1)
    return phys, grad


class Orientation:
    """status, the nine sums (d, then tensor xx xy xz yy yz zz), their scales, the rotation matrix (row-major, None unless accepted) and the margin:
    the smallest distance of a decision from its threshold (see orient)"""

    def __init__(self, status, sums, rotation, margin, weight_sum):
        self.status, self.sums, self.rotation, self.margin = status, sums, rotation, margin
        trace = sums[3] + sums[6] + sums[8]
        # what the sums are measured against: |sum of g w| <= sqrt(sum of g^2 w) sqrt(sum of w), and the tensor's trace
        self.scale_d, self.scale_t = float(np.sqrt(trace * weight_sum)), float(trace)


def orient(vol, units, candidate, beta=0.9, gamma=0.4, gradient_threshold=0.0000000001, **_):
    vol = np.asarray(vol, np.float64)
    units = [float(u) for u in units]
    centre = [float(candidate["x"]), float(candidate["y"]), float(candidate["z"])]
    sigma_w = 1.5 * float(candidate["scale"])
    radius = 3.0 * sigma_w
    below = [radius / u for u in units]
    above = [radius / units[0], radius * units[1], radius / units[2]]   # :870
    phys, grad = _grid(vol, centre, units, below, above)
    norm = np.sqrt((phys ** 2).sum(1))
    keep = norm <= radius
    w = np.exp(-0.5 * (norm[keep] / sigma_w) ** 2)
    g = grad[keep]
    d = (g * w[:, None]).sum(0)
    t = np.array([(g[:, a] * g[:, b] * w).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    sums = np.concatenate([d, t])
    d2 = float(d @ d)
    margin = abs(d2 - gradient_threshold) / gradient_threshold
    if d2 < gradient_threshold:
        return Orientation(1, sums, None, margin, w.sum())
    s = np.array([[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]])
    lam, vec = np.linalg.eigh(s)
    lam, vec = lam[::-1], vec[:, ::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r10, r21 = lam[1] / lam[0], lam[2] / lam[1]
    for m in (abs(r10 - beta), abs(r21 - beta)):
        if not np.isnan(m):
            margin = min(margin, m)
    if r10 > beta or r21 > beta or abs(lam[0] - lam[1]) < EPS or abs(lam[1] - lam[2]) < EPS or abs(lam[2] - lam[0]) < EPS:
        return Orientation(2, sums, None, margin, w.sum())
    q = [vec[:, 0].copy(), vec[:, 1].copy()]
    cos_phi = np.inf
    for a in range(2):
        q_d = float(q[a] @ d)
        cos_phi = min(cos_phi, abs(q_d / (np.linalg.norm(q[a]) * np.linalg.norm(d))))
        q[a] *= 1.0 if q_d > 0 else -1.0
    margin = min(margin, abs(cos_phi - gamma))
    if cos_phi < gamma:
        return Orientation(3, sums, None, margin, w.sum())
    return Orientation(0, sums, np.concatenate([q[0], q[1], np.cross(q[0], q[1])]), margin, w.sum())


def _tile_search(g):
    """(first tile meeting each ray or -1, barycentric coordinates) for rays g (n, 3): cartisan2Barycentric, :579-623"""
    n = len(g)
    hit = np.full(n, -1)
    bary = np.zeros((n, 3))
    for t, (a, b, c) in enumerate(TILES):
        v0, v1, v2 = VERT[a], VERT[b], VERT[c]
        e1, e2, tt = v1 - v0, v2 - v0, -v0
        p = np.cross(g, e2)
        q = np.cross(tt, e1)
        det = p @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            bz = inv * (g @ q)
            by = inv * (p @ tt)
            bx = 1.0 - by - bz
            k = inv * float(q @ e2)
            res = k[:, None] * g - bx[:, None] * v0 - by[:, None] * v1 - bz[:, None] * v2
            ok = (np.abs(det) >= 10 * EPS) & (k >= 0) & (bx >= -10 * EPS) & (by >= -10 * EPS) & (bz >= -10 * EPS) & ~(np.sqrt((res ** 2).sum(1)) > 10 * EPS)
        new = ok & (hit < 0)
        hit[new] = t
        bary[new] = np.stack([bx, by, bz], 1)[new]
    return hit, bary


def describe(vol, units, keypoint, rotation=None, truncate_threshold=0.2 * 128 / 768, **_):
    """768 float64; ``rotation``: the matrix to use instead of the record's (the model's own, say)"""
    vol = np.asarray(vol, np.float64)
    units = [float(u) for u in units]
    centre = [float(c) for c in keypoint["coor_layer"]]
    R = np.asarray(keypoint["rotation_matrix"] if rotation is None else rotation, np.float64).reshape(3, 3)
    sigma = 5.0 * np.sqrt(2.0) * float(keypoint["scale"])
    sphere = 2.0 * sigma
    cube = sphere / np.sqrt(2.0)
    reach = [sphere / u for u in units]
    phys, grad = _grid(vol, centre, units, reach, reach)
    dist = np.sqrt((phys ** 2).sum(1))
    sub = 2.0 * (phys @ R.T + cube) / cube - 0.5
    keep = (dist <= sphere) & np.all((sub > -0.5) & (sub < 3.5), 1)
    dist, sub, grad = dist[keep], sub[keep], grad[keep]
    g = (grad * np.exp(-0.5 * (dist / sigma) ** 2)[:, None]) @ R.T
    mag = np.sqrt((g ** 2).sum(1))
    keep = ~(mag * mag < 10 * EPS)
    sub, g, mag = sub[keep], g[keep], mag[keep]
    hit, bary = _tile_search(g)
    keep = hit >= 0
    sub, mag, hit, bary = sub[keep], mag[keep], hit[keep], bary[keep]
    dec = sub - np.floor(sub)
    base = np.trunc(sub).astype(int)   # (int): toward zero
    bins = np.zeros(768)
    tiles = np.array(TILES)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                loc = base + np.array([dx, dy, dz])
                ok = np.all((loc >= 0) & (loc < 4), 1)
                wgt = (dec[:, 0] if dx else 1 - dec[:, 0]) * (dec[:, 1] if dy else 1 - dec[:, 1]) * (dec[:, 2] if dz else 1 - dec[:, 2])
                cube_idx = loc[:, 0] + loc[:, 1] * 4 + loc[:, 2] * 16
                for b in range(3):
                    np.add.at(bins, (cube_idx * 12 + tiles[hit, b])[ok], (mag * wgt * bary[:, b])[ok])
    bins *= 1.0 / (np.sqrt((bins ** 2).sum()) + EPS)
    bins = np.minimum(bins, truncate_threshold)
    bins *= 1.0 / (np.sqrt((bins ** 2).sum()) + EPS)
    return bins

"""Float64 model of FeatureAffine2D/3D (src/oc_feature_affine.cpp under the deterministic contract of DESIGN.md 4.12), written
in NumPy independently of the kernel and of tests/cpp/feature_affine_twin.cpp: brute-force candidate sets, the integer sample
generator restated, ``numpy.linalg.lstsq`` fits and a float64 consensus.

What the contract fixes in float32 -- which keypoints are candidates (d2 < r * r), their order, the POI-centred coordinates -- is
float32 here too: it defines the input of the arithmetic under test, not the arithmetic.  Fits, errors, sums and means are
float64.  A POI is *decidable* when no candidate error of an executed trial lies within ``1e-4 * threshold`` of the threshold
and no exit comparison lies within that band: on those POIs a correct float32 implementation must report the model's status,
trial count and inlier count."""
import numpy as np

M64 = (1 << 64) - 1
F = np.float32


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def sample_positions(base, trial, n, s):
    """Partial Fisher-Yates over 0 ... n-1, fresh every trial."""
    perm = list(range(n))
    for j in range(s):
        h = splitmix64((base + ((trial << 8) | j)) & M64)
        k = j + (((h >> 32) * (n - j)) >> 32)
        perm[j], perm[k] = perm[k], perm[j]
    return perm[:s]


class Grid:
    """The uniform grid over the reference keypoints (pitch a little above the radius, capped cell count), in float32."""

    def __init__(self, ref, radius):
        ndim = ref.shape[1]
        mn, mx = np.zeros(3, F), np.zeros(3, F)
        for a in range(ndim):
            col = ref[:, a][~np.isnan(ref[:, a])]
            if col.size:
                mn[a], mx[a] = col.min(), col.max()
        pitch = F(radius) * F(1.001)
        span = max(F(mx[a] - mn[a]) for a in range(3))
        cap = F(4096.0 if ndim == 2 else 256.0)
        if not pitch > F(span / cap):
            pitch = F(span / cap)
        if not pitch > 0:
            pitch = F(1.0)
        self.origin = mn
        self.inv_pitch = F(F(1.0) / pitch)
        self.nc = [int(F(F(mx[a] - mn[a]) * self.inv_pitch)) + 1 if a < ndim else 1 for a in range(3)]
        self.ndim = ndim

    def cells(self, pts):
        """(n, 3) integer cells of (n, ndim) float32 points"""
        pts = np.atleast_2d(pts).astype(F)
        out = np.zeros((pts.shape[0], 3), np.int64)
        for a in range(self.ndim):
            t = ((pts[:, a] - self.origin[a]).astype(F) * self.inv_pitch).astype(F)
            with np.errstate(invalid="ignore"):
                c = np.where(t >= 0, np.where(t < self.nc[a], np.trunc(np.nan_to_num(t)), self.nc[a] - 1), 0)
            out[:, a] = c.astype(np.int64)
        return out


def _dist2(p, ref):
    d = (p[0] - ref[:, 0]).astype(F)
    acc = (d * d).astype(F)
    for a in range(1, ref.shape[1]):
        d = (p[a] - ref[:, a]).astype(F)
        acc = (acc + (d * d).astype(F)).astype(F)
    return acc


def _knn(p, ref, K):
    d2 = _dist2(p, ref)
    idx = np.arange(ref.shape[0])
    keep = ~np.isnan(d2)
    order = np.lexsort((idx[keep], d2[keep]))
    return idx[keep][order][:K]


def _fit(rows_ref, rows_tar):
    A = np.concatenate([rows_ref, np.ones((rows_ref.shape[0], 1))], axis=1)
    X, _, rank, _ = np.linalg.lstsq(A, rows_tar, rcond=None)
    return X if rank == A.shape[1] else None


def run(ref, tar, pois, radius, nmin, trials, samples, threshold, seed=0, adaptive=None):
    """Per POI: status (0 / -1 / -2), trials, inliers, X (the (ndim + 1, ndim) affine matrix, float64), decidable, the
    POI-centred float32 rows of the largest consensus set (for the float32-QR bar) and, in self-adaptive mode, the updated
    (x, y, radius_x, radius_y)."""
    ref, tar = np.asarray(ref, F), np.asarray(tar, F)
    ndim = ref.shape[1]
    D = ndim + 1
    grid = Grid(ref, radius)
    kp_cells = grid.cells(ref)
    r2 = F(F(radius) * F(radius))
    thr = float(F(threshold))
    band = 1e-4 * thr
    exit_mean = float(F(F(threshold) / F(nmin)))
    out = []
    for poi in pois:
        p = np.array(poi[:ndim], F)
        rec = dict(status=0, trials=0, inliers=0, X=None, decidable=True, rows=None, update=None)
        out.append(rec)
        base = splitmix64((seed ^ (_bits(p[0]) | (_bits(p[1]) << 32))) & M64)
        if ndim == 3:
            base = splitmix64(base ^ _bits(p[2]))
        if adaptive:
            feature_min, radius_min, width, height = adaptive
            pick = _knn(p, ref, feature_min)
            if pick.size < samples:
                rec["status"] = -1
                continue
            xs, ys = ref[pick, 0], ref[pick, 1]
            x_min, x_max = min(F(width), xs.min()), max(F(-1), xs.max())
            y_min, y_max = min(F(height), ys.min()), max(F(-1), ys.max())
            if x_min <= p[0] <= x_max and y_min <= p[1] <= y_max:
                srx = int(max(abs(F(x_max - p[0])), abs(F(p[0] - x_min))))
                sry = int(max(abs(F(y_max - p[1])), abs(F(p[1] - y_min))))
            else:
                p = np.array([int(F(0.5) * F(x_max + x_min)), int(F(0.5) * F(y_max + y_min))], F)
                srx, sry = int(F(0.5) * F(x_max - x_min)), int(F(0.5) * F(y_max - y_min))
            rec["update"] = (float(p[0]), float(p[1]), float(max(srx, radius_min)), float(max(sry, radius_min)))
        else:
            d2 = _dist2(p, ref)
            pc = grid.cells(p)[0]
            inside = np.nonzero((d2 < r2) & (np.abs(kp_cells - pc).max(axis=1) <= 1))[0]
            if inside.size < samples:
                rec["status"] = -1
                continue
            if inside.size < nmin:
                pick = _knn(p, ref, nmin)
            else:
                c = kp_cells[inside]
                pick = inside[np.lexsort((inside, c[:, 0], c[:, 1], c[:, 2]))]
        lref = (ref[pick] - p).astype(F)
        ltar = (tar[pick] - p).astype(F)
        R, T = lref.astype(np.float64), ltar.astype(np.float64)
        n = pick.size
        best = np.zeros(0, np.int64)
        t = 0
        while True:
            smp = sample_positions(base, t, n, samples)
            X = _fit(R[smp], T[smp])
            if X is None:
                inl, mean = np.zeros(0, np.int64), float("nan")
            else:
                err = np.sqrt(((R @ X[:ndim] + X[ndim] - T) ** 2).sum(axis=1))
                if np.any(np.abs(err - thr) <= band):
                    rec["decidable"] = False
                inl = np.nonzero(err < thr)[0]
                mean = err[inl].sum() / inl.size if inl.size else float("nan")
            if inl.size > best.size:
                best = inl
            t += 1
            if best.size >= nmin and abs(mean - exit_mean) <= band:
                rec["decidable"] = False
            if not (t < trials and (best.size < nmin or mean > exit_mean)):
                break
        rec["trials"], rec["inliers"] = t, int(best.size)
        X = _fit(R[best], T[best]) if best.size >= D else None
        if X is None:
            rec["status"] = -2
            continue
        rec["X"], rec["rows"] = X, (lref[best], ltar[best])
    return out


def deformation(X, ndim):
    """The deformation floats of the record from the affine matrix (src/oc_feature_affine.cpp:319-324 / :579-590)."""
    if ndim == 2:
        return np.array([X[2, 0], X[0, 0] - 1, X[1, 0], X[2, 1], X[0, 1], X[1, 1] - 1])
    out = []
    for r in range(3):
        out += [X[3, r]] + [X[a, r] - (1 if a == r else 0) for a in range(3)]
    return np.array(out)

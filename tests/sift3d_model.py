"""A plain float64 NumPy model of SIFT3D's scale space (createGaussianPyramid, createDogPyramid, detectExtrema of
src/oc_sift.cpp:676-847): the stages of tests/cpp/sift3d_twin.cpp stated a second time, with whole-array operations in place of
the voxel loops, a closed form in place of the two mirror functions, and its own plan.  It shares nothing with the twin or with
opencorr_amd/csrc/host/sift3d_plan.h.

The plan's scalars (kappa, scale, sigma, the radii) are formed with float32 operations, because they are float32 values in the
reference and the integer radii depend on them; weights, blur sums, differences and comparisons are float64.
"""
import numpy as np

F = np.float32
EPS = np.finfo(np.float32).eps


class Layer:
    def __init__(self):
        self.dims = None      # (x, y, z)
        self.units = None     # (x, y, z), float32
        self.octave = 0
        self.scale = F(0)
        self.sigma = F(0)
        self.source = -1      # Gaussian layer it is made from, -1 = the input
        self.blurred = True
        self.radius = (0, 0, 0)
        self.weights = []     # float64 arrays, one per axis x, y, z
        self.vol = None       # (z, y, x) float64
        self.max_abs = -1.0


def plan(shape_zyx, n_octave_layers=3, min_dimension=8, sigma_source=1.15, sigma_base=1.6, units=(1.0, 1.0, 1.0)):
    """(n_octave, Gaussian layers without voxels)."""
    dz, dy, dx = shape_zyx
    n_octave = max(1, int(np.floor(np.log2(F(min(dx, dy, dz))) - np.log2(F(min_dimension)))) + 1)
    per = n_octave_layers + 3
    kappa = np.power(F(2), F(1) / F(n_octave_layers), dtype=F)
    first = F(1) / kappa * F(sigma_base)
    octave0_scale = [first]
    for _ in range(1, per):
        octave0_scale.append(kappa * octave0_scale[-1])
    step = np.sqrt(kappa * kappa - F(1), dtype=F)
    layers = []
    for m in range(n_octave):
        for n in range(per):
            L = Layer()
            L.octave = m
            L.dims = (dx >> m, dy >> m, dz >> m)
            L.units = tuple(F(u) * F(2 ** m) for u in units)
            if n == 0 and m > 0:
                L.source = (m - 1) * per + n_octave_layers
                L.blurred = False
                L.scale = layers[L.source].scale
            else:
                L.source = m * per + n - 1 if n > 0 else -1
                if n == 0:
                    L.scale = first
                    with np.errstate(invalid="ignore"):
                        L.sigma = np.sqrt(first * first - F(sigma_source) * F(sigma_source), dtype=F)
                else:
                    L.scale = kappa * layers[-1].scale
                    L.sigma = step * octave0_scale[n - 1]
                sigma = L.sigma if L.sigma > 0 else F(0)          # (a NaN is not > 0)
                base = max(1, int(np.ceil(F(3) * sigma))) if sigma > 0 else 1
                umax = max(L.units)
                L.radius = tuple(int(base * np.floor(umax / u + F(0.5))) for u in L.units)
                L.weights = [weights(sigma, r) for r in L.radius]
            layers.append(L)
    return n_octave, layers


def weights(sigma, radius):
    i = np.arange(1, radius + 1, dtype=np.float64)
    with np.errstate(over="ignore"):
        x = i / (np.float64(sigma) + np.float64(EPS))
        tail = np.exp(-0.5 * x * x)
    w0 = 1.0 / (1.0 + 2.0 * tail.sum())
    return np.concatenate(([w0], tail * w0))


def reflect(i, n):
    """The mirrored index of both ends in closed form: inside the axis min(|i|, 2(n-1) - i) is i, below it |i|, above it
    2(n-1) - i (ONE reflection, as the reference's, not a triangle wave); then clamped into the axis."""
    i = np.asarray(i)
    return np.clip(np.minimum(np.abs(i), 2 * (n - 1) - i), 0, n - 1)


def blur_axis(vol, axis_zyx, w):
    n = vol.shape[axis_zyx]
    c = np.arange(n)
    out = w[0] * vol
    for r in range(1, len(w)):
        out = out + w[r] * (np.take(vol, reflect(c - r, n), axis=axis_zyx) + np.take(vol, reflect(c + r, n), axis=axis_zyx))
    return out


def scale_space(volume, n_octave_layers=3, min_dimension=8, alpha=0.1, sigma_source=1.15, sigma_base=1.6, units=(1.0, 1.0, 1.0)):
    """(n_octave, Gaussian layers, DoG layers, candidates as a list of (x, y, z, octave, layer)) of a (z, y, x) volume."""
    v = np.asarray(volume, dtype=np.float64)
    n_octave, gauss = plan(v.shape, n_octave_layers, min_dimension, sigma_source, sigma_base, units)
    for L in gauss:
        src = v if L.source < 0 else gauss[L.source].vol
        if not L.blurred:
            dx, dy, dz = L.dims
            L.vol = src[0:2 * dz:2, 0:2 * dy:2, 0:2 * dx:2].copy()
            continue
        t = blur_axis(src, 2, L.weights[0])     # x
        t = blur_axis(t, 1, L.weights[1])       # y
        L.vol = blur_axis(t, 0, L.weights[2])   # z
    per, dper = n_octave_layers + 3, n_octave_layers + 2
    dog = []
    for m in range(n_octave):
        for n in range(dper):
            a, b = gauss[m * per + n], gauss[m * per + n + 1]
            D = Layer()
            D.dims, D.units, D.octave, D.scale = a.dims, a.units, m, a.scale
            D.vol = b.vol - a.vol
            D.max_abs = float(np.abs(D.vol).max())
            dog.append(D)
    candidates = []
    alpha32 = np.float64(F(alpha))
    for m in range(n_octave):
        for n in range(1, n_octave_layers + 1):
            D, lo, hi = dog[m * dper + n], dog[m * dper + n - 1].vol, dog[m * dper + n + 1].vol
            if min(D.vol.shape) < 3:
                continue
            c = D.vol[1:-1, 1:-1, 1:-1]
            others = [D.vol[:-2, 1:-1, 1:-1], D.vol[2:, 1:-1, 1:-1], D.vol[1:-1, :-2, 1:-1], D.vol[1:-1, 2:, 1:-1], D.vol[1:-1, 1:-1, :-2],
                      D.vol[1:-1, 1:-1, 2:], lo[1:-1, 1:-1, 1:-1], hi[1:-1, 1:-1, 1:-1]]
            top = np.ones(c.shape, bool)
            bottom = np.ones(c.shape, bool)
            for o in others:
                top &= c > o
                bottom &= c < o
            keep = (np.abs(c) >= alpha32 * D.max_abs) & (top | bottom)
            for z, y, x in np.argwhere(keep):
                candidates.append((int(x) + 1, int(y) + 1, int(z) + 1, m, n))
    return n_octave, gauss, dog, candidates

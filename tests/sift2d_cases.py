"""Seeded images and the case list of the SIFT2D detector tests (NumPy only): Gaussian speckle quantised to 0 ... 255, the same with
non-integer float32 values, and the planted images (constant; constant along x).  Shapes are (rows, cols)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotation_sift2d.npz")


def speckle(rows, cols, seed, spot=1.2, as_float=False):
    """Dark Gaussian spots of radius `spot` (one per 12 pixels) on a bright ground; uint8, or float32 with fractions (as_float)."""
    rng = np.random.default_rng(seed)
    n = max(rows * cols // 12, 4)
    cy, cx = rng.random(n) * rows, rng.random(n) * cols
    amp = 0.5 + 0.5 * rng.random(n)
    size = spot * (0.7 + 0.9 * rng.random(n))
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.zeros((rows, cols))
    for k in range(n):
        img += amp[k] * np.exp(-((x - cx[k]) ** 2 + (y - cy[k]) ** 2) / (2 * size[k] ** 2))
    img = 230.0 - 200.0 * np.clip(img, 0, 1)
    if as_float:
        return (img + 0.37 * np.sin(0.91 * x + 1.3 * y)).astype(np.float32)
    return np.round(img).astype(np.uint8)


def blob_lattice(rows, cols, seed, as_float=False, pitch=40):
    """Dark Gaussian blobs at full contrast on a flat bright ground, one per `pitch` pixels and far enough apart not to interact:
    one strong keypoint per blob.  The centres lie near k + 0.75 (an integer cell of the doubled base and of the octave above
    it), the sigmas are those at which the DoG extremum falls near a layer: the decisions of such a keypoint have wide margins."""
    rng = np.random.default_rng(seed)
    sigmas = (1.2, 1.4, 1.8, 2.2, 2.4, 2.8, 3.0, 3.4, 3.6, 3.8)
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.zeros((rows, cols))
    for gy in range(pitch // 2, rows - pitch // 2 + 1, pitch):
        for gx in range(pitch // 2, cols - pitch // 2 + 1, pitch):
            cx, cy = gx + 0.75 + 0.2 * (rng.random() - 0.5), gy + 0.75 + 0.2 * (rng.random() - 0.5)
            sg = sigmas[rng.integers(len(sigmas))]
            img += np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sg ** 2))
    img = 245.0 - 235.0 * img
    if as_float:
        return (img + 0.05 * np.sin(0.91 * x + 1.3 * y)).astype(np.float32)
    return np.round(img).astype(np.uint8)


def low_contrast(rows, cols, seed, keep=0.1):
    """speckle squeezed to `keep` of its contrast around mid-grey: no keypoint survives, many extrema lie near the integer threshold of the scan"""
    return np.round(128.0 + keep * (speckle(rows, cols, seed).astype(np.float64) - 128.0)).astype(np.uint8)


class Case:
    def __init__(self, name, shape, seed, as_float=False, **settings):
        self.name, self.shape, self.seed, self.as_float = name, shape, seed, as_float
        self.settings = dict(n_features=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6)
        self.settings.update(settings)

    def image(self):
        if self.name == "golden_512":
            return np.load(GOLDEN)["ref"]
        return speckle(self.shape[0], self.shape[1], self.seed, as_float=self.as_float)

    def __repr__(self):
        return self.name


# the smallest shapes at which the kernels can still go wrong
CASES = [
    Case("three_octaves", (20, 24), 1),                 # 24 x 20: octaves of 48 x 40, 24 x 20, 12 x 10 -- the top one has no scan region
    Case("odd_sides", (29, 37), 2),                     # 37 x 29: 74 x 58 -> 37 x 29 -> 18 x 14: the nearest-neighbour rule on odd sides
    Case("repeated_reflection", (16, 16), 3),           # R = 13 on the 8 x 8 octave: the reflection repeats
    Case("wide", (33, 200), 4),                         # 400 columns: two row tiles, 7 column tiles; the top octaves are narrower than R
    Case("tall", (200, 33), 5),                         # 400 rows: 7 line tiles
    Case("float_130", (130, 130), 6, as_float=True),    # non-integer float32 pixels; 260 columns: one row tile and four pixels
    # one layer per octave: the fourth Gaussian layer's sigma is 6.93 sigma, so the default 1.6 gives R = 44 and is refused (contract
    # item 1, REFUSED_SETTINGS below); 1.1 gives R = 31, the widest blur the detector takes with this setting
    Case("one_layer", (40, 44), 7, n_octave_layers=1, sigma=1.1),
    Case("five_layers", (40, 44), 8, n_octave_layers=5),
    Case("sigma_1_2", (40, 44), 9, sigma=1.2),
    Case("golden_512", (512, 512), 0),                  # the reference's rotation_000 at full size
]
CASE_BY_NAME = {c.name: c for c in CASES}


def planted(kind, shape=(40, 44), seed=11):
    """"constant": one value everywhere; "along_x": a speckle column repeated along x, so that every pixel ties with its two
    neighbours on its row: plateau candidates whose localisation meets an exactly zero pivot and which all die at det <= 0."""
    if kind == "constant":
        return np.full(shape, 97, np.uint8)
    assert kind == "along_x"
    v = speckle(shape[0], shape[1], seed)
    return np.ascontiguousarray(np.broadcast_to(v[:, 7:8], shape))


# contract item 1: what is refused, and with which status (1 = OC_HIP_ERR_INVALID, 5 = OC_HIP_ERR_UNSUPPORTED)
INVALID, UNSUPPORTED = 1, 5
REFUSED_SETTINGS = [
    (dict(n_octave_layers=0), INVALID), (dict(n_octave_layers=9), INVALID),
    (dict(sigma=0.0), INVALID), (dict(sigma=-1.0), INVALID), (dict(sigma=float("nan")), INVALID), (dict(sigma=float("inf")), INVALID),
    (dict(n_octave_layers=1), UNSUPPORTED),             # at the default sigma: R = 44
    (dict(sigma=0.01), UNSUPPORTED),                     # a blur sigma below 0.0625: a single tap, R = 0
    (dict(sigma=4.5), UNSUPPORTED),                      # the last layer's sigma gives a blur radius above 32
    (dict(n_features=100), UNSUPPORTED), (dict(n_features=-1), UNSUPPORTED),
]
REFUSED_SHAPES = [((1, 40), INVALID), ((40, 1), INVALID), ((23171, 23171), UNSUPPORTED)]   # 4 * 23171^2 > 2^31 - 1

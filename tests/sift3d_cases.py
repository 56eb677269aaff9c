"""Seeded volumes and the case list of the SIFT3D scale-space tests (NumPy only): smoothed noise quantised to 0 ... 255, and the
planted volumes whose every comparison is a tie on one axis.  Shapes are (z, y, x); units are (x, y, z)."""
import numpy as np


def smooth_noise(shape, seed, passes=2):
    """Uniform noise, box-smoothed `passes` times over the 3 x 3 x 3 neighbourhood (periodic), stretched to 0 ... 255 and rounded."""
    rng = np.random.default_rng(seed)
    v = rng.random(shape)
    for _ in range(passes):
        for axis in range(3):
            v = (np.roll(v, 1, axis) + v + np.roll(v, -1, axis)) / 3.0
    v = (v - v.min()) / (v.max() - v.min())
    return np.round(v * 255.0).astype(np.float32)


class Case:
    def __init__(self, name, shape, seed, **settings):
        self.name, self.shape, self.seed = name, shape, seed
        self.settings = dict(n_octave_layers=3, min_dimension=8, alpha=0.1, sigma_source=1.15, sigma_base=1.6, units=(1.0, 1.0, 1.0))
        self.settings.update(settings)

    def volume(self):
        return smooth_noise(self.shape, self.seed)

    def __repr__(self):
        return self.name


# the smallest shapes at which the kernels can still go wrong
CASES = [
    Case("two_octaves_odd", (18, 33, 40), 1),            # octave 1 is (9, 16, 20): R = 8 = dim - 1 in z, the last defined reflection
    Case("clamp", (16, 16, 16), 2),                      # octave 1 is 8^3 and R = 8 > 7: the clamp rule
    Case("halving_floors", (19, 21, 37), 3),
    Case("one_octave_wide", (9, 70, 130), 4),            # x crosses one and two wavefront widths, y crosses a tile
    Case("units_112", (20, 40, 40), 5, units=(1.0, 1.0, 2.0)),   # R = 16 on x and y
    Case("two_layers", (18, 33, 40), 6, n_octave_layers=2),
    Case("four_layers", (18, 33, 40), 7, n_octave_layers=4),
    Case("alpha_0", (18, 33, 40), 8, alpha=0.0),         # every strict extremum is a candidate
]
CASE_BY_NAME = {c.name: c for c in CASES}


def planted(kind, shape=(18, 33, 40), seed=11):
    """"constant": one value everywhere; "along_x" / "along_y" / "along_z": smoothed noise repeated along that axis, so that every
    voxel ties with its two neighbours on it."""
    if kind == "constant":
        return np.full(shape, 97.0, np.float32)
    axis = {"along_z": 0, "along_y": 1, "along_x": 2}[kind]
    v = smooth_noise(shape, seed)
    index = [slice(None)] * 3
    index[axis] = slice(0, 1)
    return np.ascontiguousarray(np.broadcast_to(v[tuple(index)], shape)).astype(np.float32)


PLANTED = ("constant", "along_x", "along_y", "along_z")

"""The case list of the SIFT3D orientation / descriptor tests (NumPy only): the smallest shapes at which these stages can still go
wrong.  Shapes are (z, y, x); units are (x, y, z).  Shared by tests/test_sift3d_features_cpu.py and tests/test_gpu_sift3d_features.py.

Every orientation window (radius 4.5 scale >= 7.2 voxels) and every descriptor window (radius 14.1 scale >= 22.6 voxels) of the
scale-space cases is clamped by the layer; only the centre voxel of BIG is not, and its descriptor windows are reached through planted
keypoint records (big_centre_keypoints).  A case's candidate list is cut to MAX_KEYPOINTS
records, evenly spaced, so that the twin stays within seconds."""
import numpy as np

import sift3d_cases
from sift3d_cases import Case, smooth_noise

MAX_KEYPOINTS = 48

# the scale-space cases whose windows are all clamped (octave 1 present), and the two unit settings that see :870
CASES = [sift3d_cases.CASE_BY_NAME[n] for n in ("two_octaves_odd", "halving_floors", "units_112", "two_layers", "four_layers", "alpha_0")] + [
    Case("unit_y_half", (20, 44, 40), 21, units=(1.0, 0.5, 1.0)),   # radius * unit_y < radius / unit_y: :870 cuts the sphere
    Case("unit_y_two", (20, 40, 40), 22, units=(1.0, 2.0, 1.0)),    # radius * unit_y > radius / unit_y: the sphere test decides
]
CASE_BY_NAME = {c.name: c for c in CASES}
DEFAULT_CASES = ("two_octaves_odd", "halving_floors", "units_112")   # the three the issue's prototype counted

# the one volume that holds an unclamped descriptor window: 73^3 around the centre voxel at layer 3 (radius 35.9)
BIG = Case("big_planted", (76, 78, 80), 23)


def cut(candidates, limit=MAX_KEYPOINTS):
    """At most ``limit`` records of the list, evenly spaced, in list order."""
    if len(candidates) <= limit:
        return candidates
    return candidates[np.unique(np.linspace(0, len(candidates) - 1, limit).round().astype(int))]


def candidate(dtype, x, y, z, octave, layer, scale):
    c = np.zeros(1, dtype)
    c["x"], c["y"], c["z"], c["octave"], c["layer"], c["scale"] = x, y, z, octave, layer, scale
    return c


def big_candidates(dtype, gauss):
    """Planted candidates of BIG (``gauss``: the layer records of its pyramid, dims as (x, y, z)): the centre voxel at layers 1 and
    3, one voxel next to each face and one at a corner (layer 1)."""
    nx, ny, nz = (int(v) for v in gauss[0].dims)
    cx, cy, cz = nx // 2, ny // 2, nz // 2
    s1, s3 = gauss[1].scale, gauss[3].scale
    spots = [(cx, cy, cz, 1, s1), (cx, cy, cz, 3, s3), (1, cy, cz, 1, s1), (nx - 2, cy, cz, 1, s1), (cx, 1, cz, 1, s1), (cx, ny - 2, cz, 1, s1),
             (cx, cy, 1, 1, s1), (cx, cy, nz - 2, 1, s1), (1, 1, 1, 1, s1), (nx - 1, ny - 1, nz - 1, 1, s1), (0, 0, 0, 3, s3)]
    return np.concatenate([candidate(dtype, x, y, z, 0, layer, scale) for x, y, z, layer, scale in spots])


def _oblique():
    """a fixed orthonormal matrix with no zero entry: the turn by 37 degrees about (1, sqrt 2, sqrt 3), rounded to float32.  (An axis
    through lattice points, such as (1, 2, 3), leaves the voxels on it where they are: (-4, -8, -12) would then sit on subregion
    coordinate 0 of layer 1, where (int) against floor jumps and the side taken is a matter of the last bit.)"""
    a = np.array([1.0, np.sqrt(2.0), np.sqrt(3.0)]) / np.sqrt(6.0)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(37.0)
    return (np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)).astype(np.float32).ravel()


BIG_ROTATIONS = {"identity": np.array((1, 0, 0, 0, 1, 0, 0, 0, 1), np.float32), "oblique": _oblique()}


def big_centre_keypoints(dtype, gauss):
    """Planted KEYPOINT records at BIG's centre voxel, layers 1 and 3, each with the identity and with the oblique matrix: the
    orientation stage rejects the centre candidates of this volume, so only planted records put the unclamped windows (47^3 at layer
    1, 73^3 at layer 3) through describe.  Order: (layer 1, identity), (layer 1, oblique), (layer 3, identity), (layer 3, oblique)."""
    nx, ny, nz = (int(v) for v in gauss[0].dims)
    kp = np.zeros(4, dtype)
    kp["coor_layer"] = (nx // 2, ny // 2, nz // 2)
    kp["coor_img"] = kp["coor_layer"]
    kp["octave"] = 0
    kp["layer"] = (1, 1, 3, 3)
    kp["scale"] = [gauss[1].scale, gauss[1].scale, gauss[3].scale, gauss[3].scale]
    kp["rotation_matrix"] = [BIG_ROTATIONS[r] for r in ("identity", "oblique", "identity", "oblique")]
    return kp


def unclamped(keypoint, gauss_layer):
    """True when the descriptor window of the record (the loops of src/oc_sift.cpp:1066-1079) is not cut by IMG_BORDER on any side"""
    reach = 10.0 * np.sqrt(2.0) * float(keypoint["scale"])
    for a in range(3):
        c, u, dim = float(keypoint["coor_layer"][a]), float(gauss_layer.units[a]), int(gauss_layer.dims[a])
        if np.floor(c - reach / u) < 1 or np.ceil(c + reach / u) > dim - 1:
            return False
    return True


def planted_volume(kind, shape=(30, 32, 34)):
    """"constant": status 1; "blob": an isotropic Gaussian centred on a voxel (status 1 or 2); "z_ramp": the linear ramp v = 3 z, a
    tensor of rank 1 with exact zeros (0 / 0 in :973-974, rejected by :975-977) and the volume of the describe cases;
    "oblique_ramp": linear in all three coordinates, of rank 1 only up to the rounding of its terms."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    if kind == "constant":
        return np.full(shape, 97.0, np.float32)
    if kind == "blob":
        c = [n // 2 for n in shape]
        return (200.0 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * 4.0 ** 2))).astype(np.float32)
    if kind == "z_ramp":
        return (3.0 * z).astype(np.float32)
    if kind == "oblique_ramp":
        return (2.0 * x + 3.0 * y + 5.0 * z).astype(np.float32)
    raise ValueError(kind)


PLANTED_VOLUMES = ("constant", "blob", "z_ramp", "oblique_ramp")


def planted_candidates(dtype, gauss):
    """the centre voxel and two off-centre ones at layers 1 and 2 of a planted volume"""
    nx, ny, nz = (int(v) for v in gauss[0].dims)
    out = []
    for layer in (1, 2):
        for dx, dy, dz in ((0, 0, 0), (3, -2, 1), (-5, 4, -3)):
            out.append(candidate(dtype, nx // 2 + dx, ny // 2 + dy, nz // 2 + dz, 0, layer, gauss[layer].scale))
    return np.concatenate(out)


ROTATIONS = {
    "identity": (1, 0, 0, 0, 1, 0, 0, 0, 1),
    "quarter_turn_about_x": (1, 0, 0, 0, 0, -1, 0, 1, 0),   # maps the z gradient onto -y
    "zero": (0,) * 9,                                          # every voxel fails the magnitude test: the descriptor is all zeros
}


def planted_keypoints(dtype, gauss, rotation):
    """keypoints for describe on "z_ramp": the centre voxel and one near a face, with the named rotation matrix.  Layer 2, not 1:
    there cube_radius is 16 and, under these axis-aligned matrices, whole planes of voxels sit on subregion coordinate 0, where (int)
    against floor jumps (:1174-1187) and the side taken is a matter of the last bit."""
    nx, ny, nz = (int(v) for v in gauss[0].dims)
    kp = np.zeros(2, dtype)
    kp["coor_layer"] = [(nx // 2, ny // 2, nz // 2), (2, ny // 2, nz - 3)]
    kp["coor_img"] = kp["coor_layer"]
    kp["octave"], kp["layer"], kp["scale"] = 0, 2, gauss[2].scale
    kp["rotation_matrix"] = np.array(ROTATIONS[rotation], np.float32)
    return kp


def shift_pair(seed=31, shape=(44, 48, 48), shift=4, depth=40):
    """ref = V[0:depth], tar = V[shift:shift + depth] of one volume: every feature moves by exactly (0, 0, -shift) in (x, y, z)"""
    v = smooth_noise(shape, seed)
    return np.ascontiguousarray(v[:depth]), np.ascontiguousarray(v[shift:shift + depth])


SETTINGS = Case("defaults", (1, 1, 1), 0).settings

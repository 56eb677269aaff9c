"""The arithmetic contract of SIFT3D's orientation and descriptor stages (include/opencorr_hip.h; assignOrientation and
constructDescriptor, src/oc_sift.cpp:849-1249) on a CPU: its restatement tests/cpp/sift3d_features_twin.cpp against the float64 model
tests/sift3d_features_model.py on the cases of tests/sift3d_features_cases.py, the planted slips, the planted volumes and keypoints,
the plan header (opencorr_amd/csrc/host/sift3d_feature_plan.h, through tests/cpp/sift3d_feature_plan_check.cpp, once more under
-fsanitize=undefined,address) and the pipeline property.  tests/test_gpu_sift3d_features.py then asks kernel == twin bit for bit.

Measured distances (x86-64, g++ -O2 -ffp-contract=off, glibc libm; `python tests/test_sift3d_features_cpu.py --measure`): the twin in
its REFERENCE-ACCUMULATION mode (sequential float32 `+=`, what the reference does) against the model, largest over the case list:

    the nine sums, relative to their scale     1.27e-6   (d sums against sqrt(trace * sum of weights), tensor sums against the trace)
    rotation matrix entries                    7.21e-6
    descriptor entries                         2.25e-6

The bars are 4 x those (the convention of DESIGN.md section 3).  The contract mode (exact sums) measures 4.0e-7 / 3.7e-7 / 1.6e-7.
No candidate of any case changes its status between twin and model, in either mode.

The planted slips: six of the seven leave the bars (or flip decisions far from any threshold) on a case that exposes them.  The
seventh, "the last tile that meets the ray wins", cannot: two tiles both meet a ray only inside the 10 FLT_EPSILON band around their
common edge, where they give the same bins and barycentric coordinates that differ by rounding (measured: at most 7.5e-9 per
descriptor entry, 7 of 192 rows change bits).  It is caught where the contract is exact instead: on the z ramp the first tile puts
an exact zero into every bin of direction 8 and touches no bin of direction 9, the last tile writes rounding residue into direction 9.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import image_domains
import sift3d_features_cases as cases
import sift3d_features_model as model
import sift3d_features_twin as twin
import sift3d_twin
from sift3d_cases import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, 1, 5

# the reference-accumulation mode against the model (see the module docstring), and the bars
DISTANCE = dict(sums=1.27e-6, rotation=7.21e-6, descriptor=2.25e-6)
BAR_FACTOR = 4.0
BARS = {k: BAR_FACTOR * v for k, v in DISTANCE.items()}
MARGIN, MAX_FLIPPED = 1e-4, 0.01

# a voxel at distance exactly window_radius: kappa = 2, scale = sigma_base = 2 in layer 1, sigma_w = 3, radius 9 = |(1, 4, 8)|
SPHERE_TIE = Case("sphere_tie", (24, 26, 28), 41, n_octave_layers=1, sigma_base=2.0, sigma_source=0.5)
LISTS = [c.name for c in cases.CASES] + ["big_detected", "big_planted", "sphere_tie"]


@functools.lru_cache(maxsize=None)
def _scale_space(name):
    c = cases.BIG if name.startswith("big_") else SPHERE_TIE if name == "sphere_tie" else cases.CASE_BY_NAME[name]
    v = c.volume()
    ss = sift3d_twin.scale_space(v, **c.settings)
    if name == "big_planted":
        cand = cases.big_candidates(twin.CANDIDATE, ss.gauss)
    else:
        cand = cases.cut(ss.candidates)
    return c, ss, twin.Pyramid(ss.gauss, c.settings["n_octave_layers"]), twin.grid_exponent(v, c.settings["units"]), cand


@functools.lru_cache(maxsize=None)
def _model(name):
    """the model's Orientation of every candidate of the list"""
    _, ss, pyr, _, cand = _scale_space(name)
    out = []
    for c in cand:
        g = ss.gauss[pyr.layer_index(c["octave"], c["layer"])]
        out.append(model.orient(g.vol, g.units, c))
    return out


@functools.lru_cache(maxsize=None)
def _twin(name, mode, slip=twin.SLIP_NONE):
    _, _, pyr, e, cand = _scale_space(name)
    with twin.slip(slip):
        status, sums, slots = twin.orient(pyr, cand, e, mode=mode)
        desc = twin.describe(pyr, slots[status == 0], e, mode=mode)
    return status, sums, slots, desc


def _distances(name, mode, slip=twin.SLIP_NONE):
    """(sums, rotation, descriptor distances of the twin from the model, [(candidate, twin status, model status, margin)] of the
    candidates whose status differs, number of candidates)"""
    _, ss, pyr, _, cand = _scale_space(name)
    status, sums, slots, desc = _twin(name, mode, slip)
    d = dict(sums=0.0, rotation=0.0, descriptor=0.0)
    flipped, row = [], 0
    for m, (c, o) in enumerate(zip(cand, _model(name))):
        for lo, hi, scale in ((0, 3, o.scale_d), (3, 9, o.scale_t)):
            delta = np.abs(sums[m, lo:hi].astype(np.float64) - o.sums[lo:hi]).max()
            if delta > 0:
                d["sums"] = max(d["sums"], delta / scale)
        if o.status != status[m]:
            flipped.append((m, int(status[m]), o.status, o.margin))
        if status[m] == 0:
            if o.status == 0:
                g = ss.gauss[pyr.layer_index(c["octave"], c["layer"])]
                d["rotation"] = max(d["rotation"], np.abs(slots[m]["rotation_matrix"].astype(np.float64) - o.rotation).max())
                want = model.describe(g.vol, g.units, slots[m], rotation=o.rotation)
                d["descriptor"] = max(d["descriptor"], np.abs(desc[row].astype(np.float64) - want).max())
            row += 1
    return d, flipped, len(cand)


def test_case_list_holds_every_verdict():
    """the prototype's counts: 23 / 9 / 31 candidates with the defaults; over the whole list enough of every verdict and octave 1"""
    assert [len(_scale_space(n)[4]) for n in cases.DEFAULT_CASES] == [23, 9, 31]
    counts, octave_1 = np.zeros(4, int), 0
    for name in [c.name for c in cases.CASES] + ["big_detected"]:
        assert len(_scale_space(name)[4]) <= cases.MAX_KEYPOINTS
        status, _, slots, _ = _twin(name, 0)
        counts += np.bincount(status, minlength=4)
        octave_1 += int((slots[status == 0]["octave"] >= 1).sum())
    assert counts[twin.ACCEPTED] >= 20 and counts[twin.REJECT_EIGENVALUES] >= 3 and counts[twin.REJECT_ANGLE] >= 10 and octave_1 >= 2, (counts, octave_1)


@pytest.mark.parametrize("name", LISTS)
def test_contract_mode_is_inside_the_bars(name):
    d, flipped, n = _distances(name, 0)
    print(name, d, flipped)
    for k in BARS:
        assert d[k] <= BARS[k], (name, k, d[k])
    assert all(margin < MARGIN for _, _, _, margin in flipped) and len(flipped) <= MAX_FLIPPED * n, flipped


def test_reference_accumulation_measures_what_the_bars_were_made_from():
    """the recorded distances are the reference-accumulation mode's: not exceeded (another libm may move the last digits), and not
    far above what it measures (a bar made from a stale, larger figure would be a wider bar)"""
    worst = dict(sums=0.0, rotation=0.0, descriptor=0.0)
    for name in LISTS:
        d, flipped, n = _distances(name, 1)
        assert all(margin < MARGIN for _, _, _, margin in flipped) and len(flipped) <= MAX_FLIPPED * n, (name, flipped)
        for k in worst:
            worst[k] = max(worst[k], d[k])
    print(worst)
    for k in worst:
        assert DISTANCE[k] / 1.25 <= worst[k] <= DISTANCE[k] * 1.05, (k, worst[k])


# the slip, a list that exposes it, what leaves its bar there (None: decisions flip far from their thresholds)
EXPOSED = [
    (twin.SLIP_FLOOR_INDEX, "two_octaves_odd", "descriptor"),
    (twin.SLIP_DIVIDE_870, "unit_y_half", "sums"),
    (twin.SLIP_STRICT_SPHERE, "sphere_tie", "sums"),
    (twin.SLIP_NO_TRUNCATION, "two_octaves_odd", "descriptor"),
    (twin.SLIP_TRANSPOSED, "two_octaves_odd", "rotation"),
    (twin.SLIP_ASCENDING, "two_octaves_odd", None),
]


@pytest.mark.parametrize("slip,name,what", EXPOSED)
def test_planted_slip_is_outside_the_bars(slip, name, what):
    d, flipped, n = _distances(name, 0, slip)
    print(slip, name, d, len(flipped))
    if what is None:
        assert len(flipped) > MAX_FLIPPED * n and any(margin >= MARGIN for _, _, _, margin in flipped)
    else:
        assert d[what] > BARS[what], (d, BARS)


def test_unit_y_two_does_not_see_870():
    """radius * unit_y > radius / unit_y there: the bound of :870 lies outside the sphere and the sphere test decides"""
    a, b = _twin("unit_y_two", 0), _twin("unit_y_two", 0, twin.SLIP_DIVIDE_870)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[0], b[0])


@functools.lru_cache(maxsize=None)
def _planted(kind):
    v = cases.planted_volume(kind)
    ss = sift3d_twin.scale_space(v, **cases.SETTINGS)
    return ss, twin.Pyramid(ss.gauss, 3), twin.grid_exponent(v, cases.SETTINGS["units"])


def test_planted_volumes():
    """constant: every sum zero, status 1.  blob: d = 0 at its centre (status 1), an isotropic tensor elsewhere (status 2).  z ramp
    (v = 3 z): the tensor is zz alone, eigenvalues (t, 0, 0), 0 / 0 in :974 is not > beta, :976 rejects.  oblique ramp: every term
    rounds, so the tensor is of rank 1 only up to rounding and the two small eigenvalues are not equal: it is rejected, by the
    eigenvalue tests or by the angle test (d is parallel to the first eigenvector, cos(phi) of the second is 0)."""
    verdicts = {}
    for kind in cases.PLANTED_VOLUMES:
        ss, pyr, e = _planted(kind)
        status, sums, _ = twin.orient(pyr, cases.planted_candidates(twin.CANDIDATE, ss.gauss), e)
        verdicts[kind] = status.tolist()
        assert not np.isnan(sums).any()
        if kind == "constant":
            assert not sums.any()
    assert verdicts["constant"] == [1] * 6
    assert verdicts["blob"][0] == 1 and set(verdicts["blob"][1:]) <= {1, 2}
    assert verdicts["z_ramp"] == [2] * 6
    assert set(verdicts["oblique_ramp"]) <= {2, 3}


def test_planted_keypoints_on_the_z_ramp():
    """identity: the gradient ray (0, 0, g) meets the edge between directions 0 and 1; tile 0 = (1, 0, 8) is the first to meet it, so
    the bins of directions 0 and 1 share every contribution (equal up to the roundings of the barycentric coordinates, < 1e-6
    relative: ten float32 operations) and nothing else is written.  quarter turn: the ray becomes (0, -g, 0), the edge between 6
    and 7.  zero matrix: every voxel fails the magnitude test, the descriptor is all zeros and 1 / (0 + FLT_EPSILON) makes no NaN."""
    ss, pyr, e = _planted("z_ramp")
    for rotation, pair in (("identity", (0, 1)), ("quarter_turn_about_x", (6, 7)), ("zero", None)):
        kp = cases.planted_keypoints(twin.KEYPOINT, ss.gauss, rotation)
        d = twin.describe(pyr, kp, e).reshape(len(kp), 64, 12)
        assert not np.isnan(d).any()
        if pair is None:
            assert not d.any()
            continue
        others = [t for t in range(12) if t not in pair]
        assert d[:, :, pair[0]].any() and not d[:, :, others].any()
        assert np.all(np.abs(d[:, :, pair[0]] - d[:, :, pair[1]]) <= 1e-6 * d[:, :, pair[0]])
        g = ss.gauss[2]
        for row, k in zip(d.reshape(len(kp), 768), kp):
            assert np.abs(row - model.describe(g.vol, g.units, k)).max() <= BARS["descriptor"]


def test_unclamped_centre_windows_of_the_big_volume():
    """The orientation stage rejects both centre candidates of BIG (status 3 at layer 1, 2 at layer 3), so its unclamped descriptor
    windows -- 47^3 at layer 1, 73^3 at layer 3, the largest a default pyramid has -- are reached through planted keypoint records.
    Twin against model on three of the four; (layer 1, identity) is computed but not compared: cube_radius is 16 there, so under the
    identity whole planes of voxels sit on subregion coordinates 0 (where (int) against floor jumps), -0.5 and 3.5 (the cube test),
    and float32 and float64 take different sides.  The kernel is held to the twin's bits on all four
    (tests/test_gpu_sift3d_features.py)."""
    _, ss, pyr, e, _ = _scale_space("big_planted")
    status = _twin("big_planted", 0)[0]
    assert status[0] != 0 and status[1] != 0            # (why the records are planted)
    kp = cases.big_centre_keypoints(twin.KEYPOINT, ss.gauss)
    assert all(cases.unclamped(k, ss.gauss[k["layer"]]) for k in kp)
    for mode in (0, 1):
        d = twin.describe(pyr, kp, e, mode=mode)
        assert not np.isnan(d).any() and all(np.count_nonzero(row) == 768 for row in d)
        for i, k in enumerate(kp):
            if i == 0:
                continue
            g = ss.gauss[k["layer"]]
            delta = np.abs(d[i].astype(np.float64) - model.describe(g.vol, g.units, k)).max()
            print(mode, i, delta)
            assert delta <= (BARS["descriptor"] if mode == 0 else DISTANCE["descriptor"]), (mode, i, delta)
    with twin.slip(twin.SLIP_FLOOR_INDEX):
        g = ss.gauss[3]
        assert np.abs(twin.describe(pyr, kp[3:], e)[0] - model.describe(g.vol, g.units, kp[3])).max() > BARS["descriptor"]


def test_last_tile_slip_is_caught_where_the_contract_is_exact():
    """see the module docstring: inside the bars everywhere, visible in the exact zeros of the z ramp"""
    ss, pyr, e = _planted("z_ramp")
    kp = cases.planted_keypoints(twin.KEYPOINT, ss.gauss, "identity")
    first = twin.describe(pyr, kp, e).reshape(len(kp), 64, 12)
    with twin.slip(twin.SLIP_LAST_TILE):
        last = twin.describe(pyr, kp, e).reshape(len(kp), 64, 12)
    assert not first[:, :, 9].any() and last[:, :, 9].any()
    d, _, _ = _distances("big_planted", 0, twin.SLIP_LAST_TILE)
    print(d)
    assert d["descriptor"] <= BARS["descriptor"]


def test_gradient_in_float_gives_the_double_expression_bits():
    """`0.5 * (a - b) / unit` (double, rounded on assignment) against (0.5f * (a - b)) / unit on random bit patterns: the halving is
    exact and a double rounding of the division is innocuous at 53 >= 2 * 24 + 2 bits -- wherever the quotient and the halved
    difference are normal numbers.  Subnormal ones (below 2^-126) are outside the claim and cannot matter: with |E| <= 60 every
    quantum is at least 2^-160 ... 2^-100 times larger than what such a gradient contributes, and the term rounds to 0 on the grid."""
    import ctypes
    rng = np.random.default_rng(5)
    L = twin.lib()
    tiny = float(np.finfo(np.float32).tiny)
    n = same = 0
    words = rng.integers(0, 2 ** 32, size=(40000, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    # ... and ordinary magnitudes, where random bit patterns are sparse
    plain = (rng.standard_normal((20000, 3)) * np.array([300.0, 300.0, 1.0]) + np.array([0.0, 0.0, 1.5])).astype(np.float32)
    for a, b, u in np.concatenate([words, plain]):
        with np.errstate(over="ignore", invalid="ignore"):
            diff = np.float32(a) - np.float32(b)
        if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(u) and np.isfinite(diff)) or u == 0:
            continue
        x, y = ctypes.c_float(), ctypes.c_float()
        L.oc_twin_features_gradient_forms(float(a), float(b), float(u), ctypes.byref(x), ctypes.byref(y))
        if (x.value != 0 and abs(x.value) < tiny) or (diff != 0 and abs(float(diff)) < 2 * tiny):
            continue
        n += 1
        same += int(np.float32(x.value).view(np.uint32) == np.float32(y.value).view(np.uint32) or (np.isnan(x.value) and np.isnan(y.value)))
    assert n > 50000 and same == n, (n, same)


def test_pipeline_recovers_the_shift():
    """ref = V[0:40], tar = V[4:44]: matched pairs whose tar - ref is exactly the shift are more than half of all pairs, at least 5"""
    ref, tar = cases.shift_pair()
    for bidirectional in (False, True):
        r, t, a, b = twin.pipeline(ref, tar, cases.SETTINGS, bidirectional=bidirectional)
        exact = int(((t - r) == np.array([0, 0, -4], np.float32)).all(1).sum())
        print(bidirectional, len(a.keypoints), len(b.keypoints), len(r), exact)
        assert exact >= 5 and 2 * exact > len(r)


# ---- the plan header -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("sift3d_feature_plan")
    built = []
    for tag, flags in (("", ("-O2",)), ("_san", ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(out / ("sift3d_feature_plan_check" + tag))
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "opencorr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sift3d_feature_plan_check.cpp"), "-o", exe], check=True, timeout=600)
        built.append(exe)
    return built


def _ask(exe, shape, n_octave_layers=3, units=(1.0, 1.0, 1.0), max_abs=255.0):
    out = subprocess.run([exe, *(repr(a) for a in (*shape, n_octave_layers, *units, max_abs))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    plan = dict(status=int(lines[0].split()[1]), why=lines[0].split(" ", 2)[2] if len(lines[0].split(" ", 2)) > 2 else "", tables=[])
    if plan["status"] == OK:
        plan["exponent"] = int(lines[1].split()[1])
        for line in lines[2:]:
            t = line.split()
            plan["tables"].append(dict(stage=t[1], layer=int(t[2]), half=tuple(int(v) for v in t[4:7]), entries=int(t[8]), outside=int(t[10]), mismatches=int(t[12])))
    return plan


@pytest.mark.parametrize("shape,layers,units", [((18, 33, 40), 3, (1.0, 1.0, 1.0)), ((20, 40, 40), 3, (1.0, 1.0, 2.0)), ((20, 44, 40), 3, (1.0, 0.5, 1.0)),
                                                ((20, 40, 40), 2, (1.0, 2.0, 1.0)), ((76, 78, 80), 4, (1.0, 1.0, 1.0))])
def test_plan_tables_are_the_inline_expression(exes, shape, layers, units):
    """every entry of every table bit for bit, the sentinel exactly where norm > radius, the half-extents cover the sphere"""
    for exe in exes:
        plan = _ask(exe, shape, layers, units)
        assert plan["status"] == OK
        ss = sift3d_twin.scale_space(np.zeros(shape, np.float32), n_octave_layers=layers, min_dimension=8, alpha=0.1, sigma_source=1.15, sigma_base=1.6, units=units)
        n_used = ss.n_octave * layers
        assert len(plan["tables"]) == 2 * n_used
        for t in plan["tables"]:
            assert t["mismatches"] == 0 and 0 < t["outside"] < t["entries"], t
            g = ss.gauss[t["layer"]]
            assert 1 <= t["layer"] % (layers + 3) <= layers
            radius = (4.5 if t["stage"] == "orient" else 10.0 * np.sqrt(2.0)) * float(g.scale)
            for a in range(3):   # (beyond radius / unit no voxel passes the sphere test, whatever :870 lets the loop visit)
                assert t["half"][a] >= int(np.ceil(radius / float(g.units[a]))), (t, a)


def _exponent(max_abs, unit_min):
    """the smallest integer E with 2^E >= 2 A / min(unit), in exact rational arithmetic"""
    from fractions import Fraction
    bound = 2 * Fraction(float(np.float32(max_abs))) / Fraction(float(np.float32(unit_min)))
    e = 0
    while Fraction(2) ** e < bound:
        e += 1
    while Fraction(2) ** (e - 1) >= bound:
        e -= 1
    return e


def test_grid_exponents_of_the_image_domains(exes):
    """8-bit data and the `unit`, `u16` and `pedestal` ranges of tests/image_domains.py, on unit and non-unit voxels"""
    assert set(("unit", "u16", "pedestal")) <= set(image_domains.NAMES)
    for max_abs in (255.0, 256.0, 1.0, 0.999, 65535.0, 255.0 * 1e4 + 3e7, 1e-3, 0.0):
        for units in ((1.0, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 1.0, 2.0), (3.0, 3.0, 3.0)):
            plan = _ask(exes[0], (18, 33, 40), 3, units, max_abs)
            want = 0 if max_abs == 0 else _exponent(max_abs, min(units))
            assert plan["status"] == OK and plan["exponent"] == want, (max_abs, units, plan)
            assert twin.lib().oc_twin_features_grid_exponent(max_abs, min(units)) == want
    assert _exponent(255.0, 1.0) == 9 and _exponent(256.0, 1.0) == 9 and _exponent(1.0, 1.0) == 1 and _exponent(65535.0, 1.0) == 17 and _exponent(255.0, 0.5) == 10


def test_plan_refusals(exes):
    for exe in exes:
        for bad in ("inf", "nan"):
            out = subprocess.run([exe, "18", "33", "40", "3", "1.0", "1.0", "1.0", bad], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and out.stdout.split()[1] == str(ERR_INVALID) and "non-finite" in out.stdout
        assert _ask(exe, (18, 33, 40), max_abs=1e18)["status"] == ERR_UNSUPPORTED          # E = 61
        assert _ask(exe, (18, 33, 40), max_abs=5e17)["exponent"] == 60
        assert _ask(exe, (18, 33, 40), max_abs=1e-19)["status"] == ERR_UNSUPPORTED         # E = -62
        assert _ask(exe, (18, 33, 40), max_abs=1e-18)["exponent"] == -58
        plan = _ask(exe, (18, 33, 40), units=(1.0, 1.0, 0.25))                             # descriptor half-extent 144 on z
        assert plan["status"] == ERR_UNSUPPORTED and "half-extent" in plan["why"]
        plan = _ask(exe, (150, 150, 150), units=(0.5, 0.5, 0.5))                           # 147^3 voxels, every half-extent within 80
        assert plan["status"] == ERR_UNSUPPORTED and "voxels" in plan["why"]
        assert _ask(exe, (40, 40, 40), units=(0.5, 0.5, 0.5))["status"] == OK              # the same window clamped to 38^3


if __name__ == "__main__" and "--measure" in sys.argv:
    for mode in (1, 0):
        worst = dict(sums=0.0, rotation=0.0, descriptor=0.0)
        for name in LISTS:
            d, flipped, n = _distances(name, mode)
            print("mode", mode, name, n, d, flipped)
            worst = {k: max(worst[k], d[k]) for k in worst}
        print("mode", mode, "largest", worst)

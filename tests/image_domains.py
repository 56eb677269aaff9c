"""Intensity domains other than 8-bit speckle, and the queues the domain tests run on them.

TEST INFRASTRUCTURE ONLY (a plain helper: no fixtures, no pytest hooks).  Shared by tests/test_oracle_domains.py (CPU, oracle
alone), tests/test_oracle_vs_ref_domains.py (CPU, oracle against the compiled reference) and tests/test_gpu_domains.py (HIP
engines against the oracle).

Every other parity test feeds the kernels integer grey levels 0 ... 255 on a background of 20.  There every window sum is a sum
of integers below 2^24 (exact however it is associated), the gradient numerator is exact however it is bracketed, and no
interpolated sample comes near zero.  The domains below all derive from ONE 8-bit synth pair and take those three comforts away:

    u16       round(clip(f * 257, 0, 65535))   integer valued, but subset and window sums exceed 2^24: they round
    unit      f / 255                          full 24-bit mantissas, magnitudes <= 1
    pedestal  f * 1e4 + 3e7                    a large common offset: cancellation in every zero-mean step
    dark      clip(img8 - off, 0)              interpolated samples straddle zero: the reference's `< 0` -> -3 rule on its edge
    flat      f, a block set to 77.25          zero norm, NaN ZNCC surface (strict `>` arg-max), singular Hessian
    signed    (f - mean(f)) * 0.0173           negative intensities: ICGN rejects every POI (-3), NR2D1 and IC-LM converge

with f = img8 + 0.37 * N(0, 1) formed in float32, one seeded generator for the reference and another for the target.

----------------------------------------------------------------------------------------------------------------------------------
Measured float bars (regenerate with `python tests/image_domains.py --measure`; CPU only, nothing below comes from GPU output)
----------------------------------------------------------------------------------------------------------------------------------
Machine state: x86-64, g++ -O2 -ffp-contract=off builds of the oracle (oracle/liboc_oracle.so) and of the reference's own sources
(oracle/_ref/liboc_ref.so), NumPy float64 (pocketfft) as the yardstick, the pairs and queues of this file.

FFTCC ZNCC -- FFTCC_DISTANCE[domain][shape class] = max |oracle ZNCC - float64 NumPy restatement of the same window correlation|
over the queues of fftcc_queue2d / fftcc_queue3d (records whose ZNCC is NaN on both sides excluded).  Shape classes and the bars
the 8-bit tests already use for them, GPU against oracle: "2d_square" 1e-5 (tests/test_gpu_parity_2d.py), "2d_rect" 3e-5 (the
rectangular and fuzz cases), "3d" 1e-4.  The GPU bar of a domain is the existing bar where the distance stays below a quarter of
it, else 4 x the distance (icgn_model64.BAR_FACTOR: room for another legitimate association of the same float32 sums, no more).

Float64 model -- MODEL_DISTANCE[domain][family][group] = distance of the COMPILED REFERENCE from tests/icgn_model64.py in the
ordinary run (conv 1e-3; stop 10 for ICGN2D2 at r = (9, 11), stop 20 for ICGN3D1 at r = (5, 6, 4)) over the clean records of both
queues (integer FFTCC guesses and their noisy copy).  The bar is the family's existing ordinary-run bar (icgn_model64.BARS) where
the reference stays within a quarter of it, else 4 x the measured distance.

None of these figures has been measured on a GPU: they are CPU distances that bound what a correct GPU kernel may do.
"""
import numpy as np

NAMES = ("u16", "unit", "pedestal", "dark", "flat", "signed")
ROUNDING = ("u16", "unit", "pedestal")     # the domains on which float32 sums round: an association shows in the bits

SHAPE2D, SEED2D = (160, 176), 5            # h, w: the smallest pair that holds every window and subset below
SHAPE3D, SEED3D = (44, 46, 48), 9          # dz, dy, dx
R2D, R3D = (9, 11), (5, 6, 4)              # solver radii
# `u16` has a mean grey level of 13 086 (2D) / 11 225 (3D): a sum of N of its integers passes 2^24 -- and rounds -- from N = 1 282
# (1 495) on.  The 19 x 23 subset of R2D (437 samples) and the 24 x 24 window stay below: THEIR sums are exact in every
# association, on `u16` as on 8-bit data (`unit` and `pedestal` round at every size).  So `u16` is also run at R_WIDE2D: 41 x 41 =
# 1 681 samples, a 40 x 40 FFTCC window.  In 3D the 12^3 window passes 2^24, the 11 x 13 x 9 subvolume on part of the POIs.
R_WIDE2D = (20, 20)
R_GUESS2D, R_GUESS3D = 12, 6               # FFTCC radii of the solver queues' guesses
CONV, STOP2D, STOP3D = 1e-3, 10, 20
DARK_OFF2D, DARK_OFF3D = 17.5, 17.0
FLAT_VALUE = 77.25
FLAT2D = (slice(40, 100), slice(40, 110))
FLAT3D = (slice(12, 32),) * 3
N_CLEAN2D, N_CLEAN3D = 56, 48              # records in front of the planted ones
N_PLANTED = 4

FFTCC2D_SHAPES = {"2d_square": [(12, 12), (16, 16), (20, 20)], "2d_rect": [(9, 11), (4, 32)]}
FFTCC3D_SHAPES = {"3d": [(6, 6, 6), (5, 6, 4)]}
FFTCC_EXISTING_BAR = {"2d_square": 1e-5, "2d_rect": 3e-5, "3d": 1e-4}

# --- measured tables (see the module docstring) -------------------------------------------------------------------------------
FFTCC_DISTANCE = {
    "u16": {"2d_square": 1.315e-06, "2d_rect": 5.076e-07, "3d": 8.273e-07},
    "unit": {"2d_square": 8.955e-07, "2d_rect": 4.545e-07, "3d": 9.507e-07},
    "pedestal": {"2d_square": 8.939e-07, "2d_rect": 6.838e-07, "3d": 8.543e-07},
    "dark": {"2d_square": 5.853e-06, "2d_rect": 2.674e-06, "3d": 7.453e-06},
    "flat": {"2d_square": 1.354e-05, "2d_rect": 8.670e-06, "3d": 5.944e-06},
    "signed": {"2d_square": 9.534e-07, "2d_rect": 5.609e-07, "3d": 1.139e-06},
}
# records of the reference that used the exception of model_distance (of 112 in 2D2, 96 in 3D).  An engine in another legitimate
# association may use it on MODEL_EXCEPTION_MARGIN records more: the exception exists for POIs whose deciding |dp| sits on the
# criterion, where the last bits of a sum decide -- the reference's own count says how many such POIs a queue holds, and a
# different order of the same sums cannot find many more of them.
MODEL_EXCEPTION_MARGIN = 2
MODEL_EXCEPTIONS = {"u16": {"2D2": 0, "3D": 1}, "unit": {"2D2": 0, "3D": 0}, "pedestal": {"2D2": 1, "3D": 2}}
MODEL_DISTANCE = {
    "u16": {"2D2": {"disp": 3.461e-06, "grad": 9.977e-07, "grad2": 1.559e-07, "conv": 1.376e-05, "zncc": 3.427e-08},
            "3D": {"disp": 2.608e-06, "grad": 9.652e-07, "conv": 2.367e-06, "zncc": 3.091e-08}},
    "unit": {"2D2": {"disp": 3.348e-06, "grad": 1.061e-06, "grad2": 1.429e-07, "conv": 1.039e-05, "zncc": 3.365e-08},
             "3D": {"disp": 3.333e-06, "grad": 1.565e-06, "conv": 2.912e-06, "zncc": 3.029e-08}},
    "pedestal": {"2D2": {"disp": 9.955e-05, "grad": 3.182e-05, "grad2": 7.422e-06, "conv": 1.753e-04, "zncc": 1.703e-07},
                 "3D": {"disp": 5.853e-04, "grad": 1.341e-04, "conv": 1.782e-04, "zncc": 2.793e-07}},
}


def _bar(existing, distance):
    from icgn_model64 import BAR_FACTOR
    return existing if distance <= existing / BAR_FACTOR else BAR_FACTOR * distance


def fftcc_bar(domain, shape_class):
    """The GPU-against-oracle ZNCC bar of a domain.  `dark`, `flat` and `signed` are plain rescalings / clippings of 8-bit data
    (ZNCC is scale free): they are measured like the others."""
    return _bar(FFTCC_EXISTING_BAR[shape_class], FFTCC_DISTANCE[domain][shape_class])


def model_bars(domain, family):
    """{group: bar} of the ordinary run of ICGN2D2 ("2D2") / ICGN3D1 ("3D") against the float64 model on a rounding domain."""
    import icgn_model64 as m64
    out = {}
    for g, d in MODEL_DISTANCE[domain][family].items():
        existing = m64.BARS[family][g][0 if g == "zncc" else m64.ORDINARY]
        out[g] = _bar(existing, d)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------------------
def _domains(ref8, tar8, seed, dark_off, flat):
    out = {}
    fs = []
    for k, img8 in enumerate((ref8, tar8)):
        rng = np.random.default_rng([seed, k])
        img8 = np.ascontiguousarray(img8, dtype=np.float32)
        fs.append(img8 + np.float32(0.37) * rng.standard_normal(img8.shape, dtype=np.float32))
    f32 = np.float32

    def both(fn):
        return tuple(np.ascontiguousarray(fn(a), dtype=np.float32) for a in fs)

    out["u16"] = both(lambda f: np.round(np.clip(f * f32(257.0), f32(0.0), f32(65535.0))))
    out["unit"] = both(lambda f: f / f32(255.0))
    out["pedestal"] = both(lambda f: f * f32(1e4) + f32(3e7))
    out["dark"] = tuple(np.ascontiguousarray(np.clip(np.asarray(a, dtype=np.float32) - f32(dark_off), f32(0.0), None), dtype=np.float32)
                        for a in (ref8, tar8))

    def flatten(f):
        g = f.copy()
        g[flat] = f32(FLAT_VALUE)
        return g
    out["flat"] = both(flatten)
    out["signed"] = both(lambda f: (f - f32(f.mean(dtype=np.float64))) * f32(0.0173))
    for a, b in out.values():
        assert a.dtype == np.float32 and b.dtype == np.float32 and a.flags.c_contiguous and b.flags.c_contiguous
    return out


def domains2d(ref8, tar8, seed=SEED2D):
    """name -> (ref, tar), contiguous float32, from one 8-bit pair."""
    return _domains(ref8, tar8, seed, DARK_OFF2D, FLAT2D)


def domains3d(ref8, tar8, seed=SEED3D):
    return _domains(ref8, tar8, seed, DARK_OFF3D, FLAT3D)


_cache = {}


def pair2d():
    if "p2" not in _cache:
        from opencorr_amd import synth
        _cache["p2"] = synth.speckle_pair_2d(*SHAPE2D, seed=SEED2D)
    return _cache["p2"]


def pair3d():
    if "p3" not in _cache:
        from opencorr_amd import synth
        _cache["p3"] = synth.speckle_pair_3d(*SHAPE3D, seed=SEED3D)
    return _cache["p3"]


def images2d(name):
    """(ref, tar) of a domain: computed once per process, shared, never written to."""
    if "d2" not in _cache:
        _cache["d2"] = domains2d(*pair2d())
        for a, b in _cache["d2"].values():
            a.flags.writeable = b.flags.writeable = False
    return _cache["d2"][name]


def images3d(name):
    if "d3" not in _cache:
        _cache["d3"] = domains3d(*pair3d())
        for a, b in _cache["d3"].values():
            a.flags.writeable = b.flags.writeable = False
    return _cache["d3"][name]


# ---------------------------------------------------------------------------------------------------------------------------------
# queues
# ---------------------------------------------------------------------------------------------------------------------------------
def grid2d(margin=16):
    """The 8 x 7 POI grid inside `margin`."""
    from opencorr_amd import synth
    return synth.poi_grid_2d(SHAPE2D[0], SHAPE2D[1], 8, 7, margin)


def grid3d(margin=10):
    """The 4 x 4 x 3 POI grid inside `margin`."""
    from opencorr_amd import synth
    return synth.poi_grid_3d(*SHAPE3D, 4, 4, 3, margin)


def solver_queues2d(ref, tar):
    """(integer queue, noisy queue) for the 2D solvers at R2D.  Records [:N_CLEAN2D]: the grid with the oracle's FFTCC2D guesses
    (r = 12) -- integer translations with zero gradients, the value-plane path of icgn2d.hip -- resp. the same guesses with
    N(0, 0.3) on u, v and N(0, 0.01) on the four gradients.  Behind them, in both: a NaN guess, a record rejected with zncc = -1,
    a far-off guess, and a POI on the guard's border (x = rx exactly) with a good guess."""
    import oracle
    P = oracle.P2
    xs, ys = grid2d()
    pois = oracle.make_pois2d(xs, ys)
    oracle.fftcc2d(ref, tar, R_GUESS2D, R_GUESS2D, pois)
    assert len(pois) == N_CLEAN2D
    e = oracle.make_pois2d([122.0, 122.0, 122.0, float(R2D[0])], [120.0, 120.0, 120.0, 90.0])
    e[:, P["u"]], e[:, P["v"]] = 2.0, -2.0
    e[0, P["u"]] = np.nan
    e[1, P["zncc"]] = -1.0
    e[2, P["u"]] += 9.0
    rng = np.random.default_rng(6501)
    noisy = pois.copy()
    for k in ("u", "v"):
        noisy[:, P[k]] += rng.normal(0, 0.3, len(noisy)).astype(np.float32)
    for k in ("ux", "uy", "vx", "vy"):
        noisy[:, P[k]] = rng.normal(0, 0.01, len(noisy)).astype(np.float32)
    return (np.ascontiguousarray(np.concatenate([pois, e]), dtype=np.float32),
            np.ascontiguousarray(np.concatenate([noisy, e]), dtype=np.float32))


def solver_queues3d(ref, tar):
    """(integer queue, noisy queue) for ICGN3D1 at R3D: the grid with the oracle's FFTCC3D guesses (r = 6), resp. N(0, 0.3) on
    u, v, w; behind them a NaN guess, a rejected record (zncc = -1), a far-off guess and a POI on the guard's border."""
    import oracle
    P = oracle.P3
    xs, ys, zs = grid3d()
    pois = oracle.make_pois3d(xs, ys, zs)
    oracle.fftcc3d(ref, tar, R_GUESS3D, R_GUESS3D, R_GUESS3D, pois)
    assert len(pois) == N_CLEAN3D
    e = oracle.make_pois3d([34.0, 34.0, 34.0, float(R3D[0])], [33.0, 33.0, 33.0, 24.0], [34.0, 34.0, 34.0, 22.0])
    e[:, P["u"]], e[:, P["v"]], e[:, P["w"]] = 2.0, -2.0, 1.0
    e[0, P["w"]] = np.nan
    e[1, P["zncc"]] = -1.0
    e[2, P["u"]] += 6.0
    rng = np.random.default_rng(6502)
    noisy = pois.copy()
    for k in ("u", "v", "w"):
        noisy[:, P[k]] += rng.normal(0, 0.3, len(noisy)).astype(np.float32)
    return (np.ascontiguousarray(np.concatenate([pois, e]), dtype=np.float32),
            np.ascontiguousarray(np.concatenate([noisy, e]), dtype=np.float32))


def wide_queue2d(ref, tar):
    """A 6 x 5 grid inside 26 with the oracle's FFTCC2D guesses at R_WIDE2D, for the solvers at R_WIDE2D."""
    import oracle
    from opencorr_amd import synth
    xs, ys = synth.poi_grid_2d(SHAPE2D[0], SHAPE2D[1], 6, 5, 26)
    pois = oracle.make_pois2d(xs, ys)
    oracle.fftcc2d(ref, tar, R_WIDE2D[0], R_WIDE2D[1], pois)
    return pois


def center_offsets2d(n):
    rng = np.random.default_rng(6503)
    off = rng.uniform(-2.5, 2.5, (n, 2)).astype(np.float32)
    off[::4] = np.round(off[::4])
    return off


def self_adaptive_radii2d(n):
    rng = np.random.default_rng(6504)
    return np.stack([rng.integers(4, R2D[0] + 1, n), rng.integers(4, R2D[1] + 1, n)], 1).astype(np.float32)


def fftcc_queue2d(rx, ry):
    """The 8 x 7 grid inside max(rx, ry) + 4 with guesses that displace the target window -- none on a quarter, integers on a
    half, fractions (the reference truncates, src/oc_fftcc.cpp:190-216) on the rest --, then two POIs the guard rejects and one
    whose guess puts the target window outside (all three stay untouched)."""
    import oracle
    P = oracle.P2
    xs, ys = grid2d(max(rx, ry) + 4)
    pois = oracle.make_pois2d(np.concatenate([xs, [2.0, SHAPE2D[1] - 2.0, 88.0]]), np.concatenate([ys, [80.0, 80.0, 80.0]]))
    rng = np.random.default_rng(6505 + 100 * rx + ry)
    n = len(xs)
    g = rng.integers(-2, 3, (n, 2)).astype(np.float32)
    g[: n // 4] = 0.0
    g[3 * n // 4:] = rng.uniform(-3, 3, (n - 3 * n // 4, 2)).astype(np.float32)
    pois[:n, P["u"]], pois[:n, P["v"]] = g[:, 0], g[:, 1]
    pois[-1, P["u"]] = 500.0
    return np.ascontiguousarray(pois, dtype=np.float32)


def fftcc_queue3d():
    """The 4 x 4 x 3 grid inside 10 with integer and fractional guesses, for r = 6 and (5, 6, 4); at r = 16 most of its windows
    are clamped at a face of the 44 x 46 x 48 volumes."""
    import oracle
    P = oracle.P3
    xs, ys, zs = grid3d()
    pois = oracle.make_pois3d(xs, ys, zs)
    rng = np.random.default_rng(6506)
    n = len(xs)
    g = rng.integers(-2, 3, (n, 3)).astype(np.float32)
    g[: n // 4] = 0.0
    g[3 * n // 4:] = rng.uniform(-2.5, 2.5, (n - 3 * n // 4, 3)).astype(np.float32)
    for a, k in enumerate(("u", "v", "w")):
        pois[:, P[k]] = g[:, a]
    return np.ascontiguousarray(pois, dtype=np.float32)


# `flat`, planted on the block's border.  A constant window matters in two ways: when BOTH windows are constant the packed transform
# of zeros is zero by itself; when exactly ONE is, the kernels' `norm == 0` branch (oc_device.h) decides.  The grid queues above
# meet the second case by chance or not at all, so these queues plant it, in both directions and along two axes.  A window
# [c - r, c + r) is top-aligned in the block (c = end - r): moving it by +3 leaves the block.
FLAT_BORDER_KINDS = ("both", "ref", "tar", "ref", "tar")     # which window of each planted record is constant


def _border(c_fast, c_slow, step=3):
    """(centres, guesses) along the fastest and the slowest axis: both constant; reference constant / target pushed out; target
    pulled in / reference out; and the last two again along the slow axis."""
    cf = [c_fast, c_fast, c_fast + step, c_fast, c_fast]
    cs = [c_slow, c_slow, c_slow, c_slow, c_slow + step]
    gf = [0.0, step, -step, 0.0, 0.0]
    gs = [0.0, 0.0, 0.0, step, -step]
    return cf, cs, gf, gs


def flat_border_queue2d(rx, ry):
    """Five records on the border of FLAT2D (FLAT_BORDER_KINDS) for a (rx, ry) window that fits the 70 x 60 block, then one the
    guard rejects.  (4, 32) does not fit -- its window is 64 rows tall -- so the rectangular kernel is asked at (32, 4)."""
    import oracle
    P = oracle.P2
    assert 2 * rx + 3 <= 70 and 2 * ry + 3 <= 60
    xs, ys, gu, gv = _border(FLAT2D[1].stop - rx, FLAT2D[0].stop - ry)
    pois = oracle.make_pois2d(xs + [2.0], ys + [80.0])
    pois[:5, P["u"]], pois[:5, P["v"]] = gu, gv
    return np.ascontiguousarray(pois, dtype=np.float32)


FLAT_WIDE3D = (slice(4, 40),) * 3          # a 36^3 box: the 20^3 one of `flat` holds no 28^3 or 32^3 window


def flat_wide3d():
    """The `flat` pair with the box widened to FLAT_WIDE3D, for the FFTCC3D kernels of large cubic windows (r = 14: plane-wise,
    r = 16: register kernel).  Computed once, shared, never written to."""
    if "fw3" not in _cache:
        out = []
        for a in images3d("flat"):
            g = a.copy()
            g[FLAT_WIDE3D] = np.float32(FLAT_VALUE)
            g.flags.writeable = False
            out.append(g)
        _cache["fw3"] = tuple(out)
    return _cache["fw3"]


def flat_border_queue3d(r, box=FLAT3D):
    """Five records on the border of the flat box (FLAT_BORDER_KINDS; x and z are the axes moved) for radii r = (rx, ry, rz).  Every
    window, moved or not, lies inside both volumes."""
    import oracle
    P = oracle.P3
    xs, zs, gu, gw = _border(box[2].stop - r[0], box[0].stop - r[2])
    pois = oracle.make_pois3d(xs, [float(box[1].stop - r[1])] * 5, zs)
    pois[:, P["u"]], pois[:, P["w"]] = gu, gw
    for c, g, rr, d in ((xs, gu, r[0], SHAPE3D[2]), (zs, gw, r[2], SHAPE3D[0])):
        assert all(ci + min(gi, 0) - rr >= 0 and ci + max(gi, 0) + rr - 1 <= d - 1 for ci, gi in zip(c, g))
    return np.ascontiguousarray(pois, dtype=np.float32)


def constant_windows(ref, tar, r, pois):
    """(reference window constant, target window constant) per record, from the pixels: the window of a POI at c with guess g
    is [trunc(c) - r, trunc(c) + r) in the reference and the same moved by trunc(g) in the target (src/oc_fftcc.cpp:190-216)."""
    nd = ref.ndim
    r = tuple(r)
    out = np.zeros((len(pois), 2), bool)
    for i, p in enumerate(pois):
        c = [int(p[a]) for a in range(nd)]
        g = [int(p[nd + 4 * a]) for a in range(nd)] if nd == 3 else [int(p[2]), int(p[8])]
        for k, (img, move) in enumerate(((ref, [0] * nd), (tar, g))):
            sl = tuple(slice(c[a] + move[a] - r[a], c[a] + move[a] + r[a]) for a in reversed(range(nd)))
            w = img[sl]
            assert w.shape == tuple(2 * x for x in reversed(r))
            out[i, k] = bool((w == w.flat[0]).all())
    return out[:, 0], out[:, 1]


def check_flat_border(solved, ref_const, tar_const, zcol):
    """The planted records are what FLAT_BORDER_KINDS says -- at least one with both windows constant and, in each direction, one
    with exactly one -- and each of them carries a NaN ZNCC."""
    want = {"both": (True, True), "ref": (True, False), "tar": (False, True)}
    for i, kind in enumerate(FLAT_BORDER_KINDS):
        assert (bool(ref_const[i]), bool(tar_const[i])) == want[kind], (i, kind, bool(ref_const[i]), bool(tar_const[i]))
    assert (ref_const & tar_const).sum() >= 1 and (ref_const & ~tar_const).sum() >= 1 and (~ref_const & tar_const).sum() >= 1
    assert np.isnan(solved[:5, zcol]).all(), solved[:5, zcol].tolist()


def inner16(pois):
    """Records of a 3D queue whose 32^3 windows lie inside both volumes (the rule of
    tests/test_gpu_fuzz.py::test_fuzz_fftcc3d_32_cubed_windows_anywhere)."""
    import oracle
    P = oracle.P3
    dz, dy, dx = SHAPE3D
    inner = np.ones(len(pois), bool)
    for axis, d in (("x", dx), ("y", dy), ("z", dz)):
        c = pois[:, P[axis]]
        g = pois[:, P[{"x": "u", "y": "v", "z": "w"}[axis]]]
        for lo in (c - 16, c - 16 + g):
            inner &= (np.trunc(lo) >= 0) & (np.trunc(lo + 31) <= d - 1) & (lo >= 0)
    return inner


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle on a domain (prepared fields computed once per process)
# ---------------------------------------------------------------------------------------------------------------------------------
SOLVERS2D = ("icgn2d1", "icgn2d2", "iclm2d1", "iclm2d2", "nr2d1")


def prepared2d(name):
    """(oracle.Prepared2D, oracle.PreparedNR2D) of a domain."""
    import oracle
    key = ("prep2", name)
    if key not in _cache:
        ref, tar = images2d(name)
        _cache[key] = (oracle.Prepared2D(ref, tar), oracle.PreparedNR2D(ref, tar))
    return _cache[key]


def prepared3d(name):
    import oracle
    key = ("prep3", name)
    if key not in _cache:
        _cache[key] = oracle.Prepared3D(*images3d(name))
    return _cache[key]


def queues2d(name):
    key = ("q2", name)
    if key not in _cache:
        _cache[key] = solver_queues2d(*images2d(name))
    return tuple(q.copy() for q in _cache[key])


def queues3d(name):
    key = ("q3", name)
    if key not in _cache:
        _cache[key] = solver_queues3d(*images3d(name))
    return tuple(q.copy() for q in _cache[key])


def oracle2d(name, solver, q, order, center_offsets=None, self_adaptive=False, r=None):
    """A copy of `q` solved by the oracle's `solver` at R2D (or `r`), CONV, STOP2D in summation order `order` (64 lanes)."""
    import oracle
    rx, ry = r or R2D
    prep, prep_nr = prepared2d(name)
    out = np.ascontiguousarray(q, dtype=np.float32).copy()
    if solver == "nr2d1":
        oracle.nr2d1(prep_nr, rx, ry, CONV, STOP2D, out, order=order, lanes=64)
    elif solver.startswith("iclm"):
        getattr(oracle, solver)(prep, rx, ry, CONV, STOP2D, out, order=order, lanes=64)
    else:
        getattr(oracle, solver)(prep, rx, ry, CONV, STOP2D, out, order=order, lanes=64, center_offsets=center_offsets,
                                self_adaptive=self_adaptive)
    return out


def oracle3d(name, q, order, lanes=256):
    import oracle
    out = np.ascontiguousarray(q, dtype=np.float32).copy()
    oracle.icgn3d1(prepared3d(name), R3D[0], R3D[1], R3D[2], CONV, STOP3D, out, order=order, lanes=lanes)
    return out


def with_radii(q):
    """A copy of a 2D queue with per-POI subset radii (setSelfAdaptive)."""
    out = q.copy()
    out[:, 23:25] = self_adaptive_radii2d(len(q))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Element-wise identity as in tests/test_gpu_fuzz.py::_same: the same bits, or NaN on both sides (the sign of a default NaN
    is the machine's: negative on x86, positive on gfx950)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, what=""):
    ok = same(got, want)
    bad = np.argwhere(~ok)
    assert bad.size == 0, (what, "%d floats differ; first (record, field): %s" % (len(bad), bad[:8].tolist()),
                           [(float(np.asarray(got)[i, j]), float(np.asarray(want)[i, j])) for i, j in bad[:4]])


def zncc_distance(got, want, col):
    """max |got - want| of the ZNCC column over the records where it is a number on the `want` side; NaN must meet NaN."""
    g, w = got[:, col].astype(np.float64), want[:, col].astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)), ("NaN ZNCC at", np.flatnonzero(np.isnan(g) != np.isnan(w))[:8].tolist())
    ok = ~np.isnan(w)
    return float(np.abs(g[ok] - w[ok]).max()) if ok.any() else 0.0


def check_fftcc(got, want, P, keys, bar, what=""):
    """The FFTCC bar: integers identical (records with NaN ZNCC included), ZNCC NaN on the same records and within `bar`
    elsewhere, every other field untouched.  Returns the ZNCC distance."""
    for k in keys:
        assert np.array_equal(got[:, P[k]], want[:, P[k]]), (what, k, np.flatnonzero(got[:, P[k]] != want[:, P[k]])[:8].tolist())
    d = zncc_distance(got, want, P["zncc"])
    assert d <= bar, (what, "ZNCC distance %.3e beyond the bar %.3e" % (d, bar))
    rest = [c for c in range(got.shape[1]) if c not in [P[k] for k in keys] + [P["zncc"]]]
    assert_same(got[:, rest], want[:, rest], (what, "untouched fields"))
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# the conditions that keep a domain from passing emptily (asserted on the reference's result, on the oracle's, and -- through
# the oracle -- on the GPU box)
# ---------------------------------------------------------------------------------------------------------------------------------
def _codes(p, zcol):
    z = p[:, zcol]
    return np.where(z < 0, z, np.float32(0))


def check_converges(name, solved, zcol, n_clean, what=""):
    """`u16`, `unit`, `pedestal` (and NR2D1 / IC-LM on `signed`): at least 80 % of the clean POIs converge."""
    share = float((solved[:n_clean, zcol] > 0.5).mean())
    assert share >= 0.8, (name, what, share)


def check_dark(solved, zcol, n_clean, what=""):
    """`dark`: the share of -3 among the clean POIs lies between 5 % and 90 %: the rule decides, in both directions."""
    share = float((solved[:n_clean, zcol] == -3).mean())
    assert 0.05 <= share <= 0.9, (what, share)


def check_flat(fftcc_solved, icgn_solved):
    """`flat`: at least 5 FFTCC2D records with NaN ZNCC, at least 10 negative ICGN2D1 records."""
    import oracle
    z = oracle.P2["zncc"]
    assert int(np.isnan(fftcc_solved[:, z]).sum()) >= 5, int(np.isnan(fftcc_solved[:, z]).sum())
    assert int((icgn_solved[:, z] < 0).sum()) >= 10, int((icgn_solved[:, z] < 0).sum())


def check_signed_rejected(solved, zcol, n_clean, what=""):
    """`signed`: every clean ICGN record is -3."""
    assert (solved[:n_clean, zcol] == -3).all(), (what, solved[:n_clean, zcol].tolist())


def check_orders_differ(seq, lanes, n_clean, what=""):
    """The rounding domains: ORDER_SEQ and ORDER_LANES differ in at least one bit on most clean POIs -- the domain can see an
    association."""
    differ = (bits(seq[:n_clean]) != bits(lanes[:n_clean])).any(axis=1)
    assert differ.mean() > 0.5, (what, float(differ.mean()))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatements of the window correlation (the FFTCC yardstick) and the measurement of the tables above
# ---------------------------------------------------------------------------------------------------------------------------------
def fftcc2d_zncc64(ref, tar, rx, ry, poi):
    """ZNCC at the peak of one POI's window correlation in float64 (tests/test_oracle_fftcc_numpy.py::fftcc2d_numpy)."""
    from test_oracle_fftcc_numpy import fftcc2d_numpy
    with np.errstate(invalid="ignore", divide="ignore"):
        return fftcc2d_numpy(ref, tar, rx, ry, poi[0], poi[1], poi[2], poi[8])[2]


def fftcc3d_zncc64(ref, tar, r, poi):
    """The same in 3D for radii (rx, ry, rz): the window's floats, filled x-fastest, are transformed as an array
    [2rx][2ry][2rz] (tests/test_oracle_vs_ref.py::test_fftcc3d_against_reference); the peak HEIGHT over the norms needs no
    decoding of its position."""
    f32 = np.float32
    idx, tdx = [], []
    for c, rr, g in zip(poi[0:3], r, (poi[3], poi[7], poi[11])):
        base = f32(c) + np.arange(2 * rr, dtype=np.float32) - f32(rr)
        idx.append(base.astype(np.int64))
        tdx.append((base + f32(g)).astype(np.int64))
    rwin = ref[np.ix_(idx[2], idx[1], idx[0])].astype(np.float64)
    twin = tar[np.ix_(tdx[2], tdx[1], tdx[0])].astype(np.float64)
    rwin -= rwin.mean()
    twin -= twin.mean()
    a = rwin.reshape(-1).reshape(2 * r[0], 2 * r[1], 2 * r[2])
    b = twin.reshape(-1).reshape(2 * r[0], 2 * r[1], 2 * r[2])
    surf = np.fft.irfftn(np.conj(np.fft.rfftn(a)) * np.fft.rfftn(b), s=a.shape, axes=(0, 1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        return surf.max() / np.sqrt((rwin ** 2).sum() * (twin ** 2).sum())


def measure_fftcc(only=None):
    """FFTCC_DISTANCE (of one domain: `only`), from the oracle and NumPy alone."""
    import oracle
    out = {}
    for name in NAMES if only is None else (only,):
        out[name] = {}
        ref, tar = images2d(name)
        for cls, shapes in FFTCC2D_SHAPES.items():
            worst = 0.0
            for rx, ry in shapes:
                q = fftcc_queue2d(rx, ry)
                got = q.copy()
                oracle.fftcc2d(ref, tar, rx, ry, got)
                for i in range(len(q) - 3):
                    z64 = fftcc2d_zncc64(ref, tar, rx, ry, q[i])
                    z32 = got[i, oracle.P2["zncc"]]
                    if not (np.isnan(z64) or np.isnan(z32)):
                        worst = max(worst, abs(float(z32) - z64))
            out[name][cls] = worst
        ref, tar = images3d(name)
        worst = 0.0
        for r in FFTCC3D_SHAPES["3d"]:
            q = fftcc_queue3d()
            got = q.copy()
            oracle.fftcc3d(ref, tar, r[0], r[1], r[2], got)
            for i in range(len(q)):
                z64 = fftcc3d_zncc64(ref, tar, r, q[i])
                z32 = got[i, oracle.P3["zncc"]]
                if not (np.isnan(z64) or np.isnan(z32)):
                    worst = max(worst, abs(float(z32) - z64))
        out[name]["3d"] = worst
    return out


def model_case(name, family):
    """(radii, ref, tar, prep, clean records of both queues, model records, model |dp| lists) of the ordinary run on a domain."""
    import oracle
    import icgn_model64 as m64
    key = ("model", name, family)
    if key not in _cache:
        if family == "2D2":
            ref, tar = images2d(name)
            qi, qn = solver_queues2d(ref, tar)
            pois = np.ascontiguousarray(np.concatenate([qi[:N_CLEAN2D], qn[:N_CLEAN2D]]))
            prep = oracle.Prepared2D(ref, tar)
            model, norms = m64.icgn2d2(m64.Fields2D(prep), R2D[0], R2D[1], CONV, STOP2D, pois)
            _cache[key] = (R2D, ref, tar, prep, pois, model, norms)
        else:
            ref, tar = images3d(name)
            qi, qn = solver_queues3d(ref, tar)
            pois = np.ascontiguousarray(np.concatenate([qi[:N_CLEAN3D], qn[:N_CLEAN3D]]))
            prep = oracle.Prepared3D(ref, tar)
            model, norms = m64.icgn3d1(m64.Fields3D(prep), R3D[0], R3D[1], R3D[2], CONV, STOP3D, pois)
            _cache[key] = (R3D, ref, tar, prep, pois, model, norms)
    return _cache[key]


def model_distance(name, family, got, exception_bar=None):
    """(records that used an exception, {group: distance}) of `got` -- the records some engine made of model_case(name, family)'s
    queue -- from the float64 model in the ordinary run.  Flags and iteration counts are asserted by
    icgn_model64.compare_ordinary, with its one exception stated for both exits of the loop: a POI whose MODEL |dp| at the deciding
    iteration lies within the domain's convergence bar of the criterion may stop one iteration apart from the model, or -- when
    that iteration is the last one the stop condition allows -- carry -4 on one side and a result on the other (the same
    comparison `|dp| >= conv`, src/oc_icgn.cpp:857 and :886-889).  Such records leave the distances.  `exception_bar`: the
    convergence bar to judge with (default: the domain's own, model_bars)."""
    import icgn_model64 as m64
    _, _, _, _, _, model, norms = model_case(name, family)
    ndim, P, stop = (3, m64.P3, STOP3D) if family == "3D" else (2, m64.P2, STOP2D)
    if exception_bar is None:
        exception_bar = model_bars(name, family)["conv"]
    conv = float(np.float32(CONV))
    g = np.asarray(got, dtype=np.float64)
    it_g, it_m, z_g, z_m = g[:, P["iteration"]], model[:, P["iteration"]], g[:, P["zncc"]], model[:, P["zncc"]]
    keep = np.ones(len(g), bool)
    for i in range(len(g)):
        k = int(min(it_g[i], it_m[i]))
        one_off = abs(it_g[i] - it_m[i]) == 1
        at_stop = it_g[i] == it_m[i] == stop and ((z_g[i] == -4) != (z_m[i] == -4)) and z_g[i] != -3 and z_m[i] != -3
        # a record that stops one iteration apart carries a result on both sides, or -4 on the side that ran into the stop condition
        if one_off and not (z_g[i] >= 0 and z_m[i] >= 0):
            late_g = it_g[i] > it_m[i]
            one_off = max(it_g[i], it_m[i]) == stop and (z_g[i] if late_g else z_m[i]) == -4 and (z_m[i] if late_g else z_g[i]) >= 0
        if (one_off or at_stop) and k >= 1:
            bar = max(exception_bar, m64.BARS[family]["conv"][min(k, 5) - 1])
            if abs(norms[i][k - 1] - conv) <= bar:
                keep[i] = False
    used, dist = m64.compare_ordinary(ndim, family, g[keep], model[keep], [norms[i] for i in np.flatnonzero(keep)], CONV)
    return used + int((~keep).sum()), dist


def reference_model_run(name, family):
    """The compiled reference on model_case's queue."""
    from oracle import ref as oref
    r, ref, tar, _, pois, _, _ = model_case(name, family)
    got = pois.copy()
    if family == "2D2":
        oref.solve2d(oref.ICGN2D2, ref, tar, r[0], r[1], CONV, STOP2D, got)
    else:
        oref.icgn3d1(ref, tar, r[0], r[1], r[2], CONV, STOP3D, got)
    return got


def measure_model():
    """MODEL_DISTANCE and the exceptions used, from the compiled reference and the model alone."""
    out, exc = {}, {}
    for name in ROUNDING:
        out[name], exc[name] = {}, {}
        for family in ("2D2", "3D"):
            used, dist = model_distance(name, family, reference_model_run(name, family), exception_bar=float("inf"))
            out[name][family] = dist
            exc[name][family] = used
    return out, exc


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, ".."))
    sys.path.insert(0, here)
    if "--measure" in sys.argv:
        d = measure_fftcc()
        print("FFTCC_DISTANCE = {")
        for name, row in d.items():
            print('    "%s": {%s},' % (name, ", ".join('"%s": %.3e' % kv for kv in row.items())))
        print("}")
        for name, row in d.items():
            print("#   %-9s %s" % (name, "  ".join("%s bar %.1e" % (c, _bar(FFTCC_EXISTING_BAR[c], v)) for c, v in row.items())))
        from oracle import ref as oref
        if oref.available():
            m, exc = measure_model()
            print("MODEL_DISTANCE = {")
            for name, fams in m.items():
                print('    "%s": {%s},' % (name, ", ".join('"%s": {%s}' % (f, ", ".join('"%s": %.3e' % kv for kv in g.items()))
                                                          for f, g in fams.items())))
            print("}\n# one-iteration exceptions used by the reference:", exc)

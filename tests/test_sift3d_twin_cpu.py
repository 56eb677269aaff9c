"""The CPU twin of SIFT3D's scale space (tests/cpp/sift3d_twin.cpp: float32, the reference's loops) against the float64 model
(tests/sift3d_model.py).  CPU only.  The reference's own source does not compile against the stand-in headers of the oracle and
ships no table for SIFT3D's internals, so there is no compiled-reference pin for this stage: the twin read against the cited
lines, this model and the planted slips are the pin.

BAR on every Gaussian and DoG voxel: 4 x the twin-to-model distance measured on the cases of tests/sift3d_cases.py
(DISTANCE, the largest |twin - model| over all layers, cases and both arithmetic modes; volumes 0 ... 255).  Candidate lists must
be identical to the model's.  Every planted slip must change a candidate list or exceed the bar by more than 10 x.
"""
import functools

import numpy as np
import pytest

import sift3d_cases as cases
import sift3d_model as model
import sift3d_twin as twin

DISTANCE = 2.131e-4   # measured: units_112 (radius 16 on x and y), Gaussian layers, separate rounding; 1.0e-4 with every radius <= 8
BAR = 4 * DISTANCE


def _list(candidates):
    return [tuple(int(c[f]) for f in ("x", "y", "z", "octave", "layer")) for c in candidates]


def _distance(result, gauss, dog):
    d = 0.0
    for got, want in list(zip(result.gauss, gauss)) + list(zip(result.dog, dog)):
        assert got.vol.shape == want.vol.shape
        d = max(d, float(np.abs(got.vol.astype(np.float64) - want.vol).max()))
    return d


@functools.lru_cache(maxsize=None)
def _model(name):
    c = cases.CASE_BY_NAME[name]
    return model.scale_space(c.volume(), **c.settings)


@pytest.mark.parametrize("fma", (0, 1))
@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_twin_equals_model(case, fma):
    n_octave, gauss, dog, candidates = _model(case.name)
    got = twin.scale_space(case.volume(), fma=fma, **case.settings)
    assert got.n_octave == n_octave and len(got.gauss) == len(gauss) and len(got.dog) == len(dog)
    d = _distance(got, gauss, dog)
    print("%s fma=%d: twin-to-model distance %.4g (bar %.4g), %d candidates" % (case.name, fma, d, BAR, len(candidates)))
    assert d <= BAR
    for g, w in zip(got.dog, dog):
        assert abs(float(g.max_abs) - w.max_abs) <= BAR
    assert _list(got.candidates) == candidates and len(candidates) >= 1
    for c in got.candidates:                                               # scale: the DoG layer's (src/oc_sift.cpp:838)
        assert c["scale"] == got.dog[c["octave"] * (case.settings["n_octave_layers"] + 2) + c["layer"]].scale


def test_enough_candidates_over_all_cases():
    assert sum(len(_model(c.name)[3]) for c in cases.CASES) >= 30


@pytest.mark.parametrize("kind", cases.PLANTED)
def test_planted_ties_give_no_candidate(kind):
    """a constant volume, and volumes constant along one axis: every layer ties along it, and a tie is no extremum"""
    v = cases.planted(kind)
    got = twin.scale_space(v, alpha=0.0)
    assert len(got.candidates) == 0 and model.scale_space(v, alpha=0.0)[3] == []
    axis = {"along_z": 0, "along_y": 1, "along_x": 2}.get(kind)
    for layer in got.gauss + got.dog:
        if axis is None:
            assert np.all(layer.vol == layer.vol.flat[0])
        else:
            assert np.all(layer.vol == np.take(layer.vol, [0], axis=axis))


def _blob():
    """one bright blob: its centre is the largest |DoG| of its layer and a strict extremum, so with alpha = 1 it is the one candidate"""
    z, y, x = np.mgrid[0:18, 0:33, 0:40]
    return np.round(200 * np.exp(-((z - 9) ** 2 + (y - 16) ** 2 + (x - 20) ** 2) / (2 * 2.5 * 2.5))).astype(np.float32)


def _near_ties():
    """240 + k / 64, k = 0 ... 16: DoG values four orders below the voxels, so that neighbours differ by a few float32 steps of
    the sums.  A float64 model cannot see a summation order by size (either order is inside the bar); it sees it where the wrong
    order decides a near-tie differently.  The seed is one where the right order agrees with the model on every comparison."""
    rng = np.random.default_rng(12)
    return (240 + np.round(rng.random((12, 20, 24)) * 16) * (0.25 / 16)).astype(np.float32)


# slip -> (volume, settings) of a case that shows it
SLIP_CASES = {
    twin.SLIP_NOT_STRICT: lambda: (cases.planted("along_x"), dict(alpha=0.0)),
    twin.SLIP_NO_SCALE_NEIGHBOURS: lambda: (cases.CASES[0].volume(), cases.CASES[0].settings),
    twin.SLIP_BORDER_0: lambda: (cases.CASES[0].volume(), cases.CASES[0].settings),
    twin.SLIP_REFLECTION: lambda: (cases.CASES[0].volume(), cases.CASES[0].settings),
    twin.SLIP_DESCENDING: lambda: (_near_ties(), dict(alpha=0.0)),
    twin.SLIP_THRESHOLD: lambda: (_blob(), dict(alpha=1.0)),
}


@pytest.mark.parametrize("which", twin.SLIPS)
def test_model_catches_every_planted_slip(which):
    volume, settings = SLIP_CASES[which]()
    n_octave, gauss, dog, candidates = model.scale_space(volume, **settings)
    right = twin.scale_space(volume, **settings)
    assert _list(right.candidates) == candidates and _distance(right, gauss, dog) <= BAR    # the case itself is sound ...
    if which in (twin.SLIP_THRESHOLD, twin.SLIP_DESCENDING):
        assert len(candidates) >= 1
    with twin.slip(which):
        wrong = twin.scale_space(volume, **settings)
    d = _distance(wrong, gauss, dog)
    print("slip %d: %d candidates against %d, distance %.4g = %.1f x bar" % (which, len(wrong.candidates), len(candidates), d, d / BAR))
    assert _list(wrong.candidates) != candidates or d > 10 * BAR                             # ... and the slip shows
    if which == twin.SLIP_REFLECTION:
        assert d > 10 * BAR

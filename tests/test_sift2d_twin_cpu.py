"""The float32 twin of SIFT2D's detector (tests/cpp/sift2d_twin.cpp) against the float64 model (tests/sift2d_model.py), CPU only.

Layers, the bound of the issue.  A blur pass forms, per pixel, w[0] s[c] + sum_r w[r] (s[lo] + s[hi]): R + 1 products, R pair sums and R
accumulations.  With u = 2^-24 and every operand bounded by max|I| (the weights are positive and sum to 1 within (R + 1) u), the
running-error bound gives |fl(sum) - sum| <= (R + 2) u max|I|: each term takes part in its pair sum, its product and the accumulations
after it, weighted by its own w[r], and the weights sum to 1.  The model uses the twin's float32 weights as they are, so the weights
add nothing.  A pass does not amplify what its input carries (the weights sum to 1), so after `passes` passes -- the upscale counted
as one -- a Gaussian layer lies within passes * (R_max + 2) * 2^-24 * max|I| of the model's, and a DoG layer within the bound of its
upper layer taken twice.  The nearest-neighbour resample copies values: it adds nothing.  Every layer is held to this.

Layers, the same derivation kept per layer (`_bounds`): it is what the keypoint comparison uses, and every layer is held to it too.
The upscale is two stages of two products and one sum of values <= max|I|: 4 u max|I|.  A pass with radius R and weights w adds
u max|I| (1 + 1 + sum_{k=1..R} W_k), W_k = w[0] + 2 (w[1] + ... + w[k]) <= 1 the weight gathered when the k-th accumulation rounds (the
pair sums and the products, each weighted by w[r], give the two ones; an accumulation rounds a partial sum of at most W_k max|I|).
gauss[o][i] carries the bound of the layer it was made from plus its own two passes with ITS radius; dog[o][i] carries the bounds of
gauss[o][i + 1] and gauss[o][i] plus u max|dog|.

Keypoints.  A decision reads DoG layers of one octave; eps(octave, top) is the largest bound among the DoG layers up to the highest
one its path has read (`top`), plus 4 u max|D| for the roundings of the derivative stencils.  The model reports, per starting
extremum, the smallest margin of the decisions on its path in grey levels of a DoG value (sift2d_model.decision, the one margin rule:
the 26 comparisons, the threshold, the 0.5 tests, the roundings of a step, the contrast and the edge tests).  A start is decidable when
that margin exceeds eps.  Every decidable model candidate is among the twin's starts and every decidable model keypoint is in the
twin's list with the same start, octave, layer, row and column; every twin start is a model candidate or an undecidable pixel, every
twin keypoint a model keypoint or an undecidable start.  Position, size and response agree within eps times the spread of each (what
one grey level of DoG error moves it by: through H^-1 for the offsets, contr_spread for the response, size ln 2 / n per unit of the
layer offset for the size) plus the float32 solve's own error and the few roundings of the final expression.

Undecidable keypoints must be at most 5 % of the model's keypoints on EVERY test image.
"""
import functools

import numpy as np
import pytest

import sift2d_cases as cases
import sift2d_model as model
import sift2d_twin as twin

U = 2.0 ** -24
# The test images.  Blobs: well-separated blobs at full contrast, one strong keypoint each.  Speckle: odd sides and four octaves;
# float pixels; five and two layers per octave; sigma 1.2 -- weak, crowded keypoints, some of which leave their starting cell.
# The issue lets the seeds be chosen so that the model alone meets the 5 % condition.  They are chosen: over seeds 21 ... 40 the
# share of undecidable keypoints is 1.5 - 20 % on the 61 x 53 image (7 seeds of 20 at or below 5 %), 0 - 15 % on the float image
# (7 of 20), 0 - 11 % at sigma 1.2 (12 of 20), 7 - 20 % with five layers per octave at spot 1.2 (none; the sharper spot 0.9 gives
# 0 of 82 at seed 48), 2 - 5 % with two layers (seeds 41 ... 60).  On the reference's 512 x 512 rotation image it is
# 9.97 % (798 of 8 008; rotation_170: 758 of 7 636) (not a test image here: the model takes several seconds on it).
BLOBS = {
    "blobs_u8": (lambda: cases.blob_lattice(200, 240, 1), {}),
    "blobs_f32": (lambda: cases.blob_lattice(200, 240, 3, as_float=True), {}),
}
SPECKLE = {
    "u8_61x53": (lambda: cases.speckle(53, 61, 21), {}),
    "f32_48x64": (lambda: cases.speckle(64, 48, 25, as_float=True), {}),
    "u8_5_layers": (lambda: cases.speckle(48, 52, 48, spot=0.9), dict(n_octave_layers=5)),
    "u8_2_layers": (lambda: cases.speckle(48, 52, 45), dict(n_octave_layers=2)),
    "u8_sigma_1_2": (lambda: cases.speckle(50, 50, 31), dict(sigma=1.2)),
}
# no keypoint, many extrema near the scan's integer threshold: the image on which a threshold that is not floored shows
LOW_CONTRAST = {"u8_low_contrast": (lambda: cases.low_contrast(80, 90, 25), {})}
IMAGES = dict(BLOBS, **SPECKLE, **LOW_CONTRAST)
MAX_UNDECIDABLE = 0.05


@functools.lru_cache(maxsize=None)
def _model(name):
    make, settings = IMAGES[name] if name in IMAGES else (lambda: cases.planted(name), {})
    img = make()
    n, sigma = settings.get("n_octave_layers", 3), settings.get("sigma", 1.6)
    p = model.build(img, n, sigma)
    located, margins = model.detect(p, sigma=sigma)
    return img, settings, p, located, margins


def _bounds(p, img):
    """(per-layer bounds of gauss[o][i], of dog[o][i], the issue's bound of gauss[o][i]); see the module docstring"""
    peak = float(np.abs(np.asarray(img, np.float64)).max())
    r_max = max(max(r) for r in p.radii)
    issue = [[model.layer_bound(c, r_max, peak) for c in row] for row in p.passes]
    n = p.n_octave_layers

    def one_pass(sigma, radius):
        w = model.weights_of(sigma, radius).astype(np.float64)
        gathered = w[0] + 2 * np.cumsum(w[1:])
        return U * peak * (2 + float(np.minimum(gathered, 1.0).sum()))

    gauss, dog = [], []
    for o in range(p.n_octave):
        row = []
        for i in range(n + 3):
            if i == 0 and o > 0:
                row.append(gauss[o - 1][n])
            else:
                row.append((4 * U * peak if i == 0 else row[i - 1]) + 2 * one_pass(p.sigmas[o][i], p.radii[o][i]))
        gauss.append(row)
        dog.append([row[i + 1] + row[i] + U * float(np.abs(p.dog[o][i]).max()) for i in range(n + 2)])
    return gauss, dog, issue


def _eps(p, img):
    """eps[o][top]: what a DoG value read by a decision whose path reached DoG layer `top` of octave o may carry"""
    _, dog, _ = _bounds(p, img)
    d_max = max(float(np.abs(d).max()) for octave in p.dog for d in octave)
    return [[max(row[:top + 1]) + 4 * U * d_max for top in range(len(row))] for row in dog]


def check(name):
    """the whole comparison of the twin (as it is now: a slip may be planted) with the model; returns the figures"""
    img, settings, p, located, margins = _model(name)
    t = twin.detector(img, **settings)
    n = p.n_octave_layers
    eps = _eps(p, img)
    g_bound, d_bound, issue_bound = _bounds(p, img)
    assert t.n_octave == p.n_octave and t.threshold == p.threshold
    for o in range(p.n_octave):
        for i in range(n + 3):
            g = t.gauss[o * (n + 3) + i]
            assert g.data.shape == p.gauss[o][i].shape
            err = np.abs(g.data.astype(np.float64) - p.gauss[o][i]).max()
            assert g_bound[o][i] <= issue_bound[o][i] and err <= g_bound[o][i], ("gauss", o, i, err)
        for i in range(n + 2):
            d = t.dog[o * (n + 2) + i]
            err = np.abs(d.data.astype(np.float64) - p.dog[o][i]).max()
            assert d_bound[o][i] <= 2 * issue_bound[o][i + 1] + U * 255 and err <= d_bound[o][i], ("dog", o, i, err)
    twin_starts = {(int(s["octave"]), int(s["layer"]), int(s["row"]), int(s["col"])): bool(s["accepted"]) for s in t.starts}
    accepted = t.starts[t.starts["accepted"] == 1]
    twin_kp = {(int(s["octave"]), int(s["layer"]), int(s["row"]), int(s["col"])): k for s, k in zip(accepted, t.keypoints)}
    assert len(twin_kp) == len(t.keypoints)
    model_by_start = {m.start: m for m in located}
    # candidates, both ways (a candidate's comparisons read the DoG layers up to its own + 1)
    for m in located:
        cand_margin = margins[(m.start[0], m.start[1])][1][m.start[2], m.start[3]]
        if cand_margin > eps[m.start[0]][m.start[1] + 1]:
            assert m.start in twin_starts, ("a decidable model candidate is missing", m.start)
    for start in twin_starts:
        cand, margin = margins[(start[0], start[1])]
        assert cand[start[2], start[3]] or margin[start[2], start[3]] <= eps[start[0]][start[1] + 1], ("a twin start is decidably no candidate", start)
    # keypoints, both ways
    undecidable = 0
    worst = 0.0
    n_model = sum(m.accepted for m in located)
    for m in located:
        if not m.accepted:
            continue
        e = eps[m.start[0]][m.top]
        if not m.margin > e:
            undecidable += 1
            continue
        assert m.start in twin_kp, ("a decidable model keypoint is missing", m.start)
        k = twin_kp[m.start]
        assert (int(k["octave"]), int(k["layer"]), int(k["row"]), int(k["col"])) == (m.octave, m.layer, m.row, m.col), m.start
        scale = 2.0 ** m.start[0] * 0.5
        bound = e * m.x_spread + scale * m.solve_spread * U + 4 * U * max(abs(m.x), abs(m.y), 1.0)
        err = max(abs(float(k["x"]) - m.x), abs(float(k["y"]) - m.y))
        assert err <= bound, ("position", m.start, err, bound)
        worst = max(worst, err)
        # size = sigma 2^((layer + xi) / n) 2^o: the layer offset moves it by size ln 2 / n per unit; the division, 2^t, the products
        # and the float32 sigma: 6 roundings
        d_xi = e * m.xi_spread + m.solve_spread * U
        assert abs(float(k["size"]) - m.size) <= m.size * (np.log(2.0) / n * d_xi + 6 * U), ("size", m.start)
        # response = |v s + 0.5 dD . offset|: contr_spread per grey level, the solve's error through 0.5 |dD| . 1, and the roundings of
        # s = 1.f / 255, the two products, the three-term dot product and the sum: 8 u of the magnitudes involved
        dD_sum = m.contr_spread   # (>= s, and >= 0.5 |dD| . x_spread: a bound of the magnitudes that does not need dD itself)
        d_resp = e * m.contr_spread + m.solve_spread * U * dD_sum + 8 * U * (m.response + dD_sum)
        assert abs(float(k["response"]) - m.response) <= d_resp, ("response", m.start, abs(float(k["response"]) - m.response), d_resp)
    for start in twin_kp:
        m = model_by_start.get(start)
        if m is None:
            continue   # (an undecidable pixel: checked with the starts above)
        assert m.accepted or not m.margin > eps[start[0]][m.top], ("a twin keypoint is decidably rejected by the model", start)
    return dict(model_keypoints=n_model, twin_keypoints=len(t.keypoints), undecidable=undecidable, worst_position_error=worst,
                moved=sum(m.moved for m in located if m.accepted))


def _report(name, got, capsys):
    with capsys.disabled():
        print("\n[sift2d twin vs model] %s: %d model keypoints, %d twin keypoints, %d undecidable (%.2f %%), %d moved, worst position error %.2e px"
              % (name, got["model_keypoints"], got["twin_keypoints"], got["undecidable"], 100.0 * got["undecidable"] / max(got["model_keypoints"], 1),
                 got["moved"], got["worst_position_error"]))


@pytest.mark.parametrize("name", sorted(IMAGES) + ["along_x"])
def test_twin_equals_model(name, capsys):
    got = check(name)
    _report(name, got, capsys)
    assert got["undecidable"] <= MAX_UNDECIDABLE * got["model_keypoints"]
    if name in BLOBS:
        assert got["model_keypoints"] >= 30
    if name in SPECKLE:
        assert got["model_keypoints"] >= 40 and got["moved"] >= 1


def test_plateau_image():
    """constant along x: every pixel ties exactly with its row neighbours in any arithmetic; the plateau's pixels are all starts, in
    the model and in the twin, and none survives (det <= 0 after the zero pivot)"""
    got = check("along_x")
    _, _, _, located, _ = _model("along_x")
    assert len(located) > 0 and got["model_keypoints"] == 0 and got["twin_keypoints"] == 0


def test_low_contrast_image_has_starts_near_the_threshold():
    img, _, p, located, _ = _model("u8_low_contrast")
    near = sum(1 for m in located if abs(p.dog[m.start[0]][m.start[1]][m.start[2], m.start[3]]) <= 1.7)
    assert p.threshold == 1 and near >= 20


# the image on which each planted slip must show
SLIP_IMAGE = {"strict": "along_x", "no_layer_neighbours": "u8_61x53", "border_4": "u8_61x53", "plain_reflect": "u8_61x53", "truncate": "u8_61x53",
              "threshold_not_floored": "u8_low_contrast", "no_half": "blobs_u8", "edge_inverted": "u8_61x53"}


@pytest.mark.parametrize("name", sorted(twin.SLIPS))
def test_planted_slip_is_caught(name):
    assert len(twin.SLIPS) >= 8 and set(SLIP_IMAGE) == set(twin.SLIPS)
    check(SLIP_IMAGE[name])   # (passes as it is)
    with twin.slip(twin.SLIPS[name]):
        with pytest.raises(AssertionError):
            check(SLIP_IMAGE[name])


def test_blobs_are_found():
    """Gaussian blobs of sigma 3 at known sub-pixel centres on a 96 x 96 image: each centre has a model keypoint within 0.5 px.  The
    2x upscale maps source s to doubled 2 s + 0.5, and a doubled x is reported as x / 2: a systematic +0.25 px, which stays."""
    centres = [(24.3, 22.6), (70.75, 25.2), (47.5, 48.1), (23.9, 71.4), (71.2, 70.6)]   # (x, y)
    y, x = np.mgrid[0:96, 0:96]
    img = np.full((96, 96), 40.0)
    for cx, cy in centres:
        img += 170.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * 3.0 ** 2))
    p = model.build(img)
    located, _ = model.detect(p)
    found = np.array([[m.x, m.y] for m in located if m.accepted])
    offsets = []
    for cx, cy in centres:
        d = np.hypot(found[:, 0] - cx, found[:, 1] - cy)
        k = int(np.argmin(d))
        assert d[k] < 0.5, (cx, cy, d[k])
        offsets.append(found[k] - (cx, cy))
    mean = np.mean(offsets, axis=0)
    print("\n[sift2d blobs] mean offset of the model's keypoints from the planted centres: %+.4f, %+.4f px" % (mean[0], mean[1]))
    assert 0.15 < mean[0] < 0.35 and 0.15 < mean[1] < 0.35
    t = twin.detector(img.astype(np.float32))
    for cx, cy in centres:
        assert np.hypot(t.keypoints["x"] - cx, t.keypoints["y"] - cy).min() < 0.5

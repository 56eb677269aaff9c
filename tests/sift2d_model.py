"""float64 NumPy model of SIFT2D's detector, written from the arithmetic contract of DESIGN.md section 4.13 (cv::SIFT as the
reference's SIFT2D::compute() creates it, src/oc_sift.cpp:22-30, 60-93) and from nothing else: it shares no code with the twin
(tests/cpp/sift2d_twin.cpp), the plan header or the kernels.  Sigmas and blur weights are the contract's float32 values (they are
inputs of the arithmetic, made in double and rounded once); everything computed from pixels is float64.

Besides the result the model reports, for every decision a keypoint's path took, how far the decision was from going the other
way (``margin``): by how much every DoG value the decision reads would have to move, in grey levels, before it could change.
The twin and the kernels work in float32, and a decision whose margin is not above the error bound of a DoG value
(tests/test_sift2d_twin_cpu.py derives it) may legitimately fall either way there.  The rule lives in ONE function, ``decision``.
"""
import math

import numpy as np

BORDER = 5
MAX_STEPS = 5
INT_MAX_3 = (2 ** 31 - 1) // 3


def cv_round(v):
    return int(np.rint(v))  # halves to even


def radius_of(sigma):
    return (cv_round(float(sigma) * 8 + 1) | 1) // 2


def weights_of(sigma, radius):
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    t = np.exp(-(x * x) / (2.0 * float(sigma) * float(sigma)))
    return (t / t.sum()).astype(np.float32)[radius:]


def plan(width, height, n_octave_layers=3, sigma=1.6, contrast_threshold=0.04):
    """(n_octave, [(cols, rows)] per octave, float32 sigma per layer of an octave, base sigma, integer threshold)"""
    n_octave = max(cv_round(math.log(min(2 * width, 2 * height)) / math.log(2.0) - 2), 1)
    dims = [(2 * width, 2 * height)]
    for _ in range(1, n_octave):
        dims.append((dims[-1][0] // 2, dims[-1][1] // 2))
    s = float(np.float32(sigma))
    k = 2.0 ** (1.0 / n_octave_layers)
    sig = [np.float32(sigma)]
    for i in range(1, n_octave_layers + 3):
        prev = k ** (i - 1) * s
        total = prev * k
        sig.append(np.float32(math.sqrt(total * total - prev * prev)))
    s32 = np.float32(sigma)
    base = np.sqrt(np.maximum(s32 * s32 - np.float32(4) * np.float32(0.5) * np.float32(0.5), np.float32(0.01)), dtype=np.float32)
    threshold = math.floor(0.5 * float(np.float32(contrast_threshold)) / n_octave_layers * 255)
    return n_octave, dims, sig, np.float32(base), threshold


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def blur(img, sigma):
    """rows first, then columns; per pixel w[0] s[c] + sum over r ascending of w[r] (s[lo] + s[hi]), reflect-101 repeated"""
    R = radius_of(sigma)
    w = weights_of(sigma, R).astype(np.float64)
    out = img
    for axis in (1, 0):
        n = out.shape[axis]
        idx = np.arange(n)
        acc = w[0] * out
        for r in range(1, R + 1):
            acc = acc + w[r] * (np.take(out, reflect101(idx - r, n), axis=axis) + np.take(out, reflect101(idx + r, n), axis=axis))
        out = acc
    return out


def upscale(img):
    """2x bilinear: destination x samples the source at (x + 0.5) * 0.5 - 0.5, indices clamped to the edge"""
    def along(a, axis):
        n = a.shape[axis]
        pos = (np.arange(2 * n) + 0.5) * 0.5 - 0.5
        i0 = np.floor(pos).astype(int)
        f = pos - i0
        lo, hi = np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1)
        shape = [1, 1]
        shape[axis] = 2 * n
        f = f.reshape(shape)
        return (1 - f) * np.take(a, lo, axis=axis) + f * np.take(a, hi, axis=axis)
    return along(along(img, 1), 0)


def nearest_half(img, cols, rows):
    sr, sc = img.shape
    iy = np.minimum(np.floor(np.arange(rows) * (sr / rows)).astype(int), sr - 1)
    ix = np.minimum(np.floor(np.arange(cols) * (sc / cols)).astype(int), sc - 1)
    return img[np.ix_(iy, ix)]


class Pyramid:
    def __init__(self, n_octave, n_octave_layers, gauss, dog, sigmas, radii, threshold, passes):
        self.n_octave, self.n_octave_layers, self.gauss, self.dog = n_octave, n_octave_layers, gauss, dog
        self.sigmas, self.radii, self.threshold, self.passes = sigmas, radii, threshold, passes


def build(image, n_octave_layers=3, sigma=1.6, contrast_threshold=0.04):
    """gauss[o][i], dog[o][i] as float64 (rows, cols) arrays; passes[o][i]: the blur passes (two per blur) a Gaussian layer has behind
    it, the upscale counted as one."""
    img = np.asarray(image, dtype=np.float64)
    h, w = img.shape
    n_octave, dims, sig, base_sigma, threshold = plan(w, h, n_octave_layers, sigma, contrast_threshold)
    gauss, dog, sigmas, radii, passes = [], [], [], [], []
    for o in range(n_octave):
        layers, sg, count = [], [], []
        for i in range(n_octave_layers + 3):
            if o == 0 and i == 0:
                layers.append(blur(upscale(img), base_sigma))
                sg.append(base_sigma)
                count.append(3)
            elif i == 0:
                layers.append(nearest_half(gauss[o - 1][n_octave_layers], dims[o][0], dims[o][1]))
                sg.append(np.float32(0))
                count.append(passes[o - 1][n_octave_layers])
            else:
                layers.append(blur(layers[i - 1], sig[i]))
                sg.append(sig[i])
                count.append(count[i - 1] + 2)
        gauss.append(layers)
        dog.append([layers[i + 1] - layers[i] for i in range(n_octave_layers + 2)])
        sigmas.append(sg)
        radii.append([radius_of(s) if s > 0 else 0 for s in sg])
        passes.append(count)
    return Pyramid(n_octave, n_octave_layers, gauss, dog, sigmas, radii, threshold, passes)


def decision(value, spread):
    """THE margin rule, for scalars and arrays.  A decision is `value > 0` (or >= 0, < 0 ...) of a float64 expression; `spread`
    bounds how far the same expression may move when every DoG value it reads moves by one grey level (the sum of the magnitudes of
    its first derivatives with respect to those values; for the solved offset, through the inverse of H).  The margin is
    |value| / spread: how far, in grey levels, the inputs must move before the decision can change.  A spread of zero -- the
    expression reads no DoG value that can move, as in a comparison between two values that are one value (an exact tie made by
    identical operations on identical data: a plateau of an image constant along an axis, the same tie in float32) -- is decided:
    margin inf."""
    value, spread = np.asarray(value, dtype=np.float64), np.asarray(spread, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(spread == 0, np.inf, np.abs(value) / np.where(spread == 0, 1.0, spread))
    return float(m) if m.ndim == 0 else m


def candidates(p, o, layer):
    """(is_candidate, margin) arrays over the layer; outside the 5-pixel border: False, inf"""
    d, below, above = p.dog[o][layer], p.dog[o][layer - 1], p.dog[o][layer + 1]
    rows, cols = d.shape
    cand = np.zeros(d.shape, bool)
    margin = np.full(d.shape, np.inf)
    if rows <= 2 * BORDER or cols <= 2 * BORDER:
        return cand, margin
    sl = (slice(BORDER, rows - BORDER), slice(BORDER, cols - BORDER))
    v = d[sl]
    nb = []
    for k, lay in enumerate((d, below, above)):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if k == 0 and dr == 0 and dc == 0:
                    continue
                nb.append(lay[BORDER + dr:rows - BORDER + dr, BORDER + dc:cols - BORDER + dc])
    nb = np.stack(nb)
    hi, lo = nb.max(axis=0), nb.min(axis=0)
    over = np.abs(v) > p.threshold
    is_max, is_min = (v > 0) & (v >= hi), (v < 0) & (v <= lo)
    cand[sl] = over & (is_max | is_min)
    # the decisions: |v| - threshold (one value: spread 1) and, for the sign the pixel has, v against each neighbour (a difference
    # of two values: spread 2; against a neighbour that ties exactly: spread 0, see `decision`).  Of the 26 comparisons the one
    # nearest to changing the verdict has the smallest margin.
    gaps = np.where(v > 0, v - nb, nb - v)
    m_ext = decision(gaps, np.where(nb == v, 0.0, 2.0)).min(axis=0)
    m_thr = decision(np.abs(v) - p.threshold, 1.0)
    # a pixel that fails decidedly on one test is decided whatever the others say; one that passes both needs both
    fail_thr, fail_ext = ~over, ~(is_max | is_min)
    # (for a pixel that is no extremum only the comparisons it fails count: it stays none unless all of them turn)
    m_fail = np.where(gaps < 0, decision(gaps, 2.0), -np.inf).max(axis=0)
    m = np.minimum(m_thr, m_ext)
    m_fail = np.minimum(m_fail, np.where(p.threshold > 0, np.inf, np.abs(v)))   # (threshold 0: a change of sign makes another pixel of it)
    m = np.where(fail_thr & fail_ext, np.maximum(m_thr, m_fail), np.where(fail_thr, m_thr, np.where(fail_ext, m_fail, m)))
    margin[sl] = m
    return cand, margin


class Located:
    """One starting extremum after localisation.  margin: the smallest margin (in grey levels of a DoG value) of the decisions on its
    path, the rejecting one included; accepted records carry the keypoint."""

    def __init__(self, start):
        self.start = start
        self.accepted = False
        self.margin = math.inf
        self.moved = False
        self.solve_spread = 0.0
        self.top = start[1] + 1   # the highest DoG layer of the octave a decision on the path has read


def localize(p, o, layer, r, c, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
    n = p.n_octave_layers
    out = Located((o, layer, r, c))
    rows, cols = p.dog[o][0].shape
    s = 1.0 / 255
    contrast_threshold, edge_threshold = float(np.float32(contrast_threshold)), float(np.float32(edge_threshold))

    def note(value, spread):
        out.margin = min(out.margin, decision(value, spread))

    for step in range(MAX_STEPS + 1):
        if step == MAX_STEPS:
            return out
        img, prev, nxt = p.dog[o][layer], p.dog[o][layer - 1], p.dog[o][layer + 1]
        out.top = max(out.top, layer + 1)
        dD = np.array([(img[r, c + 1] - img[r, c - 1]) * 0.5 * s, (img[r + 1, c] - img[r - 1, c]) * 0.5 * s, (nxt[r, c] - prev[r, c]) * 0.5 * s])
        v2 = 2 * img[r, c]
        dxx = (img[r, c + 1] + img[r, c - 1] - v2) * s
        dyy = (img[r + 1, c] + img[r - 1, c] - v2) * s
        dss = (nxt[r, c] + prev[r, c] - v2) * s
        dxy = (img[r + 1, c + 1] - img[r + 1, c - 1] - img[r - 1, c + 1] + img[r - 1, c - 1]) * 0.25 * s
        dxs = (nxt[r, c + 1] - nxt[r, c - 1] - prev[r, c + 1] + prev[r, c - 1]) * 0.25 * s
        dys = (nxt[r + 1, c] - nxt[r - 1, c] - prev[r + 1, c] + prev[r - 1, c]) * 0.25 * s
        H = np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]])
        singular = abs(np.linalg.det(H)) < 1e-300 or not np.all(np.isfinite(H))
        if singular:
            # the contract's zero pivot: X = 0, the loop stops here; the verdict falls at det <= 0 or at the contrast test
            X = np.zeros(3)
            x_spread = np.zeros(3) if not H.any() else np.full(3, np.inf)
        else:
            Hinv = np.linalg.inv(H)
            X = Hinv @ dD
            # X = H^-1 dD, so dX = H^-1 (d(dD) - dH X): moving every DoG value by eps moves dD_j by at most eps s (two values times
            # 0.5 s), a diagonal entry of H by 4 eps s and an off-diagonal one by eps s (four values times 0.25 s), so
            # |dX_k| <= sum_j |H^-1[k][j]| s (1 + 4 |X_j| + sum_{l != j} |X_l|) eps
            ax = np.abs(X)
            x_spread = np.abs(Hinv) @ (s * (1 + 3 * ax + ax.sum()))
            # ... and a float32 elimination with partial pivoting returns X within 9 cond(H) |X|_inf u, u = 2^-24 (n = 3: the
            # textbook 3 n u growth-factor bound with growth <= 4)
            out.solve_spread = 9 * np.abs(H).sum(axis=1).max() * np.abs(Hinv).sum(axis=1).max() * np.abs(X).max()
        off = -X  # (xc, xr, xi)
        slack = out.solve_spread * 2.0 ** -24 if not singular else 0.0   # what the float32 solve itself may move an offset by
        if np.all(np.abs(off) < 0.5):
            for k in range(3):
                note(max(0.5 - abs(off[k]) - slack, 0.0), x_spread[k])
            break
        # the step is taken: whichever offsets are not below 0.5 decide that; the cells moved to depend on the rounding
        big = int(np.argmax(np.abs(off)))
        note(max(abs(off[big]) - 0.5 - slack, 0.0), x_spread[big])
        if np.any(np.abs(off) > INT_MAX_3):
            return out
        for k in range(3):
            frac = abs(off[k]) - math.floor(abs(off[k]))
            note(max(abs(frac - 0.5) - slack, 0.0), x_spread[k])
        c += cv_round(off[0])
        r += cv_round(off[1])
        layer += cv_round(off[2])
        out.moved = True
        if layer < 1 or layer > n or c < BORDER or c >= cols - BORDER or r < BORDER or r >= rows - BORDER:
            return out
    img = p.dog[o][layer]
    contr = img[r, c] * s + 0.5 * float(dD @ off)
    # contr = v s + 0.5 dD.off: v moves it by s eps, dD by 0.5 |off|_1 s eps, the offset by 0.5 |dD| . |d off|
    contr_spread = s * (1 + 0.5 * np.abs(off).sum()) + 0.5 * float(np.abs(dD) @ x_spread) if np.all(np.isfinite(x_spread)) else math.inf
    note(abs(contr) * n - contrast_threshold, contr_spread * n)
    if abs(contr) * n < contrast_threshold:
        return out
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    # dxx, dyy move by 4 s eps each, dxy by s eps
    det_spread = s * (4 * abs(dyy) + 4 * abs(dxx) + 2 * abs(dxy))
    note(det, det_spread)
    if det <= 0:
        return out
    e = edge_threshold
    edge = (e + 1) * (e + 1) * det - tr * tr * e
    note(edge, (e + 1) * (e + 1) * det_spread + 2 * abs(tr) * e * 8 * s)
    if edge <= 0:
        return out
    out.accepted = True
    scale = float(2 ** o)
    out.octave, out.layer, out.row, out.col = o - 1, layer, r, c
    out.xc, out.xr, out.xi = off
    out.x, out.y = (c + off[0]) * scale * 0.5, (r + off[1]) * scale * 0.5
    out.x_spread = scale * 0.5 * max(x_spread[0], x_spread[1])   # of x and y, per eps
    out.xi_spread = x_spread[2]
    out.contr_spread = contr_spread
    out.size = float(np.float32(sigma)) * 2.0 ** ((layer + off[2]) / n) * scale
    out.response = abs(contr)
    return out


def detect(p, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
    """(located, candidate margins): `located` lists every starting extremum in scan order (octave, layer, row, column);
    margins[(o, layer)] = (is_candidate, margin) arrays of `candidates`"""
    located, margins = [], {}
    for o in range(p.n_octave):
        for layer in range(1, p.n_octave_layers + 1):
            cand, margin = candidates(p, o, layer)
            margins[(o, layer)] = (cand, margin)
            for r, c in zip(*np.nonzero(cand)):
                one = localize(p, o, layer, int(r), int(c), contrast_threshold, edge_threshold, sigma)
                one.margin = min(one.margin, margin[r, c])
                located.append(one)
    return located, margins


def layer_bound(passes, r_max, peak):
    """|float32 layer - float64 layer| <= passes * (r_max + 2) * 2^-24 * peak (derivation: tests/test_sift2d_twin_cpu.py)"""
    return passes * (r_max + 2) * 2.0 ** -24 * peak

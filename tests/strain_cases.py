"""Strain / RegionFit on regular grids, exact ties, collinear clouds and capped cell grids: a brute-force float64 model and the
case builders shared by tests/test_oracle_strain_cases.py, test_oracle_vs_ref_strain_cases.py and test_gpu_strain_cases.py.
NumPy only (`oracle_result` alone imports the oracle, when called).

THE MODEL (`model`) restates Strain::compute(POI2D / POI3D queue) (src/oc_strain.cpp:149-247, :372-488) and
RegionFit2D/3D::compute (src/oc_region_fit.cpp:94-174, :251-342) the way tests/stereo_numpy.py: strain_neighbours does for the
stereo record, and shares nothing with the oracle's restatement: no cell grid -- every query is compared with every POI of the
cloud; squared distances accumulate in float32 in axis order as (query - point)^2; the radius test is the strict
`d < float32(r) * float32(r)`; with fewer than nmin POIs inside, the nmin smallest by (distance, queue index) are taken instead and
NaN distances never enter; Strain keeps the rows whose ZNCC reaches the threshold and skips queries whose own ZNCC does not,
RegionFit keeps every row; a result needs at least nmin rows.  The plane is fitted by numpy.linalg.lstsq in float64 over the rows
[1, float32(neighbour - query)].  RANK RULE: a column (order 1, dx, dy, dz) whose residual against the kept columns before it is
at most 1e-12 of its own squared norm is dropped and its coefficient is 0 -- the engines' documented "a pivot that vanishes zeroes
that gradient component" (a row of POIs along x has no dy column, a diagonal line leaves dx and drops dy, coincident POIs keep the
constant alone).  A dropped column makes the matrix singular to 1e-6, so fits of at least as many rows as columns with cond < 1e5 are full rank and skip that test.
The Cauchy / Green formulas are float32 in the reference's operand order.

THE CASES (`strain_cases`, `regionfit_cases`): fixed seeds, at most 3000 POIs, queue order shuffled by a fixed permutation so that
index order is never spatial order, displacements an affine field about the cloud's centre plus N(0, 0.02) noise in float32 (one
wrong neighbour moves a strain by about 1e-5), every float of a record that is no input filled with noise, every result field
at a sentinel.  `verify_case` asserts on the CPU what keeps a case from going soft:

  decisive     `grid_r_eq_k_spacing`: the model with `<=` for `<` moves more than half of the fitted POIs by over 10 x the value
               bound.  `grid_knn_ties*`: the model with the tie broken by DESCENDING index selects another set for at least a
               quarter of the K-nearest queries -- where the lattice allows it.  K = 6 (2D) and K = 8 (3D) cut the shell of
               diagonal / face neighbours at every POI; K = 5 completes a shell in the interior and is tied on the rim only, so
               those grids are 14 x 12 (29 % rim); K = 9 completes a shell at every POI of a rectangular lattice (interior
               1 + 4 + 4, edge 1 + 3 + 2 + 3, corner 1 + 2 + 1 + 2 + 2 + 1) but the eight edge POIs next to a corner
               (1 + 3 + 2 + 2, the ninth among three at sqrt(5) s): the quarter cannot be had, the expected count is eight and
               asserted as such.  Those cases still order equal distances inside the insertion and the sums.
  cap active   the grid rule of strain_make_grid, restated in `grid_rule`, yields pitch > 1.001 r in the cap cases only.
  bounded walk the K-nearest kernel walks whole shells of cells serially in one thread (about 4/3 R^3 cells in 2D, 2 R^4 in 3D
               for R rings), and a query that never collects K finite distances walks every ring of the grid.  For every query
               on that path sqrt(d_K) / pitch + 2 (or the grid's reach + 1 where fewer than K finite distances exist) is at most
               32 in 2D and 12 in 3D.  The stretch points of the cap cases have ZNCC 0.1 for that reason (cloud members, never
               queries); the cap clouds get no query outside the blob and no NaN query; 3D queries outside the bounding box stay
               within 8 pitches of it (2D: 20).
"""
import numpy as np

F32 = np.float32
# float offsets of the records (src/oc_poi.h:102-136, :187-222)
REC = {2: dict(floats=25, u=2, v=8, zncc=16, strain=[20, 21, 22], plane=[2, 3, 4, 8, 9, 10]),
       3: dict(floats=31, u=3, v=7, w=11, zncc=18, strain=[22, 23, 24, 25, 26, 27], plane=list(range(3, 15)))}
SENTINEL = F32(77.0)          # strain fields before Strain
PLANE_SENTINEL = F32(55.0)    # deformation fields of a RegionFit query
WALK_LIMIT = {2: 32.0, 3: 12.0}
GRAD = {2: np.array([[0.10, 0.03], [0.02, -0.05]]),
        3: np.array([[0.10, 0.03, -0.02], [0.02, -0.05, 0.04], [-0.03, 0.01, 0.06]])}


# ---- the model ------------------------------------------------------------------------------------------------------------------
def distances(query, cloud):
    """float32 squared distances (m, n): sum over the axes, in order, of (query - point)^2."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = None
        for a in range(cloud.shape[1]):
            t = query[:, None, a] - cloud[None, :, a]
            d = t * t if d is None else d + t * t
    return d


def neighbour_sets(query, cloud, radius, nmin, closed=False, tie_descending=False):
    """Per query the cloud indices of the fit before any ZNCC gate, and the mask of the queries on the K-nearest path, and the
    K-th distance there (NaN where fewer than nmin finite distances exist).  closed / tie_descending: the two planted mistakes."""
    r2 = F32(radius) * F32(radius)
    n = len(cloud)
    sets, knn, dk = [], np.zeros(len(query), dtype=bool), np.full(len(query), np.nan)
    index = np.arange(n)
    for lo in range(0, len(query), 512):
        d = distances(query[lo:lo + 512], cloud)
        inside = (d <= r2) if closed else (d < r2)
        for j in range(len(d)):
            k = np.flatnonzero(inside[j])
            if len(k) < nmin:
                knn[lo + j] = True
                finite = np.flatnonzero(~np.isnan(d[j]))
                key = -index[finite] if tie_descending else index[finite]
                k = finite[np.lexsort((key, d[j][finite]))[:nmin]]
                if len(k) == nmin:
                    dk[lo + j] = d[j][k[-1]]
            sets.append(k)
    return sets, knn, dk


def fit_plane(A, rhs):
    """Least squares over the kept columns of A (see RANK RULE).  Returns (coefficients (D, nrhs), kept mask, cond)."""
    D = A.shape[1]
    g, _, _, sv = np.linalg.lstsq(A, rhs, rcond=None)
    if len(A) >= D and sv[-1] > 1e-5 * sv[0]:
        return g, np.ones(D, dtype=bool), sv[0] / sv[-1]
    kept = np.zeros(D, dtype=bool)
    for j in range(D):
        c = A[:, j]
        res = c
        if kept.any():
            res = c - A[:, kept] @ np.linalg.lstsq(A[:, kept], c, rcond=None)[0]
        kept[j] = res @ res > 1e-12 * (c @ c)
    g = np.zeros((D, rhs.shape[1]))
    gk, _, _, sv = np.linalg.lstsq(A[:, kept], rhs, rcond=None)
    g[kept] = gk
    return g, kept, sv[0] / sv[-1]


def model(dim, cloud, radius, nmin, queries=None, threshold=0.9, closed=False, tie_descending=False):
    """queries None: Strain over `cloud` itself; else RegionFit of `queries` over `cloud`.  Returns a dict: `coef` (m, dim, dim + 1)
    float64 [value, d/dx, d/dy(, d/dz)] per displacement component, `fitted`, `knn`, `rank` (kept columns), `cond`, `dk`, `sets`."""
    L = REC[dim]
    xyz = np.ascontiguousarray(cloud[:, :dim], dtype=F32)
    strain_mode = queries is None
    q = xyz if strain_mode else np.ascontiguousarray(queries[:, :dim], dtype=F32)
    with np.errstate(invalid="ignore"):
        gate = (cloud[:, L["zncc"]] >= F32(threshold)) if strain_mode else np.ones(len(cloud), dtype=bool)
    rhs_cols = [L["u"], L["v"]] + ([L["w"]] if dim == 3 else [])
    rhs = cloud[:, rhs_cols].astype(np.float64)
    sets, knn, dk = neighbour_sets(q, xyz, radius, nmin, closed, tie_descending)
    m = len(q)
    coef = np.zeros((m, dim, dim + 1))
    fitted = np.zeros(m, dtype=bool)
    rank = np.zeros(m, dtype=int)
    cond = np.zeros(m)
    for i in range(m):
        if strain_mode and not gate[i]:
            continue
        k = sets[i][gate[sets[i]]]
        if len(k) < nmin:
            continue
        A = np.hstack([np.ones((len(k), 1)), (xyz[k] - q[i]).astype(np.float64)])   # float32 differences, neighbour - query
        g, kept, cond[i] = fit_plane(A, rhs[k])
        coef[i] = g.T
        rank[i] = kept.sum()
        fitted[i] = True
    return dict(coef=coef, fitted=fitted, knn=knn, rank=rank, cond=cond, dk=dk, sets=sets)


def strain_values(coef, dim, approximation):
    """Cauchy (1) / Green (2) strains in float32 from float32-rounded gradients (src/oc_strain.cpp:220-234, :446-466)."""
    g = coef[:, :, 1:].astype(F32)
    h = F32(0.5)
    if dim == 2:
        ux, uy, vx, vy = g[:, 0, 0], g[:, 0, 1], g[:, 1, 0], g[:, 1, 1]
        if approximation == 1:
            e = [ux, vy, h * (uy + vx)]
        else:
            e = [ux + h * (ux * ux + vx * vx), vy + h * (uy * uy + vy * vy), h * (uy + vx + uy * ux + vy * vx)]
    else:
        (ux, uy, uz), (vx, vy, vz), (wx, wy, wz) = [[g[:, r, c] for c in range(3)] for r in range(3)]
        if approximation == 1:
            e = [ux, vy, wz, h * (uy + vx), h * (vz + wy), h * (wx + uz)]
        else:
            e = [ux + h * (ux * ux + vx * vx + wx * wx), vy + h * (uy * uy + vy * vy + wy * wy), wz + h * (uz * uz + vz * vz + wz * wz),
                 h * (uy + vx + uy * ux + vy * vx + wy * wx), h * (vz + wy + uz * uy + vz * vy + wz * wy),
                 h * (wx + uz + ux * uz + vx * vz + wx * wz)]
    return np.stack(e, axis=1).astype(F32)


def plane_values(coef):
    """What RegionFit writes: u ux uy(, uz) v vx vy ... in float32."""
    return coef.reshape(len(coef), -1).astype(F32)


def value_bound(res, values, dim, approximation=1, plane=False):
    """Per written value: 16 cond^2 2^-53 max(|g|, 1) for the double normal equations the engines solve (the term of
    tests/test_gpu_stereo.py) plus 2 spacing(float32(|value|)) for the one or two float32 roundings of the result.  Green strains are
    float32 polynomials of the gradients with |d e / d g| <= 1 + sum |g|: the first term and one spacing of the largest gradient
    pass through that factor, and the evaluation adds a few roundings of the result (8 spacings, as in
    test_strain_poi2ds_on_the_table).  No floor."""
    c = res["coef"] if plane else res["coef"][:, :, 1:]
    g = np.abs(c).reshape(len(c), -1)
    gmax = g.max(axis=1)
    first = (16.0 * res["cond"] ** 2 * 2.0 ** -53 * np.maximum(gmax, 1.0))[:, None]
    own = np.spacing(np.abs(values).astype(F32)).astype(np.float64)
    if approximation == 1 or plane:
        return first + 2 * own
    return (1.0 + g.sum(axis=1))[:, None] * (first + np.spacing(gmax.astype(F32)).astype(np.float64)[:, None]) + 8 * own


# ---- the grid rule of strain_make_grid, restated (float32) ----------------------------------------------------------------------
def grid_rule(dim, xyz, radius):
    """(pitch, cells per axis) of the engines' uniform grid over a cloud."""
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(xyz)
        mn = np.array([xyz[ok[:, a], a].min() if ok[:, a].any() else 0 for a in range(dim)], dtype=F32)
        mx = np.array([xyz[ok[:, a], a].max() if ok[:, a].any() else 0 for a in range(dim)], dtype=F32)
    pitch = F32(radius) * F32(1.001)
    cut = (mx - mn).max() / F32(4096.0 if dim == 2 else 256.0)
    if not pitch > cut:
        pitch = cut
    if not pitch > 0:
        pitch = F32(1)
    return pitch, [int((mx[a] - mn[a]) * (F32(1) / pitch)) + 1 for a in range(dim)]


# ---- records ---------------------------------------------------------------------------------------------------------------------
def make_records(dim, xyz, seed, zncc=0.99, centre=None):
    """A queue over the float32 coordinates `xyz` (n, dim), in the order given."""
    L = REC[dim]
    rng = np.random.default_rng(seed)
    n = len(xyz)
    p = rng.uniform(-1, 1, (n, L["floats"])).astype(F32)
    p[:, :dim] = xyz
    x = np.nan_to_num(p[:, :dim].astype(np.float64))
    c = np.nanmean(np.where(np.isnan(xyz), np.nan, x), axis=0) if centre is None else np.asarray(centre, dtype=np.float64)
    c = np.nan_to_num(c)
    base = [1.5, -0.5, 0.25]
    for r, k in enumerate(["u", "v", "w"][:dim]):
        p[:, L[k]] = (base[r] + (x - c) @ GRAD[dim][r]).astype(F32) + rng.normal(0, 0.02, n).astype(F32)
    p[:, L["zncc"]] = zncc
    p[:, L["strain"]] = SENTINEL
    return p


def make_queries(dim, xyz, seed):
    """RegionFit queries: failed POIs waiting for a new initial guess."""
    L = REC[dim]
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1, 1, (len(xyz), L["floats"])).astype(F32)
    q[:, :dim] = xyz
    q[:, L["plane"]] = PLANE_SENTINEL
    q[:, L["zncc"]] = -4.0
    return q


def shuffled(xyz, seed):
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    return np.ascontiguousarray(xyz[np.random.default_rng(seed).permutation(len(xyz))])


def lattice(origin, spacing, shape):
    axes = [F32(o) + F32(spacing) * np.arange(n, dtype=F32) for o, n in zip(origin, shape)]
    return np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], axis=1).astype(F32)


class Case:
    """name, dim, cloud records, radius, nmin; queries (RegionFit) or None (Strain); threshold; flags:
    kind ('r_eq', 'knn_ties', 'cap' or None), tie_quarter (the lattice admits a changed set at a quarter of the K-nearest queries),
    tie_corner_only (it admits a change at the eight POIs next to a corner only), ranks (the set of ranks every fitted POI must have, for the line cases), ref (the compiled reference
    is deterministic here: no query on the K-nearest path)."""

    def __init__(self, name, dim, cloud, radius, nmin, queries=None, threshold=0.9, kind=None, tie_quarter=False, tie_corner_only=False,
                 ranks=None, ref=False, spacing=None):
        self.name, self.dim, self.cloud, self.radius, self.nmin = name, dim, cloud, float(radius), int(nmin)
        self.queries, self.threshold, self.kind, self.ranks, self.ref = queries, threshold, kind, ranks, ref
        self.tie_quarter, self.tie_corner_only, self.spacing = tie_quarter, tie_corner_only, spacing
        assert len(cloud) <= 3000 and (queries is None or len(queries) <= 3000)
        self._model = None

    def __repr__(self):
        return self.name

    @property
    def regionfit(self):
        return self.queries is not None

    def model(self, **kw):
        if kw:
            return model(self.dim, self.cloud, self.radius, self.nmin, self.queries, self.threshold, **kw)
        if self._model is None:
            self._model = model(self.dim, self.cloud, self.radius, self.nmin, self.queries, self.threshold)
        return self._model

    def walk(self):
        """Rings of cells the K-nearest kernel visits for the queries on that path (see the module docstring)."""
        res = self.model()
        pitch, nc = grid_rule(self.dim, self.cloud[:, :self.dim], self.radius)
        L = REC[self.dim]
        on_path = res["knn"].copy()
        if not self.regionfit:
            with np.errstate(invalid="ignore"):
                on_path &= self.cloud[:, L["zncc"]] >= F32(self.threshold)
        rings = np.where(np.isnan(res["dk"]), max(nc) + 1.0, np.sqrt(res["dk"]) / float(pitch) + 2.0)
        return rings[on_path], float(pitch)


# GRIDS of the tie cases: (spacing, radius = k spacing), origins chosen so that every coordinate is an exact float32 integer
GRIDS_2D = [(10.0, 30.0, (37.0, 21.0)), (5.0, 25.0, (-60.0, 15.0)), (7.0, 35.0, (3.0, -98.0))]
GRID_3D = (8.0, 16.0, (16.0, -40.0, 8.0))


def _below(r, limit2):
    """The float32 radius r, one step down if its float32 square exceeds limit2 (so that `d < r * r` excludes d = limit2)."""
    r = F32(r)
    return r if r * r <= F32(limit2) else np.nextafter(r, F32(0))


def strain_cases():
    out = []
    # --- neighbours at distance exactly r (3-4-5 triples at k = 5: twelve of them)
    for j, (s, r, o) in enumerate(GRIDS_2D):
        xy = shuffled(lattice(o, s, (26, 22)), 100 + j)
        out.append(Case("grid_r_eq_k_spacing-2d-s%g-r%g" % (s, r), 2, make_records(2, xy, 200 + j), r, 6, kind="r_eq", ref=True, spacing=s))
    s, r, o = GRID_3D
    xyz = shuffled(lattice(o, s, (12, 11, 10)), 110)
    out.append(Case("grid_r_eq_k_spacing-3d-s%g-r%g" % (s, r), 3, make_records(3, xyz, 210), r, 6, kind="r_eq", ref=True, spacing=s))
    # --- K-nearest path with tied candidates: radius < s, = s, = s sqrt(2) (the largest float32 whose square does not pass 2 s^2)
    for j, (s, _, o) in enumerate(GRIDS_2D):
        radii = [("lt", F32(0.6 * s)), ("eq", F32(s)), ("sqrt2", _below(s * np.sqrt(2.0), 2 * s * s))]
        for i, (tag, r) in enumerate(radii):
            K = ((5, 6, 9), (6, 9, 6), (9, 5, 6))[j][i]        # K = 5 has no K-nearest path at s sqrt(2): five POIs lie inside
            xy = shuffled(lattice(o, s, (14, 12)), 120 + 3 * j + i)
            out.append(Case("grid_knn_ties-2d-s%g-r_%s-K%d" % (s, tag, K), 2, make_records(2, xy, 220 + 3 * j + i), r, K, kind="knn_ties",
                            tie_quarter=K != 9, tie_corner_only=K == 9, spacing=s))
    s, _, o = GRID_3D
    for i, (tag, r) in enumerate([("lt", F32(0.6 * s)), ("eq", F32(s)), ("sqrt2", _below(s * np.sqrt(2.0), 2 * s * s))]):
        xyz = shuffled(lattice(o, s, (9, 8, 7)), 140 + i)
        out.append(Case("grid_knn_ties-3d-s%g-r_%s-K8" % (s, tag), 3, make_records(3, xyz, 240 + i), r, 8, kind="knn_ties", tie_quarter=True,
                        spacing=s))
    # --- the same with 20 % of the POIs below the threshold: tied candidates are filtered afterwards, some POIs stay untouched
    for dim, (s, o, shape, K) in ((2, (10.0, (37.0, 21.0), (14, 12), 6)), (3, (8.0, (16.0, -40.0, 8.0), (9, 8, 7), 8))):
        x = shuffled(lattice(o, s, shape), 150 + dim)
        p = make_records(dim, x, 250 + dim)
        p[np.random.default_rng(260 + dim).random(len(p)) < 0.2, REC[dim]["zncc"]] = 0.5
        out.append(Case("grid_knn_ties_gated-%dd-s%g-r_eq-K%d" % (dim, s, K), dim, p, s, K, kind="knn_ties", tie_quarter=True, spacing=s))
    # --- negative coordinates: the ordered-uint bounding box of the kernel, cells counted from a negative anchor
    rng = np.random.default_rng(300)
    out.append(Case("negative_coordinates-2d-grid", 2, make_records(2, shuffled(lattice((-500.0, -410.0), 10.0, (26, 22)), 301), 302), 25.0, 6,
                    ref=True))
    out.append(Case("negative_coordinates-2d-grid-straddling", 2, make_records(2, shuffled(lattice((-125.0, -105.0), 10.0, (26, 22)), 303), 304),
                    25.0, 6, ref=True))
    out.append(Case("negative_coordinates-2d-scatter", 2, make_records(2, (rng.random((1500, 2)) * [300, 240] - [400, 300]).astype(F32), 305),
                    30.0, 5, ref=True))
    out.append(Case("negative_coordinates-2d-scatter-straddling", 2,
                    make_records(2, (rng.random((1500, 2)) * [300, 240] - [150, 120]).astype(F32), 306), 30.0, 5, ref=True))
    out.append(Case("negative_coordinates-3d-grid-straddling", 3, make_records(3, shuffled(lattice((-44.0, -40.0, -36.0), 8.0, (12, 11, 10)), 307), 308),
                    14.0, 6, ref=True))
    out.append(Case("negative_coordinates-3d-scatter", 3, make_records(3, (rng.random((2000, 3)) * 60 - [70, 30, 90]).astype(F32), 309), 15.0, 5,
                    ref=True))
    # --- far from the origin: coordinates that are no exact multiples of the spacing, cell rounding far from the anchor's scale
    out.append(Case("far_offset-2d-s0.1", 2, make_records(2, shuffled(lattice((1000.3, 77.7), 0.1, (26, 22)), 310), 311), 0.35, 6, ref=True))
    out.append(Case("far_offset-2d-s10", 2, make_records(2, shuffled(lattice((10000.0, -20000.0), 10.0, (26, 22)), 312), 313), 35.0, 6, ref=True))
    # (3D at spacing 0.1: noise gradients of 0.2 over seven to 33 rows, where the reference's float32 QR alone is 2e-6 from the
    # float64 model -- no reference bar there; the 0.5 lattice carries it)
    out.append(Case("far_offset-3d-s0.1", 3, make_records(3, shuffled(lattice((1000.3, 77.7, -310.1), 0.1, (12, 11, 10)), 314), 315), 0.25, 6))
    out.append(Case("far_offset-3d-s0.5", 3, make_records(3, shuffled(lattice((1000.3, 77.7, -310.1), 0.5, (12, 11, 10)), 316), 317), 1.25, 6,
                    ref=True))
    # --- collinear and coincident clouds: the vanishing pivot
    t = np.arange(60, dtype=F32) * F32(4)
    zero = np.zeros_like(t)
    lines = [("row_x", np.stack([t + 11, zero + 40], 1), {2}), ("column_y", np.stack([zero - 7, t - 100], 1), {2}),
             ("diagonal", np.stack([t, F32(0.5) * t + F32(3)], 1), {2}),
             ("two_rows", np.concatenate([np.stack([t, zero + 8], 1), np.stack([t, zero + 12], 1)]), {3}),
             ("coincident", np.tile(np.array([[12.5, -3.25]], dtype=F32), (50, 1)), {1})]
    for j, (tag, xy, ranks) in enumerate(lines):
        out.append(Case("lines-2d-" + tag, 2, make_records(2, shuffled(xy, 320 + j), 330 + j), 13.0, 5, ranks=ranks))
    # 3D: every pattern of dead and live pivots of the four-column solve -- dx alone, dy alone (a dead pivot, then a live one, then a
    # dead one), dz alone (two dead, then a live one), a line oblique to all axes, two live of three in each order, none
    plane = lattice((0.0, 0.0), 4.0, (20, 15))
    flat = np.full((len(plane), 1), 6, F32)
    lines3 = [("row_x", np.stack([t, zero + 5, zero - 9], 1), 13.0, 5, {2}), ("column_y", np.stack([zero - 7, t - 100, zero + 2], 1), 13.0, 5, {2}),
              ("line_z", np.stack([zero + 31, zero - 4, t - 60], 1), 13.0, 5, {2}),
              ("diagonal", np.stack([t, F32(0.5) * t + F32(3), F32(-0.25) * t + F32(1)], 1), 13.0, 5, {2}),
              ("two_rows", np.concatenate([np.stack([t, zero + 8, zero - 2], 1), np.stack([t, zero + 12, zero - 2], 1)]), 13.0, 5, {3}),
              ("plane_z", np.hstack([plane, flat]), 9.0, 6, {3}), ("plane_y", np.hstack([plane[:, :1], flat, plane[:, 1:]]), 9.0, 6, {3}),
              ("plane_x", np.hstack([flat, plane]), 9.0, 6, {3}),
              ("coincident", np.tile(np.array([[12.5, -3.25, 7.75]], dtype=F32), (50, 1)), 13.0, 5, {1})]
    for j, (tag, xyz, r, nmin, ranks) in enumerate(lines3):
        out.append(Case("lines-3d-" + tag, 3, make_records(3, shuffled(xyz, 3200 + j), 3300 + j), r, nmin, ranks=ranks))
    # --- the cell cap: stretch points far away widen the bounding box until span / 4096 (2D), span / 256 (3D) exceeds 1.001 r
    rng = np.random.default_rng(340)
    blob = lattice((1000 - 14.5 * 0.25, 1000 - 14.5 * 0.25), 0.25, (30, 30)) + rng.uniform(-0.05, 0.05, (900, 2)).astype(F32)
    xy = np.concatenate([blob, np.array([[0, 0], [0, 2600], [2600, 0], [2600, 2600]], dtype=F32)]).astype(F32)
    far = (xy[:, 0] < 500) | (xy[:, 0] > 2000)
    perm = np.random.default_rng(341).permutation(len(xy))
    for r in (0.6, 0.3):
        p = make_records(2, xy[perm], 342, centre=(1000, 1000))
        p[far[perm], REC[2]["zncc"]] = 0.1
        out.append(Case("cell_cap_2d-r%g" % r, 2, p, r, 6, kind="cap", ref=r == 0.6))
    blob = lattice((100 - 4.5 * 0.5,) * 3, 0.5, (10, 10, 10)) + rng.uniform(-0.05, 0.05, (1000, 3)).astype(F32)
    xyz = np.concatenate([blob, np.array([[0, 0, 0], [400, 400, 400]], dtype=F32)]).astype(F32)
    far = (xyz[:, 0] < 50) | (xyz[:, 0] > 200)
    perm = np.random.default_rng(343).permutation(len(xyz))
    for r in (1.2, 0.6):
        p = make_records(3, xyz[perm], 344, centre=(100, 100, 100))
        p[far[perm], REC[3]["zncc"]] = 0.1
        out.append(Case("cell_cap_3d-r%g" % r, 3, p, r, 6, kind="cap", ref=r == 1.2))
    # --- the whole cloud in one cell
    rng = np.random.default_rng(350)
    out.append(Case("one_cell-2d", 2, make_records(2, (rng.random((2000, 2)) * 50 + [5, -20]).astype(F32), 351), 80.0, 6, ref=True))
    out.append(Case("one_cell-3d", 3, make_records(3, (rng.random((1200, 3)) * 20 + [5, -20, 3]).astype(F32), 352), 40.0, 6, ref=True))
    # --- NaN coordinates: 1 % in x, 1 % in y (, 1 % in z): neither neighbours nor, as queries, fitted
    for dim, n, ext, r in ((2, 2000, [300, 240], 25.0), (3, 2000, [60, 60, 60], 12.0)):
        rng = np.random.default_rng(360 + dim)
        x = (rng.random((n, dim)) * ext).astype(F32)
        for a in range(dim):
            x[rng.random(n) < 0.01, a] = np.nan
        out.append(Case("nan_coordinates-%dd" % dim, dim, make_records(dim, x, 362 + dim), r, 6))
    # --- neighbor_number_min at both ends of its range
    rng = np.random.default_rng(370)
    xy = (rng.random((1500, 2)) * [300, 240]).astype(F32)
    out.append(Case("k_limits-2d-nmin1-r3", 2, make_records(2, xy, 371), 3.0, 1))
    out.append(Case("k_limits-2d-nmin64-all_knn", 2, make_records(2, xy, 372), 12.0, 64))
    out.append(Case("k_limits-2d-nmin64-all_inside", 2, make_records(2, xy, 373), 90.0, 64))
    xyz = (rng.random((1500, 3)) * 50).astype(F32)
    out.append(Case("k_limits-3d-nmin1-r2", 3, make_records(3, xyz, 374), 2.0, 1))
    out.append(Case("k_limits-3d-nmin64-all_knn", 3, make_records(3, xyz, 375), 6.0, 64))
    out.append(Case("k_limits-3d-nmin64-all_inside", 3, make_records(3, xyz, 376), 45.0, 64))
    # --- queue lengths around the 256-thread block (and the 64-thread block of the K-nearest kernel); below K nothing is written
    for n in (1, 63, 64, 255, 256, 257, 513):
        rng = np.random.default_rng(380 + n)
        out.append(Case("block_edges-2d-n%d" % n, 2, make_records(2, (rng.random((n, 2)) * [100, 80]).astype(F32), 381 + n), 30.0, 64))
    for n in (1, 63, 64, 255, 256, 257, 513):
        rng = np.random.default_rng(390 + n)
        out.append(Case("block_edges-3d-n%d" % n, 3, make_records(3, (rng.random((n, 3)) * 40).astype(F32), 391 + n), 18.0, 64))
    return out


def _query_points(dim, cloud_xyz, radius, seed, outside, nan, one_radius):
    """Queries of a RegionFit case: on nodes, at midpoints between a node and its successor in the queue's spatial sort, exactly
    one radius from a node where `one_radius` (an exact offset of that length) is given, `outside` pitches outside the bounding box,
    NaN coordinates."""
    rng = np.random.default_rng(seed)
    near = cloud_xyz[~np.isnan(cloud_xyz).any(axis=1)]
    nodes = near[rng.choice(len(near), min(150, len(near)), replace=False)]
    parts = [nodes]
    order = near[np.lexsort(near.T[::-1])]
    mid = (F32(0.5) * (order[:-1] + order[1:]))[:: max(1, len(order) // 150)]
    parts.append(mid.astype(F32))
    if one_radius is not None:
        parts.append((nodes[:60] + np.asarray(one_radius, dtype=F32)).astype(F32))
        parts.append((nodes[:60] - np.asarray(one_radius, dtype=F32)).astype(F32))
    if outside:
        pitch = F32(radius) * F32(1.001)
        lo, hi = near.min(axis=0), near.max(axis=0)
        k = 120
        p = (lo + rng.random((k, dim)) * (hi - lo)).astype(F32)
        side = rng.integers(0, 2 * dim, k)
        dist = (rng.random(k) * outside * pitch).astype(F32)
        for j in range(k):
            a = side[j] // 2
            p[j, a] = hi[a] + dist[j] if side[j] % 2 else lo[a] - dist[j]
        p[:2 ** dim] = [[(hi[a] + outside * pitch * F32(0.5)) if (c >> a) & 1 else (lo[a] - outside * pitch * F32(0.5)) for a in range(dim)]
                        for c in range(2 ** dim)]   # beyond the corners: outside on every axis
        parts.append(p)
    if nan:
        p = nodes[:3 * dim].copy()
        for j in range(len(p)):
            p[j, j % dim] = np.nan
        p[-1] = np.nan
        parts.append(p)
    return shuffled(np.concatenate(parts), seed + 1)


def regionfit_cases():
    out = []
    sc = {c.name: c for c in strain_cases()}

    def add(tag, src, radius, nmin, outside, nan, one_radius, kind=None, ranks=None, ref=False):
        c = sc[src]
        cloud = c.cloud.copy()
        blob = cloud[cloud[:, REC[c.dim]["zncc"]] >= 0.9]   # the cap clouds: no query near a stretch point
        q = make_queries(c.dim, _query_points(c.dim, blob[:, :c.dim], radius, 400 + len(out), outside, nan, one_radius), 450 + len(out))
        out.append(Case("regionfit_" + tag, c.dim, cloud, radius, nmin, queries=q, kind=kind, ranks=ranks, ref=ref))

    add("grid-2d", "grid_r_eq_k_spacing-2d-s10-r30", 30.0, 7, 20, True, (18.0, 24.0), ref=True)
    add("grid-3d", "grid_r_eq_k_spacing-3d-s8-r16", 15.0, 7, 8, True, (9.0, 12.0, 0.0), ref=True)
    add("negative-2d", "negative_coordinates-2d-scatter-straddling", 30.0, 6, 20, True, (18.0, 24.0), ref=True)
    add("negative-3d", "negative_coordinates-3d-scatter", 15.0, 6, 8, True, (9.0, 12.0, 0.0), ref=True)
    add("line-2d", "lines-2d-row_x", 13.0, 5, 20, True, (5.0, 12.0), ranks={2})
    add("line-3d", "lines-3d-row_x", 13.0, 5, 8, False, (5.0, 12.0, 0.0), ranks={2})   # 19 cells long: a NaN query would walk 20 rings
    add("cap-2d", "cell_cap_2d-r0.6", 0.6, 6, 0, False, None, kind="cap", ref=True)
    add("cap-3d", "cell_cap_3d-r1.2", 1.2, 6, 0, False, None, kind="cap", ref=True)
    # a cloud of K - 1 POIs: nothing can be fitted
    for dim, src in ((2, "grid_r_eq_k_spacing-2d-s10-r30"), (3, "grid_r_eq_k_spacing-3d-s8-r16")):
        cloud = np.ascontiguousarray(sc[src].cloud[:6])
        pts = np.concatenate([cloud[:, :dim], cloud[:3, :dim] + F32(1.5)]).astype(F32)
        c = Case("regionfit_cloud_of_K-1-%dd" % dim, dim, cloud, 40.0, 7, queries=make_queries(dim, pts, 470 + dim))
        c.untouched = True
        out.append(c)
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = strain_cases() + regionfit_cases()
    return _ALL


def case_by_name(name):
    return {c.name: c for c in all_cases()}[name]


# ---- what keeps a case from going soft ------------------------------------------------------------------------------------------
def written_values(case, res, approximation):
    return plane_values(res["coef"]) if case.regionfit else strain_values(res["coef"], case.dim, approximation)


def verify_case(case):
    """The three builder conditions (decisive, cap active, bounded walk) and what each case claims about itself.  Returns figures
    for the design record."""
    res = case.model()
    dim = case.dim
    info = dict(fitted=int(res["fitted"].sum()), knn=int(res["knn"].sum()))
    # cap active in the cap cases and nowhere else
    pitch, nc = grid_rule(dim, case.cloud[:, :dim], case.radius)
    capped = bool(pitch > F32(case.radius) * F32(1.001))
    assert capped == (case.kind == "cap"), (case.name, float(pitch), nc)
    info["pitch"], info["cells"] = float(pitch), nc
    if case.name.startswith("one_cell"):
        assert all(n == 1 for n in nc), (case.name, nc)
    # bounded walk
    rings, _ = case.walk()
    info["rings"] = float(rings.max()) if len(rings) else 0.0
    assert info["rings"] <= WALK_LIMIT[dim], (case.name, info["rings"])
    if case.ref:
        q = case.queries if case.regionfit else case.cloud
        usable = ~np.isnan(q[:, :dim]).any(axis=1)
        info["ref_queries"] = int((usable & ~res["knn"]).sum())
        if not case.regionfit:
            with np.errstate(invalid="ignore"):
                queried = case.cloud[:, REC[dim]["zncc"]] >= F32(case.threshold)
            assert not res["knn"][queried].any(), case.name   # every queried POI has nmin POIs strictly inside the radius
    if case.ranks is not None:
        assert res["fitted"].any() and set(res["rank"][res["fitted"]]) <= case.ranks, (case.name, set(res["rank"][res["fitted"]]))
    if case.kind == "r_eq":
        # a neighbour at distance exactly r exists for the fitted POIs, and counting it changes the result
        other = case.model(closed=True)
        a, b = written_values(case, res, 1), written_values(case, other, 1)
        both = res["fitted"] & other["fitted"]
        moved = (np.abs(a.astype(np.float64) - b) > 10 * value_bound(res, a, dim)).any(axis=1)
        info["decisive"] = float(moved[both].mean())
        assert both.sum() == res["fitted"].sum() and info["decisive"] >= 0.5, (case.name, info["decisive"])
    if case.kind == "knn_ties":
        assert res["knn"].all(), case.name                    # every query takes the K-nearest path
        other = case.model(tie_descending=True)
        changed = np.array([set(a) != set(b) for a, b in zip(res["sets"], other["sets"])])
        info["decisive"] = float(changed.mean())
        if case.tie_corner_only:
            assert changed.sum() == 8, (case.name, int(changed.sum()))
        if case.tie_quarter:
            assert info["decisive"] >= 0.25, (case.name, info["decisive"])
    return info


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def input_queue(case):
    """The queue an engine is given to write into."""
    return case.queries if case.regionfit else case.cloud


def oracle_result(case, approximation=1, cloud=None):
    """The queue after the oracle's strain2d / strain3d / region_fit (the only use of the oracle in this module: imported here)."""
    import oracle
    cloud = case.cloud if cloud is None else cloud
    if case.regionfit:
        got = case.queries.copy()
        oracle.region_fit(np.ascontiguousarray(cloud), got, case.radius, case.nmin)
        return got
    got = cloud.copy()
    (oracle.strain2d if case.dim == 2 else oracle.strain3d)(got, case.radius, case.nmin, case.threshold, approximation)
    return got


def compare_with_model(case, got, approximation):
    """`got`: the queue after Strain / RegionFit.  The same POIs written (by sentinel), every other float of the record untouched,
    the written values within `value_bound` of the model wherever cond <= 1e6 (at most 2 % of a case's fitted POIs may lie beyond,
    none in a line case).  Returns (worst error, worst error / bound, excluded)."""
    res = case.model()
    L = REC[case.dim]
    src = input_queue(case)
    cols = L["plane"] if case.regionfit else L["strain"]
    rest = np.setdiff1d(np.arange(src.shape[1]), cols + ([L["zncc"]] if case.regionfit else []))
    assert np.array_equal(_bits(got[:, rest]), _bits(src[:, rest])), case.name
    written = (_bits(got[:, cols]) != _bits(src[:, cols])).any(axis=1)
    assert np.array_equal(written, res["fitted"]), (case.name, int(written.sum()), int(res["fitted"].sum()))
    if case.regionfit:
        assert (got[written, L["zncc"]] == 0).all()                # src/oc_region_fit.cpp:162 / :330
        assert np.array_equal(_bits(got[~written, L["zncc"]]), _bits(src[~written, L["zncc"]]))
    if getattr(case, "untouched", False):
        assert not written.any()
    values = written_values(case, res, approximation)
    bound = value_bound(res, values, case.dim, approximation, plane=case.regionfit)
    err = np.abs(got[:, cols].astype(np.float64) - values)
    check = res["fitted"] & (res["cond"] <= 1e6)
    excluded = int((res["fitted"] & ~check).sum())
    assert excluded <= 0.02 * res["fitted"].sum() and (case.ranks is None or excluded == 0), (case.name, excluded)
    if not check.any():
        return 0.0, 0.0, excluded
    ratio = (err / bound)[check]
    assert ratio.max() <= 1.0, (case.name, float(err[check].max()), float(ratio.max()))
    return float(err[check].max()), float(ratio.max()), excluded

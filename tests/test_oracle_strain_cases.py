"""The oracle's Strain / RegionFit against the brute-force float64 model of tests/strain_cases.py on regular grids, exact ties at
the radius and among the K nearest, negative and far coordinates, collinear clouds, capped cell grids, NaN coordinates, both ends
of neighbor_number_min and queue lengths around the block sizes.  The oracle's radius search walks the same 3 x 3 (x 3) cell block as
the HIP kernels, so a neighbour that rule loses is lost by both; the model has no grid.

Checked per case, with approximation 1 and 2: the same POIs written (by sentinel), every other float of the record bit-identical
to the input, the values of every fitted POI of full or of the documented reduced rank within
16 cond^2 2^-53 max(|g|, 1) + 2 spacing(float32(|value|)) (Green strains: through their polynomial, strain_cases.value_bound; no floor).
The builder conditions (decisive, cap active, bounded walk) are asserted by strain_cases.verify_case before anything is compared.
Each case prints its worst error / bound; the table is in DESIGN.md section 3.
"""
import numpy as np
import pytest

import strain_cases as sc


@pytest.mark.parametrize("case", sc.all_cases(), ids=repr)
def test_oracle_equals_the_brute_force_model(case):
    info = sc.verify_case(case)
    for approximation in ((1,) if case.regionfit else (1, 2)):
        err, ratio, excluded = sc.compare_with_model(case, sc.oracle_result(case, approximation), approximation)
        print("%-46s approx %d: fitted %4d, knn %4d, rings %4.1f, decisive %s, max error %.2e, error / bound %.3f, excluded %d"
              % (case.name, approximation, info["fitted"], info["knn"], info["rings"],
                 "%.2f" % info["decisive"] if "decisive" in info else "   -", err, ratio, excluded))


def test_the_cases_cover_what_they_claim():
    cases = sc.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for family in ("grid_r_eq_k_spacing", "grid_knn_ties-", "grid_knn_ties_gated", "negative_coordinates", "far_offset", "lines", "cell_cap",
                   "one_cell", "nan_coordinates", "k_limits", "block_edges", "regionfit_"):
        assert {c.dim for c in cases if c.name.startswith(family)} == {2, 3}, family
    by = {c.name: c for c in cases}
    # queue order is never spatial order
    for c in cases:
        if len(c.cloud) > 8 and "coincident" not in c.name and not c.name.startswith("regionfit_cloud_of"):
            x = c.cloud[:, :c.dim]
            x = x[~np.isnan(x).any(axis=1)]
            assert not np.array_equal(x, x[np.lexsort(x.T[::-1])]) and not np.array_equal(x, x[np.lexsort(x.T)]), c.name
    # the gated tie case filters tied candidates and leaves some gated-in POIs untouched; the NaN cases leave their NaN POIs alone
    c = by["grid_knn_ties_gated-2d-s10-r_eq-K6"]
    res = c.model()
    good = c.cloud[:, sc.REC[2]["zncc"]] >= 0.9
    assert 0.1 < (good & ~res["fitted"]).mean() and (good & res["fitted"]).mean() > 0.1
    for dim in (2, 3):
        c = by["nan_coordinates-%dd" % dim]
        bad = np.isnan(c.cloud[:, :dim]).any(axis=1)
        assert bad.sum() >= 2 * dim and not c.model()["fitted"][bad].any() and c.model()["fitted"][~bad].mean() > 0.9
        q = by["regionfit_grid-%dd" % dim]
        bad = np.isnan(q.queries[:, :dim]).any(axis=1)
        assert bad.sum() >= 3 and not q.model()["fitted"][bad].any() and q.model()["fitted"][~bad].all()
    # k_limits: all on the K-nearest path / none; block_edges: below K nothing is written
    assert by["k_limits-2d-nmin64-all_knn"].model()["knn"].all() and not by["k_limits-2d-nmin64-all_inside"].model()["knn"].any()
    assert by["k_limits-3d-nmin64-all_knn"].model()["knn"].all() and not by["k_limits-3d-nmin64-all_inside"].model()["knn"].any()
    assert {1, 2, 3} <= set(by["k_limits-2d-nmin1-r3"].model()["rank"])
    for n in (1, 63):
        assert not by["block_edges-2d-n%d" % n].model()["fitted"].any()
    assert by["block_edges-2d-n64"].model()["fitted"].all()
    # RegionFit queries exactly one radius from a node exist, and some queries lie outside the cloud's bounding box
    for dim in (2, 3):
        c = by["regionfit_grid-%dd" % dim]
        d = sc.distances(np.ascontiguousarray(c.queries[:, :dim]), np.ascontiguousarray(c.cloud[:, :dim]))
        r2 = np.float32(c.radius) * np.float32(c.radius)
        assert ((d == r2).any(axis=1)).sum() >= 60
        x, q = c.cloud[:, :dim], c.queries[:, :dim]
        with np.errstate(invalid="ignore"):
            assert ((q < x.min(axis=0)) | (q > x.max(axis=0))).any(axis=1).sum() >= 100

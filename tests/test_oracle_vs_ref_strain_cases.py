"""The oracle's Strain / RegionFit against the REFERENCE's own sources (oracle/_ref, see tests/test_oracle_vs_ref_strain.py) on the
cases of tests/strain_cases.py where the reference is deterministic: every queried POI has at least neighbor_number_min POIs
strictly inside the radius -- regular grids with neighbours at distance exactly r, negative and far coordinates, a cloud in one
cell, the radius variants of the capped grids, and the RegionFit queries of those clouds that stay on the radius path.  Left out:
the K-nearest ties and the collinear clouds, which nanoflann's traversal and Eigen's column pivoting decide (that file's
docstring).  Bars as there, unchanged: identical written sets, every other float untouched, 1e-6 on strains and fitted gradients,
1e-5 on fitted displacements.  The comparisons are skipped where the reference tree is not mounted.
"""
import numpy as np
import pytest

import oracle
from oracle import ref as oref

import strain_cases as sc

needs_reference = pytest.mark.skipif(not oref.available(), reason="reference tree not mounted: oracle/_ref cannot be built")


def compare(got, want, cols, tol):
    """The bar of tests/test_oracle_vs_ref_strain.py: `cols` may differ by `tol`, every other float is bit-identical."""
    rest = np.setdiff1d(np.arange(got.shape[1]), cols)
    assert np.array_equal(sc._bits(got[:, rest]), sc._bits(want[:, rest]))
    d = np.abs(got[:, cols].astype(np.float64) - want[:, cols].astype(np.float64))
    assert d.max() <= tol, d.max()
    return d.max()

REF_CASES = [c for c in sc.all_cases() if c.ref]


def test_the_deterministic_families_are_all_here():
    names = [c.name for c in REF_CASES]
    for family in ("grid_r_eq_k_spacing", "negative_coordinates", "far_offset", "one_cell", "cell_cap_2d", "cell_cap_3d", "regionfit_"):
        assert any(n.startswith(family) for n in names), family
    assert not any(n.startswith(("grid_knn_ties", "lines", "regionfit_line")) for n in names)


@needs_reference
@pytest.mark.parametrize("case", [c for c in REF_CASES if not c.regionfit], ids=repr)
def test_strain_matches_the_reference_sources(case):
    L = sc.REC[case.dim]
    assert not case.model()["knn"][case.cloud[:, L["zncc"]] >= np.float32(case.threshold)].any()
    for approximation in (1, 2):
        want = case.cloud.copy()
        oref.strain(want, case.radius, case.nmin, case.threshold, approximation)
        got = sc.oracle_result(case, approximation)
        written_ref = (want[:, L["strain"]] != sc.SENTINEL).any(axis=1)
        written = (got[:, L["strain"]] != sc.SENTINEL).any(axis=1)
        assert np.array_equal(written, written_ref) and written.sum() >= 0.99 * len(want) - 4
        print("%-46s approx %d: max |oracle - reference| %.2e" % (case.name, approximation, compare(got, want, L["strain"], 1e-6)))


@needs_reference
@pytest.mark.parametrize("case", [c for c in REF_CASES if c.regionfit], ids=repr)
def test_region_fit_matches_the_reference_sources(case):
    L = sc.REC[case.dim]
    res = case.model()
    # the radius path (no tie among the K nearest decides) and a fit of full rank: a query below a face of a 3D lattice sees one
    # layer of POIs, a constant dz column, and what Eigen's pivoting makes of it
    keep = ~res["knn"] & ~np.isnan(case.queries[:, :case.dim]).any(axis=1) & (res["rank"] == case.dim + 1)
    assert keep.sum() >= 200 and res["fitted"][keep].all()
    q = np.ascontiguousarray(case.queries[keep])
    want, got = q.copy(), q.copy()
    oref.region_fit(case.cloud, want, case.radius, case.nmin)
    oracle.region_fit(case.cloud, got, case.radius, case.nmin)
    assert np.array_equal(got[:, L["zncc"]] == 0.0, want[:, L["zncc"]] == 0.0) and (got[:, L["zncc"]] == 0.0).all()
    d = compare(got, want, L["plane"] + [L["zncc"]], 1e-5)
    D = case.dim + 1
    grads = [c for j, c in enumerate(L["plane"]) if j % D]
    dg = np.abs(got[:, grads].astype(np.float64) - want[:, grads]).max()
    print("%-46s max |oracle - reference| %.2e, gradients %.2e" % (case.name, d, dg))
    assert dg <= 1e-6

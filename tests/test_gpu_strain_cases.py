"""Strain / RegionFit on the GPU over the cases of tests/strain_cases.py: regular grids with neighbours at distance exactly r, ties
among the K nearest in shuffled queues (the `d == bd && idx < bi` insertion of strain_knn_kernel), negative coordinates (the
ordered-uint bounding box), collinear and coincident clouds (the dead pivot), the cell cap of strain_make_grid, NaN coordinates,
neighbor_number_min = 1 and 64, queue lengths around the 256- and 64-thread blocks, a cloud in one cell, a cloud smaller than K.

Bar: bit-identical to the oracle over the whole record, which tests/test_oracle_strain_cases.py pins to a brute-force float64
model on the same cases.  No case holds a far isolated query: strain_cases.verify_case bounds the ring walk of the K-nearest
kernel for every query of every case before anything runs here.
"""
import numpy as np
import pytest

import strain_cases as sc
import stereo_numpy as sn

pytestmark = pytest.mark.gpu

_WANT = {}


def want(case, approximation=1):
    """The oracle's result, computed once per (case, approximation) and never modified."""
    key = (case.name, 1 if case.regionfit else approximation)
    if key not in _WANT:
        sc.verify_case(case)
        _WANT[key] = sc.oracle_result(case, approximation)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def assert_same_record_bits(got, expect, src, what):
    """Bit-identical over the whole record; a NaN may differ in sign or payload only where the input held a NaN."""
    g, w = sc._bits(got), sc._bits(expect)
    ok = (g == w) | (np.isnan(got) & np.isnan(expect) & np.isnan(src))
    bad = np.argwhere(~ok)
    assert bad.size == 0, "%s: %d floats differ, first %s: %r vs %r" % (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], expect[tuple(bad[0])])


def run_engine(case, approximation, device, cloud=None, engine=None):
    """Strain / RegionFit through the Python classes, from host arrays or from device tensors on the current torch stream."""
    import torch
    import opencorr_amd as eng
    cloud = case.cloud if cloud is None else cloud

    def put(a):
        return torch.from_numpy(a.copy()).cuda() if device else a.copy()

    def fetch(t):
        if device:
            torch.cuda.synchronize()
            return t.cpu().numpy()
        return t

    e = engine
    if case.regionfit:
        e = e or eng.RegionFit(case.radius, case.nmin)
        if device:
            e.set_stream(torch.cuda.current_stream().cuda_stream)
        c, q = put(cloud), put(case.queries)
        e.set_neighbor(c)
        e.prepare()
        e.compute(q)
        out = fetch(q)
    else:
        if e is None:
            e = eng.Strain(case.radius, case.nmin)
        else:
            e.set_subregion_radius(case.radius)
            e.set_neighbor_min(case.nmin)
        e.set_zncc_threshold(case.threshold)
        e.set_approximation(approximation)
        if device:
            e.set_stream(torch.cuda.current_stream().cuda_stream)
        p = put(cloud)
        e.prepare(p)
        e.compute(p)
        out = fetch(p)
    if engine is None:
        e.close()
    return out


@pytest.mark.parametrize("case", sc.all_cases(), ids=repr)
def test_bit_identical_to_the_oracle_from_host_and_device_queues(case):
    for approximation in ((1,) if case.regionfit else (1, 2)):
        expect = want(case, approximation)
        for device in (False, True):
            got = run_engine(case, approximation, device)
            assert_same_record_bits(got, expect, sc.input_queue(case), "%s, approximation %d, %s queue" % (case.name, approximation, "device" if device else "host"))


@pytest.mark.parametrize("names", [("cell_cap_2d-r0.3", "grid_knn_ties-2d-s10-r_eq-K6", "k_limits-2d-nmin64-all_knn", "block_edges-2d-n63", "lines-2d-diagonal"),
                                   ("cell_cap_3d-r0.6", "grid_knn_ties-3d-s8-r_eq-K8", "block_edges-3d-n257", "nan_coordinates-2d", "one_cell-3d")],
                         ids=["2d", "3d_then_2d"])
def test_one_strain_handle_prepared_on_one_case_then_on_another(names):
    """Cell tables (16.8 million cells, then a few dozen), the list and counter of the K-nearest path and the record buffer of one
    handle serve queues of other sizes, radii, K and dimensions in turn; nothing of the earlier queue may show."""
    import opencorr_amd as eng
    st = eng.Strain(1.0, 5)
    for device in (False, True):
        for name in names:
            case = sc.case_by_name(name)
            expect = want(case, 1)
            got = run_engine(case, 1, device, engine=st)
            assert_same_record_bits(got, expect, case.cloud, "%s on a reused handle" % name)
    st.close()


@pytest.mark.parametrize("names", [("regionfit_cap-2d", "regionfit_grid-2d", "regionfit_cloud_of_K-1-2d", "regionfit_line-2d"),
                                   ("regionfit_cap-3d", "regionfit_grid-3d", "regionfit_cloud_of_K-1-3d", "regionfit_negative-3d")], ids=["2d", "3d"])
def test_one_region_fit_handle_prepared_on_one_cloud_then_on_another(names):
    import opencorr_amd as eng
    rf = eng.RegionFit(1.0, 5)
    for name in names:
        case = sc.case_by_name(name)
        rf.set_search_radius(case.radius)
        rf.set_neighbor_min(case.nmin)
        expect = want(case)
        got = run_engine(case, 1, False, engine=rf)
        assert_same_record_bits(got, expect, case.queries, "%s on a reused handle" % name)
    rf.close()


@pytest.mark.parametrize("name", ["grid_knn_ties_gated-2d-s10-r_eq-K6", "cell_cap_2d-r0.3", "k_limits-3d-nmin64-all_knn", "nan_coordinates-3d"])
def test_compute_twice_on_one_prepared_queue_with_other_displacements(name):
    """prepare() once; the second compute() sees other displacements (and, sharing the K-nearest list, the same fallbacks)."""
    import opencorr_amd as eng
    case = sc.case_by_name(name)
    L = sc.REC[case.dim]
    second = case.cloud.copy()
    rng = np.random.default_rng(7)
    for k in ["u", "v", "w"][:case.dim]:
        second[:, L[k]] = (-1.5 * second[:, L[k]] + rng.normal(0, 0.02, len(second))).astype(np.float32)
    expect1, expect2 = want(case, 1), sc.oracle_result(case, 1, cloud=second)
    st = eng.Strain(case.radius, case.nmin)
    st.prepare(case.cloud)
    got1 = st.compute(case.cloud.copy())
    got2 = st.compute(second.copy())
    got1b = st.compute(case.cloud.copy())
    st.close()
    assert_same_record_bits(got1, expect1, case.cloud, name + ", first compute")
    assert_same_record_bits(got2, expect2, second, name + ", second compute")
    assert_same_record_bits(got1b, expect1, case.cloud, name + ", first queue again")
    assert not np.array_equal(sc._bits(got1[:, L["strain"]]), sc._bits(got2[:, L["strain"]]))


def _poi2ds_queue(xy, seed):
    """POI2DS records over image positions xy: ref_coor a smooth surface plus jitter, u v w an affine field of it plus noise."""
    rng = np.random.default_rng(seed)
    n = len(xy)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    cx, cy = x.mean(), y.mean()
    ref = np.stack([0.05 * (x - cx), 0.05 * (y - cy), 40 + 2e-4 * ((x - cx) ** 2 - (y - cy) ** 2)], axis=1) + rng.normal(0, 0.01, (n, 3))
    G = np.array([[0.010, 0.003, -0.002], [0.002, -0.005, 0.004], [-0.003, 0.001, 0.006]])
    q = np.zeros((n, 28), dtype=np.float32)
    q[:, 0:2] = xy
    q[:, 14:17] = ref
    q[:, 2:5] = (ref.astype(np.float32).astype(np.float64) - ref.mean(axis=0)) @ G.T + rng.normal(0, 2e-4, (n, 3))
    q[:, 5:8] = 0.99
    q[:, 20:26] = -7.5
    q[:, 26:28] = 16
    return q


@pytest.mark.parametrize("name", ["grid_r_eq_k_spacing-2d-s10-r30", "grid_knn_ties-2d-s10-r_eq-K6"])
def test_poi2ds_on_the_tie_cases(name):
    """The stereo record over the two tie grids (neighbours over (x, y), shuffled queue) against stereo_numpy.strain_poi2ds with the
    tolerance of test_strain_poi2ds_sparse_cloud_takes_the_k_nearest_path."""
    import opencorr_amd as eng
    case = sc.case_by_name(name)
    q = _poi2ds_queue(case.cloud[:, :2], 11)
    expect = sn.strain_poi2ds(q[:, 0:2], q[:, 14:17], q[:, 2:5], q[:, 5:8], case.radius, case.nmin, 0.9, 1)
    assert expect["fitted"].all() and expect["knn"].all() == (case.kind == "knn_ties") and expect["knn"].any() == (case.kind == "knn_ties")
    # the case is decisive for this record too: with the tie broken the other way (r_eq: with `<=`) other rows enter the fit
    other = sc.neighbour_sets(q[:, 0:2].copy(), q[:, 0:2].copy(), case.radius, case.nmin, closed=case.kind == "r_eq", tie_descending=case.kind == "knn_ties")[0]
    mine = sc.neighbour_sets(q[:, 0:2].copy(), q[:, 0:2].copy(), case.radius, case.nmin)[0]
    assert np.mean([set(a) != set(b) for a, b in zip(mine, other)]) >= 0.5
    st = eng.Strain(case.radius, case.nmin)
    got = q.copy()
    st.prepare(got)
    st.compute(got)
    st.close()
    assert np.array_equal(sc._bits(got[:, :20]), sc._bits(q[:, :20])) and (got[:, 26:28] == 16).all()
    assert (got[:, 20:26] != np.float32(-7.5)).all()
    g = np.abs(expect["grad"]).max(axis=1)
    tol = np.maximum(1e-6, 16 * expect["cond"] ** 2 * 2.0 ** -53 * np.maximum(g, 1.0)) + np.spacing(np.float32(np.maximum(g, 1e-30)))
    err = np.abs(got[:, 20:26].astype(np.float64) - expect["strain"]).max(axis=1)
    print("%s as POI2DS: cond max %.3g, max error %.3g, max error / bound %.3g" % (name, expect["cond"].max(), err.max(), (err / tol).max()))
    assert (err <= tol).all()


def test_neighbor_min_at_the_limit_of_the_k_nearest_path():
    import opencorr_amd as eng
    st = eng.Strain(10.0, 5)
    st.set_neighbor_min(64)
    with pytest.raises(eng.capi.OpenCorrHipError):
        st.set_neighbor_min(65)
    st.close()
    rf = eng.RegionFit(10.0, 64)
    with pytest.raises(eng.capi.OpenCorrHipError):
        rf.set_neighbor_min(65)
    with pytest.raises(eng.capi.OpenCorrHipError):
        eng.Strain(10.0, 65)
    rf.close()

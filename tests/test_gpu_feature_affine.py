"""FeatureAffine2D/3D on the GPU (opencorr_amd/csrc/feature_affine.hip) == the CPU twin (tests/cpp/feature_affine_twin.cpp) in every
bit of every record, and the recovery of a planted affine field.  The twin itself is held against an independent float64 model
in tests/test_feature_affine_twin_cpu.py.

The fixture of the candidate counts has more than the 2 000 keypoints the other fixtures stay below: a POI with about 3 000
candidates needs that many keypoints around it."""
import ctypes

import numpy as np
import pytest

import feature_affine_cases as cases
import feature_affine_model as model
import feature_affine_twin as twin

pytestmark = pytest.mark.gpu

NOISY_SEEDS = {2: 2001, 3: 3001}   # the seeds of tests/test_feature_affine_twin_cpu.py


def _engine(case, seed=0, **over):
    import opencorr_amd as oc
    ndim = case["ndim"]
    subset = case.get("subset", (8, 8, 8)[:ndim])
    e = oc.FeatureAffine2D(*subset) if ndim == 2 else oc.FeatureAffine3D(*subset)
    d = dict(twin.DEFAULTS[ndim], threshold=case["threshold"])
    d.update(over)
    e.set_search(case["radius"], d["nmin"])
    e.set_ransac_config(d["trials"], d["samples"], d["threshold"])
    e.set_seed(seed)
    return e


def _gpu(case, seed=0, device_queue=False, pois=None, adaptive=None, **over):
    e = _engine(case, seed, **over)
    if adaptive:
        e.set_subset_adjustment(adaptive[0], adaptive[1])
        e.set_images(adaptive[3], adaptive[2])
        e.set_self_adaptive(True)
    e.set_keypoint_pair(case["ref"], case["tar"])
    e.prepare()
    q = np.array(case["pois"] if pois is None else pois, np.float32, order="C")
    if device_queue:
        import torch
        t = torch.from_numpy(q).cuda()
        e.compute(t)
        e.synchronize()
        q = t.cpu().numpy()
    else:
        e.compute(q)
    e.close()
    return q


def _twin(case, seed=0, pois=None, adaptive=None, **over):
    return twin.compute(case["ref"], case["tar"], case["pois"] if pois is None else pois, case["radius"], seed=seed, adaptive=adaptive,
                        **dict(dict(threshold=case["threshold"]), **over))


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
    rows = np.nonzero((a != b).any(axis=1))[0]
    assert rows.size == 0, "%s: %d records differ, first %d: columns %s" % (what, rows.size, rows[0], np.nonzero(a[rows[0]] != b[rows[0]])[0])


def _noisy(ndim, **kw):
    return cases.noisy(ndim, NOISY_SEEDS[ndim], **kw)


@pytest.mark.parametrize("ndim", [2, 3])
def test_candidate_counts_at_wave_and_list_boundaries(ndim):
    """0, s-1, s, neighbor_min-1, neighbor_min, 63, 64, 65, 129, 1025 (one past the LDS part of the list) and 3000 candidates"""
    d = twin.DEFAULTS[ndim]
    wanted = [0, d["samples"] - 1, d["samples"], d["nmin"] - 1, d["nmin"], 63, 64, 65, 129, 1025, 3000]
    case = cases.counts(ndim, wanted)
    expect = _twin(case)
    z, f = cases.ZNCC[ndim], cases.FEATURE[ndim]
    assert list(expect[:2, z]) == [-1, -1] and (expect[2:, z] == 0).all()
    assert expect[9, f] > 700 and expect[10, f] > 2000   # (four fifths of the candidates are planted inliers)
    _same(_gpu(case), expect, "counts %dD" % ndim)


@pytest.mark.parametrize("ndim", [2, 3])
def test_noisy_field_host_and_device_queues(ndim):
    case = _noisy(ndim)
    expect = _twin(case)
    it = expect[:, cases.ITER[ndim]]
    assert (it > 1).any() and (expect[:, cases.ZNCC[ndim]] == 0).all()
    _same(_gpu(case), expect, "host queue")
    _same(_gpu(case, device_queue=True), expect, "device queue")


@pytest.mark.parametrize("ndim", [2, 3])
def test_exact_field_exits_at_trial_one_with_ties_fallback_and_isolated_pois(ndim):
    for case in (cases.exact(ndim), cases.ties(ndim)):
        expect = _twin(case)
        ok = expect[:, cases.ZNCC[ndim]] == 0
        assert (expect[ok, cases.ITER[ndim]] == 1).sum() >= 10 and (expect[-4:, cases.ZNCC[ndim]] == -1).all()
        assert (expect[ok, cases.FEATURE[ndim]] <= twin.DEFAULTS[ndim]["nmin"]).any(), "the KNN fallback"
        _same(_gpu(case), expect, "exact %dD" % ndim)


@pytest.mark.parametrize("ndim", [2, 3])
def test_outlier_heavy_field_runs_to_trial_number(ndim):
    case = _noisy(ndim, outliers=0.8, n_poi=64)
    expect = _twin(case)
    assert (expect[:, cases.ITER[ndim]] == twin.DEFAULTS[ndim]["trials"]).sum() >= 8
    _same(_gpu(case), expect, "outlier-heavy %dD" % ndim)


@pytest.mark.parametrize("ndim", [2, 3])
def test_collinear_keypoints_and_isolated_poi(ndim):
    case = cases.collinear(ndim)
    got = _gpu(case)
    assert list(got[:, cases.ZNCC[ndim]]) == [-2, -1]
    _same(got, _twin(case), "collinear %dD" % ndim)
    untouched = np.delete(np.arange(got.shape[1]), cases.ZNCC[ndim])
    assert np.array_equal(got[1, untouched], case["pois"][1, untouched])


@pytest.mark.parametrize("ndim", [2, 3])
def test_six_samples(ndim):
    case = _noisy(ndim, n_poi=64)
    _same(_gpu(case, samples=6), _twin(case, samples=6), "sample_number 6")


def test_self_adaptive_subsets():
    """both branches of src/oc_feature_affine.cpp:160-173 and the radius floor"""
    case = _noisy(2)
    # some POIs outside the cloud, two of them far: their nearest keypoints lie to one side, so the POI moves to the box's centre
    pois = np.concatenate([case["pois"][:96], cases.queue(np.array([[-30.0, 50.0], [230.0, 240.0], [100.0, -25.0], [5000.0, -3000.0], [100.0, 1e6]], np.float32))])
    for adaptive in ((14, 10, 200, 200), (30, 6, 200, 200)):
        expect = _twin(case, pois=pois, adaptive=adaptive)
        moved = (expect[:, 0] != pois[:, 0]) | (expect[:, 1] != pois[:, 1])
        assert moved.any() and not moved.all()
        if adaptive[1] == 10:
            assert (expect[:, 23] == 10).any() and (expect[:, 23] > 10).any()
        _same(_gpu(case, pois=pois, adaptive=adaptive), expect, "self-adaptive %s" % (adaptive,))


@pytest.mark.parametrize("ndim", [2, 3])
def test_records_do_not_depend_on_the_queue_the_run_or_the_other_pois(ndim):
    case = _noisy(ndim, n_poi=128)
    whole = _gpu(case)
    _same(_gpu(case), whole, "second run")
    _same(_gpu(case, pois=case["pois"][::-1])[::-1], whole, "reversed queue")
    halves = np.concatenate([_gpu(case, pois=case["pois"][:50]), _gpu(case, pois=case["pois"][50:])])
    _same(halves, whole, "queue split in two")
    other = _gpu(case, seed=12345)
    _same(other, _twin(case, seed=12345), "seed 12345")
    assert (other[:, cases.ITER[ndim]] != whole[:, cases.ITER[ndim]]).any(), "two seeds, one sequence of samples"


def test_matched_pairs_gathered_on_the_device():
    import torch
    case = _noisy(3, n_poi=64)
    rng = np.random.default_rng(5)
    n = case["ref"].shape[0]
    ref_idx = rng.permutation(3 * n)[:n].astype(np.int32)
    tar_idx = rng.permutation(2 * n)[:n].astype(np.int32)
    ref_kp = rng.random((3 * n, 3)).astype(np.float32)
    tar_kp = rng.random((2 * n, 3)).astype(np.float32)
    ref_kp[ref_idx], tar_kp[tar_idx] = case["ref"], case["tar"]
    e = _engine(case)
    e.set_matched_pairs(torch.from_numpy(ref_kp).cuda(), torch.from_numpy(tar_kp).cuda(), torch.from_numpy(ref_idx).cuda(),
                        torch.from_numpy(tar_idx).cuda())
    e.prepare()
    q = case["pois"].copy()
    e.compute(q)
    _same(q, _gpu(case), "set_matched against set_keypoints")


def test_refusals_leave_the_queue_untouched():
    import opencorr_amd as oc
    from opencorr_amd import capi
    L = capi.lib()

    case = _noisy(3, n_poi=16)
    e = _engine(case)
    h = e._h
    assert L.oc_hip_feature_affine_set_ransac(h, 32, 3, 3.2) == capi.ERR_UNSUPPORTED      # sample_number below ndim + 1
    assert L.oc_hip_feature_affine_set_ransac(h, 32, 9, 3.2) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_feature_affine_set_ransac(h, 0, 4, 3.2) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_feature_affine_set_ransac(h, 1025, 4, 3.2) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_feature_affine_set_search(h, 10.0, 65) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_feature_affine_set_self_adaptive(h, 1, 14, 10, 100, 100) == capi.ERR_UNSUPPORTED   # 3D has none
    assert L.oc_hip_set_tuning(h, b"arith_fma", 1) == capi.ERR_UNSUPPORTED
    dev = (ctypes.c_int * 1)(0)
    assert L.oc_hip_set_devices(h, dev, 1) == capi.ERR_UNSUPPORTED
    handles = (ctypes.c_void_p * 1)(h)
    assert L.oc_hip_compute_chain(handles, 1, None, 0, 124, capi.HOST) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_compute(h, None, 0, 124, capi.HOST) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_set_images3d(h, None, None, 32, 32, 32, capi.HOST) == capi.ERR_UNSUPPORTED
    e2 = oc.FeatureAffine2D(16, 16)
    assert L.oc_hip_set_images2d(e2._h, None, None, 32, 32, capi.ROW_MAJOR, capi.HOST) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_feature_affine_set_self_adaptive(e2._h, 1, 65, 10, 100, 100) == capi.ERR_UNSUPPORTED
    q = case["pois"].copy()
    p = ctypes.c_void_p(q.ctypes.data)
    assert L.oc_hip_feature_affine_compute(h, p, q.shape[0], q.strides[0], capi.HOST) == capi.ERR_INVALID   # no prepare yet
    e.set_keypoint_pair(case["ref"], case["tar"])
    e.prepare()
    # 2^31 keypoints: refused before a pointer is looked at; the prepared state stays (the run below is the untouched engine's)
    dummy = ctypes.c_void_p(q.ctypes.data)
    assert L.oc_hip_feature_affine_set_keypoints(h, dummy, dummy, 2 ** 31, capi.HOST) == capi.ERR_UNSUPPORTED
    assert L.oc_hip_feature_affine_set_matched(h, dummy, dummy, dummy, dummy, 2 ** 31, capi.DEVICE) == capi.ERR_UNSUPPORTED
    assert np.array_equal(q, case["pois"])
    assert L.oc_hip_feature_affine_compute(h, p, q.shape[0], q.strides[0], capi.HOST) == capi.OK
    _same(q, _twin(case), "after the refused keypoint lists")
    q[:] = case["pois"]
    q[3, 1] = np.nan
    before = q.copy()
    assert L.oc_hip_feature_affine_compute(h, p, q.shape[0], q.strides[0], capi.HOST) == capi.ERR_INVALID
    assert b"POI 3" in L.oc_hip_last_error()
    assert np.array_equal(q.view(np.uint32), before.view(np.uint32))
    # more than 16384 keypoints inside the radius of POI 1
    rng = np.random.default_rng(9)
    ref = np.concatenate([case["ref"], (30.0 + rng.random((16500, 3))).astype(np.float32)])
    e.set_keypoint_pair(ref, ref)
    e.prepare()
    q = cases.queue(np.array([[5.0, 5.0, 5.0], [30.5, 30.5, 30.5]], np.float32))
    before = q.copy()
    assert L.oc_hip_feature_affine_compute(h, ctypes.c_void_p(q.ctypes.data), 2, q.strides[0], capi.HOST) == capi.ERR_UNSUPPORTED
    assert b"POI 1" in L.oc_hip_last_error()
    assert np.array_equal(q, before)


def test_matched_pairs_with_a_negative_index_are_refused():
    import torch
    from opencorr_amd import capi
    case = _noisy(3, n_poi=4)
    e = _engine(case)
    kp = torch.from_numpy(case["ref"]).cuda()
    idx = torch.arange(64, dtype=torch.int32).cuda()
    bad = idx.clone()
    bad[17] = -1
    with pytest.raises(capi.OpenCorrHipError) as err:
        e.set_matched_pairs(kp, kp, idx, bad)
    assert err.value.status == capi.ERR_INVALID and "pair 17" in str(err.value)
    with pytest.raises(capi.OpenCorrHipError):
        e.prepare()   # the engine holds no keypoints
    e.set_matched_pairs(kp, kp, idx, idx)
    e.prepare()


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_list_of_16384_candidates_works(ndim):
    """the largest candidate count: identical bits with the list's tail in the global slice"""
    rng = np.random.default_rng(31 + ndim)
    ref = (20.0 + rng.random((16384, ndim)) * 4.0).astype(np.float32)
    M, t = cases.field(ndim)
    tar = cases.apply(M, t, ref) + (rng.standard_normal(ref.shape) * 0.1).astype(np.float32)
    case = dict(ref=ref, tar=tar, pois=cases.queue(np.full((1, ndim), 22.0, np.float32)), radius=10.0, threshold=twin.DEFAULTS[ndim]["threshold"],
                ndim=ndim)
    expect = _twin(case)
    assert expect[0, cases.FEATURE[ndim]] > 16000
    _same(_gpu(case), expect, "16384 candidates")


@pytest.mark.parametrize("ndim", [2, 3])
def test_planted_field_is_recovered(ndim):
    """30 % of the pairs displaced by at least 10 x threshold: at least 99 % of the POIs with enough neighbours report exactly
    the planted inliers among their candidates, and their deformation is the model's fit on those inliers within the bar of
    tests/test_feature_affine_twin_cpu.py (cases.BAR = 2.96e-5, 4 x the float32-QR distance measured there).

    The fixture was chosen with the twin on the CPU and is NOT the `noisy` fixture of the other tests: noise 0.01 per axis
    (theirs: 0.1), 2 000 keypoints in 2D and 1 000 in 3D, seed 11, and neighbor_number_min = 16 in both dimensions (the 2D default
    is 7).  The property is one of the reference's exit rule, which ends the loop on the first trial with a small mean error once
    some set reached neighbor_number_min, whether or not that set is the planted one: a sample of two planted pairs and a
    displaced one fits the pairs near the line through the two, and with noise a sample of close pairs extrapolates badly.  What
    the twin recovers elsewhere (seeds 11, 12, 13, 2001): about 88 - 90 % at noise 0.1 with neighbor_number_min
    16, about 91 % at noise 0.01 with the 2D default of 7, 241 of 249 in 3D with seed 2001."""
    case = cases.noisy(ndim, 11, sigma=0.01, n_kp=2000 if ndim == 2 else 1000)
    nmin = 16
    got = _gpu(case, nmin=nmin)
    r2 = np.float32(case["radius"]) * np.float32(case["radius"])
    enough = hit = 0
    for row, poi in zip(got, case["pois"]):
        p = poi[:ndim]
        inside = model._dist2(p, case["ref"]) < r2
        if inside.sum() < nmin:
            continue
        enough += 1
        planted = inside & case["planted"]
        if row[cases.ZNCC[ndim]] != 0 or row[cases.FEATURE[ndim]] != planted.sum():
            continue
        X = model._fit((case["ref"][planted] - p).astype(np.float64), (case["tar"][planted] - p).astype(np.float64))
        if np.abs(row[cases.DEFORMATION[ndim]] - model.deformation(X, ndim)).max() <= cases.BAR:
            hit += 1
    print("recovered %d of %d POIs with enough neighbours" % (hit, enough))
    assert enough >= 200 and hit >= 0.99 * enough

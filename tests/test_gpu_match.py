"""The descriptor matcher on the GPU (opencorr_amd/csrc/match.hip) == its CPU restatement (tests/cpp/match_twin.cpp), bit for bit,
in both arithmetic modes: matched_idx, best_sq and second_sq as raw bits and both pair lists.  The twin is the reference's
sequential scan; the kernel folds tiles, threads and candidate parts under the lexicographic (distance, index) order."""
import ctypes

import numpy as np
import pytest

import match_cases as cases
import match_twin as twin

pytestmark = pytest.mark.gpu

QUERIES = (1, 2, 63, 64, 65, 129)       # around the 64-query workgroup
CANDIDATES = (1, 3, 64, 65, 257)        # around the 64-candidate tile
DIMS = (32, 128, 768, 96)               # 128 and 768 have compile-time trip counts, 32 and 96 take the run-time loop


def _matcher(dim, ratio, fma=0, splits=0):
    from opencorr_amd import DescriptorMatcher
    m = DescriptorMatcher(dim, ratio)
    m.set_tuning("arith_fma", fma)
    m.set_tuning("match_splits", splits)
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(m, ref, tar, ratio, fma, what):
    """every output of the matcher `m` (descriptors already set) against the twin"""
    for direction, (q, c) in enumerate(((ref, tar), (tar, ref))):
        idx, best, second = m.nearest(direction)
        t_idx, t_best, t_second, _ = twin.nearest(q, c, ratio, fma)
        assert np.array_equal(idx, t_idx), (what, direction)
        assert np.array_equal(_bits(best), _bits(t_best)), (what, direction)
        assert np.array_equal(_bits(second), _bits(t_second)), (what, direction)
    for mode in (0, 1):
        ri, ti = m.match(mode)
        t_ri, t_ti = twin.pairs(ref, tar, ratio, mode, fma)
        assert np.array_equal(ri, t_ri) and np.array_equal(ti, t_ti), (what, mode)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_equals_twin_around_tile_and_block_edges(dim, fma):
    m = _matcher(dim, 0.85, fma)
    matched = 0
    for nq in QUERIES:
        for nc in CANDIDATES:
            ref, tar = cases.seeded_sets(1000 + nq + nc, nq, nc, dim)
            m.set_descriptors(0, ref)
            m.set_descriptors(1, tar)
            _check(m, ref, tar, 0.85, fma, (nq, nc, dim))
            matched += len(m.match(0)[0])
    assert matched > 100  # (the sets do produce matches)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dim", [128, 768])
def test_candidate_splits_do_not_change_a_bit(dim, fma):
    """65 x 257 with one target row planted at indices 10, 70, 200 and 256 -- in different parts under 2, 3 and 7 splits: exact ties
    for nearest and runner-up across the seams."""
    ref, tar = cases.with_seam_ties(*cases.seeded_sets(5, 65, 257, dim))
    t_idx, t_best, t_second, _ = twin.nearest(ref, tar, 1.25, fma)
    assert t_idx[5] == 10 and t_best[5] == t_second[5]  # the planted tie is the nearest of its source row: lowest index wins
    results = []
    for splits in (1, 2, 3, 7, 0):
        m = _matcher(dim, 1.25, fma, splits)
        m.set_descriptors(0, ref)
        m.set_descriptors(1, tar)
        _check(m, ref, tar, 1.25, fma, ("splits", splits))
        near = m.nearest(0)
        results.append((near[0], _bits(near[1]), _bits(near[2])) + m.match(0) + m.match(1))
        m.set_ratio(0.85)
        _check(m, ref, tar, 0.85, fma, ("splits", splits, 0.85))
    for r in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], r))


@pytest.mark.parametrize("fma", [0, 1])
def test_planted_cases(fma):
    for name, (ref, tar) in cases.planted().items():
        for ratio in cases.RATIOS + (1.25,):
            m = _matcher(32, ratio, fma)
            m.set_descriptors(0, ref)
            m.set_descriptors(1, tar)
            _check(m, ref, tar, ratio, fma, (name, ratio))


def test_device_buffers_user_stream_and_replaced_descriptors():
    import torch
    ref, tar = cases.seeded_sets(8, 129, 257, 128)
    ref2, tar2 = cases.seeded_sets(9, 65, 64, 128)
    stream = torch.cuda.Stream()
    m = _matcher(128, 0.85)
    m.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        d_ref, d_tar = torch.from_numpy(ref).cuda(), torch.from_numpy(tar).cuda()
        m.set_descriptors(0, d_ref)
        m.set_descriptors(1, d_tar)
        idx, best, second = m.nearest(0)
        ri, ti = m.match(0)
        assert idx.is_cuda and ri.is_cuda
        stream.synchronize()
        t_idx, t_best, t_second, _ = twin.nearest(ref, tar, 0.85)
        assert np.array_equal(idx.cpu().numpy(), t_idx)
        assert np.array_equal(_bits(best.cpu().numpy()), _bits(t_best)) and np.array_equal(_bits(second.cpu().numpy()), _bits(t_second))
        t_ri, t_ti = twin.pairs(ref, tar, 0.85, 0)
        assert np.array_equal(ri.cpu().numpy(), t_ri) and np.array_equal(ti.cpu().numpy(), t_ti)
        # the second set replaces the first: one side from the host, one on the device, smaller counts
        d_tar2 = torch.from_numpy(tar2).cuda()
        m.set_descriptors(0, ref2)
        m.set_descriptors(1, d_tar2)
        _check(m, ref2, tar2, 0.85, 0, "replaced")
        # and back to larger host sets
        m.set_descriptors(0, ref)
        m.set_descriptors(1, tar)
        _check(m, ref, tar, 0.85, 0, "replaced again")


def test_refusals():
    from opencorr_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    for dim in (0, 16, 48, 1056, 100, -32):
        assert L.oc_hip_matcher_create(dim, 0.85, 0, ctypes.byref(h)) == capi.ERR_INVALID
        assert not h.value
    assert L.oc_hip_matcher_create(128, float("nan"), 0, ctypes.byref(h)) == capi.ERR_INVALID
    capi.check(L.oc_hip_matcher_create(128, 0.85, 0, ctypes.byref(h)))
    try:
        kind = ctypes.c_int()
        capi.check(L.oc_hip_get_kind(h, ctypes.byref(kind)))
        assert kind.value == capi.MATCHER == 13
        ref, tar = cases.seeded_sets(1, 64, 65, 128)
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)
        capi.check(L.oc_hip_matcher_set_descriptors(h, 0, vp(ref), len(ref), capi.HOST))
        capi.check(L.oc_hip_matcher_set_descriptors(h, 1, vp(tar), len(tar), capi.HOST))
        assert L.oc_hip_matcher_set_descriptors(h, 2, vp(tar), len(tar), capi.HOST) == capi.ERR_INVALID
        want = twin.pairs(ref, tar, 0.85, 0)
        assert len(want[0]) > 4
        # a short capacity: refused, nothing written, n_pairs carries the need
        ri = np.full(64, -7, np.int32)
        ti = np.full(64, -7, np.int32)
        n = ctypes.c_size_t(123)
        assert L.oc_hip_matcher_match(h, 0, vp(ri), vp(ti), len(want[0]) - 1, ctypes.byref(n), capi.HOST) == capi.ERR_INVALID
        assert n.value == len(want[0])
        assert (ri == -7).all() and (ti == -7).all()
        capi.check(L.oc_hip_matcher_match(h, 0, vp(ri), vp(ti), n.value, ctypes.byref(n), capi.HOST))
        assert np.array_equal(ri[:n.value], want[0]) and np.array_equal(ti[:n.value], want[1]) and (ri[n.value:] == -7).all()
        # n_matched, null best / second
        idx = np.empty(64, np.int32)
        nm = ctypes.c_size_t()
        capi.check(L.oc_hip_matcher_nearest(h, 0, vp(idx), None, None, ctypes.byref(nm), capi.HOST))
        assert nm.value == twin.nearest(ref, tar, 0.85)[3] == int((idx >= 0).sum())
        # what a matcher does not do
        two = (ctypes.c_int * 2)(0, 0)
        assert L.oc_hip_set_devices(h, two, 2) == capi.ERR_UNSUPPORTED
        pois = np.zeros((4, 25), np.float32)
        assert L.oc_hip_compute(h, vp(pois), 4, 100, capi.HOST) == capi.ERR_UNSUPPORTED
        assert L.oc_hip_compute_one(h, vp(pois)) == capi.ERR_UNSUPPORTED
        img = np.zeros((16, 16), np.float32)
        assert L.oc_hip_set_images2d(h, vp(img), vp(img), 16, 16, capi.ROW_MAJOR, capi.HOST) == capi.ERR_UNSUPPORTED
        vol = np.zeros((16, 16, 16), np.float32)
        assert L.oc_hip_set_images3d(h, vp(vol), vp(vol), 16, 16, 16, capi.HOST) == capi.ERR_UNSUPPORTED
        assert L.oc_hip_set_tuning(h, b"match_splits", 65) == capi.ERR_INVALID
        assert L.oc_hip_set_tuning(h, b"match_splits", -1) == capi.ERR_INVALID
        # the matcher still works afterwards
        capi.check(L.oc_hip_matcher_match(h, 1, vp(ri), vp(ti), 64, ctypes.byref(n), capi.HOST))
        wb = twin.pairs(ref, tar, 0.85, 1)
        assert np.array_equal(ri[:n.value], wb[0]) and np.array_equal(ti[:n.value], wb[1])
    finally:
        L.oc_hip_destroy(h)
    # match_splits belongs to the matcher alone
    capi.check(L.oc_hip_fftcc2d_create(16, 16, 0, ctypes.byref(h)))
    try:
        assert L.oc_hip_set_tuning(h, b"match_splits", 2) == capi.ERR_UNSUPPORTED
        assert L.oc_hip_matcher_set_ratio(h, 0.5) == capi.ERR_INVALID
    finally:
        L.oc_hip_destroy(h)

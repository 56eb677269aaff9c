"""SIFT3D's orientation and descriptor stages on the GPU (opencorr_amd/csrc/sift3d_features.hip) == their CPU restatement
(tests/cpp/sift3d_features_twin.cpp), bit for bit: the status, the nine sums, every keypoint record and every descriptor row, on the
cases of tests/sift3d_features_cases.py, with both arithmetic modes of the scale space underneath, through explicit host lists and
through the lists that never leave the device.  Then what exact sums promise (the same bits in any order, in any split, on a second
run), the planted volumes and keypoints, the validation table, the hand-over to the matcher and the whole pipeline."""
import ctypes
import functools

import numpy as np
import pytest

import image_domains
import match_twin
import sift3d_features_cases as cases
import sift3d_features_twin as twin
import sift3d_twin

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cases.CASES]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(settings, fma=0):
    from opencorr_amd import SIFT3DScaleSpace
    s = SIFT3DScaleSpace()
    s.set_tuning("arith_fma", fma)
    s.set_config(settings["n_octave_layers"], settings["min_dimension"], settings["alpha"], settings["sigma_source"], settings["sigma_base"])
    s.set_physical_unit(*settings["units"])
    return s


def _built(volume, settings, fma=0):
    s = _engine(settings, fma)
    s.set_volume(volume)
    s.build()
    return s


@functools.lru_cache(maxsize=None)
def _want(name, fma):
    """the twin's whole extraction of a case (every candidate: the lists are short) or of BIG with its planted candidates"""
    if name.startswith("big_"):
        ss = sift3d_twin.scale_space(cases.BIG.volume(), fma=fma, **cases.BIG.settings)
        cand = cases.big_candidates(twin.CANDIDATE, ss.gauss) if name == "big_planted" else cases.cut(ss.candidates)
        return twin.extract(cases.BIG.volume(), cases.BIG.settings, fma=fma, candidates=cand)
    c = cases.CASE_BY_NAME[name]
    return twin.extract(c.volume(), c.settings, fma=fma)


def _case(name):
    return cases.BIG if name.startswith("big_") else cases.CASE_BY_NAME[name]


def _same_orientation(got, want, what):
    kp, status, sums = got
    assert np.array_equal(status, want.status), what
    assert np.array_equal(_bits(sums), _bits(want.sums)), what
    assert kp.tobytes() == want.keypoints.tobytes(), what


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", NAMES + ["big_planted", "big_detected"])
def test_kernel_equals_twin_on_host_lists(name, fma):
    want = _want(name, fma)
    candidates = {"big_planted": lambda: cases.big_candidates(twin.CANDIDATE, want.scale_space.gauss),
                  "big_detected": lambda: cases.cut(want.scale_space.candidates)}.get(name, lambda: want.scale_space.candidates)()
    assert len(candidates) <= cases.MAX_KEYPOINTS and len(want.keypoints) >= 1
    if name == "big_detected":
        assert (want.keypoints["octave"] >= 1).any()
    s = _built(_case(name).volume(), _case(name).settings, fma)
    got = s.orient(candidates, with_status=True)
    _same_orientation(got, want, (name, fma))
    desc = s.describe(got[0])
    assert np.array_equal(_bits(desc), _bits(want.descriptors)), (name, fma)
    s.close()


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_twin_on_device_resident_lists(name, fma):
    """detect, orient(None), describe(None): the candidate list and the keypoints never leave the device"""
    import torch
    want = _want(name, fma)
    s = _built(_case(name).volume(), _case(name).settings, fma)
    assert len(s.detect()) == len(want.status)
    _same_orientation(s.orient(None, with_status=True), want, (name, fma))
    out = torch.full((len(want.keypoints), 768), -7.0, dtype=torch.float32, device="cuda")
    s.describe(None, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want.descriptors)), (name, fma)
    # ... and without a detect in front, as device tensors in and out
    from opencorr_amd import capi
    s.build()
    n = ctypes.c_size_t(77)
    capi.check(capi.lib().oc_hip_sift3d_candidate_count(s._h, ctypes.byref(n)))
    assert n.value == len(want.status)
    kp, status, sums = s.orient(None, with_status=True, on_device=True)
    torch.cuda.synchronize()
    assert kp.is_cuda and kp.cpu().numpy().tobytes() == want.keypoints.tobytes()
    assert np.array_equal(status.cpu().numpy(), want.status) and np.array_equal(_bits(sums.cpu().numpy()), _bits(want.sums))
    desc = s.describe(kp)
    torch.cuda.synchronize()
    assert desc.is_cuda and np.array_equal(_bits(desc.cpu().numpy()), _bits(want.descriptors))
    s.close()


@pytest.mark.parametrize("fma", [0, 1])
def test_unclamped_centre_windows_of_the_big_volume(fma):
    """the largest windows a default pyramid has, 47^3 at layer 1 and 73^3 at layer 3, cut by no border: planted keypoint records at
    BIG's centre (its centre candidates are rejected by the orientation stage), the identity and an oblique matrix"""
    ss = sift3d_twin.scale_space(cases.BIG.volume(), fma=fma, **cases.BIG.settings)
    pyr, e = twin.Pyramid(ss.gauss, 3), twin.grid_exponent(cases.BIG.volume(), cases.BIG.settings["units"])
    kp = cases.big_centre_keypoints(twin.KEYPOINT, ss.gauss)
    assert len(kp) == 4 and all(cases.unclamped(k, ss.gauss[k["layer"]]) for k in kp)
    want = twin.describe(pyr, kp, e)
    assert all(np.count_nonzero(row) == 768 for row in want)
    s = _built(cases.BIG.volume(), cases.BIG.settings, fma)
    got = s.describe(kp)
    assert got.shape == (4, 768) and np.array_equal(_bits(got), _bits(want))
    import torch
    dev = torch.from_numpy(kp.view(np.int32).reshape(4, 18)).cuda()
    assert np.array_equal(_bits(s.describe(dev).cpu().numpy()), _bits(want))
    s.close()


def test_same_bits_reversed_split_and_again():
    name = "two_octaves_odd"
    want = _want(name, 0)
    cand = want.scale_space.candidates
    s = _built(_case(name).volume(), _case(name).settings)
    kp, status, sums = s.orient(cand, with_status=True)
    _same_orientation((kp, status, sums), want, "first")
    _same_orientation(s.orient(cand, with_status=True), want, "second run")
    rkp, rstatus, rsums = s.orient(cand[::-1].copy(), with_status=True)
    assert np.array_equal(rstatus[::-1], status) and np.array_equal(_bits(rsums[::-1]), _bits(sums)) and rkp[::-1].tobytes() == kp.tobytes()
    half = len(cand) // 2
    a, b = s.orient(cand[:half], with_status=True), s.orient(cand[half:], with_status=True)
    assert np.concatenate([a[0], b[0]]).tobytes() == kp.tobytes() and np.array_equal(np.concatenate([a[1], b[1]]), status)
    assert np.array_equal(_bits(np.concatenate([a[2], b[2]])), _bits(sums))
    desc = s.describe(kp)
    assert np.array_equal(_bits(desc), _bits(want.descriptors))
    assert np.array_equal(_bits(s.describe(kp)), _bits(desc))
    assert np.array_equal(_bits(s.describe(kp[::-1].copy())[::-1]), _bits(desc))
    half = len(kp) // 2
    assert np.array_equal(_bits(np.concatenate([s.describe(kp[:half]), s.describe(kp[half:])])), _bits(desc))
    s.close()


@pytest.mark.parametrize("kind", cases.PLANTED_VOLUMES)
def test_planted_volumes(kind):
    v = cases.planted_volume(kind)
    ss = sift3d_twin.scale_space(v, **cases.SETTINGS)
    pyr, e = twin.Pyramid(ss.gauss, 3), twin.grid_exponent(v, cases.SETTINGS["units"])
    cand = cases.planted_candidates(twin.CANDIDATE, ss.gauss)
    status, sums, slots = twin.orient(pyr, cand, e)
    s = _built(v, cases.SETTINGS)
    kp, got_status, got_sums = s.orient(cand, with_status=True)
    assert np.array_equal(got_status, status) and np.array_equal(_bits(got_sums), _bits(sums)) and kp.tobytes() == slots[status == 0].tobytes()
    assert {"constant": status.tolist() == [1] * 6, "blob": status[0] == 1 and set(status.tolist()) <= {1, 2}, "z_ramp": status.tolist() == [2] * 6,
            "oblique_ramp": set(status.tolist()) <= {2, 3}}[kind]
    s.close()


@pytest.mark.parametrize("rotation", list(cases.ROTATIONS))
def test_planted_keypoints(rotation):
    v = cases.planted_volume("z_ramp")
    ss = sift3d_twin.scale_space(v, **cases.SETTINGS)
    pyr, e = twin.Pyramid(ss.gauss, 3), twin.grid_exponent(v, cases.SETTINGS["units"])
    kp = cases.planted_keypoints(twin.KEYPOINT, ss.gauss, rotation)
    want = twin.describe(pyr, kp, e)
    s = _built(v, cases.SETTINGS)
    got = s.describe(kp)
    assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want))
    if rotation == "zero":
        assert not got.any()
    else:
        assert got.any()
    s.close()


@pytest.mark.parametrize("domain", ["u16", "unit", "pedestal"])
def test_domains_move_the_grid(domain):
    """the ranges of tests/image_domains.py: E = 17, 1 and 26 against 9 for 8-bit data"""
    assert domain in image_domains.ROUNDING
    c = cases.CASE_BY_NAME["halving_floors"]
    f = c.volume()
    v = {"u16": np.round(f * np.float32(257.0)), "unit": f / np.float32(255.0), "pedestal": f * np.float32(1e4) + np.float32(3e7)}[domain].astype(np.float32)
    want = twin.extract(v, c.settings)
    assert want.exponent == {"u16": 17, "unit": 1, "pedestal": 26}[domain] and len(want.status) >= 1
    s = _built(v, c.settings)
    _same_orientation(s.orient(None, with_status=True), want, domain)
    assert np.array_equal(_bits(s.describe(None)), _bits(want.descriptors))
    s.close()


def test_validation_comes_before_any_launch():
    from opencorr_amd import capi
    L = capi.lib()
    c = cases.CASE_BY_NAME["two_octaves_odd"]
    want = _want(c.name, 0)
    good_c, good_k = want.scale_space.candidates[:4].copy(), want.keypoints[:4].copy()
    s = _engine(c.settings)
    n = ctypes.c_size_t(77)
    out = np.full(4 * 18, 0x5A5A5A5A, np.uint32)
    desc = np.full(4 * 768, 0x5A5A5A5A, np.uint32)

    def orient(cand):
        return L.oc_hip_sift3d_orient(s._h, ctypes.c_void_p(cand.ctypes.data), len(cand), capi.HOST, ctypes.c_void_p(out.ctypes.data), 4, ctypes.byref(n),
                                      None, None, capi.HOST)

    def describe(kp):
        return L.oc_hip_sift3d_describe(s._h, ctypes.c_void_p(kp.ctypes.data), len(kp), capi.HOST, ctypes.c_void_p(desc.ctypes.data), capi.HOST)

    s.set_volume(c.volume())
    no_build = L.oc_hip_sift3d_detect(s._h, None, 0, ctypes.byref(n), capi.HOST)
    assert no_build != capi.OK and orient(good_c) == no_build and describe(good_k) == no_build     # the error detect gives
    s.build()
    n_octave, n_layers = want.scale_space.n_octave, c.settings["n_octave_layers"]
    dims = want.scale_space.gauss[1].dims

    def bad(record, **fields):
        r = record.copy()
        for k, v in fields.items():
            r[k][1] = v
        return r

    for fields in (dict(octave=n_octave), dict(octave=-1), dict(layer=0), dict(layer=n_layers + 1), dict(layer=-3),
                   dict(scale=np.nextafter(good_c["scale"][1], np.float32(9))), dict(x=dims[0]), dict(y=-1), dict(z=dims[2] + 5)):
        assert orient(bad(good_c, **fields)) == capi.ERR_INVALID, fields
    for fields in (dict(octave=n_octave), dict(layer=0), dict(layer=n_layers + 1), dict(scale=np.nextafter(good_k["scale"][1], np.float32(9))),
                   dict(coor_layer=(3.5, 4, 5)), dict(coor_layer=(np.nan, 4, 5)), dict(coor_layer=(np.inf, 4, 5)), dict(coor_layer=(3, -1, 5)),
                   dict(coor_layer=(3, 4, dims[2])), dict(rotation_matrix=(np.nan,) + (0,) * 8), dict(rotation_matrix=(0,) * 8 + (np.inf,)),
                   dict(rotation_matrix=(3,) + (0,) * 8)):
        assert describe(bad(good_k, **fields)) == capi.ERR_INVALID, fields
    assert np.all(out == 0x5A5A5A5A) and np.all(desc == 0x5A5A5A5A)
    # ... a device-resident list is checked where it lies
    import torch
    dev = torch.from_numpy(bad(good_k, layer=0).view(np.int32).reshape(4, 18)).cuda()
    with pytest.raises(capi.OpenCorrHipError) as err:
        s.describe(dev)
    assert err.value.status == capi.ERR_INVALID
    # ... and the good records pass
    assert orient(good_c) == capi.OK and describe(good_k) == capi.OK and not np.all(desc == 0x5A5A5A5A)
    # a volume with a non-finite voxel: the scale space is built, orient and describe refuse
    v = c.volume()
    v[3, 4, 5] = np.inf
    s.set_volume(v)
    s.build()
    assert orient(good_c) == capi.ERR_INVALID and describe(good_k) == capi.ERR_INVALID
    # capacity too small: nothing written, n carries the needed size
    s.set_volume(c.volume())
    s.build()
    out[:] = 0x5A5A5A5A
    cand = want.scale_space.candidates
    rc = L.oc_hip_sift3d_orient(s._h, ctypes.c_void_p(cand.ctypes.data), len(cand), capi.HOST, ctypes.c_void_p(out.ctypes.data), 1, ctypes.byref(n), None, None,
                                capi.HOST)
    assert rc == capi.ERR_INVALID and n.value == len(want.keypoints) > 1 and np.all(out == 0x5A5A5A5A)
    s.close()


def test_descriptors_go_to_the_matcher_as_device_blocks():
    import torch
    from opencorr_amd import DescriptorMatcher
    ref, tar = cases.shift_pair()
    want_ref, want_tar, a, b = twin.pipeline(ref, tar, cases.SETTINGS)
    blocks = []
    for v, w in ((ref, a), (tar, b)):
        s = _built(v, cases.SETTINGS)
        kp = s.orient()
        assert kp.tobytes() == w.keypoints.tobytes()
        out = torch.empty((len(kp), 768), dtype=torch.float32, device="cuda")
        s.describe(None, out=out)
        blocks.append(out)
        s.close()
    m = DescriptorMatcher(768, 0.85)
    m.set_descriptors(0, blocks[0])
    m.set_descriptors(1, blocks[1])
    for mode in (0, 1):
        ri, ti = m.match(mode)
        wr, wt = match_twin.pairs(a.descriptors, b.descriptors, 0.85, mode)
        assert np.array_equal(ri.cpu().numpy(), wr) and np.array_equal(ti.cpu().numpy(), wt) and len(wr) >= 5
    m.close()


@pytest.mark.parametrize("bidirectional", [False, True])
def test_sift3d_compute_gives_the_twin_pipeline(bidirectional):
    from opencorr_amd import SIFT3D
    ref, tar = cases.shift_pair()
    want_ref, want_tar, _, _ = twin.pipeline(ref, tar, cases.SETTINGS, bidirectional=bidirectional)
    sift = SIFT3D()
    got_ref, got_tar = sift.compute(ref, tar, bidirectional=bidirectional)
    assert len(want_ref) >= 5 and np.array_equal(got_ref, want_ref) and np.array_equal(got_tar, want_tar)
    sift.close()

"""SIFT2D's detector on the GPU (opencorr_amd/csrc/sift2d.hip) == its CPU restatement (tests/cpp/sift2d_twin.cpp), bit for bit:
every Gaussian and DoG layer as raw bits, the layer tables, the keypoint count and every record.  The cases (tests/sift2d_cases.py)
are the smallest shapes at which the kernels can still go wrong, and the reference's 512 x 512 image at full size."""
import ctypes
import functools

import numpy as np
import pytest

import sift2d_cases as cases
import sift2d_twin as twin

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _twin(name):
    c = cases.CASE_BY_NAME[name]
    return twin.detector(c.image(), **c.settings)


def _engine(settings=None):
    from opencorr_amd import SIFT2DScaleSpace
    s = SIFT2DScaleSpace()
    if settings:
        s.set_config(**settings)
    return s


def _check(s, want, what):
    """everything the built engine `s` holds against the twin's result"""
    for pyramid, layers in ((0, want.gauss), (1, want.dog)):
        info = s.layers(pyramid)
        assert len(info) == len(layers), (what, pyramid)
        for i, t in enumerate(layers):
            assert tuple(info[i]["dims"]) == (t.cols, t.rows) and info[i]["octave"] == t.octave, (what, pyramid, i)
            assert _bits(info[i]["sigma"]) == _bits(t.sigma) and info[i]["radius"] == t.radius, (what, pyramid, i)
            assert info[i]["threshold"] == want.threshold, (what, pyramid, i)
            got = s.layer(pyramid, i)
            assert got.shape == t.data.shape and np.array_equal(_bits(got), _bits(t.data)), (what, pyramid, i)
    assert s.keypoint_count() == len(want.keypoints), what
    got = s.detect()
    assert got.dtype == twin.KEYPOINT and len(got) == len(want.keypoints), what
    assert got.tobytes() == want.keypoints.tobytes(), what


@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_kernel_equals_twin(case):
    want = _twin(case.name)
    s = _engine(case.settings)
    s.set_image(case.image())
    s.build()
    _check(s, want, case.name)
    s.close()


def test_cases_produce_keypoints_and_moves():
    """the equality above shows little unless the twin finds keypoints, some of which left their starting cell"""
    total = moved = 0
    for c in cases.CASES:
        r = _twin(c.name)
        total += len(r.keypoints)
        acc = r.starts[r.starts["accepted"] == 1]
        moved += int(((acc["row"] != r.keypoints["row"]) | (acc["col"] != r.keypoints["col"]) | (acc["layer"] != r.keypoints["layer"])).sum())
    assert total >= 30 and moved >= 1, (total, moved)
    assert len(_twin("three_octaves").gauss) == 3 * 6 and _twin("three_octaves").gauss[-1].cols == 12   # its top octave: no scan region


def test_u8_and_f32_pixels_give_the_same_bits():
    img = cases.CASE_BY_NAME["odd_sides"].image()
    assert img.dtype == np.uint8
    want = _twin("odd_sides")
    s = _engine()
    s.set_image(img.astype(np.float32))
    s.build()
    _check(s, want, "odd_sides as float32")
    s.close()


@pytest.mark.parametrize("kind", ["constant", "along_x"])
def test_planted_images(kind):
    """constant: every DoG layer is zero, nothing passes the threshold.  Constant along x: every pixel of a row ties with its
    neighbours, the plateau's pixels are all candidates, their systems have an exactly zero pivot and all die at det <= 0."""
    img = cases.planted(kind)
    want = twin.detector(img)
    assert len(want.keypoints) == 0
    assert (len(want.starts) > 0) == (kind == "along_x")
    s = _engine()
    s.set_image(img)
    s.build()
    _check(s, want, kind)
    s.close()


def test_device_image_and_device_list():
    import torch
    c = cases.CASE_BY_NAME["wide"]
    want = _twin("wide")
    for as_float in (False, True):
        img = c.image().astype(np.float32) if as_float else c.image()
        d_img = torch.from_numpy(img).cuda()
        s = _engine(c.settings)
        s.set_image(d_img)
        s.build()
        _check(s, want, ("device image", as_float))
        d_list = s.detect(on_device=True)
        torch.cuda.synchronize()
        assert d_list.cpu().numpy().tobytes() == want.keypoints.tobytes()
        s.close()


def test_build_twice_then_another_image():
    a, b = cases.CASE_BY_NAME["tall"], cases.CASE_BY_NAME["odd_sides"]
    s = _engine()
    s.set_image(a.image())
    s.build()
    s.build()
    _check(s, _twin("tall"), "built twice")
    s.set_image(b.image())
    s.build()
    _check(s, _twin("odd_sides"), "second image, smaller")
    s.set_image(a.image())
    s.build()
    _check(s, _twin("tall"), "third image, larger again")
    s.close()


def test_capacity_too_small_reports_the_count_and_writes_nothing():
    from opencorr_amd import capi
    want = _twin("wide")
    n_want = len(want.keypoints)
    assert n_want > 8
    s = _engine()
    s.set_image(cases.CASE_BY_NAME["wide"].image())
    s.build()
    buf = np.full(n_want, 0x5A, dtype=np.uint8).repeat(twin.KEYPOINT.itemsize).view(twin.KEYPOINT)
    before = buf.tobytes()
    n = ctypes.c_size_t()
    rc = capi.lib().oc_hip_sift2d_detect(s._h, ctypes.c_void_p(buf.ctypes.data), 8, ctypes.byref(n), capi.HOST)
    assert rc == capi.ERR_INVALID and n.value == n_want and buf.tobytes() == before
    rc = capi.lib().oc_hip_sift2d_detect(s._h, ctypes.c_void_p(buf.ctypes.data), n_want, ctypes.byref(n), capi.HOST)
    assert rc == capi.OK and n.value == n_want and buf.tobytes() == want.keypoints.tobytes()
    s.close()


@pytest.mark.parametrize("settings,status", cases.REFUSED_SETTINGS, ids=lambda v: repr(v))
def test_refused_settings(settings, status):
    from opencorr_amd import capi
    s = _engine()
    with pytest.raises(capi.OpenCorrHipError) as err:
        s.set_config(**settings)
    assert err.value.status == status
    with pytest.raises(twin.Refused) as refused:
        twin.detector(cases.speckle(20, 20, 1), **settings)
    assert refused.value.status == status
    s.close()


@pytest.mark.parametrize("shape,status", cases.REFUSED_SHAPES, ids=lambda v: repr(v))
def test_refused_shapes(shape, status):
    """sides below 2; a doubled base above 2^31-1 pixels (refused from the sides alone: the pointer is never read)"""
    from opencorr_amd import capi
    s = _engine()
    small = np.zeros((2, 2), np.uint8)
    rc = capi.lib().oc_hip_sift2d_set_image(s._h, ctypes.c_void_p(small.ctypes.data), 0, shape[1], shape[0], capi.HOST)
    assert rc == status
    s.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_pixels_are_refused(bad):
    from opencorr_amd import capi
    img = cases.speckle(21, 23, 12).astype(np.float32)
    img[20, 22] = bad
    s = _engine()
    s.set_image(img)
    with pytest.raises(capi.OpenCorrHipError) as err:
        s.build()
    assert err.value.status == capi.ERR_INVALID
    with pytest.raises(capi.OpenCorrHipError):
        s.detect()
    with pytest.raises(twin.Refused) as refused:
        twin.detector(img)
    assert refused.value.status == capi.ERR_INVALID
    s.close()


def test_tuning_and_foreign_entry_points():
    """the keys every kind accepts are taken, arith_fma = 1 is refused; the POI entry points refuse the handle"""
    from opencorr_amd import capi
    s = _engine()
    s.set_tuning("host_chunk", 0)
    s.set_tuning("arith_fma", 0)
    with pytest.raises(capi.OpenCorrHipError) as err:
        s.set_tuning("arith_fma", 1)
    assert err.value.status == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.OpenCorrHipError) as err:
        s.set_tuning("match_splits", 0)
    assert err.value.status == capi.ERR_UNSUPPORTED
    pois = np.zeros((1, capi.POI2D_FLOATS), np.float32)
    assert capi.lib().oc_hip_compute(s._h, ctypes.c_void_p(pois.ctypes.data), 1, capi.POI2D_BYTES, capi.HOST) == capi.ERR_UNSUPPORTED
    s.close()

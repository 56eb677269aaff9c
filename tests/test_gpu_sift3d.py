"""SIFT3D's scale space on the GPU (opencorr_amd/csrc/sift3d.hip) == its CPU restatement (tests/cpp/sift3d_twin.cpp), bit for bit,
in both arithmetic modes: every Gaussian and DoG layer as raw bits, max_abs, the layer tables, the candidate count and the list.
The cases (tests/sift3d_cases.py) are the smallest shapes at which the kernels can still go wrong."""
import ctypes
import functools

import numpy as np
import pytest

import sift3d_cases as cases
import sift3d_twin as twin

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _twin(name, fma):
    c = cases.CASE_BY_NAME[name]
    return twin.scale_space(c.volume(), fma=fma, **c.settings)


def _engine(settings, fma=0):
    from opencorr_amd import SIFT3DScaleSpace
    s = SIFT3DScaleSpace()
    s.set_tuning("arith_fma", fma)
    s.set_config(settings["n_octave_layers"], settings["min_dimension"], settings["alpha"], settings["sigma_source"], settings["sigma_base"])
    s.set_physical_unit(*settings["units"])
    return s


def _check(s, want, what):
    """everything the built engine `s` holds against the twin's result"""
    for pyramid, layers in ((0, want.gauss), (1, want.dog)):
        info = s.layers(pyramid)
        assert len(info) == len(layers), (what, pyramid)
        for i, t in enumerate(layers):
            assert tuple(info[i]["dims"]) == t.dims and info[i]["octave"] == t.octave, (what, pyramid, i)
            assert _bits(info[i]["units"]).tolist() == _bits(np.array(t.units)).tolist(), (what, pyramid, i)
            assert _bits(info[i]["scale"]) == _bits(t.scale), (what, pyramid, i)
            if pyramid == 0:
                assert _bits(info[i]["sigma"]) == _bits(t.sigma) and info[i]["max_abs"] == -1.0, (what, i)
            else:
                assert _bits(info[i]["max_abs"]) == _bits(t.max_abs), (what, i)
            got = s.layer(pyramid, i)
            assert got.shape == t.vol.shape and np.array_equal(_bits(got), _bits(t.vol)), (what, pyramid, i)
    got = s.detect()
    assert len(got) == len(want.candidates), what
    assert got.tobytes() == want.candidates.tobytes(), what


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_kernel_equals_twin(case, fma):
    want = _twin(case.name, fma)
    assert len(want.candidates) >= 1
    s = _engine(case.settings, fma)
    s.set_volume(case.volume())
    s.build()
    _check(s, want, (case.name, fma))
    s.close()


def test_cases_produce_candidates():
    assert sum(len(_twin(c.name, 0).candidates) for c in cases.CASES) >= 30


def test_fma_changes_bits():
    """the two arithmetic modes are two results (otherwise the fma runs above would show nothing)"""
    a, b = _twin("two_octaves_odd", 0), _twin("two_octaves_odd", 1)
    assert any(not np.array_equal(_bits(x.vol), _bits(y.vol)) for x, y in zip(a.gauss, b.gauss))


@pytest.mark.parametrize("kind", cases.PLANTED)
def test_planted_ties(kind):
    """a constant volume: every layer constant; constant along one axis: ties on it.  No candidate, even with alpha = 0"""
    v = cases.planted(kind)
    settings = dict(cases.CASES[0].settings, alpha=0.0)
    want = twin.scale_space(v, **settings)
    assert len(want.candidates) == 0
    s = _engine(settings)
    s.set_volume(v)
    s.build()
    _check(s, want, kind)
    if kind == "constant":
        for pyramid in (0, 1):
            for i in range(len(s.layers(pyramid))):
                layer = s.layer(pyramid, i)
                assert np.all(layer == layer.flat[0])
    assert len(s.detect()) == 0
    s.close()


def test_detect_capacity_too_small_writes_nothing():
    from opencorr_amd import capi
    case = cases.CASES[0]
    want = _twin(case.name, 0)
    n_want = len(want.candidates)
    s = _engine(case.settings)
    s.set_volume(case.volume())
    s.build()
    buf = np.full(n_want * 6, 0x5A5A5A5A, np.uint32)
    n = ctypes.c_size_t(77)
    rc = capi.lib().oc_hip_sift3d_detect(s._h, ctypes.c_void_p(buf.ctypes.data), n_want - 1, ctypes.byref(n), capi.HOST)
    assert rc == capi.ERR_INVALID and n.value == n_want
    assert np.all(buf == 0x5A5A5A5A)
    rc = capi.lib().oc_hip_sift3d_detect(s._h, ctypes.c_void_p(buf.ctypes.data), n_want, ctypes.byref(n), capi.HOST)
    assert rc == capi.OK and n.value == n_want and buf.tobytes() == want.candidates.tobytes()
    s.close()


def test_host_and_device_forms_give_the_same_bytes():
    import torch
    from opencorr_amd import capi
    case = cases.CASE_BY_NAME["halving_floors"]
    want = _twin(case.name, 0)
    s = _engine(case.settings)
    s.set_volume(torch.from_numpy(case.volume()).cuda())
    s.build()
    _check(s, want, "device volume, host results")
    for pyramid, layers in ((0, want.gauss), (1, want.dog)):
        for i, t in enumerate(layers):
            out = torch.full(t.vol.shape, -7.0, dtype=torch.float32, device="cuda")
            s.layer(pyramid, i, out=out)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(t.vol)), (pyramid, i)
    n_want = len(want.candidates)
    dev = torch.zeros(n_want * 6, dtype=torch.int32, device="cuda")
    n = ctypes.c_size_t()
    capi.check(capi.lib().oc_hip_sift3d_detect(s._h, ctypes.c_void_p(dev.data_ptr()), n_want, ctypes.byref(n), capi.DEVICE))
    torch.cuda.synchronize()
    assert n.value == n_want and dev.cpu().numpy().tobytes() == want.candidates.tobytes()
    s.close()


def test_second_build_does_not_depend_on_the_first():
    """one engine, two volumes of different shapes and settings, the larger first: buffers are reused, results are not"""
    first, second = cases.CASE_BY_NAME["one_octave_wide"], cases.CASE_BY_NAME["clamp"]
    s = _engine(first.settings, 1)
    s.set_volume(first.volume())
    s.build()
    assert len(s.detect()) == len(_twin(first.name, 1).candidates)
    s.set_tuning("arith_fma", 0)
    s.set_config(second.settings["n_octave_layers"], second.settings["min_dimension"], second.settings["alpha"], second.settings["sigma_source"],
                 second.settings["sigma_base"])
    s.set_volume(second.volume())
    s.build()
    _check(s, _twin(second.name, 0), "second build")
    s.set_volume(first.volume())
    s.set_tuning("arith_fma", 1)
    s.build()
    _check(s, _twin(first.name, 1), "third build")
    s.close()


def test_refusals_come_before_any_launch():
    from opencorr_amd import capi
    s = _engine(cases.CASES[0].settings)
    with pytest.raises(RuntimeError):
        s.build()                                                    # no volume
    s.set_volume(np.zeros((16, 16, 16), np.float32))
    s.set_physical_unit(1.0, 1.0, 4.5)                               # radius 40 on x and y
    assert capi.lib().oc_hip_sift3d_build(s._h) == capi.ERR_UNSUPPORTED
    n = ctypes.c_size_t()
    assert capi.lib().oc_hip_sift3d_detect(s._h, None, 0, ctypes.byref(n), capi.HOST) == capi.ERR_INVALID   # nothing was built
    dev = (ctypes.c_int * 2)(0, 0)
    assert capi.lib().oc_hip_set_devices(s._h, dev, 1) == capi.ERR_UNSUPPORTED
    assert capi.lib().oc_hip_set_tuning(s._h, b"match_splits", 2) == capi.ERR_UNSUPPORTED
    kind = ctypes.c_int()
    capi.check(capi.lib().oc_hip_get_kind(s._h, ctypes.byref(kind)))
    assert kind.value == capi.SIFT3D == 14
    s.close()

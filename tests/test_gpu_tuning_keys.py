"""oc_hip_set_tuning of the library itself against tests/engine_tuning_model.py: one engine of every kind the package creates, every
key (and the alias, an unknown key, the empty one, a null pointer) at the values around every bound of the rules -- the status
code must be the model's for the product build, and the product build's refusals of the A/B partners still say so.  No kernel
is launched.
"""
import pytest

import engine_tuning_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    import opencorr_amd
    made = {model.FFTCC2D: opencorr_amd.FFTCC2D(16, 16), model.ICGN2D1: opencorr_amd.ICGN2D1(16, 16, 0.001, 10),
            model.ICGN2D2: opencorr_amd.ICGN2D2(16, 16, 0.001, 10), model.ICLM2D1: opencorr_amd.ICLM2D1(16, 16, 0.001, 10),
            model.NR2D1: opencorr_amd.NR2D1(16, 16, 0.001, 10), model.FFTCC3D: opencorr_amd.FFTCC3D(8, 8, 8),
            model.ICGN3D1: opencorr_amd.ICGN3D1(8, 8, 8, 0.001, 10), model.STRAIN: opencorr_amd.Strain(20.0, 5),
            model.MATCHER: opencorr_amd.DescriptorMatcher(128)}
    yield made
    for e in made.values():
        e.close()


def test_every_key_at_its_boundaries_answers_like_the_model(engines):
    from opencorr_amd import capi
    L = capi.lib()
    assert (capi.ERR_INVALID, capi.ERR_UNSUPPORTED) == (model.ERR_INVALID, model.ERR_UNSUPPORTED)
    bad, asked = [], 0
    for kind, e in engines.items():
        for key in model.KEYS + ("xcd", "no_such_key", ""):
            for value in model.BOUNDARY_VALUES:
                got, want = L.oc_hip_set_tuning(e._h, key.encode(), value), model.status(kind, key, value)
                asked += 1
                if got != want:
                    bad.append((kind, key, value, got, want))
        assert L.oc_hip_set_tuning(e._h, None, 0) == capi.ERR_INVALID
        assert L.oc_hip_set_tuning(e._h, b"no_such_key", 0) == capi.ERR_INVALID
        assert b"unknown tuning key 'no_such_key'" in L.oc_hip_last_error()
    assert asked == 9 * 23 * len(model.BOUNDARY_VALUES)
    assert not bad, "%d of %d answers differ (kind, key, value, library, model), first: %s" % (len(bad), asked, bad[:8])


def test_product_build_refusals_name_the_ab_build(engines):
    from opencorr_amd import capi
    L = capi.lib()
    for kind, key, value in ((model.ICGN2D1, "icgn2d_variant", 0), (model.ICGN2D1, "icgn2d_variant", 9), (model.ICGN2D1, "icgn2d_split_chunks", 1),
                             (model.ICGN3D1, "icgn3d_mapping", 1), (model.FFTCC3D, "fftcc3d_fused", 2)):
        assert L.oc_hip_set_tuning(engines[kind]._h, key.encode(), value) == capi.ERR_UNSUPPORTED
        words = L.oc_hip_last_error().decode()
        assert "A/B" in words and key in words, words
    assert L.oc_hip_set_tuning(engines[model.ICGN3D1]._h, b"arith_onepass", 1) == capi.ERR_UNSUPPORTED
    assert "arith_onepass3d" in L.oc_hip_last_error().decode()
    assert L.oc_hip_set_tuning(engines[model.MATCHER]._h, b"match_splits", 65) == capi.ERR_INVALID
    assert L.oc_hip_last_error().decode() == "match_splits must be 0 (automatic) ... 64"
    assert L.oc_hip_set_tuning(engines[model.ICGN2D1]._h, b"icgn2d_variant", 12) == capi.ERR_INVALID
    assert L.oc_hip_last_error().decode() == "icgn2d_variant 12 out of range [-1 (automatic), 12)"
    assert L.oc_hip_set_tuning(engines[model.ICGN3D1]._h, b"icgn3d_mapping", 1) == capi.ERR_UNSUPPORTED
    assert "12 - 25 % slower" in L.oc_hip_last_error().decode()

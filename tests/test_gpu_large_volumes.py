"""The 3D engines where voxel offsets pass 2^31 and 2^32 (tests/large_volume_cases.py; the method is proved on a CPU by
tests/test_oracle_large_volume_cases.py).

One huge pair per shape, built on the device (zeros plus the pasted blocks) and handed to set_images in place; one shape and one
engine alive at a time.  The reference for a block is the oracle on its crop, stop_condition = 1, POIs shifted to the crop's origin:
every float of a record except x, y, z must come back with the same bits.  Fields are read as device-side slices.  FFTCC3D: u, v, w,
u0, v0, w0 exact, ZNCC inside the bars tests/test_gpu_parity_3d.py holds those kernels to.  Every other comparison is bit equality.
ICGN3D1 keeps seven volume-sized arrays alive (ref, tar, gx, gy, gz, coef and the prefilter's second volume): 61 GB on INDEX31,
69 GB on SLAB; REFUSED is one allocation of 18.4 GB on which ICGN3D1 must reserve nothing.

ICGN3D1's queues are short, so the locality schedule (2048 POIs and more) never starts on them: one queue per shape is padded with
repeats of itself to 2048 records and solved with the schedule off and on.  The row mapping (icgn3d_mapping = 1) exists in the A/B
build only: refused here, run on both shapes by tests/ab/test_ab_large_volumes.py.  tests/large_volume_engines.py holds what the two
files share.
"""
import gc
import time

import numpy as np
import pytest

import large_volume_cases as lv
import large_volume_engines as lve
import oracle

pytestmark = pytest.mark.gpu
P = lv.P
GB, CASES = lve.GB, lve.CASES


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    return opencorr_amd


@pytest.fixture(scope="module")
def huge(request):
    """one shape at a time: pytest ends the previous parameter's instance before it sets up the next"""
    import torch
    key = request.param
    need = CASES[key][1]
    total = torch.cuda.get_device_properties(0).total_memory
    if total < need:
        pytest.skip("%s needs %.1f GB, the device has %.1f GB in total" % (key, need / GB, total / GB))
    holder = lve.Huge(torch, key)
    yield holder
    holder.close()
    del holder
    gc.collect()
    torch.cuda.empty_cache()


def on(*keys):
    return pytest.mark.parametrize("huge", list(keys), indirect=True)


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t0))


# ---- INDEX31 and SLAB: ICGN3D1 ----------------------------------------------------------------------------------------------------
@on("INDEX31", "SLAB")
def test_prepare_fields(eng, huge):
    e = huge.get("ICGN3D1", lve.icgn3d1(eng, huge.key))
    assert huge.used() >= 7 * 4 * lve.voxels(huge.key)
    for b in lv.BLOCKS[huge.key]:
        for name, (field, margin) in lv.crop_fields(b).items():
            sl = lv.inside(b, margin)
            got = lve.read_block(e, name, b)
            assert np.array_equal(lv.bits(got[sl]), lv.bits(field[sl])), (huge.key, b.name, name)


@on("INDEX31", "SLAB")
@pytest.mark.parametrize("contract", ["lanes", "fma", "onepass"])
def test_icgn3d1(eng, huge, contract):
    e = huge.get("ICGN3D1", lve.icgn3d1(eng, huge.key))
    lve.set_contract(e, contract)
    for radii in lv.RADII[huge.key]:
        for tile in (0, 64):
            e.set_tuning("icgn3d_tile_vox", tile)
            lve.solve_and_compare(e, huge.key, contract, radii, "tile %d" % tile)
    lve.set_contract(e, "lanes")


@on("INDEX31", "SLAB")
def test_icgn3d1_under_the_locality_schedule(eng, huge):
    """2048 records (the short queue repeated): the schedule's permutation is built and followed; off and on, the same bits"""
    e = huge.get("ICGN3D1", lve.icgn3d1(eng, huge.key))
    radii = lv.RADII[huge.key][-1]
    e.set_subset(*radii)
    for contract in ("lanes", "onepass"):
        lve.set_contract(e, contract)
        q, w = lve.want(huge.key, contract, "half", radii)
        big, wbig = lv.padded(q), lv.padded(w)
        for tile in (0, 64, 8):
            e.set_tuning("icgn3d_tile_vox", tile)
            lv.assert_same_but_xyz(e.compute(big.copy()), wbig, "%s ICGN3D1 %s %s, 2048 records, tile %d" % (huge.key, radii, contract, tile))
    lve.set_contract(e, "lanes")
    e.set_tuning("icgn3d_tile_vox", 64)


@on("INDEX31", "SLAB")
def test_the_row_mapping_is_refused_by_the_product_library(eng, huge):
    from opencorr_amd import capi
    e = huge.get("ICGN3D1", lve.icgn3d1(eng, huge.key))
    if capi.LIB_PATH.endswith("libopencorr_hip_ab.so"):
        pytest.skip("the A/B build runs the row mapping: tests/ab/test_ab_large_volumes.py")
    with pytest.raises(capi.OpenCorrHipError, match="A/B") as err:
        e.set_tuning("icgn3d_mapping", 1)
    assert err.value.status == capi.ERR_UNSUPPORTED


# ---- INDEX31 and SLAB: FFTCC3D ----------------------------------------------------------------------------------------------------
def fftcc_and_compare(eng, huge, radii, fused, bar):
    f = huge.get("FFTCC3D", lambda: eng.FFTCC3D(*radii), prepare=False)
    f.set_subset(*radii)
    f.set_tuning("fftcc3d_fused", fused)
    for b in lv.BLOCKS[huge.key]:
        q = lv.fftcc_queue(b, radii)
        w = lv.fftcc(*lv.crop(b), radii, q)
        moved = lv.shift(q, b)
        got = f.compute(moved.copy())
        what = (huge.key, b.name, radii, fused)
        moving = [P[c] for c in ("u", "v", "w", "u0", "v0", "w0")]
        for c in moving:
            assert np.array_equal(lv.bits(got[:, c]), lv.bits(w[:, c])), what + (c,)
        assert np.abs(got[:, P["zncc"]] - w[:, P["zncc"]]).max() <= bar, what
        other = [c for c in range(31) if c not in moving + [P["zncc"]]]
        assert np.array_equal(lv.bits(got[:, other]), lv.bits(moved[:, other])), what
        yield b, got, w


@on("INDEX31", "SLAB")
@pytest.mark.parametrize("window,family,fused,bar", lv.FFTCC_FAMILIES, ids=[f[1] for f in lv.FFTCC_FAMILIES])
def test_fftcc3d(eng, huge, window, family, fused, bar):
    solved = sum(len(got) for _, got, _ in fftcc_and_compare(eng, huge, window, fused, bar))
    assert solved >= 9 * len(lv.BLOCKS[huge.key])


# ---- REFUSED ----------------------------------------------------------------------------------------------------------------------
@on("REFUSED")
def test_icgn3d1_refuses_a_box_its_offsets_cannot_cross(eng, huge):
    from opencorr_amd import capi
    dz, dy, dx = huge.shape
    (b,) = lv.BLOCKS[huge.key]
    assert not lv.accepted(*lv.R_REFUSED, dy, dx) and huge.tar is huge.ref
    assert lv.accepted(16, 16, 6, dy, dx)                  # a flatter subset fits the same volume: the rule, not the volume, refuses
    before_bytes = huge.used()
    e = eng.ICGN3D1(*lv.R_REFUSED, lv.CONV, lv.STOP)
    e.set_images(huge.ref, huge.tar)
    for call in (e.prepare, e.prepare_ref, e.prepare_tar):
        with pytest.raises(capi.OpenCorrHipError, match="ICGN3D1: volume") as err:
            call()
        assert err.value.status == capi.ERR_UNSUPPORTED
    q = lv.shift(oracle.make_pois3d([b.bx // 2, b.bx - 4], [b.by // 2, b.by - 4], [7, 7]), b)
    q[:, P["u"]], q[:, P["zncc"]] = 0.5, 0.25
    before = q.copy()
    with pytest.raises(capi.OpenCorrHipError, match="ICGN3D1: volume") as err:      # (asked before the queue is staged)
        e.compute(q)
    assert err.value.status == capi.ERR_UNSUPPORTED and np.array_equal(lv.bits(q), lv.bits(before))
    assert abs(huge.used() - before_bytes) < GB            # nothing volume-sized was reserved
    e.close()


@on("REFUSED")
@pytest.mark.parametrize("window,family,fused,bar", lv.FFTCC_REFUSED, ids=[f[1] for f in lv.FFTCC_REFUSED])
def test_fftcc3d_beyond_voxel_index_2_32(eng, huge, window, family, fused, bar):
    zero = lv.bits(np.zeros(1, dtype=np.float32))[0]
    for b, got, w in fftcc_and_compare(eng, huge, window, fused, bar):
        for c in "uvw":
            assert (lv.bits(got[:, P[c]]) == zero).all(), (window, c)
        assert np.abs(got[:, P["zncc"]] - 1).max() <= bar
        assert lv.voxel_index(huge.shape, int(got[:, P["z"]].max()) + window[2] - 1, b.y0, b.x0) > 1 << 32

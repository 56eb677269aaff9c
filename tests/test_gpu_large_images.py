"""The 2D engines where image offsets pass 2^31 and rows pass 65 535 (tests/large_image_cases.py; the method is proved on a CPU by
tests/test_oracle_large_image_cases.py).

One huge pair per shape, built on the device (zeros plus the pasted blocks) and handed to set_images in place; one shape and one
engine alive at a time.  The reference for a block is the oracle on its crop, stop_condition = 1, POIs shifted to the crop's
origin: every float of a record except x, y must come back with the same bits.  Fields are read as device-side slices.  FFTCC2D:
u, v, u0, v0 exact, ZNCC inside the bars tests/test_gpu_parity_2d.py holds those kernels to.  Every other comparison is bit
equality.  The largest case (ICGN_LIMIT) holds about 22 GB on the device.
"""
import ctypes
import gc

import numpy as np
import pytest

import large_image_cases as lc
import oracle

pytestmark = pytest.mark.gpu
P = lc.P
GB = 1 << 30

# shape key -> ((h, w), the target is the reference tensor, device bytes the case needs: the pair and the largest engine on it)
CASES = {key: (shape, False, 2 * 4 * shape[0] * shape[1] + (3 * 64 + 8 if key == "NR_LIMIT" else 0 if key == "FFTCC_LIMIT" else 64 + 12) * shape[0] * shape[1] + GB)
         for key, shape in lc.SHAPES.items()}
CASES.update({"REFUSED%d" % i: (shape, True, 4 * shape[0] * shape[1] + GB) for i, shape in enumerate(lc.REFUSED_FFTCC)})
assert 21 * GB < CASES["ICGN_LIMIT"][2] < 23 * GB


class Huge:
    """The pair of one shape and the one engine that is alive on it."""

    def __init__(self, torch, key):
        self.key, self.torch = key, torch
        (h, w), same, _ = CASES[key]
        self.shape = (h, w)
        self.ref = torch.zeros((h, w), dtype=torch.float32, device="cuda")     # (an allocation failure is an error, not a skip)
        self.tar = self.ref if same else torch.zeros((h, w), dtype=torch.float32, device="cuda")
        for b in lc.BLOCKS.get(key, []):
            for t, a in zip((self.ref, self.tar), lc.crop(b)):
                t[b.y0:b.y0 + b.bh, b.x0:b.x0 + b.bw] = torch.from_numpy(np.array(a)).cuda()
        torch.cuda.synchronize()
        self.engine, self.tag = None, None

    def get(self, tag, make, prepare=True):
        """the engine `tag`, made (and prepared) when another one held the device"""
        if self.tag != tag:
            self.drop()
            e = make()
            e.set_images(self.ref, self.tar)
            if prepare:
                e.prepare()
                e.synchronize()
                free, total = self.torch.cuda.mem_get_info()
                print("%s %s: %.2f GB of device memory in use after prepare()" % (self.key, tag, (total - free) / GB))
            self.engine, self.tag = e, tag
        return self.engine

    def drop(self):
        if self.engine is not None:
            self.engine.close()
        self.engine, self.tag = None, None

    def close(self):
        self.drop()
        self.ref = self.tar = None


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    return opencorr_amd


@pytest.fixture(scope="module")
def huge(request):
    """one shape at a time: pytest ends the previous parameter's instance before it sets up the next"""
    import torch
    key = request.param
    need = CASES[key][2]
    total = torch.cuda.get_device_properties(0).total_memory
    if total < need:
        pytest.skip("%s needs %.1f GB, the device has %.1f GB in total" % (key, need / GB, total / GB))
    holder = Huge(torch, key)
    yield holder
    holder.close()
    del holder
    gc.collect()
    torch.cuda.empty_cache()


def on(*keys):
    return pytest.mark.parametrize("huge", list(keys), indirect=True)


# ---- device-side slice reads ---------------------------------------------------------------------------------------------------
def _rows(e, ptr, pitch_floats, y0, x0, rows, cols, floats):
    """rows x cols entries of `floats` floats each out of a row-major device array of `pitch_floats` floats per row"""
    from opencorr_amd import capi
    out = np.empty((rows, cols * floats), dtype=np.float32)
    src = ptr + 4 * (y0 * pitch_floats + x0 * floats)
    copy2d = capi.hip_runtime().hipMemcpy2D          # (the one runtime of this process)
    copy2d.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    copy2d.restype = ctypes.c_int
    status = copy2d(out.ctypes.data, out.strides[0], src, 4 * pitch_floats, 4 * cols * floats, rows, 2)    # hipMemcpyDeviceToHost
    assert status == 0, "hipMemcpy2D: %d" % status
    return out.reshape(rows, cols, floats) if floats > 1 else out


def read_block(e, name, block):
    """the field over the block, in read_field's layout: (bh, bw) or (bh, bw, 16)"""
    from opencorr_amd import capi
    ptr, count = ctypes.c_void_p(), ctypes.c_size_t()
    capi.check(capi.lib().oc_hip_get_field(e._h, name.encode(), ctypes.byref(ptr), ctypes.byref(count)))
    e.synchronize()
    h, w = block.shape
    if name in ("lut", "lut_gx", "lut_gy"):
        assert count.value == 16 * h * w
        planes = [_rows(e, ptr.value + 16 * h * w * k, 4 * w, block.y0, block.x0, block.bh, block.bw, 4) for k in range(4)]
        return np.concatenate(planes, axis=2)
    assert count.value == h * w
    return _rows(e, ptr.value, w, block.y0, block.x0, block.bh, block.bw, 1)


def check_fields(e, block, want, what, value_plane=False):
    for name, field in want.items():
        ys, xs = lc.inside(block, lc.NR_MARGIN if name in ("lut_gx", "lut_gy") else lc.FIELD_MARGIN)
        got = read_block(e, name, block)
        assert np.array_equal(lc.bits(got[ys, xs]), lc.bits(field[ys, xs])), (what, name)
        if name == "lut" and value_plane:
            val = read_block(e, "lut_val", block)
            assert np.array_equal(lc.bits(val), lc.bits(got[..., 0])) and np.array_equal(lc.bits(val[ys, xs]), lc.bits(field[ys, xs][..., 0])), (what, "lut_val")


# ---- the oracle on the crops, once ------------------------------------------------------------------------------------------------
_want = {}


def want(key, solver, guesses, order=oracle.ORDER_LANES):
    """(the queue of all blocks of the shape in image coordinates, the oracle's records for it)"""
    k = (key, solver, guesses, order)
    if k not in _want:
        qs, ws = [], []
        for b in lc.BLOCKS[key]:
            q, _ = lc.solver_queue(b, guesses)
            p2, pnr = lc.prepared(b)
            qs.append(lc.shift(q, b))
            ws.append(lc.solve(solver, p2, pnr, q, order))
        _want[k] = (np.concatenate(qs), np.concatenate(ws))
    return _want[k]


def solve_and_compare(e, key, solver, what, order=oracle.ORDER_LANES, calls=1):
    for guesses in ("int", "half"):
        q, w = want(key, solver, guesses, order)
        for call in range(calls):
            got = e.compute(q.copy())
            assert np.array_equal(lc.bits(got[:, :2]), lc.bits(q[:, :2]))
            lc.assert_same_but_xy(got, w, "%s %s %s, %s guesses, call %d" % (key, solver, what, guesses, call + 1))


def icgn_contracts(e, key, dof, variant):
    solver, twin = ("icgn2d1", "onepass1") if dof == 6 else ("icgn2d2", "onepass2")
    e.set_tuning("icgn2d_variant", variant)
    for fma in (0, 1):
        e.set_tuning("arith_fma", fma)
        e.set_tuning("arith_onepass", 0)
        # twice: the table variants fill their set-up cache on the first call and start from it on the second
        solve_and_compare(e, key, solver, "variant %d fma %d" % (variant, fma), oracle.ORDER_LANES_FMA if fma else oracle.ORDER_LANES, calls=2)
        e.set_tuning("arith_onepass", 1)
        solve_and_compare(e, key, twin, "variant %d fma %d one-pass" % (variant, fma))
    e.set_tuning("arith_onepass", 0)
    e.set_tuning("arith_fma", 0)


def _icgn2d1(eng):
    return lambda: eng.ICGN2D1(lc.R_ICGN[0], lc.R_ICGN[1], lc.CONV, lc.STOP)


# ---- ICGN_LIMIT -------------------------------------------------------------------------------------------------------------------
@on("ICGN_LIMIT")
def test_icgn_limit_fields(eng, huge):
    e = huge.get("ICGN2D1", _icgn2d1(eng))
    for b in lc.BLOCKS[huge.key]:
        check_fields(e, b, lc.crop_fields(b)[0], "ICGN_LIMIT " + b.name, value_plane=True)


@on("ICGN_LIMIT")
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 7, 10, 11])
def test_icgn_limit_icgn2d1(eng, huge, variant):
    icgn_contracts(huge.get("ICGN2D1", _icgn2d1(eng)), huge.key, 6, variant)


@on("ICGN_LIMIT")
@pytest.mark.parametrize("variant", [3, 4, 11])
def test_icgn_limit_icgn2d2(eng, huge, variant):
    icgn_contracts(huge.get("ICGN2D2", lambda: eng.ICGN2D2(lc.R_ICGN[0], lc.R_ICGN[1], lc.CONV, lc.STOP)), huge.key, 12, variant)


@on("ICGN_LIMIT")
@pytest.mark.parametrize("dof", [6, 12])
def test_icgn_limit_iclm(eng, huge, dof):
    cls, solver = (eng.ICLM2D1, "iclm2d1") if dof == 6 else (eng.ICLM2D2, "iclm2d2")
    e = huge.get(solver, lambda: cls(lc.R_ICGN[0], lc.R_ICGN[1], lc.CONV, lc.STOP))
    for fma, order in ((0, oracle.ORDER_LANES), (1, oracle.ORDER_LANES_FMA)):
        e.set_tuning("arith_fma", fma)
        solve_and_compare(e, huge.key, solver, "default damping, fma %d" % fma, order)


# ---- NR_LIMIT ---------------------------------------------------------------------------------------------------------------------
@on("NR_LIMIT")
def test_nr_limit(eng, huge):
    e = huge.get("NR2D1", lambda: eng.NR2D1(lc.R_ICGN[0], lc.R_ICGN[1], lc.CONV, lc.STOP))
    for b in lc.BLOCKS[huge.key]:
        check_fields(e, b, lc.crop_fields(b)[1], "NR_LIMIT " + b.name)
    solve_and_compare(e, huge.key, "nr2d1", "")


# ---- WIDE and TALL ----------------------------------------------------------------------------------------------------------------
@on("WIDE0", "WIDE1", "TALL")
def test_thin_images(eng, huge):
    from opencorr_amd import capi
    e = huge.get("ICGN2D1", _icgn2d1(eng))
    for b in lc.BLOCKS[huge.key]:
        check_fields(e, b, lc.crop_fields(b)[0], huge.key, value_plane=True)
    for variant in (2, 5):
        e.set_tuning("icgn2d_variant", variant)
        solve_and_compare(e, huge.key, "icgn2d1", "variant %d" % variant, calls=2)
    # NR2D1: past its pixel limit -- refused by prepare() and by compute()
    nr = huge.get("NR2D1", lambda: eng.NR2D1(lc.R_ICGN[0], lc.R_ICGN[1], lc.CONV, lc.STOP), prepare=False)
    assert not lc.accepted("nr", *huge.shape)
    with pytest.raises(capi.OpenCorrHipError) as err:
        nr.prepare()
    assert err.value.status == capi.ERR_UNSUPPORTED
    q, _ = want(huge.key, "icgn2d1", "half")
    with pytest.raises(capi.OpenCorrHipError):
        nr.compute(q.copy())
    for rx, ry in lc.R_THIN:
        fftcc_and_compare(eng, huge, rx, ry, 1, 1.5e-5, thin=True)


# ---- FFTCC ------------------------------------------------------------------------------------------------------------------------
def fftcc_and_compare(eng, huge, rx, ry, fused, bar, thin=False):
    f = huge.get("FFTCC2D", lambda: eng.FFTCC2D(rx, ry), prepare=False)
    f.set_subset(rx, ry)
    f.set_tuning("fftcc2d_fused", fused)
    solved = 0
    for b in lc.BLOCKS[huge.key]:
        q, n = lc.fftcc_queue(b, rx, ry, thin)
        w = lc.fftcc(*lc.crop(b), rx, ry, q)
        moved = lc.shift(q, b)
        got = f.compute(moved.copy())
        what = (huge.key, b.name, rx, ry, fused)
        for c in ("u", "v", "u0", "v0"):
            assert np.array_equal(lc.bits(got[:, P[c]]), lc.bits(w[:, P[c]])), what + (c,)
        assert np.abs(got[:, P["zncc"]] - w[:, P["zncc"]]).max() <= bar, what
        other = [c for c in range(25) if c not in (P["u"], P["v"], P["u0"], P["v0"], P["zncc"])]
        assert np.array_equal(lc.bits(got[:, other]), lc.bits(moved[:, other])), what
        tripped = (w[:, P["zncc"]] == 0) & (w[:, P["u0"]] == 0)
        assert np.array_equal(lc.bits(got[tripped]), lc.bits(moved[tripped])), what
        solved += n
    return solved


@on("FFTCC_LIMIT")
@pytest.mark.parametrize("window,family,fused,bar", lc.FFTCC_FAMILIES, ids=[f[1] for f in lc.FFTCC_FAMILIES])
def test_fftcc_limit(eng, huge, window, family, fused, bar):
    assert fftcc_and_compare(eng, huge, window[0], window[1], fused, bar) >= 40


@on("REFUSED0", "REFUSED1")
def test_fftcc2d_refuses_what_its_offsets_cannot_reach(eng, huge):
    from opencorr_amd import capi
    assert not lc.accepted("fftcc", *huge.shape) and huge.tar is huge.ref
    h, w = huge.shape
    for rx, ry, fused in ((16, 16, 1), (9, 11, 1), (16, 16, 0)):          # whatever the kernel: rect and rocFFT address with size_t
        if h <= 2 * ry:
            rx = ry = 2
        f = eng.FFTCC2D(rx, ry)
        f.set_tuning("fftcc2d_fused", fused)
        f.set_images(huge.ref, huge.tar)
        q = oracle.make_pois2d([w // 2, w - rx - 1], [h // 2, h - ry - 1])
        before = q.copy()
        with pytest.raises(capi.OpenCorrHipError, match="FFTCC2D: image") as err:
            f.compute(q)
        assert err.value.status == capi.ERR_UNSUPPORTED
        assert np.array_equal(lc.bits(q), lc.bits(before))
        f.close()


# ---- ROWS -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.ROWS, ids=lambda s: "%dx%d" % s)
def test_images_of_more_than_65535_rows(eng, shape):
    ref, tar = lc.rows_pair(shape)
    r = lc.rows_radius(shape)
    p2, pnr = oracle.Prepared2D(ref, tar), oracle.PreparedNR2D(ref, tar)
    tgx, tgy = oracle.gradient2d(tar)
    e = eng.ICGN2D1(r, r, lc.ROWS_CONV, lc.ROWS_STOP)
    e.set_images(ref, tar)
    e.prepare()
    for name, field in (("gx", p2.gx), ("gy", p2.gy), ("lut", p2.lut), ("lut_val", p2.lut[..., 0]), ("ref", ref), ("tar", tar)):
        assert np.array_equal(lc.bits(e.read_field(name)), lc.bits(field)), (shape, "ICGN2D1", name)
    q = lc.rows_queue(shape)
    w = q.copy()
    oracle.icgn2d1(p2, r, r, lc.ROWS_CONV, lc.ROWS_STOP, w, order=oracle.ORDER_LANES, lanes=64)
    got = e.compute(q.copy())
    assert np.array_equal(lc.bits(got), lc.bits(w)), (shape, np.argwhere(lc.bits(got) != lc.bits(w))[:6].tolist())
    e.close()
    nr = eng.NR2D1(r, r, lc.ROWS_CONV, lc.ROWS_STOP)
    nr.set_images(ref, tar)
    nr.prepare()
    for name, field in (("gx", tgx), ("gy", tgy), ("lut", pnr.lut), ("lut_gx", pnr.lut_gx), ("lut_gy", pnr.lut_gy)):
        assert np.array_equal(lc.bits(nr.read_field(name)), lc.bits(field)), (shape, "NR2D1", name)
    nr.close()


# ---- 3D: the prepare launches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.VOLUMES, ids=lambda s: "%dx%dx%d" % s)
def test_volumes_of_more_than_65535_slices_or_rows(eng, shape):
    ref, tar = lc.volume_pair(shape)
    P3 = oracle.P3
    prep = oracle.Prepared3D(ref, tar)
    e = eng.ICGN3D1(3, 3, 3, 0.001, 5)
    e.set_images(ref, tar)
    e.prepare()
    for name in ("gx", "gy", "gz", "coef"):
        assert np.array_equal(lc.bits(e.read_field(name)), lc.bits(getattr(prep, name))), (shape, name)
    q = lc.volume_queue(shape)
    f = eng.FFTCC3D(4, 4, 4)
    f.set_images(ref, tar)
    got, w = f.compute(q.copy()), q.copy()
    f.close()
    oracle.fftcc3d(ref, tar, 4, 4, 4, w)
    for c in ("u", "v", "w", "u0", "v0", "w0"):
        assert np.array_equal(got[:, P3[c]], w[:, P3[c]]), (shape, c)
    assert np.abs(got[:, P3["zncc"]] - w[:, P3["zncc"]]).max() <= 1e-5       # (tests/test_gpu_parity_3d.py::test_fftcc3d_matches_oracle)
    assert (w[:, P3["zncc"]] > 0.5).all()
    got = e.compute(w.copy())
    oracle.icgn3d1(prep, 3, 3, 3, 0.001, 5, w, order=oracle.GPU_ORDER_3D, lanes=oracle.GPU_LANES_3D)
    assert (w[:, P3["zncc"]] > 0.9).mean() > 0.5, w[:, P3["zncc"]]
    both_nan = np.isnan(got) & np.isnan(w)
    assert not ((lc.bits(got) != lc.bits(w)) & ~both_nan).any(), (shape, np.argwhere(lc.bits(got) != lc.bits(w))[:6].tolist())
    e.close()

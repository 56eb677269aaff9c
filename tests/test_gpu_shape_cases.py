"""How the images reach the kernels (tests/shape_cases.py): edge shapes, buffers used in place at 4-byte alignment, one engine
across image sizes.  Every comparison is bit equality (NaN meeting NaN, shape_cases.same).

  * prepare fields of ICGN2D1 / ICGN2D2 / NR2D1 at every shape of SHAPES2D against the oracle, row-major and after a COL_MAJOR
    upload; the zero borders hold +0 bits;
  * device tensors carved out of a larger allocation at offsets of 1, 2 and 3 floats -- `data_ptr() % 16 != 0`, so the scalar
    prepare kernels run although the width is a multiple of 4: fields against the oracle, every solver against the same engine
    fed the same data as host arrays; then the POI queue (and every other device array an entry point takes) at a 1-float offset
    against its run on an aligned copy, with sentinels on both sides of every carved buffer;
  * one long-lived engine per kind through SEQUENCE2D / SEQUENCE3D against a fresh engine per step and, for the fields, against
    the oracle.
tests/test_oracle_shape_cases.py asserts, without a GPU, that the cases hit the paths they claim and that none passes emptily.
"""
import re

import numpy as np
import pytest

import shape_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
NOT_PREPARED = "prepare() has not been called since the last set_images"


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    return opencorr_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _check(e, fields, exp, what):
    for name, key in fields:
        sc.assert_same(e.read_field(name), exp[key], "%s: %s" % (what, name))


ICGN_FIELDS = (("gx", "gx"), ("gy", "gy"), ("lut", "lut"), ("lut_val", "val"))
NR_FIELDS = (("gx", "nr_gx"), ("gy", "nr_gy"), ("lut", "lut"), ("lut_gx", "lut_gx"), ("lut_gy", "lut_gy"))
IMAGES = (("ref", "ref"), ("tar", "tar"))
FIELDS3D = (("gx", "gx"), ("gy", "gy"), ("gz", "gz"), ("coef", "coef"))


def _zero_borders(e, shape, what, nr=False):
    """the two-pixel border of the gradients and the border of every table hold +0 bits (not -0, not a stale float)"""
    mx, my = sc.gradient_border(shape)
    assert not sc.bits(e.read_field("gx"))[mx].any(), (what, "gx border")
    assert not sc.bits(e.read_field("gy"))[my].any(), (what, "gy border")
    lb = sc.lut_border(shape)
    for name in ("lut", "lut_gx", "lut_gy") if nr else ("lut", "lut_val"):
        assert not sc.bits(e.read_field(name))[lb].any(), (what, name + " border")


# ---- 2. edge shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.SHAPES2D, ids=lambda s: "%dx%d" % s)
def test_prepare2d_fields_at_edge_shapes(eng, shape):
    from opencorr_amd import capi
    exp = sc.expected2d(shape)
    ref, tar = exp["ref"], exp["tar"]
    print(shape, sc.grad2d_kernel_of(shape[1]), sc.grad2d_grid(*shape), sorted(sc.edges2d(*shape)))
    for layout, tag in ((capi.ROW_MAJOR, "row-major"), (capi.COL_MAJOR, "col-major")):
        what = "%dx%d %s" % (shape + (tag,))
        e = eng.ICGN2D1(2, 2, sc.CONV, sc.STOP)
        e.set_images(ref, tar, layout=layout)
        e.prepare()
        _check(e, ICGN_FIELDS + IMAGES, exp, what + " ICGN2D1")
        sc.assert_same(e.read_field("lut_val"), e.read_field("lut")[..., 0], what + " ICGN2D1: lut_val against the table")
        _zero_borders(e, shape, what + " ICGN2D1")
        e.close()
        e = eng.ICGN2D2(2, 2, sc.CONV, sc.STOP)
        e.set_images(ref, tar, layout=layout)
        e.prepare()
        _check(e, (("lut_val", "val"),), exp, what + " ICGN2D2")
        e.close()
        e = eng.NR2D1(2, 2, sc.CONV, sc.STOP)
        e.set_images(ref, tar, layout=layout)
        e.prepare()
        _check(e, NR_FIELDS + IMAGES, exp, what + " NR2D1")
        _zero_borders(e, shape, what + " NR2D1", nr=True)
        e.close()


# ---- 3. buffers used in place at 4-byte alignment -----------------------------------------------------------------------------------
class Carved:
    """A device tensor of `shape` at an offset of k floats inside a larger allocation filled with a sentinel."""

    def __init__(self, torch, host, k, dtype=None):
        host = np.array(host, order="C")      # (a writable copy: torch wraps no read-only array)
        n = host.size
        self.k, self.n = k, n
        self.fill = SENTINEL if host.dtype == np.float32 else -7
        self.buf = torch.full((n + 8,), self.fill, dtype=dtype or torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[k:k + n].view(host.shape)
        self.t.copy_(torch.from_numpy(host))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 * k) % 16

    def intact(self):
        """nothing was written in front of or behind the view"""
        b = self.buf.cpu().numpy()
        return bool((b[:self.k] == self.fill).all() and (b[self.k + self.n:] == self.fill).all())

    def numpy(self):
        return self.t.cpu().numpy()


PAIRS = [(1, 2), (2, 3), (3, 1)]          # (offset of the reference, offset of the target) in floats


@pytest.mark.parametrize("kr,kt", [(0, 0)] + PAIRS)
def test_prepare_fields_of_unaligned_images(eng, torch, kr, kt):
    """offset 0: the 16-byte kernels; any other offset: the scalar ones, although width % 4 == 0"""
    exp = sc.expected2d(sc.ALIGN2D)
    r, t = Carved(torch, exp["ref"], kr), Carved(torch, exp["tar"], kt)
    assert (r.t.data_ptr() % 16 != 0) == (kr != 0) and (t.t.data_ptr() % 16 != 0) == (kt != 0)
    print("2D", (kr, kt), "ICGN2D:", sc.grad2d_kernel_of(sc.ALIGN2D[1], r.t.data_ptr()), "NR2D1:", sc.grad2d_kernel_of(sc.ALIGN2D[1], t.t.data_ptr()))
    for cls, fields in ((eng.ICGN2D1, ICGN_FIELDS + IMAGES), (eng.ICGN2D2, (("lut_val", "val"),)), (eng.NR2D1, NR_FIELDS + IMAGES)):
        e = cls(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP)
        e.set_images(r.t, t.t)
        e.prepare()
        _check(e, fields, exp, "%s at offsets %d, %d" % (cls.__name__, kr, kt))
        if cls is not eng.ICGN2D2:
            _zero_borders(e, sc.ALIGN2D, cls.__name__, nr=cls is eng.NR2D1)
        e.close()
    exp = sc.expected3d(sc.ALIGN3D)
    r, t = Carved(torch, exp["ref"], kr), Carved(torch, exp["tar"], kt)
    print("3D", (kr, kt), sc.grad3d_kernel_of(sc.ALIGN3D[2], r.t.data_ptr()), sc.prefilter3d_kernels_of(sc.ALIGN3D[2], t.t.data_ptr()))
    e = eng.ICGN3D1(sc.ALIGN_R3D_ICGN, sc.ALIGN_R3D_ICGN, sc.ALIGN_R3D_ICGN, sc.CONV, sc.STOP)
    e.set_images(r.t, t.t)
    e.prepare()
    _check(e, FIELDS3D + IMAGES, exp, "ICGN3D1 at offsets %d, %d" % (kr, kt))
    for name, m in zip(("gx", "gy", "gz"), sc.gradient_border(sc.ALIGN3D)):
        assert not sc.bits(e.read_field(name))[m].any(), name
    e.close()
    assert r.intact() and t.intact()


def _guess2d(eng):
    ref, tar = sc.pair(sc.ALIGN2D)
    f = eng.FFTCC2D(sc.ALIGN_R2D, sc.ALIGN_R2D)
    f.set_images(ref, tar)
    q = f.compute(sc.align_queue2d())
    f.close()
    assert (q[:, 16] > 0.5).mean() > 0.9
    return q


def _guess3d(eng):
    ref, tar = sc.pair(sc.ALIGN3D)
    f = eng.FFTCC3D(sc.ALIGN_R3D, sc.ALIGN_R3D, sc.ALIGN_R3D)
    f.set_images(ref, tar)
    q = f.compute(sc.align_queue3d())
    f.close()
    assert (q[:, 18] > 0.5).mean() > 0.9
    return q


# (name, constructor, tuning, starts from the FFTCC guess)
SOLVERS2D = [
    ("FFTCC2D fused", lambda g: g.FFTCC2D(sc.ALIGN_R2D, sc.ALIGN_R2D), {}, False),
    ("FFTCC2D rocFFT", lambda g: g.FFTCC2D(sc.ALIGN_R2D, sc.ALIGN_R2D), {"fftcc2d_fused": 0}, False),
    ("ICGN2D1", lambda g: g.ICGN2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {"arith_fma": 0}, True),
    ("ICGN2D1 fma", lambda g: g.ICGN2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {"arith_fma": 1}, True),
    ("ICGN2D1 onepass", lambda g: g.ICGN2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {"arith_onepass": 1}, True),
    ("ICGN2D2", lambda g: g.ICGN2D2(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {"arith_fma": 0}, True),
    ("ICGN2D2 fma", lambda g: g.ICGN2D2(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {"arith_fma": 1}, True),
    ("ICGN2D2 onepass", lambda g: g.ICGN2D2(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {"arith_onepass": 1}, True),
    ("ICLM2D1", lambda g: g.ICLM2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {}, True),
    ("NR2D1", lambda g: g.NR2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP), {}, True),
]
SOLVERS3D = [
    ("FFTCC3D fused", lambda g: g.FFTCC3D(sc.ALIGN_R3D, sc.ALIGN_R3D, sc.ALIGN_R3D), {}, False),
    ("FFTCC3D rocFFT", lambda g: g.FFTCC3D(sc.ALIGN_R3D, sc.ALIGN_R3D, sc.ALIGN_R3D), {"fftcc3d_fused": 0}, False),
    ("ICGN3D1", lambda g: g.ICGN3D1(sc.ALIGN_R3D_ICGN, sc.ALIGN_R3D_ICGN, sc.ALIGN_R3D_ICGN, sc.CONV, sc.STOP), {}, True),
]


@pytest.mark.parametrize("kr,kt", PAIRS)
@pytest.mark.parametrize("family", ["2D", "3D"])
def test_solvers_on_unaligned_images(eng, torch, family, kr, kt):
    """The same engine, the same data: once as host arrays (uploaded into the engine's own 256-byte aligned buffers), once in place
    at 4-byte alignment.  The images are read through 4-byte buffer loads and plain float indexing only (dic2d_device.h make_rsrc /
    raw_buffer_load_b32, fftcc2d*.hip, fftcc3d*.hip, icgn3d_device.h); the prepare launchers look at the address."""
    shape, solvers, guess, zcol = (sc.ALIGN2D, SOLVERS2D, _guess2d, 16) if family == "2D" else (sc.ALIGN3D, SOLVERS3D, _guess3d, 18)
    ref, tar = sc.pair(shape)
    r, t = Carved(torch, ref, kr), Carved(torch, tar, kt)
    assert r.t.data_ptr() % 16 and r.t.data_ptr() % 4 == 0
    start = guess(eng)
    blank = sc.align_queue2d() if family == "2D" else sc.align_queue3d()
    for name, make, tuning, from_guess in solvers:
        e = make(eng)
        for key, value in tuning.items():
            e.set_tuning(key, value)
        q = start if from_guess else blank
        e.set_images(ref, tar)
        e.prepare()
        want = e.compute(q.copy())
        e.set_images(r.t, t.t)
        e.prepare()
        got = e.compute(q.copy())
        sc.assert_same(got, want, "%s, images at offsets %d, %d" % (name, kr, kt))
        assert (want[:, zcol] > (0.9 if from_guess else 0.5)).mean() > 0.9, (name, want[:, zcol])
        e.close()
    assert r.intact() and t.intact()
    sc.assert_same(r.numpy(), ref, "the reference is read only")
    sc.assert_same(t.numpy(), tar, "the target is read only")


def _device_pair(torch, q, k=1):
    """(the queue carved at k floats, an aligned device copy)"""
    c = Carved(torch, q, k)
    a = torch.from_numpy(np.array(q, order="C")).cuda()
    assert a.data_ptr() % 16 == 0
    return c, a


def _both(torch, c, a, what):
    torch.cuda.synchronize()
    sc.assert_same(c.numpy(), a.cpu().numpy(), what)
    assert c.intact(), what + ": wrote outside the queue"


@pytest.mark.parametrize("family", ["2D", "3D"])
def test_solvers_on_an_unaligned_queue(eng, torch, family):
    """compute() on a device queue whose first record starts 4 bytes past a 16-byte boundary (records are addressed float by
    float everywhere: `pois + idx * stride_f`), images in place at offsets 1 and 3 -- against an aligned copy of the queue."""
    shape, solvers, guess = (sc.ALIGN2D, SOLVERS2D, _guess2d) if family == "2D" else (sc.ALIGN3D, SOLVERS3D, _guess3d)
    ref, tar = sc.pair(shape)
    r, t = Carved(torch, ref, 1), Carved(torch, tar, 3)
    start = guess(eng)
    blank = sc.align_queue2d() if family == "2D" else sc.align_queue3d()
    for name, make, tuning, from_guess in solvers:
        e = make(eng)
        for key, value in tuning.items():
            e.set_tuning(key, value)
        e.set_images(r.t, t.t)
        e.prepare()
        c, a = _device_pair(torch, start if from_guess else blank)
        assert c.t.data_ptr() % 16 == 4
        e.compute(c.t)
        e.compute(a)
        _both(torch, c, a, name + ", queue at an offset of one float")
        e.close()


def test_offsets_selection_split_and_merge_on_unaligned_device_arrays(eng, torch):
    ref, tar = sc.pair(sc.ALIGN2D)
    start = _guess2d(eng)
    n = len(start)
    e = eng.ICGN2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP)
    e.set_images(ref, tar)
    e.prepare()
    # compute_with_offsets: queue and offset array (n, 2) both at one float
    rng = np.random.default_rng(5)
    off = rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32)
    c, a = _device_pair(torch, start)
    oc, oa = _device_pair(torch, off)
    e.compute_with_offsets(c.t, oc.t)
    e.compute_with_offsets(a, oa)
    _both(torch, c, a, "compute_with_offsets")
    assert oc.intact()
    host = e.compute_with_offsets(start.copy(), off)
    sc.assert_same(c.numpy(), host, "compute_with_offsets against the host path")
    # select_best: candidates, segment starts (int32, one integer past a 16-byte boundary) and POIs
    solved = e.compute(start.copy())
    cand = np.repeat(solved, 3, axis=0)
    cand[:, 16] = rng.uniform(0.1, 0.99, len(cand)).astype(np.float32)
    cand[:, 2] = np.arange(len(cand))
    starts = (3 * np.arange(n + 1)).astype(np.int32)
    cc, ca = _device_pair(torch, cand)
    sc_, sa = Carved(torch, starts, 1, dtype=torch.int32), torch.from_numpy(starts).cuda()
    assert sc_.t.data_ptr() % 16 == 4
    pc, pa = _device_pair(torch, start)
    e.select_best(cc.t, sc_.t, pc.t)
    e.select_best(ca, sa, pa)
    _both(torch, pc, pa, "select_best")
    assert cc.intact() and sc_.intact()
    sc.assert_same(pc.numpy(), e.select_best(cand, starts.astype(np.uint32), start.copy()), "select_best against the host path")
    winners = pc.numpy()[:, 2].astype(int)
    assert (winners // 3 == np.arange(n)).all() and len(set(winners % 3)) == 3
    # split_reliable / merge_recovered: queue and the caller's `reliable` buffer at one float
    mixed = solved.copy()
    mixed[::3, 16] = 0.8                    # unreliable: between the thresholds
    mixed[1::7, 18] = 0.5                   # unreliable: not converged
    qc, qa = _device_pair(torch, mixed)
    rc, ra = _device_pair(torch, np.full((n + 2, 25), SENTINEL, np.float32))
    out_c = e.split_reliable(qc.t, 0.7, 0.9, sc.CONV, reliable=rc.t, reliable_offset=2)
    out_a = e.split_reliable(qa, 0.7, 0.9, sc.CONV, reliable=ra, reliable_offset=2)
    torch.cuda.synchronize()
    assert out_c[1] == out_a[1] and out_c[4] == out_a[4] and 0 < out_c[4] < n
    sc.assert_same(rc.numpy(), ra.cpu().numpy(), "split_reliable: reliable")
    nu = out_c[4]
    sc.assert_same(out_c[2][:nu].cpu().numpy(), out_a[2][:nu].cpu().numpy(), "split_reliable: unreliable")
    assert np.array_equal(out_c[3][:nu].cpu().numpy(), out_a[3][:nu].cpu().numpy())
    rel, n_rel, unr, idx, n_unr = e.split_reliable(mixed.copy(), 0.7, 0.9, sc.CONV, reliable=np.full((n + 2, 25), SENTINEL, np.float32), reliable_offset=2)
    assert (n_rel, n_unr) == (out_c[1], out_c[4])
    sc.assert_same(rc.numpy(), rel, "split_reliable against the host path")
    # the unreliable records come back solved: those that pass now return to the queue and join the reliable ones
    back = solved[idx[:n_unr].astype(int)]
    index = idx[:n_unr].astype(np.int32)
    uc, ua = _device_pair(torch, back)
    ic, ia = Carved(torch, index, 1, dtype=torch.int32), torch.from_numpy(index).cuda()
    got_c = e.merge_recovered(qc.t, uc.t, ic.t, n_unr, 0.9, sc.CONV, rc.t, 2 + n_rel)
    got_a = e.merge_recovered(qa, ua, ia, n_unr, 0.9, sc.CONV, ra, 2 + n_rel)
    host_q, host_u, host_i = mixed.copy(), np.concatenate([back, unr[n_unr:]]), idx.copy()
    got_h = e.merge_recovered(host_q, host_u, host_i, n_unr, 0.9, sc.CONV, rel, 2 + n_rel)
    assert got_c == got_a == got_h and got_c[0] > 0 and sum(got_c) == n_unr
    _both(torch, qc, qa, "merge_recovered: queue")
    _both(torch, rc, ra, "merge_recovered: reliable")
    _both(torch, uc, ua, "merge_recovered: unreliable")
    sc.assert_same(qc.numpy(), host_q, "merge_recovered against the host path: queue")
    sc.assert_same(rc.numpy(), rel, "merge_recovered against the host path: reliable")
    assert np.array_equal(ic.numpy()[:got_c[1]], ia.cpu().numpy()[:got_c[1]])
    assert uc.intact() and ic.intact()
    e.close()


def test_strain_and_stereo_on_unaligned_device_arrays(eng, torch):
    from opencorr_amd import P2S
    start = _guess2d(eng)
    ref, tar = sc.pair(sc.ALIGN2D)
    e = eng.ICGN2D1(sc.ALIGN_R2D, sc.ALIGN_R2D, sc.CONV, sc.STOP)
    e.set_images(ref, tar)
    e.prepare()
    solved = e.compute(start.copy())
    e.close()
    # Strain: POI2D records, neighbours within 9 pixels of a 4-pixel grid
    st = eng.Strain(9.0, 5)
    c, a = _device_pair(torch, solved)
    for q in (c.t, a):
        st.prepare(q)
        st.compute(q)
    _both(torch, c, a, "Strain.compute")
    host = solved.copy()
    st.prepare(host)
    st.compute(host)
    sc.assert_same(c.numpy(), host, "Strain.compute against the host path")
    assert (host[:, 20:23] != 0).any()
    st.close()
    # Stereovision: point lists (n, 2) and POI2DS records (n, 28)
    intr1 = np.array([812.5, 799.25, 1.75, 257.3, 166.9, -0.21, 0.083, -0.011, 0.013, -0.0047, 0.0009, 0.0012, -0.0008], dtype=np.float32)
    intr2 = np.array([805.0, 801.5, -0.5, 250.1, 170.2, -0.19, 0.07, 0.004, -0.002, 0.001, 0.0, 0.0005, 0.0003], dtype=np.float32)
    cam1 = eng.Calibration(intr1, np.zeros(6, dtype=np.float32))
    cam2 = eng.Calibration(intr2, np.array([-120.0, 2.5, 11.0, 0.01, 0.21, -0.015], dtype=np.float32))
    for cam in (cam1, cam2):
        cam.prepare(340, 520)
    stereo = eng.Stereovision(cam1, cam2)
    rng = np.random.default_rng(17)
    n = 67
    p1 = np.stack([rng.uniform(60, 440, n), rng.uniform(40, 300, n)], axis=1).astype(np.float32)
    p2 = (p1 + np.stack([rng.uniform(-60, -20, n), rng.uniform(-2, 2, n)], axis=1)).astype(np.float32)
    c1, a1 = _device_pair(torch, p1)
    c2, a2 = _device_pair(torch, p2, k=3)
    got, want = stereo.reconstruct(c1.t, c2.t), stereo.reconstruct(a1, a2)
    torch.cuda.synchronize()
    sc.assert_same(got.cpu().numpy(), want.cpu().numpy(), "Stereovision.reconstruct")
    sc.assert_same(got.cpu().numpy(), stereo.reconstruct(p1, p2), "Stereovision.reconstruct against the host path")
    assert c1.intact() and c2.intact() and np.isfinite(want.cpu().numpy()).all()
    recs = np.zeros((n, 28), dtype=np.float32)
    recs[:, [P2S["x"], P2S["y"]]] = p1
    recs[:, [P2S["r2_x"], P2S["r2_y"]]] = p2
    recs[:, [P2S["t1_x"], P2S["t1_y"]]] = p1 + np.float32(0.75)
    recs[:, [P2S["t2_x"], P2S["t2_y"]]] = p2 + np.float32(0.5)
    c, a = _device_pair(torch, recs)
    stereo.reconstruct_pois(c.t)
    stereo.reconstruct_pois(a)
    _both(torch, c, a, "Stereovision.reconstruct_pois")
    sc.assert_same(c.numpy(), stereo.reconstruct_pois(recs.copy()), "reconstruct_pois against the host path")
    assert (c.numpy()[:, [P2S["u"], P2S["v"], P2S["w"]]] != 0).any()
    stereo.close()
    cam1.close()
    cam2.close()


def test_the_matcher_refuses_an_unaligned_device_block(eng, torch):
    """match.hip reads descriptor rows as float4: capi_match.hip refuses the block before any launch"""
    from opencorr_amd import capi
    rng = np.random.default_rng(3)
    rows = rng.uniform(0, 1, (40, 32)).astype(np.float32)
    m = eng.DescriptorMatcher(32)
    for k in sc.OFFSETS:
        c = Carved(torch, rows, k)
        with pytest.raises(capi.OpenCorrHipError, match="16-byte aligned") as err:
            m.set_descriptors(0, c.t)
        assert err.value.status == capi.ERR_INVALID
    m.set_descriptors(0, Carved(torch, rows, 4).t)       # 16 bytes in: accepted
    m.set_descriptors(1, rows)
    idx, _, _ = m.nearest(0)
    assert (np.asarray(idx) >= -1).all()
    m.close()


# ---- 4. one engine across image sizes -------------------------------------------------------------------------------------------
def _hand_over(e, torch, ref, tar, how):
    from opencorr_amd import capi
    if how == "host":
        e.set_images(ref, tar)
    elif how == "col-major":
        e.set_images(ref, tar, layout=capi.COL_MAJOR)
    else:
        e.set_images(torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(tar.copy()).cuda())


def _refused_before_prepare(e, q):
    from opencorr_amd import capi
    before = q.copy()
    with pytest.raises(capi.OpenCorrHipError, match=re.escape(NOT_PREPARED)):
        e.compute(q)
    assert np.array_equal(sc.bits(q), sc.bits(before)), "a refused compute() touched the queue"


KINDS2D = {
    # name: (constructor from a radius, tuning, fields against the fresh engine and the oracle, set-up cache live)
    "ICGN2D1": (lambda g, r: g.ICGN2D1(r, r, sc.CONV, sc.STOP), {"icgn2d_variant": 5}, ICGN_FIELDS + IMAGES, True),
    "ICGN2D2": (lambda g, r: g.ICGN2D2(r, r, sc.CONV, sc.STOP), {"icgn2d_variant": 4}, ICGN_FIELDS + IMAGES, True),
    "NR2D1": (lambda g, r: g.NR2D1(r, r, sc.CONV, sc.STOP), {}, NR_FIELDS + IMAGES, False),
    "ICLM2D1": (lambda g, r: g.ICLM2D1(r, r, sc.CONV, sc.STOP), {}, ICGN_FIELDS[:3] + IMAGES, False),
    "FFTCC2D": (lambda g, r: g.FFTCC2D(r, r), {}, IMAGES, False),
}


@pytest.mark.parametrize("kind", list(KINDS2D))
def test_one_engine_across_image_sizes_2d(eng, torch, kind):
    make, tuning, fields, cached = KINDS2D[kind]
    solver = kind != "FFTCC2D"

    def build(r):
        e = make(eng, r)
        for key, value in tuning.items():
            e.set_tuning(key, value)
        return e

    old = build(sc.SEQUENCE2D[0][2])
    radius = sc.SEQUENCE2D[0][2]
    for step, (shape, how, r) in enumerate(sc.SEQUENCE2D):
        what = "%s step %d (%dx%d %s, r = %d)" % (kind, step, shape[0], shape[1], how, r)
        ref, tar = sc.pair(shape)
        exp = sc.expected2d(shape, "pair")
        blank = sc.sequence_queue2d(shape, r)
        if solver:
            f = eng.FFTCC2D(r, r)
            f.set_images(ref, tar)
            start = f.compute(blank.copy())
            f.close()
        else:
            start = blank
        if r != radius:
            old.set_subset(r, r)
            radius = r
        fresh = build(r)
        results = []
        for e in (old, fresh):
            _hand_over(e, torch, ref, tar, how)
            if solver:
                _refused_before_prepare(e, start.copy())
            e.prepare()
            _check(e, fields, exp, what + (" long-lived" if e is old else " fresh"))
            got, states = [], []
            for _ in range(2):
                got.append(e.compute(start.copy()))
                if cached:
                    states.append(e.setup_cache_last())
            # "fill" on the first compute() after every new pair, "use" on the second
            assert states == (["fill", "use"] if cached else []), (what, "long-lived" if e is old else "fresh", states)
            results.append(got)
        for k in range(2):
            sc.assert_same(results[0][k], results[1][k], "%s, compute() %d: long-lived against fresh" % (what, k + 1))
        sc.assert_same(results[1][1], results[1][0], what + ": second compute()")
        z = results[1][0][:, 16]
        assert (z > (0.9 if solver else 0.5)).mean() > 0.85, (what, z)
        fresh.close()
    old.close()


KINDS3D = {
    "FFTCC3D": (lambda g, r: g.FFTCC3D(r, r, r), IMAGES),
    "ICGN3D1": (lambda g, r: g.ICGN3D1(r, r, r, sc.CONV, sc.STOP), FIELDS3D + IMAGES),
}


@pytest.mark.parametrize("kind", list(KINDS3D))
def test_one_engine_across_image_sizes_3d(eng, torch, kind):
    make, fields = KINDS3D[kind]
    solver = kind == "ICGN3D1"
    own = (lambda r: sc.SEQUENCE_R3D_ICGN[r]) if solver else (lambda r: r)
    radius = sc.SEQUENCE3D[0][2]
    old = make(eng, own(radius))
    for step, (shape, how, r) in enumerate(sc.SEQUENCE3D):
        what = "%s step %d (%s, r = %d)" % (kind, step, "x".join(map(str, shape)), own(r))
        ref, tar = sc.pair(shape)
        exp = sc.expected3d(shape, "pair")
        blank = sc.sequence_queue3d(shape, r)
        if solver:
            f = eng.FFTCC3D(r, r, r)
            f.set_images(ref, tar)
            start = f.compute(blank.copy())
            f.close()
        else:
            start = blank
        if r != radius:
            old.set_subset(own(r), own(r), own(r))
            radius = r
        fresh = make(eng, own(r))
        results = []
        for e in (old, fresh):
            _hand_over(e, torch, ref, tar, how)
            if solver:
                _refused_before_prepare(e, start.copy())
            e.prepare()
            _check(e, fields, exp, what + (" long-lived" if e is old else " fresh"))
            results.append([e.compute(start.copy()), e.compute(start.copy())])
        for k in range(2):
            sc.assert_same(results[0][k], results[1][k], "%s, compute() %d: long-lived against fresh" % (what, k + 1))
        z = results[1][0][:, 18]
        assert (z > (0.9 if solver else 0.5)).mean() > 0.85, (what, z)
        fresh.close()
    old.close()


def test_a_borrower_keeps_the_pair_it_borrowed(eng, torch):
    """share_images hands the borrower a reference to the donor's pair (`img` is a shared_ptr): new images on the donor leave the
    borrower on the pair it borrowed -- across compute() and prepare() -- until it borrows again."""
    (shape_a, _, r), (shape_b, _, _) = sc.SEQUENCE2D[0], sc.SEQUENCE2D[1]
    ref_a, tar_a = sc.pair(shape_a)
    ref_b, tar_b = sc.pair(shape_b)
    exp_a, exp_b = sc.expected2d(shape_a, "pair"), sc.expected2d(shape_b, "pair")
    donor = eng.FFTCC2D(r, r)
    donor.set_images(ref_a, tar_a)
    start = donor.compute(sc.sequence_queue2d(shape_a, r))
    e = eng.ICGN2D1(r, r, sc.CONV, sc.STOP)
    e.share_images(donor)
    e.prepare()
    _check(e, ICGN_FIELDS + IMAGES, exp_a, "borrower")
    want = e.compute(start.copy())
    assert (want[:, 16] > 0.9).mean() > 0.85
    donor.set_images(ref_b, tar_b)
    _check(donor, IMAGES, exp_b, "donor after new images")
    sc.assert_same(e.compute(start.copy()), want, "borrower after the donor received new images")
    _check(e, ICGN_FIELDS + IMAGES, exp_a, "borrower after the donor received new images")
    e.prepare()
    _check(e, ICGN_FIELDS + IMAGES, exp_a, "borrower after another prepare()")
    sc.assert_same(e.compute(start.copy()), want, "borrower after another prepare()")
    e.share_images(donor)
    _refused_before_prepare(e, start.copy())
    e.prepare()
    _check(e, ICGN_FIELDS + IMAGES, exp_b, "borrower after borrowing again")
    e.close()
    donor.close()


def test_a_borrower_keeps_device_images_alive(eng, torch):
    """A pair used in place on the device is caller memory.  The borrower holds it like the donor does: when the donor moves on
    and the caller drops the tensors, the borrower still computes on them."""
    import gc
    import weakref
    shape, _, r = sc.SEQUENCE2D[3]
    ref, tar = sc.pair(shape)
    exp = sc.expected2d(shape, "pair")
    rt, tt = torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(tar.copy()).cuda()
    alive = [weakref.ref(rt), weakref.ref(tt)]
    donor = eng.FFTCC2D(r, r)
    donor.set_images(rt, tt)
    start = donor.compute(sc.sequence_queue2d(shape, r))
    e = eng.ICGN2D1(r, r, sc.CONV, sc.STOP)
    e.share_images(donor)
    e.prepare()
    want = e.compute(start.copy())
    del rt, tt
    donor.set_images(*sc.pair(sc.SEQUENCE2D[1][0]))
    gc.collect()
    assert all(w() is not None for w in alive), "the borrower's images were released with the donor's"
    filler = torch.full((2 * ref.size + 64,), 3.25, device="cuda")          # what would land in a released block
    e.prepare()
    _check(e, ICGN_FIELDS + IMAGES, exp, "borrower of a device pair")
    sc.assert_same(e.compute(start.copy()), want, "borrower of a device pair after the donor moved on")
    del filler
    e.close()
    donor.close()

"""tests/shape_cases.py on the oracle alone (CPU, runs everywhere): the case lists hit what they claim, and what is expected of
them is sharp -- an operation order other than the reference's changes at least one float of every field.

What tests/test_gpu_shape_cases.py relies on.
"""
import numpy as np
import pytest

import oracle
import shape_cases as sc


def test_shapes_are_what_the_issue_lists():
    want = [(5, 5), (5, 8), (6, 7), (8, 5)]
    want += [(h, w) for w in (12, 13) for h in (15, 16, 17, 18, 31, 33)]
    want += [(31, 33), (32, 32), (33, 31), (5, 70), (70, 5), (64, 96)]
    assert set(want) <= set(sc.SHAPES2D)
    widths = {w for h, w in sc.SHAPES2D if 5 <= h <= 7}
    assert {1020, 1024, 1028, 255, 257, 513} <= widths
    assert len(set(sc.SHAPES2D)) == len(sc.SHAPES2D)
    assert all(h >= sc.MIN2D and w >= sc.MIN2D and h * w <= 130000 for h, w in sc.SHAPES2D)
    assert sc.SHAPES3D_MIN == [(15, 15, 15), (15, 16, 20), (16, 15, 17)]
    assert all(min(s) == sc.MIN3D for s in sc.SHAPES3D_MIN)


def test_both_kernels_of_every_family_are_selected():
    kernels = {sc.grad2d_kernel_of(w) for _, w in sc.SHAPES2D}
    assert kernels == {"grad2d4_kernel", "grad2d_kernel"}
    assert {sc.grad3d_kernel_of(s[2]) for s in sc.SHAPES3D_MIN} == {"grad3d4_kernel", "grad3d_kernel"}
    assert {sc.prefilter3d_kernels_of(s[2]) for s in sc.SHAPES3D_MIN} == {"x4 + walk4", "x + walk"}
    # alignment alone decides on the ALIGN pairs: the vector kernels at offset 0, the scalar ones at 1, 2 and 3 floats -- on
    # either side (the launchers OR the addresses together; the engine's own buffers are 256-byte aligned)
    base = 0x7f0000000000
    for w, grad, pre in ((sc.ALIGN2D[1], sc.grad2d_kernel_of, None), (sc.ALIGN3D[2], sc.grad3d_kernel_of, sc.prefilter3d_kernels_of)):
        assert w % 4 == 0
        assert grad(w, base, base + 256).endswith("4_kernel")
        for k in sc.OFFSETS:
            assert not grad(w, base + 4 * k, base + 256).endswith("4_kernel")
            if pre:
                assert pre(w, base + 4 * k, base + 256, base + 512) == "x + walk"
    assert sc.prefilter3d_kernels_of(sc.ALIGN3D[2], base, base + 256) == "x4 + walk4"


def test_every_edge_has_a_shape():
    have = {}
    for shape in sc.SHAPES2D:
        for e in sc.edges2d(*shape):
            have.setdefault(e, []).append(shape)
    assert set(have) == set(sc.EDGES2D), set(sc.EDGES2D) ^ set(have)
    # what the restated grid says about the shapes the issue names
    assert sc.grad2d_grid(5, 1020) == (255, 1, 1) and sc.grad2d_grid(6, 1024) == (256, 1, 1) and sc.grad2d_grid(7, 1028) == (1, 2, 1)
    assert sc.grad2d_grid(5, 255) == (255, 1, 5) and sc.grad2d_grid(6, 257) == (1, 2, 6) and sc.grad2d_grid(7, 513) == (1, 3, 7)
    assert sc.grad2d_grid(33, 12) == (3, 1, 3) and sc.grad2d_grid(33, 13) == (13, 1, 33)
    assert have["vector, below the walk"] and (15, 12) in have["vector, below the walk"]
    assert have["vector, one walk"] == [(16, 12)] and sorted(have["vector, just past the walk"]) == [(17, 12), (18, 12)]
    assert sorted(have["scalar, walk heights"]) == [(h, 13) for h in (15, 16, 17, 18, 31, 33)]
    assert sc.transposer_tiles(31, 33) == (2, 1, 1, 31) and sc.transposer_tiles(33, 31) == (1, 2, 31, 1)
    assert sc.transposer_tiles(32, 32) == (1, 1, 32, 32) and sc.transposer_tiles(64, 96) == (3, 2, 32, 32)
    assert sc.transposer_tiles(5, 70) == (3, 1, 6, 5) and sc.transposer_tiles(70, 5) == (1, 3, 5, 6)
    # the alignment and re-use cases: sizes that change every image-dependent quantity both ways
    sizes = [s[0] * s[1] for s, _, _ in sc.SEQUENCE2D]
    assert sizes[0] == sizes[-1] == max(sizes) and sizes[1] == min(sizes) and len({s for s, _, _ in sc.SEQUENCE2D}) == 4
    assert [how for _, how, _ in sc.SEQUENCE2D] == ["host", "host", "col-major", "device", "host"]
    assert sum(a[2] != b[2] for a, b in zip(sc.SEQUENCE2D, sc.SEQUENCE2D[1:])) >= 2       # set_subset before two of the steps
    assert [s for s, _, _ in sc.SEQUENCE3D] == [(24, 26, 28), (15, 16, 20), (20, 33, 17), (24, 26, 28)]


def test_images_have_fractional_values():
    for shape in sc.SHAPES2D + sc.SHAPES3D_MIN:
        for a in sc.noise(shape):
            assert a.dtype == np.float32 and a.shape == tuple(shape) and a.flags.c_contiguous
            assert (sc.bits(a) & 0xFF != 0).mean() > 0.9      # full mantissas
    for shape in [sc.ALIGN2D, sc.ALIGN3D] + [s for s, _, _ in sc.SEQUENCE2D + sc.SEQUENCE3D]:
        for a in sc.pair(shape):
            assert a.dtype == np.float32 and a.shape == tuple(shape) and (a != np.round(a)).mean() > 0.99 and a.min() > 0


@pytest.mark.parametrize("shape", sc.SHAPES2D + [sc.ALIGN2D], ids=lambda s: "%dx%d" % s)
def test_expected_fields_are_sharp(shape):
    """The NumPy restatement in the reference's order IS the oracle's field; the four gradient terms taken last to first, and the
    table's sum with n as the outer loop, each change at least one float -- so a kernel that reassociates cannot pass."""
    h, w = shape
    exp = sc.expected2d(shape)
    gx, gy = sc.gradient2d_numpy(exp["ref"])
    assert np.array_equal(sc.bits(gx), sc.bits(exp["gx"])) and np.array_equal(sc.bits(gy), sc.bits(exp["gy"]))
    rx, ry = sc.gradient2d_numpy(exp["ref"], reverse=True)
    # (every shape has an interior: h, w >= 5 leaves columns 2 ... w - 3 and rows 1 ... h - 3)
    assert (sc.bits(rx) != sc.bits(gx)).any(), "gx does not see the order of its four terms"
    assert (sc.bits(ry) != sc.bits(gy)).any(), "gy does not see the order of its four terms"
    # ... and on the target, whose gradients NR2D1 tabulates
    tx, ty = sc.gradient2d_numpy(exp["tar"])
    assert np.array_equal(sc.bits(tx), sc.bits(exp["nr_gx"])) and np.array_equal(sc.bits(ty), sc.bits(exp["nr_gy"]))
    for img, key in ((exp["tar"], "lut"), (exp["nr_gx"], "lut_gx"), (exp["nr_gy"], "lut_gy")):
        lut = sc.bspline2d_lut_numpy(img)
        assert np.array_equal(sc.bits(lut), sc.bits(exp[key])), key
        other = sc.bspline2d_lut_numpy(img, n_outer=True)
        # (swapping the m and n loops reorders a sum only where its non-zero terms span two rows AND two columns: the x gradient
        # of a 5-pixel-wide image is one column, its table a sum along n alone whichever loop is outside)
        nz = img != 0
        if nz.any(axis=1).sum() >= 2 and nz.any(axis=0).sum() >= 2:
            assert (sc.bits(other) != sc.bits(lut)).any(), key + " does not see its loop order"
    # the zero borders hold +0 bits, the value plane is the table's leading coefficient
    mx, my = sc.gradient_border(shape)
    assert not (sc.bits(exp["gx"])[mx]).any() and not (sc.bits(exp["gy"])[my]).any()
    assert not sc.bits(exp["lut"])[sc.lut_border(shape)].any()
    assert np.array_equal(sc.bits(exp["val"]), sc.bits(exp["lut"][..., 0]))
    assert (~mx).sum() == h * (w - 4) and (~my).sum() == (h - 4) * w and (~sc.lut_border(shape)).sum() == (h - 3) * (w - 3)


def test_solver_pairs_converge_on_the_oracle():
    """The queues of the alignment and re-use tests are not empty and the textures are ones the solvers converge on."""
    Z = oracle.P2["zncc"]
    for shape, r, q in [(sc.ALIGN2D, sc.ALIGN_R2D, sc.align_queue2d())] + [(s, r, sc.sequence_queue2d(s, r)) for s, _, r in sc.SEQUENCE2D]:
        assert 20 <= len(q) <= 400, (shape, len(q))
        ref, tar = sc.pair(shape)
        oracle.fftcc2d(ref, tar, r, r, q)
        assert (q[:, Z] > 0.5).mean() > 0.9, (shape, "FFTCC")
        assert (q[:, oracle.P2["u"]] != 0).any() or (q[:, oracle.P2["v"]] != 0).any()
        prep = oracle.Prepared2D(ref, tar)
        oracle.icgn2d1(prep, r, r, sc.CONV, sc.STOP, q, order=oracle.ORDER_LANES, lanes=64)
        assert (q[:, Z] > 0.9).mean() > 0.9, (shape, "ICGN2D1", q[:, Z])
    Z = oracle.P3["zncc"]
    cases = [(sc.ALIGN3D, sc.ALIGN_R3D, sc.ALIGN_R3D_ICGN, sc.align_queue3d())]
    cases += [(s, r, sc.SEQUENCE_R3D_ICGN[r], sc.sequence_queue3d(s, r)) for s, _, r in sc.SEQUENCE3D[:3]]
    for shape, r, ri, q in cases:
        assert 20 <= len(q) <= 400, (shape, len(q))
        ref, tar = sc.pair(shape)
        oracle.fftcc3d(ref, tar, r, r, r, q)
        assert (q[:, Z] > 0.5).mean() > 0.9, (shape, "FFTCC3D", q[:, Z])
        prep = oracle.Prepared3D(ref, tar)
        oracle.icgn3d1(prep, ri, ri, ri, sc.CONV, sc.STOP, q, order=oracle.GPU_ORDER_3D, lanes=oracle.GPU_LANES_3D)
        assert (q[:, Z] > 0.9).mean() > 0.9, (shape, "ICGN3D1", q[:, Z])

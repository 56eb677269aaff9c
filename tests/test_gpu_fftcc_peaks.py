"""FFTCC peak search and decode at every surface position: the eleven restatements of the reference's tail (the strict-'>' scan with
"lowest linear index wins" across lanes, waves and workgroups, then `du = idx % sw; if (du > rx) du -= sw; ...`,
src/oc_fftcc.cpp:246-266, 391-416) on queues whose peak is PLANTED (tests/fftcc_peak_cases.py): all positions of the surface where it
has at most 1 024, otherwise every combination of the seam values of every axis plus random ones.

The expectation is a closed form -- nothing here reads the oracle or the reference:
  * u, v(, w), u0, v0(, w0) equal it on EVERY record, from the single-kernel path and from the rocFFT pipeline;
  * every other float of the record keeps the input's bits (they are filled with noise, not zeros);
  * |ZNCC - 1| <= 4 x the compiled reference's own distance from 1 on these queues (fftcc_peak_cases.MEASURED, per family), and
    within the project's bar against the exact value (2D 1e-5, 3D 1e-4).  A rolled copy differs from the original by a phase in
    every bin, so one wrong twiddle or mirror bin costs about 1/M of the peak: 1e-3 at 32 x 32, 2.4e-4 at 64 x 64.
The measured GPU maxima are printed (pytest -s) and kept beside the bars in DESIGN.md section 3.
"""
import numpy as np
import pytest

import fftcc_peak_cases as pc

pytestmark = pytest.mark.gpu

TILE_QUEUE = 2048     # the 3D single-kernel paths visit a queue in cubic blocks ("fftcc3d_tile_vox") from this many records on


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(got, queue, expected, nd, family, what):
    P = pc.P2 if nd == 2 else pc.P3
    out = pc.OUT2D if nd == 2 else pc.OUT3D
    ints = [c for c in out if c != P["zncc"]]
    wrong = np.flatnonzero((got[:, ints] != expected[:, ints]).any(axis=1))
    assert wrong.size == 0, (what, "%d of %d records" % (wrong.size, len(got)), wrong[:8].tolist(),
                             got[wrong[0], ints].tolist(), expected[wrong[0], ints].tolist())
    rest = [c for c in range(queue.shape[1]) if c not in out]
    assert np.array_equal(_bits(got[:, rest]), _bits(queue[:, rest])), what
    dist = float(np.abs(got[:, P["zncc"]].astype(np.float64) - 1.0).max())
    print("zncc %dD %-9s %-48s max |ZNCC - 1| = %.3e  (bar %.3e)" % (nd, family, what, dist, pc.bar(nd, family)))
    assert dist <= pc.bar(nd, family), (what, dist, pc.bar(nd, family))
    return dist


# ---- 2D ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guess,frac", [((0, 0), 0.0), ((3, -2), 0.5), ((-1.75, 2.25), 0.0)], ids=["plain", "int_guess_half_pixel", "fractional_guess"])
def test_fftcc2d_r16_every_position_every_body(guess, frac):
    """fftcc2d_fused32x2 on all 1 024 positions: the four <FAST_ROWS, REAL_LAST> bodies ("fftcc2d_fused" = 1, 3, 4, 5), the generic
    kernel on 32 x 32 (2) and the rocFFT pipeline (0); at half-pixel positions with an integer guess; with a fractional guess, where
    the wave takes the slow row path."""
    import opencorr_amd
    ref, tar, queue, expected = pc.queue2d(16, 16, guess, frac)
    assert len(queue) == 1024
    f = opencorr_amd.FFTCC2D(16, 16)
    f.set_images(ref, tar)
    for body in (1, 3, 4, 5, 2, 0):
        f.set_tuning("fftcc2d_fused", body)
        _check(f.compute(queue.copy()), queue, expected, 2, "fused32x2", "r16 fftcc2d_fused=%d guess %s frac %s" % (body, guess, frac))
    f.close()


CASES2D = [(fam, r) for fam in ("fusedn", "fusedr", "rect", "pipeline") for r in pc.FAMILIES2D[fam]]


@pytest.mark.parametrize("family,radii", CASES2D, ids=["%s_%dx%d" % (f, r[0], r[1]) for f, r in CASES2D])
def test_fftcc2d_every_shape(family, radii):
    """fftcc2d_fusedn / fusedp (29 squares), fusedr (42 instantiated pairs), fftcc2d_rect (33 run-time shapes) and the pipeline
    alone (sides above 64): the single kernel, then the rocFFT pipeline on the same queue."""
    import opencorr_amd
    rx, ry = radii
    ref, tar, queue, expected = pc.queue2d(rx, ry)
    f = opencorr_amd.FFTCC2D(rx, ry)
    f.set_images(ref, tar)
    if (rx, ry) == (16, 16):
        f.set_tuning("fftcc2d_fused", 2)       # fftcc2d_fusedn's instance, not fftcc2d_fused.hip
    _check(f.compute(queue.copy()), queue, expected, 2, family, "%s %s" % (family, radii))
    if family != "pipeline":
        f.set_tuning("fftcc2d_fused", 0)
        _check(f.compute(queue.copy()), queue, expected, 2, family, "%s %s pipeline" % (family, radii))
    f.close()


# ---- 3D ----------------------------------------------------------------------------------------------------------------------------
CASES3D = [(fam, r) for fam in ("fusedn", "fused32", "planes", "box", "pipeline") for r in pc.FAMILIES3D[fam]]


@pytest.mark.parametrize("family,radii", CASES3D, ids=["%s_%dx%dx%d" % ((f,) + r) for f, r in CASES3D])
def test_fftcc3d_every_shape(family, radii):
    """fftcc3d_fusedn (r = 4 ... 13), fftcc3d_fused32 (16), fftcc3d_planes (every instantiated side 28 ... 64 but 32), fftcc3d_box (one
    shape per line length on each axis, and two whose three sides all differ) and the pipeline through "fftcc3d_fused" = 0."""
    import opencorr_amd
    ref, tar, queue, expected = pc.queue3d(*radii)
    f = opencorr_amd.FFTCC3D(*radii)
    f.set_images(ref, tar)
    if family != "pipeline":
        _check(f.compute(queue.copy()), queue, expected, 3, family, "%s %s" % (family, radii))
    f.set_tuning("fftcc3d_fused", 0)
    _check(f.compute(queue.copy()), queue, expected, 3, family, "%s %s pipeline" % (family, radii))
    f.close()


@pytest.mark.parametrize("family,radii", [("fusedn", (4, 4, 4)), ("fused32", (16, 16, 16)), ("planes", (14, 14, 14)), ("box", (4, 6, 8))])
def test_fftcc3d_planted_queue_in_block_order(family, radii):
    """The queue repeated to 2 048 records, the length from which the single-kernel paths visit it in cubic blocks: default blocks,
    8-voxel blocks and queue order; every repetition must give the records of the first."""
    import opencorr_amd
    ref, tar, queue, expected = pc.queue3d(*radii)
    reps = -(-TILE_QUEUE // len(queue))
    big, want = np.tile(queue, (reps, 1)), np.tile(expected, (reps, 1))
    assert len(big) >= TILE_QUEUE
    f = opencorr_amd.FFTCC3D(*radii)
    f.set_images(ref, tar)
    for tile_vox in (64, 8, 0):
        f.set_tuning("fftcc3d_tile_vox", tile_vox)
        _check(f.compute(big.copy()), big, want, 3, family, "%s %s x%d tile_vox=%d" % (family, radii, reps, tile_vox))
    f.close()

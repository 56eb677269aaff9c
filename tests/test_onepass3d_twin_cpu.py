"""The one-pass arithmetic contract of ICGN3D1 (`oc_hip_set_tuning("arith_onepass3d", 1)`) on the CPU.

tests/cpp/icgn3d_onepass_twin.cpp restates the contract -- one sweep per iteration over e' = g (t - c) - r~ with 3 + 12 running
sums in the 512-lane association of the kernel, the mean / norm / ZNSSD / numerator recovered from them --
and the kernel equals it bit for bit (tests/test_gpu_arith_onepass3d.py).  Here the twin itself meets the distance bars the
other two contracts meet: against the reference's loop order (oracle.ORDER_SEQ) and against the float64 model of the iteration.
No GPU.
"""
import numpy as np
import pytest

import icgn_model64 as m64
import onepass3d_twin as twin
import oracle


@pytest.fixture(scope="module")
def small_case():
    ref, tar = twin.small_pair()
    return twin.grid_queue(ref, tar), oracle.Prepared3D(ref, tar)


@pytest.mark.parametrize("r", [(8, 8, 8), (5, 7, 6)])
def test_twin_against_the_reference_order(small_case, r):
    """The four conditions the header states for `arith_fma`, for the one-pass contract: identical failure codes, >= 99.5 %
    identical iteration counts, |d u|, |d v|, |d w| <= 1e-4 and |d ZNCC| <= 1e-5 against ORDER_SEQ -- and another arithmetic than
    the fused contract's, not a renamed one."""
    pois, prep = small_case
    rx, ry, rz = r
    seq = pois.copy()
    oracle.icgn3d1(prep, rx, ry, rz, 0.001, 20, seq, order=oracle.ORDER_SEQ)
    got = twin.icgn3d1(prep, rx, ry, rz, 0.001, 20, pois.copy())
    res = twin.vs_reference_order(got, seq)
    print("r %s: code mismatches %d, equal iterations %.5f (%d POIs), max |d disp| %.3e, max |d zncc| %.3e, converged %d of %d"
          % (r, int(res["code_mismatch"].sum()), res["iteration_agreement"], res["same_it"], res["max_abs_d_disp"],
             res["max_abs_d_zncc"], int((got[:, 18] >= 0).sum()), len(got)))
    assert (got[-4:, 18] == np.float32([-3, -3, -1, -3])).all()
    assert not res["code_mismatch"].any()
    assert res["iteration_agreement"] >= 0.995
    assert res["max_abs_d_disp"] <= 1e-4
    assert res["max_abs_d_zncc"] <= 1e-5
    assert (got[:-4, 18] >= 0).all()
    # fields the solver does not write stay untouched, and so does everything but the flag of a failed record
    P = oracle.P3
    untouched = [c for c in range(31) if c in (0, 1, 2) or (c > P["convergence"] and c < 28)]
    assert np.array_equal(got[:, untouched].view(np.uint32), pois[:, untouched].view(np.uint32))
    keep = [c for c in range(31) if c != P["zncc"]]
    assert np.array_equal(got[-4:][:, keep].view(np.uint32), pois[-4:][:, keep].view(np.uint32))
    fma = pois.copy()
    oracle.icgn3d1(prep, rx, ry, rz, 0.001, 20, fma, order=oracle.ORDER_LANES_FMA, lanes=512)
    assert not np.array_equal(got[:-4].view(np.uint32), fma[:-4].view(np.uint32))


def test_twin_3d_within_the_bars_of_the_float64_model():
    """tests/icgn_model64.py, families 3D and 3DE: the state after exactly k = 1 ... 5 iterations and the ordinary run, every
    field group (ZNCC included) inside the committed bars -- 4 x the compiled reference's own distance from the model."""
    cs = m64.cases3d()
    models = [m64.model_runs(c) for c in cs]

    def run(case, conv, stop):
        _, r, _, _, prep, _, pois = case
        return twin.icgn3d1(prep, r[0], r[1], r[2], conv, stop, pois.copy())

    dist, exc = m64.measure(cs, run, models)
    lines, bad = m64.check_within_bars(dist, "one-pass 3D twin")
    print("\n".join(lines))
    print("one-pass 3D twin one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)


def test_the_element_path_poi_is_not_a_box():
    """The GPU file runs one POI whose reference subvolume must be addressed per element (Subset3D::fill truncates
    float(start + k) per element): x = 13 - 2^-20 with rx = 5.  There float32(start + 10) rounds up to 18 while the box that
    starts at int(start) = 7 has 17 -- the case is not vacuous.  The other off-grid centres are boxes."""
    per_element, box = twin.reference_indices(twin.ELEMENT_PATH_X, twin.ELEMENT_PATH_RX)
    assert per_element[10] == 18 and box[10] == 17
    assert (per_element != box).any()
    pois = twin.offgrid_queue()
    assert pois[0, 0] == twin.ELEMENT_PATH_X
    for row in pois[1:]:
        for c, r in zip(row[:3], (5, 7, 6)):
            pe, bx = twin.reference_indices(c, r)
            assert np.array_equal(pe, bx)
    assert (pois[1:, :3] != np.floor(pois[1:, :3])).any(axis=1).all()


def test_twin_reads_the_reference_per_element():
    """... and the twin follows the per-element indices, as the reference's loop does.  Directly: the element-path POI (record 0)
    reads the reference columns 7 ... 15, 17 and 18, never 16 (a box would read 7 ... 17).  Overwriting column 16 of the reference
    volume (the gradients keep their values) leaves its record unchanged in every bit; overwriting column 18 changes it.  Against
    ORDER_SEQ, which indexes per element too, the whole off-grid queue stays inside the bars."""
    import copy
    ref, tar = twin.small_pair()
    prep = oracle.Prepared3D(ref, tar)
    pois = twin.offgrid_queue()
    per_element, box = twin.reference_indices(pois[0, 0], 5)
    assert sorted(set(box) - set(per_element)) == [16] and sorted(set(per_element) - set(box)) == [18]
    got = twin.icgn3d1(prep, 5, 7, 6, 0.001, 20, pois.copy())
    for column, same in ((16, True), (18, False)):
        other = copy.copy(prep)
        other.ref = prep.ref.copy()
        other.ref[:, :, column] = 255.0 - other.ref[:, :, column]
        again = twin.icgn3d1(other, 5, 7, 6, 0.001, 20, pois[:1].copy())
        assert np.array_equal(again.view(np.uint32), got[:1].view(np.uint32)) == same, column
    seq = pois.copy()
    oracle.icgn3d1(prep, 5, 7, 6, 0.001, 20, seq, order=oracle.ORDER_SEQ)
    res = twin.vs_reference_order(got, seq)
    assert not res["code_mismatch"].any()
    assert res["iteration_agreement"] >= 0.995 and (got[:, 18] >= 0).all()
    assert res["max_abs_d_disp"] <= 1e-4 and res["max_abs_d_zncc"] <= 1e-5


def _csrc(name):
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "opencorr_amd", "csrc", name)) as fh:
        return fh.read()


def _code(text, first, last):
    """The statements from the line that starts with ``first`` to the line that starts with ``last``: comments and blank lines
    dropped, white space squeezed."""
    import re
    lines = text.split("\n")
    a = next(i for i, l in enumerate(lines) if l.strip().startswith(first))
    b = next(i for i in range(a, len(lines)) if lines[i].strip().startswith(last))
    out = []
    for l in lines[a:b + 1]:
        l = re.sub(r"\s+", " ", l.split("//")[0]).strip()
        if l:
            out.append(l)
    return out


def test_the_copied_launch_rule_and_box_block_are_the_default_kernels():
    """icgn3d_onepass.hip restates the default kernel's launch-shape rule and its coefficient-box / staging block (icgn3d.hip keeps
    its code, so nothing is shared).  A later tuning of the default must not leave the one-pass kernel on the old shape silently:
    the statements are compared here, and whoever changes one side sees this test."""
    a, b = _csrc("icgn3d.hip"), _csrc("icgn3d_onepass.hip")
    rule = ("const int want = 2 * p.rx + 1 + 5;", "(void)hipGetLastError();")
    ra, rb = _code(a, *rule), _code(b, *rule)
    assert len(ra) > 12 and ra == rb
    assert "grid = (grid + 7) / 8 * 8;" in a and "grid = (grid + 7) / 8 * 8;" in b
    box = ("const int M = P.samples_per_pass;", "for (int m = 0; m < M; m++, w.next()) {")
    ba, bb = _code(a, *box), _code(b, *box)
    # the one-pass walk also carries the voxel offset of the sample's reference voxel; the default's ablation switch is not there
    ba = [l.replace("Walk3 w(tid, SX, SY, round0 * M);", "Walk3 w(tid, SX, SY, round0 * M, DX, DY);")
           .replace("if (staged && !(OC_ABLATE & 1)) {", "if (staged) {") for l in ba]
    assert len(ba) > 80 and ba == bb

"""The one-pass arithmetic contract of ICGN3D1 on the GPU (`oc_hip_set_tuning("arith_onepass3d", 1)`).

An iteration is the tap sweep alone: every sample forms e' = g (t - c) - r~ and joins 3 + 12 running sums, nothing is stored, and
mean, norm, ZNSSD and numerator are recovered from the sums after one block reduction (opencorr_amd/csrc/icgn3d_onepass.hip,
DESIGN.md section 3).  Not bit-identical to the other two contracts: it is pinned on its own CPU restatement,
tests/cpp/icgn3d_onepass_twin.cpp, which the kernel must equal in EVERY bit -- untouched fields and the records of rejected POIs
included -- and it meets the bars of the float64 model (tests/test_onepass3d_twin_cpu.py asserts the distances of the twin on the
CPU).  The queues are those of tests/test_gpu_parity_3d.py (built in tests/onepass3d_twin.py): the smallest at which each mechanism
of the kernel can go wrong.
"""
import numpy as np
import pytest

import icgn_model64 as m64
import onepass3d_twin as twin

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same_bits(got, want, what=""):
    mism = np.argwhere(_bits(got) != _bits(want))
    assert mism.size == 0, (what, len(mism), "first mismatches (poi, field): %s" % mism[:10].tolist())


@pytest.fixture(scope="module")
def eng():
    import opencorr_amd
    return opencorr_amd


@pytest.fixture(scope="module")
def small():
    import oracle
    ref, tar = twin.small_pair()
    return ref, tar, oracle.Prepared3D(ref, tar), twin.grid_queue(ref, tar)


@pytest.fixture(scope="module")
def big():
    import oracle
    ref, tar = twin.big_pair()
    return ref, tar, oracle.Prepared3D(ref, tar)


def _engine(eng, r, ref, tar, conv=0.001, stop=20):
    icgn = eng.ICGN3D1(r[0], r[1], r[2], conv, stop)
    icgn.set_images(ref, tar)
    icgn.prepare()
    icgn.set_tuning("arith_onepass3d", 1)
    return icgn


# (8,8,8): 4 913 samples = 9 x 512 + 305; (5,7,6): 2 145 = 4 x 512 + 97; (3,3,3): 343 < 512 -- lanes and whole waves without a sample
@pytest.mark.parametrize("r", [(8, 8, 8), (5, 7, 6), (3, 3, 3)])
def test_gpu_equals_twin_bit_for_bit(eng, small, r):
    """The 4 x 3 x 3 grid with FFTCC3D guesses and the four trippers (guard reject, out of the volume inside the loop, rejected on
    entry with its flag kept, NaN guess); queues of 1, 12 and all 40 records."""
    ref, tar, prep, pois = small
    want = twin.icgn3d1(prep, r[0], r[1], r[2], 0.001, 20, pois.copy())
    icgn = _engine(eng, r, ref, tar)
    for n in (1, 12, len(pois)):
        _assert_same_bits(icgn.compute(pois[:n].copy()), want[:n], (r, n))
    assert (want[-4:, 18] == np.float32([-3, -3, -1, -3])).all()
    if r != (3, 3, 3):   # (7^3 voxels hold a handful of speckles: whatever the twin finds there, the kernel must find too)
        assert (want[:-4, 18] >= 0).all()
    keep = [c for c in range(31) if c != 18]
    _assert_same_bits(want[-4:][:, keep], pois[-4:][:, keep], "a failed record keeps everything but its flag")


def test_trajectories_stop_k(eng, small):
    """conv = 0, stop = k: the record after exactly k iterations (k = 1 is the exit with g = 1 and c = the reference mean)."""
    ref, tar, prep, pois = small
    icgn = _engine(eng, (8, 8, 8), ref, tar)
    for k in (1, 2, 5):
        icgn.set_iteration(0.0, k)
        want = twin.icgn3d1(prep, 8, 8, 8, 0.0, k, pois.copy())
        _assert_same_bits(icgn.compute(pois.copy()), want, k)
        assert (want[:-4, 19] == k).all() and (want[:-4, 18] == -4.0).all()


def test_non_integer_centres_and_the_per_element_reference_path(eng, small):
    """Non-integer centres, and one POI (record 0) whose reference subvolume is not a box: the kernel must address it per element
    (tests/test_onepass3d_twin_cpu.py::test_the_element_path_poi_is_not_a_box)."""
    ref, tar, prep, _ = small
    pois = twin.offgrid_queue()
    per_element, box = twin.reference_indices(pois[0, 0], 5)
    assert (per_element != box).any()
    want = twin.icgn3d1(prep, 5, 7, 6, 0.001, 20, pois.copy())
    _assert_same_bits(_engine(eng, (5, 7, 6), ref, tar).compute(pois.copy()), want)
    assert (want[:, 18] >= 0).all()


def test_config_e_shape_six_staged_passes(eng, big):
    """r = 16 (33^3 subvolume, six staged passes of 12 x 512 samples per sweep): the 27 FFTCC3D-guessed POIs plus the border,
    out-of-volume, rejected and NaN records; queue lengths 1, 12 and whole; host and device queue."""
    import torch
    ref, tar, prep = big
    f = eng.FFTCC3D(16, 16, 16)
    f.set_images(ref, tar)
    pois = twin.config_e_queue(ref, tar, fftcc=f.compute)
    want = twin.icgn3d1(prep, 16, 16, 16, 0.001, 20, pois.copy())
    icgn = _engine(eng, (16, 16, 16), ref, tar)
    for n in (1, 12, len(pois)):
        _assert_same_bits(icgn.compute(pois[:n].copy()), want[:n], n)
    d = torch.from_numpy(pois.copy()).cuda()
    icgn.compute(d)
    _assert_same_bits(d.cpu().numpy(), want, "device queue")
    assert (want[:27, 18] > 0.97).all() and (want[:27, 19] < 20).all()
    assert want[-4, 18] == -3.0 and want[-3, 18] == -2.0 and want[-2, 18] == -3.0


def test_global_tap_fallback(eng, big):
    """30 degree rotations and a 35 % stretch as guesses, stop = 6: passes whose coefficient box is wider than the 40-float row
    pitch take their taps from global memory.  The bits must not depend on the path (the twin knows only one)."""
    ref, tar, prep = big
    pois = twin.rotated_queue()
    want = twin.icgn3d1(prep, 16, 16, 16, 0.001, 6, pois.copy())
    _assert_same_bits(_engine(eng, (16, 16, 16), ref, tar, stop=6).compute(pois.copy()), want)
    assert np.isfinite(want[:, 3]).all()


@pytest.mark.parametrize("r,kernel", [(21, "<48>"), (25, "<64>"), (30, "<0>")])
def test_large_radii_kernels(eng, big, r, kernel):
    """The other row-pitch instantiations; r = 30 is the radius of the reference's DVC example."""
    ref, tar, prep = big
    pois = twin.large_radius_queue(r)
    want = twin.icgn3d1(prep, r, r, r, 0.001, 20, pois.copy())
    _assert_same_bits(_engine(eng, (r, r, r), ref, tar).compute(pois.copy()), want, kernel)
    assert (want[:, 18] > 0.9).all(), kernel


def test_block_schedule_changes_no_bits(eng, small):
    """2 191 POIs at r = 5 (>= 2 048: visited in cubic blocks, every persistent workgroup walks several POIs of its XCD's eighth):
    tile sizes 0 (queue order), 8 and 20 give the twin's bits."""
    ref, tar, prep, _ = small
    pois = twin.schedule_queue()
    want = twin.icgn3d1(prep, 5, 5, 5, 0.001, 20, pois.copy())
    icgn = _engine(eng, (5, 5, 5), ref, tar)
    for tile in (0, 8, 20):
        icgn.set_tuning("icgn3d_tile_vox", tile)
        _assert_same_bits(icgn.compute(pois.copy()), want, tile)
    assert (want[:, 18] > 0.9).mean() > 0.9


def test_switching_contracts(eng, small):
    import oracle
    ref, tar, prep, pois = small
    want = twin.icgn3d1(prep, 8, 8, 8, 0.001, 20, pois.copy())
    sep = pois.copy()
    oracle.icgn3d1(prep, 8, 8, 8, 0.001, 20, sep, order=oracle.GPU_ORDER_3D, lanes=oracle.GPU_LANES_3D)
    fma = pois.copy()
    oracle.icgn3d1(prep, 8, 8, 8, 0.001, 20, fma, order=oracle.ORDER_LANES_FMA, lanes=oracle.GPU_LANES_3D)
    assert not np.array_equal(_bits(want), _bits(sep)) and not np.array_equal(_bits(want), _bits(fma))
    icgn = _engine(eng, (8, 8, 8), ref, tar)
    _assert_same_bits(icgn.compute(pois.copy()), want)
    icgn.set_tuning("arith_fma", 1)                    # under arith_onepass3d = 1 the value of arith_fma does not matter
    _assert_same_bits(icgn.compute(pois.copy()), want)
    icgn.set_tuning("arith_onepass3d", 0)              # back: the fused contract's bits ...
    _assert_same_bits(icgn.compute(pois.copy()), fma)
    icgn.set_tuning("arith_fma", 0)                    # ... and the default's
    _assert_same_bits(icgn.compute(pois.copy()), sep)
    icgn.set_tuning("arith_onepass3d", 1)
    _assert_same_bits(icgn.compute(pois.copy()), want)


def test_key_travels_through_a_device_group_and_is_refused_elsewhere(eng, small):
    ref, tar, prep, pois = small
    want = twin.icgn3d1(prep, 8, 8, 8, 0.001, 20, pois.copy())
    icgn = eng.ICGN3D1(8, 8, 8, 0.001, 20)
    icgn.set_devices([0, 0, 0])
    icgn.set_tuning("arith_onepass3d", 1)     # fans out over the members
    icgn.set_images(ref, tar)
    icgn.prepare()
    _assert_same_bits(icgn.compute(pois.copy()), want)
    icgn2 = eng.ICGN3D1(8, 8, 8, 0.001, 20)
    icgn2.set_tuning("arith_onepass3d", 1)    # set BEFORE the group is formed: the clones inherit it
    icgn2.set_devices([0, 0, 0])
    icgn2.set_images(ref, tar)
    icgn2.prepare()
    _assert_same_bits(icgn2.compute(pois.copy()), want)
    for make in (lambda: eng.FFTCC2D(16, 16), lambda: eng.FFTCC3D(8, 8, 8), lambda: eng.ICGN2D1(16, 16, 0.001, 10),
                 lambda: eng.ICGN2D2(16, 16, 0.001, 10), lambda: eng.NR2D1(16, 16, 0.001, 10), lambda: eng.ICLM2D1(16, 16, 0.001, 10)):
        e = make()
        with pytest.raises(Exception, match="arith_onepass3d"):
            e.set_tuning("arith_onepass3d", 1)
        e.set_tuning("arith_onepass3d", 0)
    # the 2D key on ICGN3D1 is refused with a pointer to this one
    with pytest.raises(Exception, match="arith_onepass3d"):
        eng.ICGN3D1(8, 8, 8, 0.001, 20).set_tuning("arith_onepass", 1)


def test_chain_and_single_poi_front_end(eng, small):
    import oracle
    ref, tar, prep, pois = small
    want = twin.icgn3d1(prep, 8, 8, 8, 0.001, 20, pois.copy())
    icgn = _engine(eng, (8, 8, 8), ref, tar)
    for k in (0, 1, 17, len(pois) - 4, len(pois) - 2, len(pois) - 1):
        one = pois[k].copy()
        icgn.compute_one(one)
        _assert_same_bits(one, want[k], k)
    fftcc = eng.FFTCC3D(8, 8, 8)
    fftcc.set_images(ref, tar)
    icgn.share_images(fftcc)
    icgn.prepare()
    fresh = oracle.make_pois3d(pois[:-4, 0], pois[:-4, 1], pois[:-4, 2])
    two = fresh.copy()
    fftcc.compute(two)
    icgn.compute(two)
    _assert_same_bits(eng.compute_chain([fftcc, icgn], fresh.copy()), two)
    _assert_same_bits(two, twin.icgn3d1(prep, 8, 8, 8, 0.001, 20, fftcc.compute(fresh.copy())))


def test_gpu_3d_within_the_bars_of_the_float64_model(eng):
    cs = m64.cases3d()
    models = [m64.model_runs(c) for c in cs]
    engines = {}

    def run(case, conv, stop):
        family, r, ref, tar, _, _, pois = case
        e = engines.get((family, r))
        if e is None:
            e = engines[(family, r)] = _engine(eng, r, ref, tar, conv, stop)
        e.set_iteration(conv, stop)
        return e.compute(pois.copy())

    dist, exc = m64.measure(cs, run, models)
    lines, bad = m64.check_within_bars(dist, "GPU arith_onepass3d")
    print("\n".join(lines))
    print("GPU arith_onepass3d one-iteration exceptions (used, records):", exc)
    assert not bad, "outside the bars (family, group, k index, distance, bar): %s" % bad
    for family, (used, n) in exc.items():
        assert used <= 0.05 * n, (family, used, n)


def test_environment_opt_in_of_an_unmodified_dvc_main(eng, tmp_path):
    """`OC_HIP_ARITH_ONEPASS3D=1` in the environment of a C++ main written against include/opencorr_compat (tests/cpp/shim_driver3d.cpp,
    the call order of the reference's DVC example; it creates four ICGN3D1 engines and requires them to agree): the records are those
    of `arith_onepass3d` = 1, stderr carries ONE notice, and `OC_HIP_ARITH_ONEPASS` -- the 2D variable -- leaves ICGN3D1 alone."""
    import os
    import struct
    import subprocess
    from opencorr_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "opencorr_amd", "lib")
    exe = str(tmp_path / "shim_driver3d")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "shim_driver3d.cpp"), "-o", exe, "-L" + libdir, "-lopencorr_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    dz, dy, dx = 64, 68, 72
    ref, tar = synth.speckle_pair_3d(dz, dy, dx, seed=33)
    xs, ys, zs = synth.poi_grid_3d(dz, dy, dx, 3, 3, 3, 22)
    inp = tmp_path / "in3.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<7i2f", dx, dy, dz, 8, 8, 8, len(xs), 0.001, 20.0))
        f.write(np.ascontiguousarray(ref, np.float32).tobytes())
        f.write(np.ascontiguousarray(tar, np.float32).tobytes())
        for a in (xs, ys, zs):
            f.write(a.astype(np.float32).tobytes())
    guess = eng.make_pois3d(xs, ys, zs)
    f3 = eng.FFTCC3D(8, 8, 8)
    f3.set_images(ref, tar)
    f3.compute(guess)
    icgn = eng.ICGN3D1(8, 8, 8, 0.001, 20.0)
    icgn.share_images(f3)
    icgn.prepare()
    default = icgn.compute(guess.copy())
    icgn.set_tuning("arith_onepass3d", 1)
    onepass = icgn.compute(guess.copy())
    assert not np.array_equal(_bits(default), _bits(onepass))
    for var, want, notices in (("OC_HIP_ARITH_ONEPASS3D", onepass, 1), ("OC_HIP_ARITH_ONEPASS", default, 0)):
        outp = tmp_path / (var + ".bin")
        env = {k: v for k, v in os.environ.items() if not k.startswith("OC_HIP_ARITH") and k != "OC_HIP_QUIET"}
        env[var] = "1"
        r = subprocess.run([exe, str(inp), str(outp)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        _assert_same_bits(np.fromfile(outp, dtype=np.float32).reshape(-1, 31), want, var)
        assert r.stderr.count("OC_HIP_ARITH_ONEPASS3D=1") == notices, r.stderr[-2000:]

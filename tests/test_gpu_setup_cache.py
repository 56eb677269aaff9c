"""The ICGN2D set-up cache (tuning key "icgn2d_setup_cache", icgn2d.hip CACHE): the big-queue launches of ICGN2D1 / ICGN2D2 keep
{ reference mean, norm, H^-1 } per POI from one compute() to the next and start from them while reference, gradients, radii,
arithmetic, count and the queue's coordinates stay what they were.

Bar everywhere: BIT-IDENTICAL (uint32 view) to an engine with "icgn2d_setup_cache" = 0 -- the behaviour before the cache --
on the same inputs, and the path a call took (fill / use / none) is asserted through setup_cache_last(), never inferred
from time.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, R = 640, 720, 16
X, Y, U, V, ZNCC, ITER, SRX, SRY = 0, 1, 2, 8, 16, 17, 23, 24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def case():
    """Device-resident speckle pair (used in place), a second target, and an FFTCC-initialised queue of 34 000 POIs (>= 32 768:
    variants 5 / 4 are taken by themselves)."""
    import torch
    import opencorr_amd
    from opencorr_amd import synth
    dev = torch.device("cuda", 0)
    ref, tar = synth.speckle_pair_2d(H, W, seed=20260925, device=dev)
    warp2 = dict(synth.DEFAULT_WARP_2D)
    warp2["u"] = warp2["u"] + 0.37
    warp2["v"] = warp2["v"] - 0.21
    _, tar2 = synth.speckle_pair_2d(H, W, seed=20260925, warp=warp2, device=dev)
    ref_b, _ = synth.speckle_pair_2d(H, W, seed=7, device=dev)
    xs, ys = synth.poi_grid_2d(H, W, 200, 170, 26)
    start = opencorr_amd.make_pois2d(xs, ys)
    assert len(start) == 34000
    f = opencorr_amd.FFTCC2D(R, R)
    f.set_images(ref, tar)
    q = torch.from_numpy(start).to(dev)
    f.compute(q)
    torch.cuda.synchronize()
    start = q.cpu().numpy()
    assert (start[:, ZNCC] > 0.5).mean() > 0.95
    f.close()
    return dict(dev=dev, ref=ref, tar=tar, tar2=tar2, ref_b=ref_b, start=start)


def _engine(case, dof, cache, fma=0, r=R, ref=None, tar=None, kind=None):
    import opencorr_amd
    cls = kind or (opencorr_amd.ICGN2D1 if dof == 6 else opencorr_amd.ICGN2D2)
    e = cls(r, r, 0.001, 10)
    e.set_tuning("icgn2d_setup_cache", cache)
    e.set_tuning("arith_fma", fma)
    e.set_images(case["ref"] if ref is None else ref, case["tar"] if tar is None else tar)
    e.prepare()
    return e


def _run(case, e, q, offsets=None):
    """compute() over a device copy of q -> (records, how the call treated the cache)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(q)).to(case["dev"])
    if offsets is None:
        e.compute(t)
    else:
        e.compute_with_offsets(t, torch.from_numpy(offsets).to(case["dev"]))
    state = e.setup_cache_last()
    torch.cuda.synchronize()
    return t.cpu().numpy(), state


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("dof", [6, 12])
def test_three_calls_on_one_queue_fill_use_use(case, dof, fma):
    on, off = _engine(case, dof, 1, fma), _engine(case, dof, 0, fma)
    want, state = _run(case, off, case["start"])
    assert state == "none"
    assert (want[:, ZNCC] > 0.9).mean() > 0.95
    states = []
    for _ in range(3):
        got, state = _run(case, on, case["start"])
        states.append(state)
        assert _same(got, want)
    assert states == ["fill", "use", "use"]
    on.close()
    off.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_mixed_poi_kinds_with_guesses_that_change_between_fill_and_use(case, dof):
    """Every workgroup (8 consecutive POIs of a queue row) mixes data-guard rejects (zncc < 0, NaN u, |u| >= width), a border
    POI that fails the geometric guard, a POI that starts converged (one iteration), a far-off guess (runs to the stop
    iteration or aborts) and normal POIs.  The fill call sees queue A; the use calls see queue B -- the same coordinates, but
    the POIs that A's data guard rejected now carry good guesses and other POIs carry the bad ones -- and then A again."""
    on, off = _engine(case, dof, 1), _engine(case, dof, 0)
    start = case["start"]
    solved, _ = _run(case, off, start)
    slot = np.arange(len(start)) % 8
    base = start.copy()
    base[slot == 3, X] = 3.0                               # geometric guard, in both queues
    one = slot == 4
    base[one, 2:14] = solved[one, 2:14]                    # starts converged
    base[slot == 5, U] += 6.5                              # far-off guess
    base[slot == 5, V] -= 5.5
    qa, qb = base.copy(), base.copy()
    qa[slot == 0, ZNCC] = -2.0
    qa[slot == 1, U] = np.nan
    qa[slot == 2, U] = float(W)
    qb[slot == 6, ZNCC] = -2.0
    qb[slot == 7, U] = np.nan
    qb[slot == 1, V] = -float(H)
    want_a, _ = _run(case, off, qa)
    want_b, _ = _run(case, off, qb)
    # the queues hold what the docstring says
    assert (want_a[slot == 0, ZNCC] == -2.0).all() and (want_a[slot == 1, ZNCC] == -3.0).all() and (want_a[slot == 2, ZNCC] == -3.0).all()
    assert (want_a[slot == 3, ZNCC] == -3.0).all() and (want_b[slot == 3, ZNCC] == -3.0).all()
    assert (want_b[slot == 0, ZNCC] > 0.9).mean() > 0.9 and (want_b[slot == 2, ZNCC] > 0.9).mean() > 0.9   # rejected by A, solved by B
    ok = one & (want_a[:, ZNCC] > 0)
    assert (want_a[ok, ITER] <= (1 if dof == 6 else 3)).mean() > 0.9
    assert ((want_a[slot == 5, ZNCC] == -4.0) | (want_a[slot == 5, ITER] >= 6)).mean() > 0.5
    got, state = _run(case, on, qa)
    assert state == "fill" and _same(got, want_a)
    got, state = _run(case, on, qb)
    assert state == "use" and _same(got, want_b)
    got, state = _run(case, on, qa)
    assert state == "use" and _same(got, want_a)
    on.close()
    off.close()


def test_what_the_records_depend_on_forces_a_fill(case):
    import torch
    start = case["start"]
    ref = case["ref"].clone()      # used in place by both engines; overwritten below
    tar = case["tar"].clone()
    on, off = _engine(case, 6, 1, ref=ref, tar=tar), _engine(case, 6, 0, ref=ref, tar=tar)

    def both(q, expect):
        want, none = _run(case, off, q)
        got, state = _run(case, on, q)
        assert none == "none" and state == expect, (state, expect)
        assert _same(got, want)

    both(start, "fill")
    both(start, "use")
    # one POI moved by one pixel, same count
    moved = start.copy()
    moved[12345, X] += 1.0
    both(moved, "fill")
    both(moved, "use")
    both(start, "fill")            # ... and back
    # another count
    both(start[:-100], "fill")
    both(start[:-100], "use")
    both(start, "fill")
    # other radii
    for e in (on, off):
        e.set_subset(15, 14)
    both(start, "fill")
    both(start, "use")
    # the other arithmetic contract
    for e in (on, off):
        e.set_tuning("arith_fma", 1)
    both(start, "fill")
    both(start, "use")
    for e in (on, off):
        e.set_tuning("arith_fma", 0)
    both(start, "fill")
    # the reference overwritten in place, prepare_ref()
    ref.copy_(case["ref_b"])
    torch.cuda.synchronize()
    for e in (on, off):
        e.prepare_ref()
    both(start, "fill")
    both(start, "use")
    on.close()
    off.close()


def test_new_target_in_place_is_a_use_call(case):
    """The sequence recipe: overwrite the target buffer, prepare_tar(), compute() -- the records stay."""
    import torch
    start = case["start"]
    tar = case["tar"].clone()
    on = _engine(case, 6, 1, tar=tar)
    _, state = _run(case, on, start)
    assert state == "fill"
    tar.copy_(case["tar2"])
    torch.cuda.synchronize()
    on.prepare_tar()
    got, state = _run(case, on, start)
    assert state == "use"
    fresh = _engine(case, 6, 0, tar=case["tar2"])
    want, _ = _run(case, fresh, start)
    assert _same(got, want)
    first, _ = _run(case, _engine(case, 6, 0), start)
    assert not _same(want, first)          # the new target does give other results
    on.close()
    fresh.close()


@pytest.mark.parametrize("dof", [6, 12])
def test_paths_that_go_around_the_cache(case, dof):
    import opencorr_amd
    start = case["start"]
    on, off = _engine(case, dof, 1), _engine(case, dof, 0)
    # a 10 000-POI queue runs the small-queue variants
    small = start[:10000]
    want, _ = _run(case, off, small)
    for _ in range(2):
        got, state = _run(case, on, small)
        assert state == "none" and _same(got, want)
    # centre offsets
    off_xy = np.random.default_rng(dof).uniform(-2, 2, (len(start), 2)).astype(np.float32)
    want, _ = _run(case, off, start, off_xy)
    for _ in range(2):
        got, state = _run(case, on, start, off_xy)
        assert state == "none" and _same(got, want)
    # a cached call in between is not disturbed by them
    want, _ = _run(case, off, start)
    got, state = _run(case, on, start)
    assert state == "fill" and _same(got, want)
    # self-adaptive radii
    sa = start.copy()
    sa[:, SRX] = np.random.default_rng(1).integers(8, R + 1, len(sa))
    sa[:, SRY] = np.random.default_rng(2).integers(8, R + 1, len(sa))
    for e in (on, off):
        e.set_self_adaptive(True)
    want, _ = _run(case, off, sa)
    for _ in range(2):
        got, state = _run(case, on, sa)
        assert state == "none" and _same(got, want)
    on.close()
    off.close()
    # IC-LM
    kind = opencorr_amd.ICLM2D1 if dof == 6 else opencorr_amd.ICLM2D2
    lm_on, lm_off = _engine(case, dof, 1, kind=kind), _engine(case, dof, 0, kind=kind)
    want, _ = _run(case, lm_off, start)
    for _ in range(2):
        got, state = _run(case, lm_on, start)
        assert state == "none" and _same(got, want)
    lm_on.close()
    lm_off.close()


def test_engines_sharing_images_and_a_two_member_group(case):
    import torch
    import opencorr_amd
    start = case["start"]
    want1, _ = _run(case, _engine(case, 6, 0), start)
    want2, _ = _run(case, _engine(case, 12, 0), start)
    # two engines on one shared image pair: each owns its records
    f = opencorr_amd.FFTCC2D(R, R)
    f.set_images(case["ref"], case["tar"])
    e1 = opencorr_amd.ICGN2D1(R, R, 0.001, 10)
    e2 = opencorr_amd.ICGN2D2(R, R, 0.001, 10)
    for e in (e1, e2):
        e.share_images(f)
        e.prepare()
    for expect in ("fill", "use", "use"):
        got1, s1 = _run(case, e1, start)
        got2, s2 = _run(case, e2, start)
        assert (s1, s2) == (expect, expect)
        assert _same(got1, want1) and _same(got2, want2)
    # re-binding the images makes the next call a fill
    e1.share_images(f)
    e1.prepare()
    got1, s1 = _run(case, e1, start)
    assert s1 == "fill" and _same(got1, want1)
    for e in (e1, e2, f):
        e.close()
    # a two-member group on one device (each member solves half the queue with its own records; variant 5 is named because
    # a half is below the automatic threshold)
    g = opencorr_amd.ICGN2D1(R, R, 0.001, 10)
    g.set_devices([0, 0])
    g.set_tuning("icgn2d_variant", 5)
    g.set_images(case["ref"], case["tar"])
    g.prepare()
    states = []
    for _ in range(3):
        q = torch.from_numpy(start).to(case["dev"])
        g.compute(q)
        states.append(g.setup_cache_last())
        torch.cuda.synchronize()
        assert _same(q.cpu().numpy(), want1)
    assert states == ["fill", "use", "use"]
    g.set_tuning("icgn2d_setup_cache", 0)
    q = torch.from_numpy(start).to(case["dev"])
    g.compute(q)
    assert g.setup_cache_last() == "none"
    torch.cuda.synchronize()
    assert _same(q.cpu().numpy(), want1)
    g.close()

"""The descriptor matcher's CPU restatement (tests/cpp/match_twin.cpp: the reference's sequential scan, src/oc_sift.cpp:625-674,
1251-1487, in float32) against the independent float64 model (tests/match_model.py), the planted cases whose outcome follows from
the contract alone, and three planted slips that the model comparison must catch.  No GPU."""
import numpy as np
import pytest

import match_cases as cases
import match_model as model
import match_twin as twin

FLT_MAX = np.finfo(np.float32).max
# (seed, reference keypoints, target keypoints, descriptor length); the share of doubtful queries was looked at on the CPU before
# the seeds were fixed: 0 - 0.8 % per side
SEEDED = [(1, 300, 280, 128), (2, 260, 300, 768), (3, 129, 257, 768)]
MAX_DOUBTFUL = 0.02


def _pairs(p):
    return list(zip(p[0].tolist(), p[1].tolist()))


@pytest.fixture(scope="module", params=SEEDED, ids=lambda p: "seed%d_%dx%dx%d" % p)
def seeded(request):
    seed, nr, nt, dim = request.param
    ref, tar = cases.seeded_sets(seed, nr, nt, dim)
    return ref, tar, {d: model.nearest(*(ref, tar) if d == 0 else (tar, ref), 0.85) for d in (0, 1)}, \
        {m: model.pairs(ref, tar, 0.85, m) for m in (0, 1)}


@pytest.mark.parametrize("fma", [0, 1])
def test_twin_nearest_equals_model_outside_the_margin(seeded, fma):
    ref, tar, near, _ = seeded
    for direction, (q, c) in enumerate(((ref, tar), (tar, ref))):
        m = near[direction]
        idx, best, second, n = twin.nearest(q, c, 0.85, fma)
        share = m["margin"].mean()
        print("direction %d: %d queries, %.2f %% inside the margin, %d matched" % (direction, len(q), 100 * share, n))
        assert share <= MAX_DOUBTFUL
        sure = ~m["margin"]
        assert np.array_equal(idx[sure], m["idx"][sure])
        assert n == int((idx >= 0).sum())
        assert 0.2 * len(q) < n < 0.9 * len(q)  # the ratio test decides both ways on these sets
        # the float32 sums: a sequential sum of dim non-negative terms, each a rounded square of a rounded difference, is within
        # (dim + 2) * 2^-24 relative of the exact value: 4.6e-5 for dim 768
        assert np.allclose(best, m["best"], rtol=5e-5, atol=0)
        assert np.allclose(second, m["second"], rtol=5e-5, atol=0)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_twin_pairs_equal_model_outside_the_margin(seeded, mode, fma):
    ref, tar, _, pairs = seeded
    ri, ti, doubt_r, doubt_t = pairs[mode]
    got = twin.pairs(ref, tar, 0.85, mode, fma)
    want = model.comparable(ri, ti, doubt_r, doubt_t)
    print("mode %d: %d pairs, %d compared; doubtful: %.2f %% of the reference, %.2f %% of the target keypoints"
          % (mode, len(ri), len(want), 100 * doubt_r.mean(), 100 * doubt_t.mean()))
    assert doubt_r.mean() <= MAX_DOUBTFUL and doubt_t.mean() <= MAX_DOUBTFUL
    assert len(want) > 50
    assert model.comparable(got[0], got[1], doubt_r, doubt_t) == want
    if mode == 0:
        assert np.all(np.diff(got[1]) < 0)  # descending target index, one pair per target
        groups = np.unique(twin.nearest(ref, tar, 0.85, fma)[0], return_counts=True)[1]
        assert (groups > 1).sum() >= 3      # many-to-one groups exist
    else:
        assert np.all(np.diff(got[0]) > 0)


# ---- planted cases: the exact outcome ------------------------------------------------------------------------------------
PLANTED = cases.planted()


def _run(name, ratio, fma=0):
    ref, tar = PLANTED[name]
    idx, best, second, n = twin.nearest(ref, tar, ratio, fma)
    return idx.tolist(), best, second, n, _pairs(twin.pairs(ref, tar, ratio, 0, fma)), _pairs(twin.pairs(ref, tar, ratio, 1, fma))


@pytest.mark.parametrize("fma", [0, 1])
def test_duplicate_target_rows_tie_goes_to_the_lower_index(fma):
    # targets 2 and 5 are one row: best == second, so the ratio test fails for every ratio <= 1 ...
    for ratio in (0.85, 1.0):
        idx, best, second, n, mono, bi = _run("duplicate_targets", ratio, fma)
        assert idx[0] == -1 and best[0] == second[0] == np.float32(0.015625)
    # ... and above 1 the nearest is the lower of the two
    idx, _, _, n, mono, bi = _run("duplicate_targets", 1.25, fma)
    assert idx == [2, 1, 1] and n == 3
    assert mono == [(0, 2), (1, 1)] and bi == [(0, 2), (1, 1)]


@pytest.mark.parametrize("fma", [0, 1])
def test_duplicate_reference_rows_form_a_group_with_equal_distances(fma):
    """References 0 and 1 are one row and both choose target 3.  The group's test is d0 < ratio^2 * d1 with d0 == d1: false for
    every ratio <= 1 (ratio 1.0 included: d0 < d0), so the group is eliminated; above 1 the lower reference index stays."""
    for ratio in (0.85, 1.0):
        idx, _, _, _, mono, bi = _run("duplicate_refs", ratio, fma)
        assert idx[:2] == [3, 3]
        assert all(t != 3 for _, t in mono)
        assert all(t != 3 for _, t in bi)  # (target 3's own nearest is a tie between references 0 and 1: no match back)
    idx, _, _, _, mono, bi = _run("duplicate_refs", 1.25, fma)
    assert (0, 3) in mono and (1, 3) not in mono
    assert (0, 3) in bi and (1, 3) not in bi


@pytest.mark.parametrize("fma", [0, 1])
def test_many_to_one_group_that_ends_the_list(fma):
    # ratio 1.0: references 1 and 2 both choose target 0, the last group in descending target order; reference 2 is far closer
    idx, best, _, _, mono, bi = _run("group_ends_list", 1.0, fma)
    assert idx == [-1, 0, 0, 3]
    assert mono == [(3, 3), (2, 0)]
    assert bi == [(2, 0)]
    assert best[2] < 0.7225 * best[1]


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("ratio", [0.85, 1.0])
def test_every_reference_keypoint_matched_is_processed(ratio, fma):
    idx, _, _, n, mono, bi = _run("all_matched", ratio, fma)
    assert idx == [4, 3, 2, 1, 0] and n == 5
    assert mono == [(0, 4), (1, 3), (2, 2), (3, 1), (4, 0)]  # descending target index
    assert bi == [(0, 4), (1, 3), (2, 2), (3, 1), (4, 0)]     # ascending reference index


@pytest.mark.parametrize("fma", [0, 1])
def test_nan_rows_are_never_candidates(fma):
    idx, best, second, n, mono, bi = _run("nan_rows", 0.85, fma)
    assert idx[2] == -1 and best[2] == FLT_MAX and second[2] == FLT_MAX  # the NaN reference row has no candidate
    assert 4 not in idx                                                   # the NaN target row is nobody's nearest
    assert idx == [5, 2, -1, 2, 1, 0]
    assert mono == [(0, 5), (3, 2), (4, 1), (5, 0)] and bi == mono
    ref, tar = PLANTED["nan_rows"]
    back = twin.nearest(tar, ref, 0.85, fma)[0]
    assert back[4] == -1 and 2 not in back.tolist()


@pytest.mark.parametrize("fma", [0, 1])
def test_zero_row_against_itself(fma):
    idx, best, second, _, mono, bi = _run("zero_row", 0.85, fma)
    assert idx[1] == 3 and best[1] == 0.0 and second[1] > 0  # 0 < r^2 * second passes
    assert (1, 3) in mono and (1, 3) in bi


@pytest.mark.parametrize("nr", [0, 1, 2])
@pytest.mark.parametrize("nt", [0, 1, 2])
def test_small_counts(nr, nt):
    name = "counts_%d_%d" % (nr, nt)
    ref, tar = PLANTED[name]
    for ratio in cases.RATIOS:
        idx, best, second, n, mono, bi = _run(name, ratio)
        assert len(idx) == nr
        m = model.nearest(ref, tar, ratio)
        assert idx == m["idx"].tolist()
        assert mono == _pairs(model.pairs(ref, tar, ratio, 0)) and bi == _pairs(model.pairs(ref, tar, ratio, 1))
        if nt == 0:
            assert idx == [-1] * nr and (best == FLT_MAX).all()
        if nt == 1:
            assert (second == FLT_MAX).all()  # fewer than two candidates: second stays FLT_MAX, a lone candidate passes for ratio > 0
            assert idx == ([0] * nr if ratio > 0 else [-1] * nr)
        if ratio == 0:
            assert n == 0 and mono == [] and bi == []


@pytest.mark.parametrize("name", sorted(n for n in PLANTED if not n.startswith("counts")))
@pytest.mark.parametrize("ratio", list(cases.RATIOS) + [1.25])
def test_planted_cases_equal_the_model(name, ratio):
    """The planted rows give short exact sums: float32 and float64 decide alike, ties included."""
    ref, tar = PLANTED[name]
    for fma in (0, 1):
        assert twin.nearest(ref, tar, ratio, fma)[0].tolist() == model.nearest(ref, tar, ratio)["idx"].tolist()
        for mode in (0, 1):
            assert _pairs(twin.pairs(ref, tar, ratio, mode, fma)) == _pairs(model.pairs(ref, tar, ratio, mode))
    if ratio == 0:
        assert (twin.nearest(ref, tar, ratio)[0] == -1).all()


# ---- a twin with one planted slip is caught ------------------------------------------------------------------------------
def _differs_from_model(ref, tar, ratio):
    """True when the twin, as it runs now, disagrees with the model on matched_idx or on either pair list outside the margin."""
    m = model.nearest(ref, tar, ratio)
    sure = ~m["margin"] | (m["best"] == m["second"])  # (planted exact ties are decided by the index rule, not by rounding)
    if not np.array_equal(twin.nearest(ref, tar, ratio)[0][sure], m["idx"][sure]):
        return True
    for mode in (0, 1):
        ri, ti, doubt_r, doubt_t = model.pairs(ref, tar, ratio, mode)
        got = twin.pairs(ref, tar, ratio, mode)
        if model.comparable(got[0], got[1], doubt_r, doubt_t) != model.comparable(ri, ti, doubt_r, doubt_t):
            return True
    return False


def test_planted_slips_are_caught():
    ref, tar = cases.seeded_sets(1, 300, 280, 128)
    dup_ref, dup_tar = PLANTED["duplicate_targets"]
    assert not _differs_from_model(ref, tar, 0.85)
    assert not _differs_from_model(dup_ref, dup_tar, 1.25)
    with twin.slip(twin.SLIP_LESS_EQUAL):       # `<=` in the scan: a tie goes to the higher index
        assert _differs_from_model(dup_ref, dup_tar, 1.25)
    with twin.slip(twin.SLIP_RATIO_UNSQUARED):  # best < ratio * second
        assert _differs_from_model(ref, tar, 0.85)
    with twin.slip(twin.SLIP_ASCENDING):        # monodirectional pairs in ascending target index
        assert _differs_from_model(ref, tar, 0.85)
    assert not _differs_from_model(ref, tar, 0.85)

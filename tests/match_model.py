"""Float64 model of the descriptor matcher (SIFT3D::bruteforceMatch, monodirectionalMatch, bidirectionalMatch of the reference,
src/oc_sift.cpp:625-674, 1251-1418, 1420-1487): brute-force NumPy distances in float64, arg-sorted, the ratio test, both match
modes and the behaviours this project defines where the reference is undefined:

  * the element behind the last many-to-one group counts as different (the reference reads one past the resized vector);
  * all matches are processed when every reference keypoint passed the ratio test (the reference returns nothing);
  * a distance that is not < FLT_MAX (NaN, inf) is never a candidate; ties go to the lower index.

It shares no code and no summation order with tests/cpp/match_twin.cpp or the kernel.  Decisions that hang on less than
MARGIN (relative) in float64 are flagged, so that a comparison with a float32 implementation can leave them out."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
MARGIN = 1e-4


def distances(query, cand):
    q = np.asarray(query, dtype=np.float64)
    c = np.asarray(cand, dtype=np.float64)
    out = np.empty((q.shape[0], c.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q.shape[0]):
            out[i] = ((c - q[i]) ** 2).sum(axis=1)
    return out


def _ratio_sq(ratio):
    return float(np.float32(ratio)) ** 2


def _near(a, b):
    return abs(a - b) <= MARGIN * abs(b)


def nearest(query, cand, ratio):
    """dict: idx (-1 = no match), j0 / j1 (nearest and runner-up, -1 = none), best, second, margin (bool per query)."""
    D = distances(query, cand)
    nq = D.shape[0]
    r2 = _ratio_sq(ratio)
    idx = np.full(nq, -1, np.int64)
    j0 = np.full(nq, -1, np.int64)
    j1 = np.full(nq, -1, np.int64)
    best = np.full(nq, FLT_MAX)
    second = np.full(nq, FLT_MAX)
    margin = np.zeros(nq, bool)
    for i in range(nq):
        with np.errstate(invalid="ignore"):
            cand_j = np.flatnonzero(D[i] < FLT_MAX)
        order = cand_j[np.argsort(D[i][cand_j], kind="stable")]
        if order.size >= 1:
            j0[i], best[i] = order[0], D[i][order[0]]
        if order.size >= 2:
            j1[i], second[i] = order[1], D[i][order[1]]
            margin[i] = _near(best[i], second[i])
        if order.size >= 1:
            margin[i] = margin[i] or _near(best[i], r2 * second[i])
            if best[i] < r2 * second[i]:
                idx[i] = j0[i]
    return dict(idx=idx, j0=j0, j1=j1, best=best, second=second, margin=margin)


def pairs(ref, tar, ratio, mode):
    """(ref_idx, tar_idx, doubtful_ref, doubtful_tar): the pairs in output order (mode 0: descending target index, mode 1:
    ascending reference index) and the keypoints whose float64 decision margin is below MARGIN -- a pair that involves one of
    them may legitimately differ under float32 rounding."""
    nr, nt = len(ref), len(tar)
    doubt_r, doubt_t = np.zeros(nr, bool), np.zeros(nt, bool)
    empty = np.zeros(0, np.int64)
    if nr == 0 or nt == 0:
        return empty, empty, doubt_r, doubt_t
    r2t = nearest(ref, tar, ratio)
    doubt_r |= r2t["margin"]
    r2 = _ratio_sq(ratio)
    if mode == 1:
        t2r = nearest(tar, ref, ratio)
        doubt_t |= t2r["margin"]
        keep = [i for i in range(nr) if r2t["idx"][i] >= 0 and t2r["idx"][r2t["idx"][i]] == i]
        ri = np.array(keep, np.int64)
        return ri, r2t["idx"][ri] if ri.size else empty, doubt_r, doubt_t
    # a doubtful reference keypoint may join the group of its nearest or of its runner-up
    for i in np.flatnonzero(doubt_r):
        for j in (r2t["j0"][i], r2t["j1"][i]):
            if j >= 0:
                doubt_t[j] = True
    ri, ti = [], []
    for j in range(nt - 1, -1, -1):
        members = sorted((r2t["best"][i], i) for i in np.flatnonzero(r2t["idx"] == j))
        if not members:
            continue
        d0 = members[0][0]
        d1 = members[1][0] if len(members) > 1 else FLT_MAX
        if len(members) > 1 and (_near(d0, d1) or _near(d0, r2 * d1)):
            doubt_t[j] = True
        if d0 < r2 * d1:
            ri.append(members[0][1])
            ti.append(j)
    return np.array(ri, np.int64), np.array(ti, np.int64), doubt_r, doubt_t


def comparable(ref_idx, tar_idx, doubt_r, doubt_t):
    """The pairs of a list that involve no doubtful keypoint, as a list of tuples in the list's order."""
    return [(int(i), int(j)) for i, j in zip(ref_idx, tar_idx) if not doubt_r[i] and not doubt_t[j]]

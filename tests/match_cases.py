"""Descriptor sets for the matcher's tests (tests/test_match_twin_cpu.py, tests/test_gpu_match.py): seeded sets that look like
SIFT's (unit-norm, non-negative rows; true matches planted with noise, several reference keypoints that share one target) and
small planted cases whose exact outcome follows from the contract alone."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def _unit(a):
    n = np.sqrt((a.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))
    return (a / np.where(n > 0, n, 1)).astype(np.float32)


def random_rows(rng, n, dim):
    """unit-norm non-negative rows with a few dominant components (a gradient histogram's shape)"""
    return _unit(rng.random((n, dim)) ** 4)


def seeded_sets(seed, n_ref, n_tar, dim):
    """(ref, tar): about two thirds of the reference rows have a true partner among the targets (the row plus noise of a
    strength drawn per pair, so that the ratio test passes for some and fails for others), about every tenth reference row is a
    noisy copy of an earlier one (many-to-one groups); the other targets are unrelated rows.  Targets are shuffled."""
    rng = np.random.default_rng(seed)
    ref = random_rows(rng, n_ref, dim)
    for k in range(9, n_ref, 10):
        ref[k] = _unit(ref[k - 4] + rng.uniform(0.1, 0.5) * random_rows(rng, 1, dim)[0])
    tar = random_rows(rng, n_tar, dim)
    planted = min(n_tar, (2 * n_ref) // 3)
    slots = rng.permutation(n_tar)[:planted]
    for k, j in enumerate(slots):
        tar[j] = _unit(ref[k] + rng.uniform(0.2, 1.3) * random_rows(rng, 1, dim)[0])
    return ref, tar


def with_seam_ties(ref, tar, rows=(10, 70, 200, 256), source=5):
    """The same target row at several indices (64-candidate tiles 0, 1, 3 and 4 of 257 candidates: in different parts under 2, 3
    and 7 splits): an exact tie for nearest AND runner-up of reference row `source`, and for every query that comes close."""
    tar = tar.copy()
    row = _unit(ref[source] + 0.3 * tar[rows[0]])
    for j in rows:
        if j < len(tar):
            tar[j] = row
    return ref, tar


def planted(dim=32):
    """name -> (ref, tar): the planted cases.  Rows are scaled basis-like vectors, so every distance is a short exact sum."""
    rng = np.random.default_rng(77)
    cases = {}

    def basis(n, scale=1.0):
        a = np.zeros((n, dim), np.float32)
        for i in range(n):
            a[i, (3 * i) % dim] = scale
        return a

    # duplicate target rows: the tie for the nearest of ref 0 goes to the lower j (2, not 5)
    ref = basis(3)
    tar = basis(7) * np.float32(0.5)
    tar[2] = tar[5] = ref[0] + np.float32(0.125) * basis(7)[6]
    tar[0] = basis(7)[4]
    cases["duplicate_targets"] = (ref, tar)
    # duplicate reference rows pointing at one target: a group of two with equal distances
    ref = basis(4)
    ref[1] = ref[0]
    tar = basis(5) * np.float32(0.25)
    tar[3] = ref[0] + np.float32(0.0625) * basis(5)[4]
    cases["duplicate_refs"] = (ref, tar)
    # a many-to-one group that ends the list: target 0 (the last in descending order) is chosen by refs 1 and 2, ref 2 much closer
    ref = basis(4)
    tar = basis(4) * np.float32(0.25)
    tar[0] = np.float32(0.5) * (ref[1] + ref[2])
    ref[2] = tar[0] + np.float32(0.03125) * basis(4)[3]
    cases["group_ends_list"] = (ref, tar)
    # every reference keypoint matched, one target each
    ref = basis(5)
    tar = (basis(5) * np.float32(0.875))[::-1].copy()
    cases["all_matched"] = (ref, tar)
    # a NaN row on either side
    ref = random_rows(rng, 6, dim)
    tar = _unit(ref[::-1] + 0.05 * random_rows(rng, 6, dim))
    ref[2, 7] = np.nan
    tar[4, 0] = np.nan
    cases["nan_rows"] = (ref, tar)
    # an all-zero row against itself
    ref = random_rows(rng, 4, dim)
    tar = random_rows(rng, 5, dim)
    ref[1] = 0
    tar[3] = 0
    cases["zero_row"] = (ref, tar)
    # counts 0, 1 and 2 on either side
    for nr in (0, 1, 2):
        for nt in (0, 1, 2):
            r = random_rows(rng, 2, dim)[:nr]
            t = _unit(r[::-1] + 0.05 * random_rows(rng, 2, dim)[:nr])[:nt] if nr >= nt else random_rows(rng, 2, dim)[:nt]
            cases["counts_%d_%d" % (nr, nt)] = (np.ascontiguousarray(r), np.ascontiguousarray(t))
    return cases


RATIOS = (0.85, 1.0, 0.0)

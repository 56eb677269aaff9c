#!/usr/bin/env python
"""Measures FeatureAffine3D::compute(poi_queue) on the GPU (opencorr_amd/csrc/feature_affine.hip) beside its CPU twin.

    python tools/feature_affine_bench.py [--out profiles/feature_affine.json] [--pois 50000,2000000] [--reps 3] [--twin-pois 50000] [--twin-threads 16]

The workload: the reference's 3D defaults (subset radius 8: search radius sqrt(192), 16 neighbours, 4 samples, 32 trials, threshold
3.2) over keypoints of a density that puts 256 candidates around a POI on average, under a planted affine field with noise and
30 % displaced pairs; POIs uniformly inside the cloud, device-resident.  Per queue length: the time of compute() on the device
queue (wall clock around the call, which returns when the engine's stream has drained; the median of --reps calls after one
warm-up call), the time of the compute kernel alone (hipEvents, oc_hip_profile_*), POIs per second, and the CPU twin
(tests/cpp/feature_affine_twin.cpp, OpenMP on --twin-threads threads; brute-force neighbour search) on the first
--twin-pois POIs of the same queue with a bit-for-bit comparison of the records.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SUBSET = (8, 8, 8)
CANDIDATES = 256
EDGE = 120.0


def workload(n_poi, seed=4120):
    import feature_affine_cases as cases
    rng = np.random.default_rng(seed)
    radius = float(np.sqrt(np.float32(sum(r * r for r in SUBSET))))
    density = CANDIDATES / (4.0 / 3.0 * np.pi * radius ** 3)
    n_kp = int(round(density * EDGE ** 3))
    ref = (rng.random((n_kp, 3)) * EDGE).astype(np.float32)
    M, t = cases.field(3)
    tar = cases.apply(M, t, ref) + (rng.standard_normal((n_kp, 3)) * 0.1).astype(np.float32)
    bad = rng.random(n_kp) < 0.3
    tar[bad] += (rng.standard_normal((int(bad.sum()), 3)) * 40.0).astype(np.float32)
    pois = cases.queue((radius + rng.random((n_poi, 3)) * (EDGE - 2 * radius)).astype(np.float32))
    return ref, tar.astype(np.float32), pois, radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_affine.json"))
    ap.add_argument("--pois", default="50000,2000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--twin-pois", type=int, default=50000)
    ap.add_argument("--twin-threads", type=int, default=16)
    args = ap.parse_args()

    import torch
    import opencorr_amd
    from opencorr_amd import capi
    import feature_affine_twin as twin
    if capi.device_count() < 1:
        raise SystemExit("feature_affine_bench: no GPU")
    twin.lib()
    records = []
    for n_poi in (int(v) for v in args.pois.split(",")):
        ref, tar, pois, radius = workload(n_poi)
        e = opencorr_amd.FeatureAffine3D(*SUBSET)
        e.set_keypoint_pair(ref, tar)
        t0 = time.perf_counter()
        e.prepare()
        prepare_s = time.perf_counter() - t0
        fresh = torch.from_numpy(pois).cuda()
        queue = fresh.clone()
        e.compute(queue)
        e.synchronize()
        wall, kernel = [], []
        for _ in range(args.reps):
            queue.copy_(fresh)
            torch.cuda.synchronize()
            e.profile_reset()
            e.profile_enable(True)
            t0 = time.perf_counter()
            e.compute(queue)
            e.synchronize()
            wall.append(time.perf_counter() - t0)
            ms, launches = e.profile_read()
            e.profile_enable(False)
            assert launches == 1
            kernel.append(ms)
        got = queue.cpu().numpy()
        compute_s = float(np.median(wall))
        rec = dict(n_poi=n_poi, n_keypoints=int(ref.shape[0]), candidates_per_poi=CANDIDATES, subset_radius=list(SUBSET), search_radius=radius,
                   prepare_s=prepare_s, compute_s=compute_s, compute_s_all=[float(v) for v in wall], kernel_ms=float(np.median(kernel)),
                   kernel_ms_all=[float(v) for v in kernel], pois_per_s=n_poi / compute_s, accepted=int((got[:, 18] == 0).sum()),
                   mean_trials=float(got[got[:, 18] == 0, 19].mean()))
        n_twin = min(n_poi, args.twin_pois)
        t0 = time.perf_counter()
        want = twin.compute(ref, tar, pois[:n_twin], radius, threads=args.twin_threads)
        rec["twin_pois"] = n_twin
        rec["twin_s"] = time.perf_counter() - t0
        rec["twin_pois_per_s"] = n_twin / rec["twin_s"]
        rec["twin_threads"] = args.twin_threads
        rec["equals_twin"] = bool(np.array_equal(got[:n_twin].view(np.uint32), want.view(np.uint32)))
        print(json.dumps(rec), flush=True)
        records.append(rec)
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/feature_affine_bench.py", records=records), f, indent=1)
        f.write("\n")
    if any(r["equals_twin"] is False for r in records):
        raise SystemExit("feature_affine_bench: the kernel's records differ from the twin's")


if __name__ == "__main__":
    main()

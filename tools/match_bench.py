#!/usr/bin/env python
"""Measures the descriptor matcher's distance + top-2 kernel (opencorr_amd/csrc/match.hip) on seeded descriptor sets.

    python tools/match_bench.py [--out profiles/match_bench.json] [--sizes 20000x20000x768,5000x5000x128] [--reps 5] [--no-twin]

Per size and arithmetic mode (arith_fma 0 / 1): kernel ms (hipEvents around the kernel on the engine's stream, through
oc_hip_profile_*; the median of --reps launches after two warm-up launches), pairs/s, the share of the VALU issue rate -- the
lane-operations the contract mandates per pair (a subtraction, a multiply and an addition per component: 3 * dim; fused: 2 * dim)
over the time, against 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12 lane-operations/s (the FP32 vector peak of
157.3 TFLOPS counts a fused multiply-add as two) -- and beside it the CPU restatement's time (tests/cpp/match_twin.cpp, OpenMP,
the thread count in the record) with a bit-for-bit comparison of the two results.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def descriptor_sets(seed, n_ref, n_tar, dim):
    """unit-norm non-negative rows; two thirds of the reference rows have a noisy partner among the (shuffled) targets"""
    rng = np.random.default_rng(seed)

    def rows(n):
        a = rng.random((n, dim), dtype=np.float32) ** 4
        return a / np.sqrt((a.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)

    ref, tar = rows(n_ref), rows(n_tar)
    planted = min(n_tar, (2 * n_ref) // 3)
    slots = rng.permutation(n_tar)[:planted]
    noisy = ref[:planted] + rng.uniform(0.2, 1.3, (planted, 1)).astype(np.float32) * rows(planted)
    tar[slots] = noisy / np.sqrt((noisy.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(ref), np.ascontiguousarray(tar)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    ap.add_argument("--sizes", default="20000x20000x768,5000x5000x128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-twin", action="store_true")
    args = ap.parse_args()

    import opencorr_amd
    from opencorr_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("match_bench: no GPU")
    twin = None
    if not args.no_twin:
        import match_twin as twin
        twin.lib()
    records = []
    for size in args.sizes.split(","):
        n_ref, n_tar, dim = (int(v) for v in size.split("x"))
        ref, tar = descriptor_sets(20240 + dim, n_ref, n_tar, dim)
        for fma in (0, 1):
            m = opencorr_amd.DescriptorMatcher(dim, 0.85)
            m.set_tuning("arith_fma", fma)
            m.set_descriptors(0, ref)
            m.set_descriptors(1, tar)
            for _ in range(2):
                m.nearest(0)
            times = []
            for _ in range(args.reps):
                m.profile_reset()
                m.profile_enable(True)
                idx, best, second = m.nearest(0)
                m.synchronize()
                ms, launches = m.profile_read()
                m.profile_enable(False)
                assert launches == 1
                times.append(ms)
            kernel_ms = float(np.median(times))
            pairs = float(n_ref) * n_tar
            lane_ops = pairs * dim * (2 if fma else 3)
            rec = dict(n_ref=n_ref, n_tar=n_tar, dim=dim, arith_fma=fma, kernel_ms=kernel_ms, kernel_ms_all=[float(t) for t in times],
                       pairs_per_s=pairs / (kernel_ms * 1e-3), lane_ops_per_pair=dim * (2 if fma else 3),
                       valu_issue_share=lane_ops / (kernel_ms * 1e-3) / VALU_LANE_OPS_PER_S, matched=int((idx >= 0).sum()))
            if twin is not None:
                t0 = time.perf_counter()
                t_idx, t_best, t_second, _ = twin.nearest(ref, tar, 0.85, fma)
                rec["twin_s"] = time.perf_counter() - t0
                rec["twin_threads"] = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
                rec["equals_twin"] = bool(np.array_equal(idx, t_idx) and np.array_equal(best.view(np.uint32), t_best.view(np.uint32)) and
                                          np.array_equal(second.view(np.uint32), t_second.view(np.uint32)))
            print(json.dumps(rec), flush=True)
            records.append(rec)
            m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/match_bench.py", valu_lane_ops_per_s=VALU_LANE_OPS_PER_S, records=records), f, indent=1)
        f.write("\n")
    if any(r.get("equals_twin") is False for r in records):
        raise SystemExit("match_bench: the kernel's result differs from the twin's")


if __name__ == "__main__":
    main()

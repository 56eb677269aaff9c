#!/usr/bin/env python
"""Measures SIFT3D's orientation and descriptor stages (opencorr_amd/csrc/sift3d_features.hip) on speckle volumes from
synth.speckle_pair_3d, default config.

    python tools/sift3d_features_bench.py [--out profiles/sift3d_features.json] [--sizes 256,512] [--reps 5] [--chunk 65536]
                                          [--twin-sample 512] [--twin-full 256] [--no-twin]

Per size: `orient` over every candidate of the pyramid (the list never leaves the device; the call includes the validation kernel,
the compaction and one 4-byte read-back) and `describe` over every accepted keypoint in chunks of --chunk records into one reused
device block (the descriptors of all keypoints at 512^3 do not fit a sensible buffer: 768 floats each).  Times: device events on the
stream the engine runs on (torch's current stream: the volume is a CUDA tensor), the median of --reps calls after two warm-up calls,
which also grow the buffers.  From the keypoint records: the voxels a descriptor workgroup visits (its clamped window, cut to the
weight table) and, on a sample of 256 keypoints restated in NumPy, the share of visited voxels that pass the sphere and the inscribed
cube and so reach the triangle search.  Baseline: the CPU restatement (tests/cpp/sift3d_features_twin.cpp, OpenMP, the thread count in
the record) on the same list up to --twin-full (256^3: measured, every record compared bit for bit); above that on a sample of
--twin-sample candidates spread over the list, its time scaled linearly to the list and stated as such (an extrapolation: windows
differ per layer and per clamping), with a bit-for-bit comparison of status, sums, keypoints and descriptors on the sample.  The
volume is made on the device and is not bit-reproducible from run to run (the candidate count moves by one or two).  Counters are collected in a run of their own
(rocprofv3 --pmc ... -- python tools/sift3d_features_bench.py --no-twin --reps 1 --sizes 256).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window_voxels(kp, gauss, n_octave_layers):
    """voxels each descriptor workgroup visits: the loops of src/oc_sift.cpp:1066-1079, clamped, cut to the table's half-extent"""
    g = gauss[kp["layer"] + kp["octave"] * (n_octave_layers + 3)]
    radius = np.float32(2.0) * (np.float32(5.0) * np.sqrt(np.float32(2.0)) * kp["scale"])
    total = np.ones(len(kp), np.int64)
    for a in range(3):
        reach = radius / g["units"][:, a]
        half = np.ceil(reach).astype(np.int64) + 1
        c = kp["coor_layer"][:, a].astype(np.int64)
        lo = np.maximum(np.maximum(np.floor(kp["coor_layer"][:, a] - reach).astype(np.int64), 1), c - half)
        hi = np.minimum(np.minimum(np.ceil(kp["coor_layer"][:, a] + reach).astype(np.int64), g["dims"][:, a] - 1), c + half + 1)
        total *= np.maximum(hi - lo, 0)
    return total


def contributing_share(kp, gauss, n_octave_layers, sample=256):
    """of the visited voxels of `sample` keypoints, the share inside the sphere and the inscribed cube (geometry alone)"""
    pick = kp[np.unique(np.linspace(0, len(kp) - 1, min(sample, len(kp))).round().astype(int))]
    visited = passed = 0
    for k in pick:
        g = gauss[k["layer"] + k["octave"] * (n_octave_layers + 3)]
        sigma = 5.0 * np.sqrt(2.0) * float(k["scale"])
        sphere, cube = 2.0 * sigma, 2.0 * sigma / np.sqrt(2.0)
        axes = []
        for a in range(3):
            reach = sphere / float(g["units"][a])
            c = float(k["coor_layer"][a])
            lo, hi = max(int(np.floor(c - reach)), 1), min(int(np.ceil(c + reach)), int(g["dims"][a]) - 1)
            axes.append((np.arange(lo, max(hi, lo)) - c) * float(g["units"][a]))
        x, y, z = np.meshgrid(*axes, indexing="ij")
        p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        sub = 2.0 * (p @ k["rotation_matrix"].astype(np.float64).reshape(3, 3).T + cube) / cube - 0.5
        ok = (np.sqrt((p ** 2).sum(1)) <= sphere) & np.all((sub > -0.5) & (sub < 3.5), 1)
        visited += len(p)
        passed += int(ok.sum())
    return passed / max(visited, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift3d_features.json"))
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--twin-sample", type=int, default=512)
    ap.add_argument("--twin-full", type=int, default=256, help="up to this size the twin runs the whole list, not a sample")
    ap.add_argument("--no-twin", action="store_true")
    args = ap.parse_args()

    import torch
    import opencorr_amd
    from opencorr_amd import capi, synth
    if capi.device_count() < 1:
        raise SystemExit("sift3d_features_bench: no GPU")
    twin = None
    if not args.no_twin:
        import sift3d_features_twin as twin
        twin.lib()
    records = []
    for size in (int(v) for v in args.sizes.split(",")):
        volume, _ = synth.speckle_pair_3d(size, size, size, device="cuda")
        s = opencorr_amd.SIFT3DScaleSpace()
        s.set_volume(volume)
        s.build()
        n_candidates = len(s.detect())
        torch.cuda.synchronize()

        def timed(call, reps):
            for _ in range(2):
                out = call()
            ms = []
            for _ in range(reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                out = call()
                ev[1].record()
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            return out, ms

        (kp_dev, status, _), orient_ms = timed(lambda: s.orient(None, with_status=True, on_device=True), args.reps)
        kp = kp_dev.cpu().numpy().view(opencorr_amd.SIFT3DScaleSpace.KEYPOINT).reshape(-1)
        n_kp = len(kp)
        block = torch.empty((min(args.chunk, max(n_kp, 1)), 768), dtype=torch.float32, device="cuda")

        def describe_all():
            for at in range(0, n_kp, args.chunk):
                part = kp_dev[at:at + args.chunk]
                s.describe(part, out=block[:len(part)])
            return None

        _, describe_ms = timed(describe_all, args.reps)
        gauss = s.layers(0)
        visits = int(window_voxels(kp, gauss, 3).sum()) if n_kp else 0
        o, d = float(np.median(orient_ms)), float(np.median(describe_ms))
        rec = dict(size=size, candidates=int(n_candidates), keypoints=int(n_kp), status_counts=np.bincount(status.cpu().numpy(), minlength=4).tolist(),
                   orient_ms=o, orient_ms_all=[float(t) for t in orient_ms], describe_ms=d, describe_ms_all=[float(t) for t in describe_ms],
                   describe_chunk=args.chunk, describe_chunks=(n_kp + args.chunk - 1) // args.chunk,
                   orient_candidates_per_s=n_candidates / (o * 1e-3), describe_keypoints_per_s=n_kp / (d * 1e-3) if n_kp else 0.0,
                   describe_voxel_visits=visits, describe_voxel_visits_per_s=visits / (d * 1e-3),
                   describe_contributing_share=contributing_share(kp, gauss, 3) if n_kp else 0.0, accumulation="768 int64 bins per workgroup in LDS, ds_add_u64")
        if twin is not None and n_candidates:
            import sift3d_twin
            cand = s.detect()
            whole = size <= args.twin_full
            pick = np.arange(n_candidates) if whole else np.unique(np.linspace(0, n_candidates - 1, min(args.twin_sample, n_candidates)).round().astype(int))
            layers = [sift3d_twin.Layer(tuple(int(v) for v in g["dims"]), tuple(np.float32(u) for u in g["units"]), int(g["octave"]), np.float32(g["scale"]),
                                        np.float32(g["sigma"]), np.float32(-1), (0, 0, 0), s.layer(0, i), []) for i, g in enumerate(gauss)]
            pyr = twin.Pyramid(layers, 3)
            e = twin.grid_exponent(volume.cpu().numpy(), (1.0, 1.0, 1.0))
            got_kp, got_status, got_sums = s.orient(cand[pick], with_status=True)
            got_desc = np.concatenate([s.describe(got_kp[at:at + args.chunk]) for at in range(0, max(len(got_kp), 1), args.chunk)])
            t0 = time.perf_counter()
            t_status, t_sums, t_slots = twin.orient(pyr, cand[pick], e)
            t1 = time.perf_counter()
            t_desc = twin.describe(pyr, t_slots[t_status == 0], e)
            t2 = time.perf_counter()
            rec.update(twin_whole_list=bool(whole), twin_threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)), twin_sample_candidates=int(len(pick)),
                       twin_sample_keypoints=int((t_status == 0).sum()), twin_orient_sample_s=t1 - t0, twin_describe_sample_s=t2 - t1,
                       twin_orient_s_scaled_to_list=(t1 - t0) * n_candidates / len(pick),
                       twin_describe_s_scaled_to_list=(t2 - t1) * n_kp / max(int((t_status == 0).sum()), 1),
                       equals_twin=bool(np.array_equal(got_status, t_status) and np.array_equal(got_sums.view(np.uint32), t_sums.view(np.uint32))
                                        and got_kp.tobytes() == t_slots[t_status == 0].tobytes()
                                        and np.array_equal(got_desc.view(np.uint32), t_desc.view(np.uint32))))
            del layers, pyr
        print(json.dumps(rec), flush=True)
        records.append(rec)
        s.close()
        del volume, block, kp_dev
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/sift3d_features_bench.py", records=records), f, indent=1)
        f.write("\n")
    if any(r.get("equals_twin") is False for r in records):
        raise SystemExit("sift3d_features_bench: the kernels' result differs from the twin's")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Measures SIFT3D's scale space (opencorr_amd/csrc/sift3d.hip) on speckle volumes from synth.speckle_pair_3d, default config.

    python tools/sift3d_bench.py [--out profiles/sift3d_scale_space.json] [--sizes 256,512] [--reps 5] [--no-twin]

Per size and arithmetic mode (arith_fma 0 / 1): `build` (both pyramids and max_abs) and `detect` (the candidate list, downloaded)
timed separately with device events on the stream the engine runs on (the volume is a CUDA tensor, so that is torch's current
stream; both calls end in a stream synchronise), the median of --reps calls after two warm-up calls, which also grow the buffers.
Bandwidth: the bytes the algorithm needs, stated in the record, over the time: 8 B per voxel and blur pass (one read, one write;
taps come from LDS), 8 B per voxel of a downsampled layer, 12 B per DoG voxel (two reads, one write), and for the extrema search
24 B per voxel of a searched layer (the three DoG layers read once by the count and once by the fill kernel; the face neighbours
come from cache) plus 24 B per candidate.  Share of peak: against 8 TB/s of HBM3E.  Beside it the CPU restatement's time
(tests/cpp/sift3d_twin.cpp, OpenMP, the thread count in the record: pyramids and scan together) with a bit-for-bit comparison of
max_abs, the candidate list and, up to 256^3, every layer.  Per-kernel times come from a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/sift3d_bench.py --no-twin --reps 1 ...).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12


def byte_count(gauss, dog, n_octave_layers, candidates):
    """(build bytes, detect bytes) from the layer tables alone"""
    per, dper = n_octave_layers + 3, n_octave_layers + 2
    build = 0
    for i, g in enumerate(gauss):
        vox = int(np.prod(g["dims"].astype(np.int64)))
        build += vox * (8 if i % per == 0 and i > 0 else 24)
    detect = 24 * candidates
    for d, layer in enumerate(dog):
        vox = int(np.prod(layer["dims"].astype(np.int64)))
        build += 12 * vox
        if 1 <= d % dper <= n_octave_layers:
            detect += 24 * vox
    return build, detect


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift3d_scale_space.json"))
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-twin", action="store_true")
    args = ap.parse_args()

    import torch
    import opencorr_amd
    from opencorr_amd import capi, synth
    if capi.device_count() < 1:
        raise SystemExit("sift3d_bench: no GPU")
    twin = None
    if not args.no_twin:
        import sift3d_twin as twin
        twin.lib()
    records = []
    for size in (int(v) for v in args.sizes.split(",")):
        volume, _ = synth.speckle_pair_3d(size, size, size, device="cuda")
        torch.cuda.synchronize()
        host = volume.cpu().numpy()
        for fma in (0, 1):
            s = opencorr_amd.SIFT3DScaleSpace()
            s.set_tuning("arith_fma", fma)
            s.set_volume(volume)
            for _ in range(2):
                s.build()
                cand = s.detect()
            build_ms, detect_ms = [], []
            for _ in range(args.reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                s.build()
                ev[1].record()
                cand = s.detect()
                ev[2].record()
                torch.cuda.synchronize()
                build_ms.append(ev[0].elapsed_time(ev[1]))
                detect_ms.append(ev[1].elapsed_time(ev[2]))
            gauss, dog = s.layers(0), s.layers(1)
            build_bytes, detect_bytes = byte_count(gauss, dog, 3, len(cand))
            b, d = float(np.median(build_ms)), float(np.median(detect_ms))
            rec = dict(size=size, arith_fma=fma, n_octave=int(gauss["octave"].max()) + 1, candidates=int(len(cand)),
                       build_ms=b, build_ms_all=[float(t) for t in build_ms], detect_ms=d, detect_ms_all=[float(t) for t in detect_ms],
                       build_bytes=build_bytes, detect_bytes=detect_bytes, build_bytes_per_s=build_bytes / (b * 1e-3),
                       detect_bytes_per_s=detect_bytes / (d * 1e-3), build_share_of_hbm_peak=build_bytes / (b * 1e-3) / HBM_BYTES_PER_S,
                       detect_share_of_hbm_peak=detect_bytes / (d * 1e-3) / HBM_BYTES_PER_S)
            if twin is not None:
                t0 = time.perf_counter()
                want = twin.scale_space(host, fma=fma)
                rec["twin_s"] = time.perf_counter() - t0
                rec["twin_threads"] = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
                same = cand.tobytes() == want.candidates.tobytes()
                same = same and all(np.float32(dog[i]["max_abs"]).view(np.uint32) == np.float32(t.max_abs).view(np.uint32) for i, t in enumerate(want.dog))
                if size <= 256:
                    for pyramid, layers in ((0, want.gauss), (1, want.dog)):
                        same = same and all(np.array_equal(s.layer(pyramid, i).view(np.uint32), t.vol.view(np.uint32)) for i, t in enumerate(layers))
                    rec["layers_compared"] = True
                rec["equals_twin"] = bool(same)
                del want
            print(json.dumps(rec), flush=True)
            records.append(rec)
            s.close()
        del volume
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/sift3d_bench.py", hbm_bytes_per_s=HBM_BYTES_PER_S, records=records), f, indent=1)
        f.write("\n")
    if any(r.get("equals_twin") is False for r in records):
        raise SystemExit("sift3d_bench: the kernels' result differs from the twin's")


if __name__ == "__main__":
    main()

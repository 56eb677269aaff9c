#!/usr/bin/env python
"""Measures SIFT2D's detector (opencorr_amd/csrc/sift2d.hip) on speckle images from synth.speckle_pair_2d, default config.

    python tools/sift2d_bench.py [--out profiles/sift2d_detector.json] [--sizes 4096,512] [--reps 5] [--no-twin]

Per size: `build` (the upscale and both pyramids) and `detect` (scan, localisation, compaction and the download of the list) timed
separately with device events on the stream the engine runs on (the image is a CUDA tensor, so that is torch's current stream;
both calls end in a stream synchronise), the median of --reps calls after two warm-up calls, which also grow the buffers.  A
second `detect` on one build returns the stored list; the timed one follows a fresh `build`.
Bandwidth of `build`: the bytes the algorithm needs, stated in the record, over the time: per input pixel 4 B read and 16 B written
by the upscale; per pixel of a blurred layer 8 B for the rows pass (one read, one write; taps come from LDS) and 8 B for the
columns pass, plus 8 B where a DoG layer leaves with it (the layer the blur started from read once more, the DoG layer written);
8 B per pixel of a resampled layer.  Share of peak: against 8 TB/s of HBM3E, the figure tools/sift3d_bench.py uses.
Beside it the CPU restatement's time (tests/cpp/sift2d_twin.cpp, OpenMP, the thread count in the record: pyramids, and scan with
localisation) with a bit-for-bit comparison of the keypoint list and, up to 1024^2, every layer.  What bounds `build` is not
stated here: that takes counters collected in a run of their own.  Needs a GPU; there is no fallback."""
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


def build_bytes(width, height, gauss, n_octave_layers):
    per = n_octave_layers + 3
    total = 20 * width * height
    for i, g in enumerate(gauss):
        px = int(g["dims"][0]) * int(g["dims"][1])
        if i % per == 0 and i > 0:
            total += 8 * px
        else:
            total += (16 if i % per == 0 else 24) * px
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift2d_detector.json"))
    ap.add_argument("--sizes", default="4096,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-twin", action="store_true")
    args = ap.parse_args()

    import torch
    import opencorr_amd
    from opencorr_amd import capi, synth
    if capi.device_count() < 1:
        raise SystemExit("sift2d_bench: no GPU")
    twin = None
    if not args.no_twin:
        import sift2d_twin as twin
        twin.lib()
    records = []
    for size in (int(v) for v in args.sizes.split(",")):
        image, _ = synth.speckle_pair_2d(size, size, device="cuda")
        torch.cuda.synchronize()
        host = image.cpu().numpy()
        s = opencorr_amd.SIFT2DScaleSpace()
        s.set_image(image)
        for _ in range(2):
            s.build()
            kp = s.detect()
        build_ms, detect_ms = [], []
        for _ in range(args.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            s.build()
            ev[1].record()
            kp = s.detect()
            ev[2].record()
            torch.cuda.synchronize()
            build_ms.append(ev[0].elapsed_time(ev[1]))
            detect_ms.append(ev[1].elapsed_time(ev[2]))
        gauss = s.layers(0)
        nbytes = build_bytes(size, size, gauss, 3)
        b, d = float(np.median(build_ms)), float(np.median(detect_ms))
        rec = dict(size=size, n_octave=int(gauss["octave"].max()) + 1, keypoints=int(len(kp)), build_ms=b, build_ms_all=[float(t) for t in build_ms],
                   detect_ms=d, detect_ms_all=[float(t) for t in detect_ms], build_bytes=nbytes, build_bytes_per_s=nbytes / (b * 1e-3),
                   build_share_of_hbm_peak=nbytes / (b * 1e-3) / HBM_BYTES_PER_S)
        if twin is not None:
            t0 = time.perf_counter()
            want = twin.detector(host, layers=size <= 1024)
            rec["twin_s"] = time.perf_counter() - t0
            rec["twin_threads"] = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
            same = kp.tobytes() == want.keypoints.tobytes()
            if size <= 1024:
                for pyramid, layers in ((0, want.gauss), (1, want.dog)):
                    same = same and all(np.array_equal(s.layer(pyramid, i).view(np.uint32), t.data.view(np.uint32)) for i, t in enumerate(layers))
                rec["layers_compared"] = True
            rec["equals_twin"] = bool(same)
            del want
        print(json.dumps(rec), flush=True)
        records.append(rec)
        s.close()
        del image
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/sift2d_bench.py", hbm_bytes_per_s=HBM_BYTES_PER_S, records=records), f, indent=1)
        f.write("\n")
    if any(r.get("equals_twin") is False for r in records):
        raise SystemExit("sift2d_bench: the kernels' result differs from the twin's")


if __name__ == "__main__":
    main()

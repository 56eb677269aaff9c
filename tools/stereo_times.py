"""Kernel times of the stereo chain on one GPU (hipEvents around the launches, the engines' own profile counters).

    python tools/stereo_times.py [--out FILE.json]

Measured, each after a warm-up and as 5 batches of repetitions (the mean per launch of every batch is kept; the table in
DESIGN.md quotes the median batch and the spread):
  * the undistortion-map kernel at 1200 x 1920 for both GT4 cameras (Calibration::prepare);
  * reconstruct_pois on the GT4 queue (9 997 POI2DS records) and on the same queue tiled to 1 000 000 records, device-resident;
  * Strain on POI2DS (radius 20, 5 neighbours: gather + fit + the K-nearest pass) on the 9 997-record queue and on 1 000 000
    records: the queue laid out 10 x 10 times side by side in the image plane, so that every POI keeps the neighbourhood it has
    in the original; Strain::prepare (the cell sort, with its one host synchronise) by the host clock.
Nothing here asserts; the numbers are printed as one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, BATCHES = 3, 5


def batches(engine, run, reps):
    """ms per launch group: mean of every batch of `reps` calls of run()."""
    for _ in range(WARMUP):
        run()
    engine.synchronize()
    out = []
    for _ in range(BATCHES):
        engine.profile_reset()
        for _ in range(reps):
            run()
        ms, launches = engine.profile_read()
        assert launches == reps, (launches, reps)
        out.append(ms / reps)
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), reps=reps, batches=BATCHES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import opencorr_amd
    import stereo_numpy as sn
    fx = sn.load_fixture()
    t = fx["table"]
    h, w = int(fx["height"]), int(fx["width"])
    res = dict(device=torch.cuda.get_device_name(0), height=h, width=w)
    cams = []
    for k in ("cam1", "cam2"):
        cam = opencorr_amd.Calibration(fx[k + "_intrinsics"], fx[k + "_extrinsics"])
        cam.profile_enable(True)
        res["map_" + k] = batches(cam, lambda cam=cam: cam.prepare(h, w), 50)
        cam.profile_enable(False)
        cams.append(cam)
    stereo = opencorr_amd.Stereovision(cams[0], cams[1])
    stereo.profile_enable(True)
    q = sn.table_to_pois(t)
    n_big = 1000000
    tiles = -(-n_big // len(q))
    big = np.tile(q, (tiles, 1))[:n_big].copy()
    # the strain queue: 10 x 10 copies side by side (the search runs over x, y)
    side = 10
    span_x = float(q[:, 0].max() - q[:, 0].min() + 100)
    span_y = float(q[:, 1].max() - q[:, 1].min() + 100)
    big_strain = np.tile(q, (side * side, 1))
    for k in range(side * side):
        big_strain[k * len(q):(k + 1) * len(q), 0] += (k % side) * span_x
        big_strain[k * len(q):(k + 1) * len(q), 1] += (k // side) * span_y
    big_strain = big_strain[:n_big].copy()
    for name, host, hs, reps in (("9997", q, q, 200), ("1000000", big, big_strain, 20)):
        dev = torch.from_numpy(host).cuda()
        res["reconstruct_pois_" + name] = batches(stereo, lambda dev=dev: stereo.reconstruct_pois(dev), reps)
        st = opencorr_amd.Strain(float(fx["strain_settings"][0]), int(fx["strain_settings"][1]))
        ds = torch.from_numpy(hs).cuda()
        torch.cuda.synchronize()
        prep = []
        for _ in range(WARMUP + BATCHES):
            t0 = time.perf_counter()
            st.prepare(ds)
            st.synchronize()
            prep.append((time.perf_counter() - t0) * 1e3)
        res["strain_prepare_host_clock_" + name] = dict(median_ms=float(np.median(prep[WARMUP:])), min_ms=float(min(prep[WARMUP:])),
                                                        max_ms=float(max(prep[WARMUP:])))
        st.profile_enable(True)
        res["strain_poi2ds_" + name] = batches(st, lambda ds=ds: st.compute(ds), reps)
        st.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""A/B timing of the three arithmetic contracts of ICGN3D1, in ONE process, settings interleaved round by round so that clock
drift hits all of them alike (modelled on tools/onepass_ab.py; the product library, no A/B build).

    python tools/onepass3d_ab.py E|E30 [--rounds 12] [--check 512] [--out profiles/r8a_onepass3d_ab_config_E.json]

E: 512^3 pair, r = 16, 37^3 POIs (config E).  E30: 256^3 pair, r = 30, 8^3 = 512 POIs (the shape of the reference's DVC example).
FFTCC3D guesses; the generators of tests/fullsize/run_configs.py.
Settings: the default, arith_fma = 1, arith_onepass3d = 1 -- HIP events around compute() on a device-resident queue (the block
schedule's kernels included), every shape warmed up first.  Per setting: median / min / max ms, mean iterations.  A phase account
follows: runs with convergence criterion 0 and stop = 1, 2, 3 (every POI that stays inside the volume does exactly k iterations)
under each contract -- the intercept of the line through them is set-up + launch, its slope one iteration.
Before anything is timed the one-pass records of `--check` POIs (a stride through the queue) are compared with the CPU twin
(tests/cpp/icgn3d_onepass_twin.cpp) in every bit, so that a time is never reported for wrong results."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import opencorr_amd as oc
from opencorr_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("config", choices=["E", "E30"])
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--check", type=int, default=512, help="POIs compared with the CPU twin bit for bit (0: none)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dim, r, nside = (512, 16, 37) if args.config == "E" else (256, 30, 8)
dev = torch.device("cuda", 0)
ref, tar = synth.speckle_pair_3d(dim, dim, dim, seed=20260927, device=dev)
xs, ys, zs = synth.poi_grid_3d(dim, dim, dim, nside, nside, nside, r + 8)
stream = torch.cuda.current_stream().cuda_stream
f = oc.FFTCC3D(r, r, r); f.set_stream(stream); f.set_images(ref, tar)
g = oc.ICGN3D1(r, r, r, 0.001, 20.0); g.set_stream(stream); g.share_images(f); g.prepare()
guess = torch.from_numpy(oc.make_pois3d(xs, ys, zs)).to(dev)
f.compute(guess)
q = guess.clone()

#            name               arith_fma  arith_onepass3d
SETTINGS = [("default",                0, 0),
            ("arith_fma",              1, 0),
            ("arith_onepass3d",        0, 1)]


def apply(s):
    g.set_tuning("arith_fma", s[1])
    g.set_tuning("arith_onepass3d", s[2])


def once():
    q.copy_(guess)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); g.compute(q); b.record(); b.synchronize()
    return a.elapsed_time(b)


checked = 0
if args.check > 0:
    import onepass3d_twin as twin

    class Fields:   # what oracle.Prepared3D holds, read back from the engine (bit-exact against the oracle: tests/test_gpu_parity_3d.py)
        pass

    prep = Fields()
    prep.ref = np.ascontiguousarray(ref.cpu().numpy(), dtype=np.float32)
    prep.gx, prep.gy, prep.gz, prep.coef = (np.ascontiguousarray(g.read_field(n)) for n in ("gx", "gy", "gz", "coef"))
    apply(SETTINGS[2])
    once()
    got = q.cpu().numpy()
    sample = np.arange(0, len(got), max(1, len(got) // args.check))[:args.check]
    want = twin.icgn3d1(prep, r, r, r, 0.001, 20.0, np.ascontiguousarray(guess.cpu().numpy()[sample]))
    mism = np.argwhere(got[sample].view(np.uint32) != want.view(np.uint32))
    if mism.size:
        sys.exit("arith_onepass3d differs from the CPU twin on %d values; first (sample index, field): %s" % (len(mism), mism[:10].tolist()))
    checked = len(sample)
    del prep

times = {s[0]: [] for s in SETTINGS}
iters, conv = {}, {}
for s in SETTINGS:   # warm-up of every shape
    apply(s)
    once(); once()
for rd in range(args.rounds):
    for s in SETTINGS:
        apply(s)
        times[s[0]].append(once())
        if rd == 0:
            res = q.cpu().numpy()
            ok = res[:, 18] >= 0
            iters[s[0]] = float(res[ok, 19].astype(np.float64).mean())
            conv[s[0]] = int(ok.sum())

# phase account: exactly k iterations per POI
phases = {}
for s in SETTINGS:
    apply(s)
    ms = []
    for k in (1, 2, 3):
        g.set_iteration(0.0, float(k))
        once()
        ms.append(float(np.median([once() for _ in range(5)])))
    slope = (ms[2] - ms[0]) / 2.0
    phases[s[0]] = {"ms_at_1_2_3_iterations": [round(m, 4) for m in ms], "per_iteration_ms": round(slope, 4),
                    "setup_and_launch_ms": round(ms[0] - slope, 4)}
g.set_iteration(0.001, 20.0)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4)}


med = {name: float(np.median(ts)) for name, ts in times.items()}
out = {"workload": "config %s: %d^3 pair, r = %d, %d^3 POIs, ICGN3D1 compute() on a device-resident queue incl. the block-schedule kernels, "
                   "HIP events, %d interleaved rounds, one launch per round and setting" % (args.config, dim, r, nside, args.rounds),
       "pois_equal_to_the_cpu_twin_in_every_bit": checked,
       "settings": {name: dict(stats(ts), mean_iterations=round(iters[name], 4), converged=conv[name]) for name, ts in times.items()},
       "onepass3d_over_fma": round(med["arith_onepass3d"] / med["arith_fma"], 4),
       "onepass3d_over_default": round(med["arith_onepass3d"] / med["default"], 4),
       "phases_exact_k_iterations": phases}
text = json.dumps(out, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text + "\n")

#!/usr/bin/env python
"""A/B timing of the three arithmetic contracts of ICGN2D1 / ICGN2D2 on configs B and C, in ONE process, settings interleaved
round by round so that clock drift hits all of them alike (modelled on tools/variant_ab.py; the product library, no A/B build).

    python tools/onepass_ab.py B|C [--rounds 24] [--out profiles/r7a_onepass_ab_config_B.json]

B: 4096^2, r = 16, 500 x 500 POIs, ICGN2D1.  C: 4096^2, r = 20, 316 x 316 POIs, ICGN2D2, second-order field.
Settings: the default, arith_fma = 1, arith_onepass = 1 -- HIP events around compute() on a device-resident queue (the tile-order
kernels included), every shape warmed up first.  The default and the fused contract are measured twice: as they ship (the set-up
cache serves every call after the first on one reference: "icgn2d_setup_cache" = 1) and with the cache off (every call computes
its set-up, which is what the one-pass contract always does -- it has no cache).  Per setting: median / min / max ms, mean
iterations.  A phase account follows: runs with convergence criterion 0 and stop = 1, 2, 3 (every POI does exactly k iterations)
under the fused and the one-pass contract, cache off -- the intercept of the line through them is set-up + launch, its slope one
iteration (sweep + passes + solve)."""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import opencorr_amd as oc
from opencorr_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("config", choices=["B", "C"])
ap.add_argument("--rounds", type=int, default=24)
ap.add_argument("--out", default=None)
args = ap.parse_args()

side = 4096
r, ns, engine = (16, 500, 1) if args.config == "B" else (20, 316, 2)
so = dict(uxx=2e-6, vyy=-1e-6) if engine == 2 else None
dev = torch.device("cuda", 0)
ref, tar = synth.speckle_pair_2d(side, side, seed=20260925, device=dev, second_order=so)
xs, ys = synth.poi_grid_2d(side, side, ns, ns, r + 8)
stream = torch.cuda.current_stream().cuda_stream
f = oc.FFTCC2D(r, r); f.set_stream(stream); f.set_images(ref, tar)
g = (oc.ICGN2D1 if engine == 1 else oc.ICGN2D2)(r, r, 0.001, 10.0); g.set_stream(stream); g.share_images(f); g.prepare()
guess = torch.from_numpy(oc.make_pois2d(xs, ys)).to(dev)
f.compute(guess)
q = guess.clone()

#            name                     arith_fma  arith_onepass  icgn2d_setup_cache
SETTINGS = [("default",                      0, 0, 1),
            ("arith_fma",                    1, 0, 1),
            ("arith_onepass",                0, 1, 1),
            ("default_no_setup_cache",       0, 0, 0),
            ("arith_fma_no_setup_cache",     1, 0, 0)]


def apply(s):
    g.set_tuning("arith_fma", s[1])
    g.set_tuning("arith_onepass", s[2])
    g.set_tuning("icgn2d_setup_cache", s[3])


def once():
    q.copy_(guess)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); g.compute(q); b.record(); b.synchronize()
    return a.elapsed_time(b)


times = {s[0]: [] for s in SETTINGS}
iters, conv = {}, {}
for s in SETTINGS:   # warm-up of every shape (twice: the second call of a cached setting is a "use" launch)
    apply(s)
    once(); once()
for rd in range(args.rounds):
    for s in SETTINGS:
        apply(s)
        if s[3]:
            once()   # (switching contracts invalidates the records: this call fills them, the timed one uses them)
        times[s[0]].append(once())
        if rd == 0:
            res = q.cpu().numpy()
            ok = res[:, 16] >= 0
            iters[s[0]] = float(res[ok, 17].astype(np.float64).mean())
            conv[s[0]] = int(ok.sum())

# phase account: exactly k iterations per POI
phases = {}
for name, fma, onepass in (("arith_fma", 1, 0), ("arith_onepass", 0, 1)):
    apply((name, fma, onepass, 0))
    ms = []
    for k in (1, 2, 3):
        g.set_iteration(0.0, float(k))
        once()
        ms.append(float(np.median([once() for _ in range(7)])))
    slope = (ms[2] - ms[0]) / 2.0
    phases[name] = {"ms_at_1_2_3_iterations": [round(m, 4) for m in ms], "per_iteration_ms": round(slope, 4),
                    "setup_and_launch_ms": round(ms[0] - slope, 4)}
g.set_iteration(0.001, 10.0)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4)}


out = {"workload": "config %s: 4096^2, r = %d, %d x %d POIs, ICGN2D%d compute() on a device-resident queue incl. the tile-order kernels, "
                   "HIP events, %d interleaved rounds, one launch per round and setting" % (args.config, r, ns, ns, engine, args.rounds),
       "settings": {name: dict(stats(ts), mean_iterations=round(iters[name], 4), converged=conv[name]) for name, ts in times.items()},
       "onepass_over_fma": round(float(np.median(times["arith_onepass"]) / np.median(times["arith_fma"])), 4),
       "onepass_over_fma_no_setup_cache": round(float(np.median(times["arith_onepass"]) / np.median(times["arith_fma_no_setup_cache"])), 4),
       "onepass_over_default_no_setup_cache": round(float(np.median(times["arith_onepass"]) / np.median(times["default_no_setup_cache"])), 4),
       "phases_exact_k_iterations_no_setup_cache": phases}
text = json.dumps(out, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text + "\n")

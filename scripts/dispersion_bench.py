#!/usr/bin/env python3
"""Dispersion estimation (include/octpipe.h "dispersion estimation"): prints one JSON line with
  * candidate-A-scans per second of the sweep kernel (oct_dispersion_sweep_kernel) at N = 1024 and 2048, K = 256 candidates
    (a 16 x 16 grid) x M = 512 A-scans, from device events around its launches (octpipe_debug_dispersion_metrics);
  * the wall time of Pipeline.estimate_dispersion at the Dispersion Estimator extension's defaults (N = 1024, 40 A-scans from the
    centre of frame 0, 50 samples per range, two steps) on a raw buffer in host memory.

    python scripts/dispersion_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bscans", type=int, default=16, help="B-scans of the raw buffer (the sweep reads only the A-scans it scores)")
    args = ap.parse_args()

    import numpy as np
    from octproz_amd import Pipeline, synthetic_raw, v180_benchmark_params
    from octproz_amd.pipeline import dispersion_range

    out = {"bench": "dispersion_estimation", "K": 256, "M": 512}
    c = dispersion_range(-100.0, 100.0, 16)
    d2, d3 = np.repeat(c, 16), np.tile(c, 16)
    for n in (1024, 2048):
        p = v180_benchmark_params(n, 512, args.bscans)
        raw = synthetic_raw(n, 512, args.bscans, seed=11)
        pipe = Pipeline(p, device=0)
        for _ in range(3):
            pipe.dispersion_metrics(raw, d2, d3, 0, 512, "peak")
        ms = []
        for _ in range(args.reps):
            _, _, t = pipe.dispersion_metrics(raw, d2, d3, 0, 512, "peak")
            ms.append(t)
        med = float(np.median(ms))
        out["sweep_kernel_ms_N%d" % n] = round(med, 4)
        out["sweep_cand_ascans_per_s_N%d" % n] = round(256 * 512 / (med * 1e-3))
        pipe.close()

    p = v180_benchmark_params(1024, 512, args.bscans)
    raw = synthetic_raw(1024, 512, args.bscans, seed=12)
    pipe = Pipeline(p, device=0)
    for _ in range(3):
        est = pipe.estimate_dispersion(raw)
    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        est = pipe.estimate_dispersion(raw)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["estimate_wall_ms_N1024_M40_S50"] = round(float(np.median(wall)), 3)
    out["estimate_wall_ms_min"] = round(float(np.min(wall)), 3)
    out["estimate_best"] = [est.d2, est.d3]
    pipe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Peak analysis (include/octpipe.h "peak analysis") at the headline shape, 1024 x 512 x 256, on the handle's processed volume.
  * the extensions' call: one B-scan ROI, 512 A-scans, depth [16, 512), G = 512, fit on: wall time per call on the host clock (the
    call returns with the results on the host), median of --reps;
  * peak map: G = 1 over the whole volume (256 MiB, 131 072 groups), fit off: device events around the call's kernels, median of --reps;
  * roll-off: G = 512 over the whole volume (256 groups), fit on: device events;
  * peak map with fit: G = 1, fit on: device events.
Read rates count the region's bytes once.  The data (--data): a linear-scaled mirror sweep, the case the fit is meant for (default),
or the headline's log-scaled test signal, where most fits run to maxIterations.  Prints one JSON line and writes it to --out.

    python scripts/peak_analysis_bench.py [--reps 20] [--data mirror|synthetic] [--out profiles/peak_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peak_bench.json"))
    ap.add_argument("--data", choices=("mirror", "synthetic"), default="mirror",
                    help="mirror: a linear-scaled mirror sweep (default); synthetic: the headline's log-scaled test signal")
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, synthetic_raw, v180_benchmark_params

    n, a, b = 1024, 512, 256
    out = {"bench": "peak_analysis", "shape": [n, a, b], "reps": args.reps, "data": args.data}
    p = v180_benchmark_params(n, a, b)
    if args.data == "mirror":
        # what the Axial PSF Analyzer looks at: linear scaling, no k-linearisation / dispersion / mean-line subtraction, a mirror
        # (Gaussian spectral envelope, sigma = N / 10) at a depth that moves through 0.05 N .. 0.4 N over the B-scans and tilts a little
        # across the A-scans
        p.signalLogScaling, p.resampling, p.dispersionCompensation, p.fixedPatternNoiseRemoval = 0, 0, 0, 0
        p.update_all_curves()
        k = torch.arange(n, dtype=torch.float32, device="cuda:0")
        env = torch.exp(-0.5 * ((k - n / 2) / (n / 10)) ** 2)
        z = (0.05 * n + 0.35 * n * torch.arange(b, device="cuda:0", dtype=torch.float32)[:, None] / b
             + 0.01 * torch.arange(a, device="cuda:0", dtype=torch.float32)[None, :] + 0.3)
        d_raw = torch.empty((b, a, n), dtype=torch.int16, device="cuda:0")
        for i in range(b):
            row = 2048.0 + 1500.0 * env[None, :] * torch.cos(2 * np.pi * z[i][:, None] * k[None, :] / n)
            d_raw[i] = torch.clamp(torch.round(row), 0, 4095).to(torch.int16)
    else:
        d_raw = torch.from_numpy(synthetic_raw(n, a, b, seed=1).view(np.int16)).to("cuda:0")
    pipe = Pipeline(p, device=0)
    pipe.process_device(d_raw.data_ptr())
    pipe.synchronize()
    vbytes = a * b * (n // 2) * 4

    def record(name, kw):
        for _ in range(3):
            pipe.peak_analysis_timed(**kw)
        ms = []
        for _ in range(args.reps):
            res, t = pipe.peak_analysis_timed(**kw)
            ms.append(t)
        med = float(np.median(ms))
        out["us_" + name] = round(med * 1e3, 1)
        out["TBps_" + name] = round(vbytes / (med * 1e-3) / 1e12, 3)
        out["peak_share_" + name] = round(vbytes / (med * 1e-3) / HBM_PEAK, 3)
        out["fit_converged_" + name] = int(res.fit_converged.sum())
        out["groups_" + name] = int(res.status.size)

    one = dict(bscans=(b // 2, 1), depth=(16, n // 2 - 16), ascans_per_group=a, fit=True)
    for _ in range(5):
        pipe.peak_analysis(**one)
    wall = []
    for _ in range(max(args.reps, 20)):
        t0 = time.perf_counter()
        pipe.peak_analysis(**one)
        wall.append((time.perf_counter() - t0) * 1e6)
    out["us_wall_extension_call"] = round(float(np.median(wall)), 1)
    _, ms = pipe.peak_analysis_timed(**one)
    out["us_device_extension_call"] = round(ms * 1e3, 1)
    record("map_g1_nofit", dict(ascans_per_group=1, fit=False))
    record("rolloff_g512_fit", dict(ascans_per_group=a, fit=True))
    record("map_g1_fit", dict(ascans_per_group=1, fit=True))
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

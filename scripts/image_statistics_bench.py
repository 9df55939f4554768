#!/usr/bin/env python3
"""Image statistics (include/octpipe.h "image statistics") at the headline shape, 1024 x 512 x 256, on device-resident data.  Device
events around each call's work (octpipe_debug_processed_statistics / octpipe_debug_raw_statistics), median of --reps calls:
  * processed whole buffer (256 MiB, the product's own log-scaled output), 256 bins, explicit range;
  * the same with autoRange (two passes: the read rate counts the bytes twice);
  * a constant buffer, every value in one bin (the adversarial case of the LDS histogram);
  * one B-scan ROI (512 x 512), wall time per call on the host clock (the call returns with the results on the host);
  * raw uint16 whole buffer (128 MiB), 4096 bins, lo = 0, width = 1;
  * packed 12-bit raw whole buffer (96 MiB), 4096 bins.
Prints one JSON line and writes it to --out.

    python scripts/image_statistics_bench.py [--reps 20] [--out profiles/stats_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, synthetic_raw, v180_benchmark_params

    n, a, b = 1024, 512, 256
    out = {"bench": "image_statistics", "shape": [n, a, b], "reps": args.reps}

    def record(name, nbytes, fn, passes=1):
        for _ in range(3):
            fn()
        ms = [fn()[1] for _ in range(args.reps)]
        med = float(np.median(ms))
        out["ms_" + name] = round(med, 4)
        out["GBps_" + name] = round(passes * nbytes / (med * 1e-3) / 1e9, 1)
        out["peak_share_" + name] = round(passes * nbytes / (med * 1e-3) / HBM_PEAK, 3)
        return med

    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    raw = synthetic_raw(n, a, b, seed=1)
    d_raw = torch.from_numpy(raw.view(np.int16)).to("cuda:0")
    pipe.process_device(d_raw.data_ptr())
    pipe.synchronize()
    pbytes = a * b * (n // 2) * 4
    first = pipe.processed_statistics(bins=256)  # the range the explicit case uses: the data's own
    rng = (first.lo, first.hi)
    out["processed_range"] = [rng[0], rng[1]]
    t_real = record("processed_256_explicit", pbytes, lambda: pipe.processed_statistics_timed(bins=256, range=rng))
    record("processed_256_auto", pbytes, lambda: pipe.processed_statistics_timed(bins=256), passes=2)
    const = torch.full((b, a, n // 2), 42.0, dtype=torch.float32, device="cuda:0")
    t_const = record("processed_256_constant", pbytes, lambda: pipe.processed_statistics_timed(data=const, bins=256, range=(0.0, 100.0)))
    out["constant_over_realistic"] = round(t_const / t_real, 3)
    for _ in range(5):
        pipe.processed_statistics(bscans=(b // 2, 1), bins=256, range=rng)
    wall = []
    for _ in range(max(args.reps, 50)):
        t0 = time.perf_counter()
        pipe.processed_statistics(bscans=(b // 2, 1), bins=256, range=rng)
        wall.append((time.perf_counter() - t0) * 1e6)
    out["us_wall_one_bscan_512x512"] = round(float(np.median(wall)), 1)
    _, ms = pipe.processed_statistics_timed(bscans=(b // 2, 1), bins=256, range=rng)
    out["us_device_one_bscan_512x512"] = round(ms * 1e3, 1)
    record("raw_u16_4096", a * b * n * 2, lambda: pipe.raw_statistics_timed(d_raw, bins=4096, lo=0, bin_width=1))
    del const
    pipe.close()

    pk = Pipeline(v180_benchmark_params(n, a, b), device=0, sample_format=1)
    nbytes = pk.raw_buffer_bytes()
    d_pk = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda:0")
    record("raw_p12_4096", nbytes, lambda: pk.raw_statistics_timed(d_pk, bins=4096, lo=0, bin_width=1))
    pk.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

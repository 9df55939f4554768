#!/usr/bin/env python3
"""Phase extraction (include/octpipe.h "phase extraction"): prints one JSON line with
  * the accumulate kernel's read rate (GB/s and share of the 8 TB/s HBM peak) on device-resident raw buffers: 1024 x 512 x 256 uint16
    (256 MiB), the same as packed 12 bit (192 MiB) and config 3's 2 GiB buffer (4096 x 1024 x 256 uint16), from device events around
    the kernel (octpipe_debug_phase_accumulate);
  * the wall time of one extract call (octpipe_extract_resample_curve on a given mean) at N = 1024, 2048 and 4096;
  * the end-to-end wall time of Pipeline.extract_resample_curve from one 1024 x 512 x 256 uint16 buffer in host memory.

    python scripts/phase_extraction_bench.py [--reps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import OctAlgorithmParameters, Pipeline
    import phase_model as pm

    def params(n, a, b, bit_depth=12):
        p = OctAlgorithmParameters()
        p.samplesPerLine, p.ascansPerBscan, p.bscansPerBuffer, p.bitDepth = n, a, b, bit_depth
        p.update_all_curves()
        return p

    out = {"bench": "phase_extraction"}
    for name, n, a, b, fmt in (("u16_1024x512x256", 1024, 512, 256, 0), ("p12_1024x512x256", 1024, 512, 256, 1),
                               ("u16_4096x1024x256", 4096, 1024, 256, 0)):
        pipe = Pipeline(params(n, a, b), device=0, sample_format=fmt)
        nbytes = pipe.raw_buffer_bytes()
        d = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda:0")
        pipe.phase_reset()
        for _ in range(2):
            pipe.phase_accumulate_timed(d.data_ptr())
        ms = []
        for _ in range(args.reps):
            pipe.phase_reset()
            ms.append(pipe.phase_accumulate_timed(d.data_ptr()))
        med = float(np.median(ms))
        out["acc_ms_" + name] = round(med, 4)
        out["acc_GBps_" + name] = round(nbytes / (med * 1e-3) / 1e9, 1)
        out["acc_peak_share_" + name] = round(nbytes / (med * 1e-3) / HBM_PEAK, 3)
        del d
        pipe.close()
        torch.cuda.empty_cache()

    for n in (1024, 2048, 4096):
        pipe = Pipeline(params(n, 32, 2), device=0)
        mean = pm.calibration_raw(n, 64, seed=n).astype(np.float64).mean(axis=0).astype(np.float32)
        kw = dict(mean=mean, peak=(int(0.2 * n), int(0.4 * n)), ignore_first=n // 16, ignore_last=n // 16)
        for _ in range(3):
            pipe.extract_resample_curve(**kw)
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pipe.extract_resample_curve(**kw)
            wall.append((time.perf_counter() - t0) * 1e3)
        out["extract_wall_ms_N%d" % n] = round(float(np.median(wall)), 3)
        pipe.close()

    n, a, b = 1024, 512, 256
    pipe = Pipeline(params(n, a, b), device=0)
    one = pm.calibration_raw(n, 64, seed=5)
    raw = np.ascontiguousarray(np.tile(one, (a * b // 64, 1)))
    pipe.extract_resample_curve(raws=raw, peak=(200, 400), ignore_first=64, ignore_last=64)
    wall = []
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        pipe.extract_resample_curve(raws=raw, peak=(200, 400), ignore_first=64, ignore_last=64)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["end_to_end_wall_ms_host_u16_1024x512x256"] = round(float(np.median(wall)), 2)
    pipe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

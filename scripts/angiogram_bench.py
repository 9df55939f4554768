#!/usr/bin/env python3
"""Angiography (include/octpipe.h "angiography") at the headline shape, 1024 x 512 x 256 (131 072 A-scans of 512 depth bins, 256 MiB of
float32) read as 64 slow-axis positions of M = 4 repeats, device memory throughout:
  * the volume call per method, with and without the mean volume: device events around the call's work (octpipe_debug_angiogram),
    median of --reps; it reads the 256 MiB once and writes 64 MiB (128 MiB with the mean);
  * the en face call per method with a 16-bin and a 128-bin slab, averaging and MIP, under a synthetic tilted surface z = 100 + 0.2 a +
    0.3 b (what octpipe_surface_detect / _smooth would hand over): it reads M x thickness bins per output A-scan;
  * the yardstick, measured in the same run: a device-to-device hipMemcpyAsync of the volume's 256 MiB, events around it.
Prints one JSON line and writes it to --out.

    python scripts/angiogram_bench.py [--reps 20] [--out profiles/angio_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "angio_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, v180_benchmark_params

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    n, a, b, M = 1024, 512, 256, 4
    depth, P = n // 2, b // M
    out = {"bench": "angiogram", "shape": [n, a, b], "repeats": M, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    vol = torch.rand((b, a, depth), device="cuda:0", generator=g).contiguous()
    z = (100.0 + 0.2 * torch.arange(a, device="cuda:0", dtype=torch.float32)[None, :]
         + 0.3 * torch.arange(b, device="cuda:0", dtype=torch.float32)[:, None])
    surface = torch.ceil(z).to(torch.int32).contiguous()
    angio = torch.empty((P, a, depth), dtype=torch.float32, device="cuda:0")
    mean = torch.empty((P, a, depth), dtype=torch.float32, device="cuda:0")
    image = torch.empty((P, a), dtype=torch.float32, device="cuda:0")
    copy_dst = torch.empty((b, a, depth), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vbytes, obytes = a * b * depth * 4, P * a * depth * 4

    def median_ms(call, reps=args.reps):
        for _ in range(3):
            call()
        return float(np.median([call() for _ in range(reps)]))

    def record(name, ms, nbytes):
        out["us_" + name] = round(ms * 1e3, 1)
        out["bytes_" + name] = int(nbytes)
        out["TBps_" + name] = round(nbytes / (ms * 1e-3) / 1e12, 3)
        out["peak_share_" + name] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)

    hip = C.CDLL("libamdhip64.so")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy():
        ev[0].record()
        assert hip.hipMemcpyAsync(C.c_void_p(copy_dst.data_ptr()), C.c_void_p(vol.data_ptr()), C.c_size_t(vbytes), 3, None) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    ms_copy = median_ms(copy)
    record("copy_d2d", ms_copy, 2 * vbytes)
    for method in ("variance", "decorrelation", "difference"):
        ms = median_ms(lambda: pipe.angiogram_timed(M, method, data=vol, out=angio)[1])
        record("volume_" + method, ms, vbytes + obytes)
        out["volume_%s_over_copy" % method] = round(ms / ms_copy, 3)
        ms_mean = median_ms(lambda: pipe.angiogram_timed(M, method, mean=mean, data=vol, out=angio)[1])
        record("volume_%s_with_mean" % method, ms_mean, vbytes + 2 * obytes)
        out["volume_%s_with_mean_over_copy" % method] = round(ms_mean / ms_copy, 3)
        for thickness in (16, 128):
            for fn in ("average", "mip"):
                ms_e = median_ms(lambda: pipe.angiogram_enface_timed(M, method, surface=surface, offset=0, thickness=thickness, function=fn,
                                                                     data=vol, out=image)[1])
                name = "enface_%s_t%d_%s" % (method, thickness, fn)
                record(name, ms_e, P * a * (M * thickness * 4 + 8))
                out[name + "_over_volume"] = round(ms_e / ms, 3)
    # the two forms of the en face kernel (1: one wave per A-scan, 2: teams of 16 lanes, four A-scans per wave) alternating in one loop
    for method, fn in (("variance", "average"), ("variance", "mip"), ("decorrelation", "average")):
        for thickness in (16, 64):
            t = {1: [], 2: []}
            for rep in range(3 + args.reps):
                for form in (1, 2):
                    ms = pipe.angiogram_enface_timed(M, method, surface=surface, offset=0, thickness=thickness, function=fn, data=vol, out=image,
                                                     form=form)[1]
                    if rep >= 3:
                        t[form].append(ms)
            for form, what in ((1, "wave"), (2, "team")):
                record("enface_%s_t%d_%s_%s_form" % (method, thickness, fn, what), float(np.median(t[form])), P * a * (M * thickness * 4 + 8))
            out["enface_%s_t%d_%s_team_over_wave" % (method, thickness, fn)] = round(float(np.median(t[2]) / np.median(t[1])), 3)
    # the yardstick once more at the end: the spread between two medians of the same thing in this run
    record("copy_d2d_again", median_ms(copy), 2 * vbytes)
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

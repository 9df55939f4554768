#!/usr/bin/env python3
"""Depth-resolved attenuation (include/octpipe.h "attenuation") at the headline shape, 1024 x 512 x 256 (131 072 A-scans of 512 depth bins,
256 MiB of float32 in, 256 MiB out), on a synthetic sample: speckle (chi-squared intensity) that decays exponentially below the tilted plane
z = 100 + 0.2 a + 0.3 b, a noise floor above it; stored as an intensity, as an amplitude and in decibels.
  * the volume call in device memory throughout, scale 0 / 1 / 2, with and without a gain table: device events around the call's work
    (octpipe_debug_attenuation), median of --reps; the six variants alternate;
  * yardstick: a device-to-device hipMemcpyAsync of the volume, events around it, same run; every variant is stated as a multiple of it;
  * the float64 sums of the debug entry (twice the bytes out), for the record;
  * the en face call under the detected and smoothed surface, slabs of 16 and 128 bins, averaging, per scale; bytes read are counted from
    the surface (an A-scan is read from the first bin of its slab down to the end of the window, in whole chunks of 256 bins).
Prints one JSON line and writes it to --out.

    python scripts/attenuation_bench.py [--reps 20] [--out profiles/attenuation_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attenuation_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, v180_benchmark_params

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    n, a, b = 1024, 512, 256
    depth = n // 2
    delta, mu = 0.005, 2.0
    out = {"bench": "attenuation", "shape": [n, a, b], "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    z = (100.0 + 0.2 * torch.arange(a, device="cuda:0", dtype=torch.float32)[None, :, None]
         + 0.3 * torch.arange(b, device="cuda:0", dtype=torch.float32)[:, None, None])
    d = torch.arange(depth, device="cuda:0", dtype=torch.float32)[None, None, :]
    speckle = torch.randn((b, a, depth), device="cuda:0", generator=g) ** 2
    intensity = (speckle * (1e-4 + (d >= z).to(torch.float32) * torch.exp(-2.0 * mu * delta * (d - z).clamp(min=0.0)))).contiguous()
    del speckle
    vols = {"intensity": intensity, "amplitude": intensity.sqrt().contiguous(),
            "log2": (10.0 * torch.log10(intensity.clamp(min=1e-30))).contiguous()}
    maps = {"intensity": (1.0, 0.0), "amplitude": (1.0, 0.0), "log2": (float(np.log2(10.0) / 10.0), 0.0)}
    gain = torch.exp(torch.arange(depth, device="cuda:0", dtype=torch.float32) * 2e-3).contiguous()
    result = torch.empty((b, a, depth), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rows, vbytes = a * b, a * b * depth * 4

    def record(name, ms, nbytes):
        out["us_" + name] = round(ms * 1e3, 1)
        out["bytes_" + name] = int(nbytes)
        out["TBps_" + name] = round(nbytes / (ms * 1e-3) / 1e12, 3)
        out["peak_share_" + name] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)

    def median_ms(call, reps=args.reps):
        for _ in range(3):
            call()
        return float(np.median([call() for _ in range(reps)]))

    # the six variants of the volume call, alternating
    variants = [(scale, with_gain) for scale in ("intensity", "amplitude", "log2") for with_gain in (False, True)]
    times = {v: [] for v in variants}
    for rep in range(3 + args.reps):
        for scale, with_gain in variants:
            ms = pipe.attenuation_timed(delta, scale, maps[scale], noise=1e-4, gain=gain if with_gain else None, data=vols[scale], out=result)[1]
            if rep >= 3:
                times[(scale, with_gain)].append(ms)
    # a plausible result: without a gain table the mean coefficient well below the surface is the sample's
    pipe.attenuation(delta, "intensity", noise=1e-4, data=intensity, out=result)
    pipe.synchronize()
    out["mu_mean_below_surface"] = round(result[:, :, 300:400].double().mean().item(), 3)
    out["mu_of_the_sample"] = mu
    # yardstick: a device-to-device copy of the volume
    hip = C.CDLL("libamdhip64.so")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy():
        ev[0].record()
        assert hip.hipMemcpyAsync(C.c_void_p(result.data_ptr()), C.c_void_p(intensity.data_ptr()), C.c_size_t(vbytes), 3, None) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    ms_copy = median_ms(copy)
    record("copy_d2d", ms_copy, 2 * vbytes)
    for scale, with_gain in variants:
        name = "volume_" + scale + ("_gain" if with_gain else "")
        ms = float(np.median(times[(scale, with_gain)]))
        record(name, ms, 2 * vbytes)
        out[name + "_over_copy"] = round(ms / ms_copy, 3)
    # the float64 sums (the debug entry has no device timing: events of the handle's stream around the call)
    sums = torch.empty((b, a, depth), dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.ExternalStream(pipe.stream_ptr())

    def sums_call():
        ev[0].record(stream)
        pipe.attenuation_sums(delta, "intensity", noise=1e-4, data=intensity, out=sums)
        ev[1].record(stream)
        pipe.synchronize()
        return ev[0].elapsed_time(ev[1])

    ms = median_ms(sums_call)
    record("sums_intensity", ms, 3 * vbytes)
    out["sums_intensity_over_copy"] = round(ms / ms_copy, 3)
    del sums
    # the en face call under the detected, smoothed surface
    raw_surface = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    surface = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    image = torch.empty((b, a), dtype=torch.float32, device="cuda:0")
    pipe.detect_surface(5e-3, 3, data=intensity, out=raw_surface)
    pipe.smooth_surface(raw_surface, 2, out=surface)
    pipe.synchronize()
    s = surface.cpu().numpy().astype(np.int64)
    out["surface_found"] = int((s >= 0).sum())
    out["surface_error_median"] = float(np.median(np.abs(s - np.ceil(z[:, :, 0].cpu().numpy()))[s >= 0]))
    for thickness in (16, 128):
        lo = np.maximum(s + 2, 0)
        chunks = np.where((s >= 0) & (lo < depth), -(-depth // 256) - lo // 256, 0)  # chunks of 256 bins an A-scan is walked over
        ebytes = int(np.minimum(chunks * 256, depth - np.minimum(lo, depth)).sum()) * 4 + rows * 8
        for scale in ("intensity", "amplitude", "log2"):
            ms = median_ms(lambda: pipe.attenuation_enface_timed(delta, surface, 2, thickness, "average", 0.0, scale, maps[scale], noise=1e-4,
                                                                 data=vols[scale], out=image)[1])
            name = "enface_t%d_%s" % (thickness, scale)
            record(name, ms, ebytes)
            out[name + "_over_copy"] = round(ms / ms_copy, 3)
        out["enface_t%d_median" % thickness] = round(image[(surface >= 0)].median().item(), 3)
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Repeat registration (include/octpipe.h "repeat registration") at the headline shape, 1024 x 512 x 256 (131 072 A-scans of 512 depth bins,
256 MiB of float32) read as 64 slow-axis positions of M = 4 repeats, device memory throughout.  The volume is built from shifted copies
(every repeat of a position moved by a known number of bins, plus noise), so the estimate has something to find and the registered calls
run with the shifts a user would hand them.  Device events around each call's work (the octpipe_debug_* twins), median and min / max of
--reps after three warm-up calls; calls that are compared with each other alternate in one loop:
  * the estimate (R = 8) at G = 512 (one shift per B-scan: chunk partials, then the search), G = 32 and G = 1 (the search kernel alone),
    each beside octpipe_peak_analysis with the fit off at the same G, with and without its averaged A-scans written out: the same reads;
  * the registered volume call per method beside the unregistered one (the same bytes: 256 MiB read, 64 MiB written);
  * the registered en face call per method with a 16-bin averaging slab under a tilted surface beside the unregistered one;
  * the yardstick: a device-to-device hipMemcpyAsync of the volume's 256 MiB, at the start and at the end of the run.
Prints one JSON line and writes it to --out.

    python scripts/repeat_registration_bench.py [--reps 20] [--out profiles/register_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, v180_benchmark_params

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    n, a, b, M, R = 1024, 512, 256, 4, 8
    depth, P = n // 2, b // M
    out = {"bench": "repeat_registration", "shape": [n, a, b], "repeats": M, "max_shift": R, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rng = np.random.default_rng(1)
    delta = rng.integers(-R, R + 1, (P, M))
    delta[:, 0] = 0
    vol = torch.empty((b, a, depth), device="cuda:0")
    for p in range(P):
        base = torch.rand((a, depth + 2 * R), device="cuda:0", generator=g)
        for m in range(M):
            d = int(delta[p, m])
            vol[p * M + m] = base[:, R - d:R - d + depth] + 0.03 * torch.rand((a, depth), device="cuda:0", generator=g)
    z = (100.0 + 0.2 * torch.arange(a, device="cuda:0", dtype=torch.float32)[None, :]
         + 0.3 * torch.arange(b, device="cuda:0", dtype=torch.float32)[:, None])
    surface = torch.ceil(z).to(torch.int32).contiguous()
    angio = torch.empty((P, a, depth), dtype=torch.float32, device="cuda:0")
    image = torch.empty((P, a), dtype=torch.float32, device="cuda:0")
    copy_dst = torch.empty((b, a, depth), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vbytes, obytes = a * b * depth * 4, P * a * depth * 4

    def record(name, times, nbytes=None):
        ms = float(np.median(times))
        out["us_" + name] = round(ms * 1e3, 1)
        out["us_" + name + "_min_max"] = [round(float(np.min(times)) * 1e3, 1), round(float(np.max(times)) * 1e3, 1)]
        if nbytes is not None:
            out["bytes_" + name] = int(nbytes)
            out["TBps_" + name] = round(nbytes / (ms * 1e-3) / 1e12, 3)
            out["peak_share_" + name] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)
        return ms

    def alternating(calls, reps=args.reps):
        """{name: times in ms}: the calls one after the other in every round of one loop, three warm-up rounds"""
        t = {name: [] for name, _ in calls}
        for rep in range(3 + reps):
            for name, call in calls:
                ms = call()
                if rep >= 3:
                    t[name].append(ms)
        return t

    hip = C.CDLL("libamdhip64.so")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy():
        ev[0].record()
        assert hip.hipMemcpyAsync(C.c_void_p(copy_dst.data_ptr()), C.c_void_p(vol.data_ptr()), C.c_size_t(vbytes), 3, None) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    ms_copy = record("copy_d2d", alternating([("copy", copy)])["copy"], 2 * vbytes)

    # ---- the estimate beside the peak analysis' averaging at the same G
    for G in (512, 32, 1):
        Qp = a // G
        dsh = torch.empty((P, M, Qp), dtype=torch.int32, device="cuda:0")
        reps = args.reps if G > 1 else max(5, args.reps // 2)  # (G = 1 with averaged A-scans brings 256 MiB to the host per call)
        t = alternating([("estimate", lambda: pipe.register_repeats_timed(M, G, R, data=vol, out=dsh)[1]),
                         ("peak", lambda: pipe.peak_analysis_timed(data=vol, ascans_per_group=G, fit=False, averaged=False)[1]),
                         ("peak_averaged", lambda: pipe.peak_analysis_timed(data=vol, ascans_per_group=G, fit=False, averaged=True)[1])], reps)
        ms = record("estimate_G%d" % G, t["estimate"], vbytes)
        ms_peak = record("peak_analysis_G%d" % G, t["peak"], vbytes)
        ms_avg = record("peak_analysis_averaged_G%d" % G, t["peak_averaged"], vbytes + b * Qp * depth * 4)
        out["estimate_G%d_over_copy" % G] = round(ms / ms_copy, 3)
        out["estimate_G%d_over_peak_analysis" % G] = round(ms / ms_peak, 3)
        out["estimate_G%d_over_peak_analysis_averaged" % G] = round(ms / ms_avg, 3)
        if G == a:
            pipe.synchronize()
            found = dsh.cpu().numpy()[:, :, 0]
            out["true_shifts_recovered"] = bool(np.array_equal(found, delta))
            shifts = dsh

    # ---- the registered calls beside the unregistered ones, with the shifts of G = 512
    for method in ("variance", "decorrelation", "difference"):
        t = alternating([("plain", lambda: pipe.angiogram_timed(M, method, data=vol, out=angio)[1]),
                         ("registered", lambda: pipe.angiogram_timed(M, method, data=vol, out=angio, shifts=shifts, ascans_per_group=a)[1])])
        ms_plain = record("volume_" + method, t["plain"], vbytes + obytes)
        ms_reg = record("volume_%s_registered" % method, t["registered"], vbytes + obytes)
        out["volume_%s_registered_over_unregistered" % method] = round(ms_reg / ms_plain, 3)
        out["volume_%s_registered_over_copy" % method] = round(ms_reg / ms_copy, 3)
        ekw = dict(surface=surface, offset=0, thickness=16, function="average", data=vol, out=image)
        t = alternating([("plain", lambda: pipe.angiogram_enface_timed(M, method, **ekw)[1]),
                         ("registered", lambda: pipe.angiogram_enface_timed(M, method, shifts=shifts, ascans_per_group=a, **ekw)[1])])
        ms_plain = record("enface_%s_t16" % method, t["plain"], P * a * (M * 16 * 4 + 8))
        ms_reg = record("enface_%s_t16_registered" % method, t["registered"], P * a * (M * 16 * 4 + 8))
        out["enface_%s_t16_registered_over_unregistered" % method] = round(ms_reg / ms_plain, 3)
    # the yardstick once more at the end: the spread between two medians of the same thing in this run
    record("copy_d2d_again", alternating([("copy", copy)])["copy"], 2 * vbytes)
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

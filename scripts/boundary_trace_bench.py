#!/usr/bin/env python3
"""Boundary tracing (include/octpipe.h "boundary tracing") at the headline shape, 1024 x 512 x 256 (256 B-scans of 512 A-scans of 512
depth bins, 256 MiB of float32), on the synthetic tilted surface of surface_views_bench.py: noise of 0 .. 0.2 above the plane
z = 100 + 0.2 a + 0.3 b, 1 .. 1.2 below it.  Device memory throughout, device events around each call's work (octpipe_debug_*), median
of --reps; bytes read are counted from the shapes ((H + 2k) floats per A-scan, the guide, the surface written).
  * the unguided trace over the window [16, 512): H = 496 nodes, one workgroup per B-scan; in every form that applies;
  * the guided trace, band -16 .. +16 (H = 33) around the detected and smoothed surface, one wave per B-scan; in every form;
  * the same two on ONE B-scan: the time of a chain of 512 dependent steps with the machine to itself, i.e. the time per step;
  * yardsticks in the same run: detect + smooth (what the guide costs), and a device-to-device hipMemcpyAsync of the volume.
Expectations, reported as met or missed (nothing is gated on them):
  * the guided narrow-band trace takes less time than the device-to-device copy of the volume;
  * the unguided trace of 256 B-scans stays within what the per-step latency predicts: 512 steps x the time per step measured on one
    B-scan (256 workgroups on 256 CUs run side by side); "within" allows a quarter on top.
Prints one JSON line and writes it to --out.

    python scripts/boundary_trace_bench.py [--reps 20] [--out profiles/boundary_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORM_NAMES = {0: "picked", 1: "wave_lds", 2: "wave_scratch", 3: "group_lds", 4: "group_scratch"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, v180_benchmark_params

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    n, a, b = 1024, 512, 256
    depth, first, k = n // 2, 16, 2
    window = (first, depth - first)
    out = {"bench": "boundary_trace", "shape": [n, a, b], "reps": args.reps, "device": torch.cuda.get_device_name(0), "half_width": k}
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    z = (100.0 + 0.2 * torch.arange(a, device="cuda:0", dtype=torch.float32)[None, :, None]
         + 0.3 * torch.arange(b, device="cuda:0", dtype=torch.float32)[:, None, None])
    d = torch.arange(depth, device="cuda:0", dtype=torch.float32)[None, None, :]
    vol = torch.rand((b, a, depth), device="cuda:0", generator=g) * 0.2
    vol += (d >= z).to(torch.float32)
    vol = vol.contiguous()
    truth = np.ceil(z[:, :, 0].cpu().numpy()).astype(np.int64)
    raw_surface = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    guide = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    traced = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    copy_dst = torch.empty_like(vol)
    torch.cuda.synchronize()
    vbytes = a * b * depth * 4

    def median_ms(call, reps=args.reps):
        for _ in range(3):
            call()
        return float(np.median([call() for _ in range(reps)]))

    def record(name, ms, nbytes=None):
        out["us_" + name] = round(ms * 1e3, 1)
        if nbytes is not None:
            out["bytes_" + name] = int(nbytes)
            out["GBps_" + name] = round(nbytes / (ms * 1e-3) / 1e9, 1)

    def trace(form, guided, bscans):
        kw = dict(half_width=k, max_step=1, smoothness=0.05, data=vol, depth=window, bscans=(0, bscans), form=form)
        if guided:
            return pipe.trace_boundary_timed(guide=guide[:bscans], band=(-16, 16), out=traced[:bscans], **kw)[1]
        return pipe.trace_boundary_timed(out=traced[:bscans], **kw)[1]

    # the guide: detect + smooth
    ms_detect = median_ms(lambda: pipe.detect_surface_timed(0.5, 3, data=vol, depth=window, out=raw_surface)[1])
    ms_smooth = median_ms(lambda: pipe.smooth_surface_timed(raw_surface, 2, out=guide)[1])
    record("detect", ms_detect)
    record("smooth_r2", ms_smooth)
    record("detect_plus_smooth", ms_detect + ms_smooth)

    for guided, H, forms, tag in ((False, window[1], (0, 3, 4), "unguided_h496"), (True, 33, (0, 1, 2, 3, 4), "guided_h33")):
        nbytes = a * b * ((H + 2 * k) * 4 + 4 + (4 if guided else 0))
        for form in forms:
            record("%s_%s" % (tag, FORM_NAMES[form]), median_ms(lambda: trace(form, guided, b)), nbytes)
        s = traced.cpu().numpy().astype(np.int64)
        out["error_max_" + tag] = int(np.abs(s - truth).max())
        one = median_ms(lambda: trace(0, guided, 1))
        record(tag + "_one_bscan", one)
        out["ns_per_step_" + tag] = round(one * 1e6 / a, 1)

    # yardstick: a device-to-device copy of the volume
    hip = C.CDLL("libamdhip64.so")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy():
        ev[0].record()
        assert hip.hipMemcpyAsync(C.c_void_p(copy_dst.data_ptr()), C.c_void_p(vol.data_ptr()), C.c_size_t(vbytes), 3, None) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    record("copy_d2d", median_ms(copy), 2 * vbytes)
    out["guided_over_copy"] = round(out["us_guided_h33_picked"] / out["us_copy_d2d"], 3)
    out["expectation_guided_faster_than_copy"] = "met" if out["guided_over_copy"] < 1.0 else "missed"
    predicted = out["us_unguided_h496_one_bscan"]  # 512 steps x the time per step
    out["unguided_over_predicted"] = round(out["us_unguided_h496_picked"] / predicted, 3)
    out["expectation_unguided_within_step_latency"] = "met" if out["unguided_over_predicted"] <= 1.25 else "missed"
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

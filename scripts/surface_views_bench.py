#!/usr/bin/env python3
"""Surface views (include/octpipe.h "surface views") at the headline shape, 1024 x 512 x 256 (131 072 A-scans of 512 depth bins, 256 MiB
of float32), on a synthetic tilted surface: noise of 0 .. 0.2 above the plane z = 100 + 0.2 a + 0.3 b, 1 .. 1.2 below it.
  * detect (threshold 0.5, run 3, window [16, 512)), smooth (radius 2), en face (16 bins from the surface on, averaging) and flatten
    (anchor 64, 512 output rows: as many bytes out as the volume has) on device memory throughout: device events around each call's
    work (octpipe_debug_*), median of --reps; bytes moved are counted from the shapes and the detected surface;
  * flatten in both forms of its loads (1: dword loads, 2: aligned 16-byte loads with a cross-lane shift), alternating;
  * yardstick of flatten: a device-to-device hipMemcpyAsync of the same number of bytes, events around it, same run;
  * yardstick of the en face slab: octpipe_change_displayed_enface_frame with 16 frames (the fixed-depth view) on a handle that has
    processed a buffer of that shape; both on the host clock around call + synchronise, same run.
Prints one JSON line and writes it to --out.

    python scripts/surface_views_bench.py [--reps 20] [--out profiles/surface_bench.json]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, v180_benchmark_params

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    n, a, b = 1024, 512, 256
    depth, first = n // 2, 16
    window = (first, depth - first)
    out = {"bench": "surface_views", "shape": [n, a, b], "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    p = v180_benchmark_params(n, a, b)
    p.enFaceViewEnabled = 1
    pipe = Pipeline(p, device=0)
    # the handle's own volume (for the fixed-depth yardstick): any buffer of the shape
    g = torch.Generator(device="cuda:0").manual_seed(1)
    d_raw = torch.randint(0, 4096, (b, a, n), dtype=torch.int16, device="cuda:0", generator=g)
    pipe.process_device(d_raw.data_ptr())
    pipe.synchronize()
    del d_raw
    # the synthetic volume
    z = (100.0 + 0.2 * torch.arange(a, device="cuda:0", dtype=torch.float32)[None, :, None]
         + 0.3 * torch.arange(b, device="cuda:0", dtype=torch.float32)[:, None, None])
    d = torch.arange(depth, device="cuda:0", dtype=torch.float32)[None, None, :]
    vol = torch.rand((b, a, depth), device="cuda:0", generator=g) * 0.2
    vol += (d >= z).to(torch.float32)
    vol = vol.contiguous()
    raw_surface = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    surface = torch.empty((b, a), dtype=torch.int32, device="cuda:0")
    image = torch.empty((b, a), dtype=torch.float32, device="cuda:0")
    flat = torch.empty((b, a, depth), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rows, vbytes = a * b, a * b * depth * 4

    def median_ms(call, reps=args.reps):
        for _ in range(3):
            call()
        return float(np.median([call() for _ in range(reps)]))

    def record(name, ms, nbytes):
        out["us_" + name] = round(ms * 1e3, 1)
        out["bytes_" + name] = int(nbytes)
        out["TBps_" + name] = round(nbytes / (ms * 1e-3) / 1e12, 3)
        out["peak_share_" + name] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)

    ms = median_ms(lambda: pipe.detect_surface_timed(0.5, 3, data=vol, depth=window, out=raw_surface)[1])
    s = raw_surface.cpu().numpy().astype(np.int64)
    out["surface_found"] = int((s >= 0).sum())
    out["surface_error_max"] = float(np.abs(s - np.ceil(z[:, :, 0].cpu().numpy())).max())
    steps = np.where(s >= 0, (s - first) // 256 + 1, -(-window[1] // 256))  # steps of 256 bins read per A-scan
    record("detect", ms, int(np.minimum(steps * 256, window[1]).sum()) * 4 + rows * 4)
    ms = median_ms(lambda: pipe.smooth_surface_timed(raw_surface, 2, out=surface)[1])
    record("smooth_r2", ms, rows * 8)
    ms = median_ms(lambda: pipe.surface_enface_timed(surface, 0, 16, "average", 0.0, data=vol, depth=window, out=image)[1])
    record("enface_t16", ms, rows * (16 * 4 + 8))
    sm = surface.cpu().numpy().astype(np.int64)
    lo, hi = np.maximum(sm - 64, first), np.minimum(sm - 64 + depth - 1, depth - 1)
    fbytes = int(np.where(sm >= 0, np.maximum(hi - lo + 1, 0), 0).sum()) * 4 + rows * depth * 4 + rows * 4
    # the two load forms alternate
    t = {1: [], 2: []}
    for rep in range(3 + args.reps):
        for loads in (1, 2):
            ms = pipe.flatten_timed(surface, 64, depth, 0.0, out=flat, data=vol, window=window, loads=loads)[1]
            if rep >= 3:
                t[loads].append(ms)
    record("flatten_dword_loads", float(np.median(t[1])), fbytes)
    record("flatten_wide_loads", float(np.median(t[2])), fbytes)
    ms_flat = median_ms(lambda: pipe.flatten_timed(surface, 64, depth, 0.0, out=flat, data=vol, window=window)[1])
    record("flatten", ms_flat, fbytes)
    # yardstick: a device-to-device copy of the volume's bytes
    hip = C.CDLL("libamdhip64.so")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy():
        ev[0].record()
        assert hip.hipMemcpyAsync(C.c_void_p(flat.data_ptr()), C.c_void_p(vol.data_ptr()), C.c_size_t(vbytes), 3, None) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    ms_copy = median_ms(copy)
    record("copy_d2d", ms_copy, 2 * vbytes)
    out["flatten_over_copy"] = round(ms_flat / ms_copy, 3)

    # yardstick: the fixed-depth en face view over 16 frames, host clock around call + synchronise for both
    def wall(call):
        t0 = time.perf_counter()
        call()
        pipe.synchronize()
        return (time.perf_counter() - t0) * 1e3

    w_fixed = median_ms(lambda: wall(lambda: pipe.change_displayed_enface_frame(200, 16, 0)))
    w_surf = median_ms(lambda: wall(lambda: pipe.surface_enface(surface, 0, 16, "average", 0.0, data=vol, depth=window, out=image)))
    out["us_wall_fixed_depth_enface_16"] = round(w_fixed * 1e3, 1)
    out["us_wall_surface_enface_16"] = round(w_surf * 1e3, 1)
    out["surface_enface_over_fixed_depth"] = round(w_surf / w_fixed, 3)
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Volume rendering (include/octpipe.h "volume rendering") on the volume view of the headline volume: 1024 x 512 x 256 synthetic fringes
through the pipeline with volumeViewEnabled (512 x 256 x 512 voxels, 64 MiB), every mode at 512 x 512 and 1024 x 1024, step length 0.01,
from three fixed view directions.  Per (mode, size, view): the shape is warmed up, then `reps` renders are enqueued back to back and the
host clock stops after the stream has drained; reps is chosen from a first timed call so that the window lasts about --window seconds.
Reported per (mode, size): milliseconds per frame (mean over the three views, and each view), the kernel time between device events of
single calls (median of 5), and samples per second from the box samples of the frame: the sum over the pixels of the trip count K of the
definition, computed here from the camera geometry -- exactly the voxel fetches of the march for X-ray, which never ends a ray early,
and for OCT Depth, which marches every ray from the far end without an early exit, and an upper limit for the other modes.  The
threshold is the 90th percentile of the voxels, so that every mode has structure to work on.  OCT Depth runs two kernels per frame:
its frame time holds both, `kernel_ms_median` is the ray cast, `prepass_kernel_ms_median` the surface pre-pass, and the record
`oct_depth_prepass` states the pre-pass on its own (kernel time, what the map looks like, the frame against alpha blending's).
Prints one JSON line and writes it to --out.

    python scripts/volume_render_bench.py [--window 1.0] [--out profiles/render_bench.json] [--quick]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("MIP", "DMIP", "X-ray", "Alpha blending", "MIDA", "Isosurface", "OCT Depth")
GOAL_MS = 1000.0 / 60.0


def quat(axis, degrees):
    n = math.sqrt(sum(a * a for a in axis))
    h = math.radians(degrees) / 2.0
    return (math.cos(h),) + tuple(math.sin(h) * a / n for a in axis)


VIEWS = {"front": quat((0.3, 1.0, 0.1), 12.0), "oblique": quat((1.0, 0.4, 0.2), 55.0), "side": quat((0.1, 1.0, 0.0), 80.0)}


def box_samples(np, s, dims):
    """sum over the pixels of K (steps 1 and 2 of the definition, float64), and the number of pixels that hit the box"""
    V = np.array(s.viewMatrix, dtype=np.float64).reshape(4, 4)
    R, t = V[:3, :3], V[:3, 3]
    o = -np.linalg.solve(R, t)
    f = 1.0 / math.tan(math.radians(s.fovDegrees) / 2.0)
    w, h = s.width, s.height
    cx = (2.0 * (np.arange(w) + 0.5) / w - 1.0) * (w / h)
    cy = 2.0 * (np.arange(h) + 0.5) / h - 1.0
    cx, cy = np.meshgrid(cx, cy)
    d = [cx * R[0, j] + cy * R[1, j] - f * R[2, j] for j in range(3)]
    e = np.array(dims, dtype=np.float64) * np.array(s.stretch, dtype=np.float64)
    top = e / e.max() / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, hi = [], []
        for i in range(3):
            a, b = (top[i] - o[i]) / d[i], (-top[i] - o[i]) / d[i]
            lo.append(np.fmin(a, b))
            hi.append(np.fmax(a, b))
        t0 = np.fmax(0.0, np.fmax(np.fmax(lo[0], lo[1]), lo[2]))
        t1 = np.fmin(np.fmin(hi[0], hi[1]), hi[2])
    hit = t1 > t0
    L = np.sqrt(sum(((t1 - t0) * d[i] / (2.0 * top[i])) ** 2 for i in range(3)))
    K = np.where(hit, np.minimum(np.ceil(L / s.stepLength), 1733), 0)
    return int(K.sum()), int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of rendering per (mode, size, view)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    ap.add_argument("--quick", action="store_true", help="two renders per shape and no timed window (for a profiler run)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from octproz_amd import Pipeline, synthetic_raw, v180_benchmark_params

    n, a, b = 1024, 512, 256
    p = v180_benchmark_params(n, a, b)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0  # the window that puts the synthetic image inside 0 .. 1
    p.volumeViewEnabled = 1
    pipe = Pipeline(p, device=0)
    d_raw = torch.from_numpy(synthetic_raw(n, a, b, seed=1).view(np.int16)).to("cuda:0")
    pipe.process_device(d_raw.data_ptr())
    pipe.synchronize()
    ptr, nbytes = pipe.volume_view_buffer()
    dims = (a, b, n // 2)
    vox = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(vox.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3) == 0
    q = torch.quantile(vox[:: 997].float(), torch.tensor([0.5, 0.9, 0.99], device="cuda:0")).cpu().numpy() / 255.0
    threshold = float(min(max(q[1], 0.02), 0.95))
    lut = np.stack([np.linspace(0, 255, 256), np.linspace(0, 255, 256) ** 2 / 255, 255 - np.linspace(0, 255, 256), np.full(256, 255)], axis=1)
    pipe.set_render_lut(lut.astype(np.uint8))

    out = {"bench": "volume_render", "volume": [n, a, b], "voxels": list(dims), "step_length": 0.01, "threshold": round(threshold, 4),
           "voxel_quantiles_50_90_99": [round(float(x), 4) for x in q], "window_s": args.window, "goal_ms": round(GOAL_MS, 2), "modes": {}}
    for mode in MODES:
        rec = {}
        for size in (512, 1024):
            per_view, kernel_ms, prepass_ms, samples, hits = {}, [], [], [], []
            depth = mode == "OCT Depth"

            def timed(s):
                """(pre-pass ms or None, ray cast ms) of one timed call"""
                ms = pipe.render_volume_device(s, timed=True)[2]
                return ms if depth else (None, ms)
            for name, rot in VIEWS.items():
                s = pipe.render_settings(mode, (size, size), rotation=rot, threshold=threshold, step_length=0.01, shading=1, lut=0,
                                         smooth_factor=1, output="u8")
                for _ in range(2):  # warm-up of this shape
                    pre, ms = timed(s)
                k, hitn = box_samples(np, s, dims)
                samples.append(k)
                hits.append(hitn)
                if args.quick:
                    per_view[name] = round(ms, 4)
                    kernel_ms.append(ms)
                    prepass_ms.append(pre)
                    continue
                five = [timed(s) for _ in range(5)]
                kernel_ms.append(float(np.median([m for _, m in five])))
                prepass_ms.append(float(np.median([m for m, _ in five])) if depth else None)
                reps = int(min(5000, max(5, args.window / max((ms + (pre or 0.0)) * 1e-3, 1e-5))))
                pipe.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    pipe.render_volume_device(s)
                pipe.synchronize()
                per_view[name] = round((time.perf_counter() - t0) / reps * 1e3, 4)
            mean_ms = float(np.mean(list(per_view.values())))
            rec[str(size)] = {"ms_per_frame": round(mean_ms, 4), "ms_per_view": per_view, "kernel_ms_median": round(float(np.mean(kernel_ms)), 4),
                              "box_samples_per_frame": int(np.mean(samples)), "hit_pixels": int(np.mean(hits)),
                              "Gsamples_per_s": round(float(np.mean(samples)) / (mean_ms * 1e-3) / 1e9, 2),
                              "meets_60_fps": bool(max(per_view.values()) < GOAL_MS)}
            if depth:
                rec[str(size)]["prepass_kernel_ms_median"] = round(float(np.mean(prepass_ms)), 4)
        out["modes"][mode] = rec
    # the pre-pass on its own line: its kernel time (it does not depend on the view or the viewport), the map it produces, and the
    # frame beside alpha blending's, the closest existing mode (OCT Depth does one more fetch per sample and has no early exit)
    smap = pipe.surface_map(1.5 * threshold)
    depth_rec, alpha_rec = out["modes"]["OCT Depth"], out["modes"]["Alpha blending"]
    out["oct_depth_prepass"] = {
        "depth_threshold": round(1.5 * threshold, 4), "map_bytes": int(smap.nbytes), "float_depth_volume_bytes": int(4 * dims[0] * dims[1] * dims[2]),
        "kernel_ms": {size: depth_rec[size]["prepass_kernel_ms_median"] for size in depth_rec},
        "columns_with_a_surface": round(float((smap > 0).mean()), 4), "mean_surface_index": round(float(smap.mean()), 1),
        "frame_ms_over_alpha_blending": {size: round(depth_rec[size]["ms_per_frame"] / alpha_rec[size]["ms_per_frame"], 2) for size in depth_rec}}
    pipe.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

"""The voxel scenes, views, viewports and settings that the volume rendering tests share (tests/test_volume_render.py proves on the
model alone that the excused pixels stay under the cap for exactly the cases tests/test_gpu_volume_render.py runs on the device)."""
import math

import numpy as np

import render_model as rm

# Bounds below which a pixel's closest decision counts as fragile (render_model.fragile).  Reasoning, not a fit to any result: a sample
# position carries the rounding of o + d t (|o| about 1.7, float32 epsilon 6e-8, a few operations: up to about 5e-7 in box units).  The
# scenes here have at most 64 voxels along an axis and at most one full intensity step per voxel, so the intensity changes by at most 64
# per box unit and a sample's intensity is off by at most about 5e-7 x 64 = 3e-5; the blend itself adds a few 1e-7.  kmargin is in
# samples: L / stepLength is around 100 with a relative error of a few epsilon, 1e-4 is several times that.  tmargin is in units of t
# (t around 1.5, error a few 1e-7).
MARGIN_BOUND = 3e-5
K_BOUND = 1e-4
T_BOUND = 1e-5
FRAGILE_CAP = 0.02  # of the pixels that hit the box, per image

# The model's float32 run against its float64 run over every case of cases(), worst colour difference on non-fragile pixels, as
# test_volume_render.py::test_cap_on_excused_pixels_on_the_model_alone prints it: 1.46e-4 (isosurface on the phantom and the blobs: the
# specular term pow(N.H, 600) amplifies the rounding of the four-tap normal; every other mode stays below 7.3e-5).  The device's bound
# is four times that -- the margin covering its pow / rsqrt / exp2 and the fused multiply-adds of its blends -- and never more than one
# code of the 8-bit image.
MODEL_F32_WORST = 1.46e-4
GPU_TOLERANCE = min(4.0 * MODEL_F32_WORST, 1.0 / 255.0)  # 5.84e-4


def blobs():
    """three smooth Gaussian blobs in a 48 x 40 x 32 (x, y, z) volume, quantised to uint8; peak below 0.99"""
    nx, ny, nz = 48, 40, 32
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    v = np.zeros((nz, ny, nx))
    for cx, cy, cz, s, a in ((0.35, 0.4, 0.5, 0.16, 0.93), (0.7, 0.6, 0.35, 0.11, 0.7), (0.55, 0.3, 0.75, 0.09, 0.55)):
        v += a * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / s ** 2)
    return np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8)


def phantom():
    """a tilted layered phantom in a 40 x 56 x 36 volume: smooth-edged layers of different brightness along a tilted axis, one of them
    saturated (255: the early termination of MIP), inside a rounded envelope"""
    nx, ny, nz = 40, 56, 36
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    t = 0.82 * z + 0.35 * x + 0.2 * y
    v = np.zeros((nz, ny, nx))
    for c, wdt, a in ((0.35, 0.05, 0.45), (0.6, 0.04, 1.05), (0.85, 0.06, 0.7), (1.05, 0.03, 0.3)):
        v += a * np.exp(-0.5 * ((t - c) / wdt) ** 2)
    env = np.exp(-(((x - 0.5) / 0.42) ** 6 + ((y - 0.5) / 0.45) ** 6))
    return np.clip(np.rint(v * env * 255.0), 0, 255).astype(np.uint8)


def sphere(n=48, radius=0.3, edge=0.08):
    """a soft-edged ball in an n^3 volume (the isosurface test's scene): intensity 0.5 at `radius` from the centre (box units)"""
    c = (np.arange(n) + 0.5) / n - 0.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    return np.clip(np.rint(255.0 * 0.5 * (1.0 - np.tanh((r - radius) / edge))), 0, 255).astype(np.uint8)


def pipeline_params():
    """acquisition of the pipeline-produced scene: 128 samples per line (64 depth bins), 24 A-scans, 10 B-scans, two buffers a volume"""
    from octproz_amd import v180_benchmark_params
    p = v180_benchmark_params(128, 24, 10, buffers_per_volume=2)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = 1
    return p


def pipeline_raws():
    from octproz_amd import synthetic_raw
    return [synthetic_raw(128, 24, 10, seed=70 + k) for k in range(2)]


def pipeline_volume_from_oracle():
    """the volume view [64][20][24] of the two synthetic buffers through the CPU oracle (cu:914-941)"""
    import common
    from common import octref
    p = pipeline_params()
    o = common.make_oracle(p)
    out = np.zeros(64 * 20 * 24, np.uint8)
    for k, raw in enumerate(pipeline_raws()):
        octref.volume_to_u8(o.process(raw), out, k, 10, 24, 20, 64)
    o.close()
    return out.reshape(64, 20, 24)


def quat(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    return (math.cos(h), *(math.sin(h) * a))


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw)


# three views: head-on from a little off the axis, an oblique one, and one from below and behind, closer to the volume
VIEWS = {
    "front": dict(q=quat((0.3, 1.0, 0.1), 12.0), x=0.0, y=0.0, dist=-500.0),
    "oblique": dict(q=quat((1.0, 0.4, 0.2), 55.0), x=0.1, y=-0.05, dist=-420.0),
    "behind": dict(q=qmul(quat((0.0, 1.0, 0.0), 160.0), quat((1.0, 0.0, 0.0), -35.0)), x=-0.08, y=0.04, dist=-650.0),
}
# two viewports: one not a multiple of the 16 x 16 tile (nor of the 8 x 8 wave tile), one wider than high
VIEWPORTS = {"odd": (37, 37), "wide": (64, 40)}

LUT = np.stack([np.clip(np.rint(255 * np.linspace(0, 1, 17) ** 0.5), 0, 255), np.clip(np.rint(255 * np.linspace(0, 1, 17) ** 2), 0, 255),
                np.clip(np.rint(255 * (1 - np.linspace(0, 1, 17))), 0, 255), np.full(17, 255)], axis=1).astype(np.uint8)

# per scene: the threshold (between the empty space and the structures) and the isosurface's smoothing
SCENE_SETTINGS = {
    "blobs": dict(threshold=0.22, smoothFactor=1),
    "phantom": dict(threshold=0.3, smoothFactor=0),
    "pipeline": dict(threshold=0.3, smoothFactor=0),
}


def settings(scene, mode, view, viewport, shading, lut, jitter, **over):
    v = VIEWS[view]
    w, h = VIEWPORTS[viewport] if isinstance(viewport, str) else viewport
    s = rm.default_settings()
    s.update(mode=mode, width=w, height=h, viewMatrix=rm.view_matrix(v["q"], v["x"], v["y"], v["dist"]), shadingEnabled=int(shading),
             lutEnabled=int(lut), jitterSeed=0x1234567 if jitter else 0, background=(0.08, 0.1, 0.15), material=(0.9, 0.8, 0.6),
             depthWeight=0.6, alphaExponent=1.7)
    s.update(SCENE_SETTINGS[scene])
    s.update(over)
    return s


def cases():
    """(scene, mode, view, viewport, shading, lut, jitter) of every image the GPU test renders.  Every mode sees every combination of
    the three switches on the blobs; the other two scenes run every mode from every view with the switches alternating."""
    out = []
    for mode in range(6):
        for vi, view in enumerate(VIEWS):
            for pi, viewport in enumerate(VIEWPORTS):
                for shading in (0, 1):
                    for lut in (0, 1):
                        for jitter in (0, 1):
                            out.append(("blobs", mode, view, viewport, shading, lut, jitter))
                for scene in ("phantom", "pipeline"):
                    k = mode + vi + pi + (scene == "pipeline")
                    out.append((scene, mode, view, viewport, k & 1, (k >> 1) & 1, (k >> 2) & 1))
    return out


def to_ctypes(s):
    """the dict as an octproz_amd._lib.RenderSettings"""
    from octproz_amd import _lib
    c = _lib.RenderSettings()
    for name, _ in _lib.RenderSettings._fields_:
        v = s[name]
        if name in ("viewMatrix", "stretch", "background", "material", "lightPosition"):
            for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                getattr(c, name)[i] = float(x)
        else:
            setattr(c, name, v)
    return c

"""The scenes, views and settings that the OCT Depth tests share (tests/test_depth_render.py proves on the model alone that the excused
pixels stay under render_scenes.FRAGILE_CAP for exactly the cases tests/test_gpu_depth_render.py renders on the device).  Bounds,
viewports, views, colour table and the phantom are render_scenes'; the tilted slab is this file's."""
import itertools

import numpy as np

import depth_render_model as dm
import render_model as rm
import render_scenes as sc

# The model's float32 run against its float64 run over every case of cases(), worst colour difference on non-fragile pixels, as
# test_depth_render.py::test_cap_on_excused_pixels_on_the_model_alone prints it: 1.05e-4 (phantom from behind, shaded with the colour
# table: the specular term pow(N.H, 600) inside the loop amplifies the rounding of the four-tap normal; largest fragile share 1.45 %).
# The device's bound is four times that -- the margin render_scenes.py argues for the device's pow / rsqrt / exp2 and fused
# multiply-adds -- and never more than one code of the 8-bit image.
MODEL_F32_WORST = 1.05e-4
GPU_TOLERANCE = min(4.0 * MODEL_F32_WORST, 1.0 / 255.0)  # 4.2e-4

# Views and step length.  The compare dd < 1.01 stepLength sits 0.01 stepLength from flipping wherever a ray runs along z through a
# stretch of constant surface index, and D's lateral steps (the map is an integer per column) put dd anywhere around that bound: the
# shorter the step, the more samples a ray has and the narrower the range of dd that the fixed render_scenes.MARGIN_BOUND is compared
# with.  Over render_scenes' three views and step lengths 0.01 ... 0.05 the model's largest fragile share falls from 8 % (0.01, head-on)
# to under 1.5 % at 0.03 for the two views that are not head-on; those are the cases here.
VIEWS = ("oblique", "behind")
STEP_LENGTH = 0.03


def tilted_slab():
    """a scattering sample under a tilted, slightly curved surface in a 44 x 36 x 48 (x, y, z) volume: air (0) above the surface (larger
    z), a bright surface layer, then an intensity that decays with depth and carries a fixed speckle-like texture, so that the march
    meets intensities on both sides of the render threshold and of 0.9"""
    nx, ny, nz = 44, 36, 48
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    surf = 33.0 - 0.22 * x + 0.13 * y + 3.0 * np.sin(x / 9.0) * np.cos(y / 7.0)
    below = surf - z
    rng = np.random.default_rng(5)
    texture = 0.85 + 0.15 * rng.random((nz, ny, nx))
    v = np.where(below >= 0, (0.25 + 0.72 * np.exp(-below / 9.0)) * texture, 0.0)
    return np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8)


SCENE_SETTINGS = {
    "phantom": dict(threshold=0.3),
    "slab": dict(threshold=0.35),
}


def scenes():
    return {"phantom": sc.phantom(), "slab": tilted_slab()}


def settings(scene, view, viewport, shading, lut, jitter, **over):
    s = sc.settings("phantom", dm.OCT_DEPTH, view, viewport, shading, lut, jitter, stepLength=STEP_LENGTH)
    s.update(SCENE_SETTINGS[scene])
    s.update(over)
    return s


def cases():
    """(scene, view, viewport, shading, lut, jitter) of every image the GPU test renders: both scenes x {shading, LUT, jitter} x two
    views x both viewports"""
    return [(scene, view, viewport, sh, lu, ji) for scene in ("phantom", "slab") for sh, lu, ji in itertools.product((0, 1), repeat=3)
            for view in VIEWS for viewport in sc.VIEWPORTS]

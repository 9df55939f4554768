"""The OCT Depth render mode and the surface map without a device (include/octpipe.h "volume rendering", step 4 "OCT Depth"): the ABI
surface and the status codes of calls that need no device, the numpy model (tests/depth_render_model.py) against first principles on
scenes with known answers, and the cap on excused pixels shown on the model alone for every case tests/test_gpu_depth_render.py runs."""
import ctypes as C
import math
import os
import re

import numpy as np

import depth_render_model as dm
import depth_render_scenes as ds
import render_model as rm
import render_scenes as sc
from octproz_amd import _lib, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = 1


# ---------------------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    modes = open(os.path.join(ROOT, "include", "octpipe_render_modes.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in ("octpipe_render_oct_depth", "octpipe_volume_surface_map"):
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name), name
    assert re.search(r"\boctpipe_debug_render_oct_depth\s*\(", dbg) and "octpipe_debug_render_oct_depth" in _lib.OCTPIPE_DEBUG_SYMBOLS
    assert hasattr(L, "octpipe_debug_render_oct_depth")
    assert '#include "octpipe_render_modes.h"' in pub and re.search(r"OCTPIPE_RENDER_OCT_DEPTH = 6\b", modes)
    assert _lib.RENDER_OCT_DEPTH == 6 == dm.OCT_DEPTH
    assert pipeline.render_mode_code("OCT Depth") == 6 == pipeline.render_mode_code("oct_depth")
    assert "not offered" not in pub
    # the struct is the one octpipe_render_volume takes: 168 bytes
    assert "42 x 4 = 168 bytes" in pub and C.sizeof(_lib.RenderSettings) == 168


def _settings(**over):
    s = _lib.RenderSettings()
    _lib.lib().octpipe_default_render_settings(C.byref(s))
    for k, v in over.items():
        setattr(s, k, v)
    return s


def test_status_codes_without_a_device():
    L = _lib.lib()
    vox = np.zeros(8, np.uint8)
    dims = (C.c_uint32 * 3)(2, 2, 2)
    img, n, pre, ms = C.c_void_p(), C.c_size_t(), C.c_double(), C.c_double()
    good = _settings(mode=6)

    def depth(s, dm_=dims):
        return L.octpipe_render_oct_depth(None, vox.ctypes.data, 0, dm_, C.byref(s) if s is not None else None, C.byref(img), C.byref(n))

    assert depth(good) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    assert L.octpipe_debug_render_oct_depth(None, vox.ctypes.data, 0, dims, C.byref(good), C.byref(img), C.byref(n), C.byref(pre),
                                            C.byref(ms)) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    for mode in (0, 3, 5, 7):
        assert depth(_settings(mode=mode)) == ERR_INVALID_ARGUMENT and b"mode" in L.octpipe_last_error(), mode
    assert depth(None) == ERR_INVALID_ARGUMENT and b"settings" in L.octpipe_last_error()
    # the other fields keep the ranges of octpipe_render_volume
    for s, field in ((_settings(mode=6, width=0), b"width"), (_settings(mode=6, stepLength=0.0005), b"stepLength"),
                     (_settings(mode=6, threshold=1.5), b"threshold"), (_settings(mode=6, threshold=float("nan")), b"threshold"),
                     (_settings(mode=6, alphaExponent=0.05), b"alphaExponent"), (_settings(mode=6, outputFormat=2), b"outputFormat")):
        assert depth(s) == ERR_INVALID_ARGUMENT and field in L.octpipe_last_error(), field
    assert depth(good, None) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()
    assert depth(good, (C.c_uint32 * 3)(2, 2, 4097)) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()
    # octpipe_render_volume still refuses the mode
    assert L.octpipe_render_volume(None, vox.ctypes.data, 0, dims, C.byref(good), C.byref(img), C.byref(n)) == ERR_INVALID_ARGUMENT
    assert b"mode" in L.octpipe_last_error()

    out = np.zeros(4, np.uint16)

    def surface(T, voxels=vox.ctypes.data, dm_=dims, dst=out.ctypes.data):
        return L.octpipe_volume_surface_map(None, voxels, 0, dm_, C.c_float(T), dst)

    for T in (-0.1, 1.6, float("nan"), float("inf")):
        assert surface(T) == ERR_INVALID_ARGUMENT and b"depthThreshold" in L.octpipe_last_error(), T
    for T in (0.0, 0.75, 1.5):  # inside the range: what remains is the missing handle
        assert surface(T) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error(), T
    assert surface(0.75, dst=None) == ERR_INVALID_ARGUMENT and b"map" in L.octpipe_last_error()
    assert surface(0.75, dm_=None) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()
    assert surface(0.75, dm_=(C.c_uint32 * 3)(0, 2, 2)) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()


# ---------------------------------------------------------------------------------------------------------------------- the model
def test_surface_map_against_a_plain_loop():
    rng = np.random.default_rng(21)
    for (nx, ny, nz), T in (((5, 4, 40), 0.75), ((3, 2, 31), 0.6), ((2, 2, 33), 0.0), ((4, 3, 64), 0.9), ((2, 1, 1), 0.0), ((3, 3, 40), 1.5)):
        vox = rng.integers(0, 256, size=(nz, ny, nx), dtype=np.uint8)
        vox[:, 0, 0] = 153  # 153 / 255 == 0.6 in float32: no hit at T = 0.6
        start = int(np.float32(nz) - np.float32(nz) / np.float32(32.0))
        want = np.zeros((ny, nx), np.uint16)
        for y in range(ny):
            for x in range(nx):
                for i in range(start, 0, -1):
                    if np.float32(vox[i, y, x]) / np.float32(255.0) > np.float32(T):
                        want[y, x] = i
                        break
        got = dm.surface_map(vox, T)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (nx, ny, nz, T)
    assert [dm.surface_start(z) for z in (1, 31, 32, 33, 40, 64, 4096)] == [0, 30, 31, 31, 38, 62, 3968]
    assert np.float32(153) / np.float32(255.0) == np.float32(0.6)


def _head_on(w=41, h=41, **over):
    s = rm.default_settings()
    s.update(mode=dm.OCT_DEPTH, width=w, height=h, threshold=0.3, background=(0.1, 0.2, 0.3), jitterSeed=0, shadingEnabled=0)
    s.update(over)
    return s


def test_empty_volume_gives_the_background():
    vox = np.zeros((12, 10, 14), np.uint8)
    for dt, tol in ((np.float64, 1e-7), (np.float32, 1e-6)):
        r = dm.render(vox, _head_on(33, 21, lutEnabled=1, jitterSeed=5, shadingEnabled=1), sc.LUT, dt)
        assert r["hit"].any() and not r["hit"].all() and not r["surface"].any()
        assert np.abs(r["image"][..., :3] - np.array([0.1, 0.2, 0.3])).max() <= tol
        assert np.all(r["image"][..., 3] == 1.0)


def test_flat_slab_surface_index_and_depth_at_voxel_centres():
    nx, ny, nz, j = 6, 5, 40, 23
    vox = np.zeros((nz, ny, nx), np.uint8)
    vox[:j + 1] = 200
    s = dm.surface_map(vox, dm.depth_threshold(0.3))
    assert s.shape == (ny, nx) and np.all(s == j)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = [(x.ravel() + 0.5) / nx, (y.ravel() + 0.5) / ny, (z.ravel() + 0.5) / nz]
    i = z.ravel()
    want = np.where((i >= 1) & (i < j), 1.0 - (j - 1 - i) / nz, 0.0)
    assert want[(i == j)].max() == 0.0 and np.all(want[i == j - 1] == 1.0) and np.allclose(want[i == j - 2], 1.0 - 1.0 / nz)
    assert np.allclose(dm.depth_fetch(s, (nx, ny, nz), p, np.float64), want, rtol=0, atol=1e-12)
    assert np.allclose(dm.depth_fetch(s, (nx, ny, nz), [c.astype(np.float32) for c in p], np.float32), want, rtol=0, atol=2e-5)
    # a surface above `start` is not seen; one at index 0 neither
    vox[:] = 200
    assert dm.surface_start(nz) == 38 and np.all(dm.surface_map(vox, 0.45) == 38)
    vox[1:] = 0
    assert not dm.surface_map(vox, 0.45).any()


def test_head_on_ray_equals_the_hand_computed_blend():
    """Z = 40, bytes 128 up to the surface at s = 38, a ray along -z through the middle, stepLength 0.22: five samples from the far end
    at z = 0, 0.22, 0.44, 0.66, 0.88.  D(z) = 1 - (s - 1 - (40 z - 0.5)) / 40 = 0.0625 + z between the voxel centres 1 and s - 1.  Sample 0
    sits on texel 0 (D = 0: fails D > 0.1), sample 1 has dd = 0.2825 (fails dd < 1.01 x 0.22), samples 2, 3, 4 count: three blends."""
    nz, s = 40, 38
    vox = np.zeros((nz, 8, 8), np.uint8)
    vox[:s + 1] = 128
    st = _head_on(41, 41, stepLength=0.22, alphaExponent=1.7)
    r = dm.render(vox, st, None, np.float64)
    assert np.all(r["surface"] == s)
    step = float(np.float32(0.22))
    aexp, g = float(np.float32(1.7)), float(np.float32(2.2))
    C, Ca, Dold, counted = 0.0, 0.0, 1.0, []
    for k in range(5):
        zk = k * step
        D = 0.0 if k == 0 else 1.0 - (s - 1 - (nz * zk - 0.5)) / nz
        dd, Dold = abs(D - Dold), D
        if D > 0.1 and dd < float(np.float32(1.01) * np.float32(0.22)):  # (I = 128 / 255 is above 0.3 and below 0.9)
            counted.append(k)
            ca = D ** aexp
            C = (ca * D + (1 - ca) * Ca * C)
            Ca = ca + (1 - ca) * Ca
            C = C / Ca
    assert counted == [2, 3, 4]
    bg = np.array([0.1, 0.2, 0.3], np.float32).astype(np.float64)
    bgg = np.float32(bg ** g).astype(np.float64)
    want = (Ca * C + (1 - Ca) * bgg) ** float(np.float32(1.0 / g))
    assert np.allclose(r["image"][20, 20, :3], want, rtol=0, atol=1e-7), (r["image"][20, 20], want)
    # with the colour table: rgb = LUT(D - 0.05), alpha = pow(I, alphaExponent)
    r = dm.render(vox, dict(st, lutEnabled=1), sc.LUT, np.float64)
    I = 128.0 / 255.0
    C, Ca = np.zeros(3), 0.0
    for k in (2, 3, 4):
        D = 1.0 - (s - 1 - (nz * k * step - 0.5)) / nz
        c = np.array(rm.lut_fetch(sc.LUT, np.array([D - float(np.float32(0.05))]), np.float64)).ravel()
        ca = I ** aexp
        C = ca * c + (1 - ca) * Ca * C
        Ca = ca + (1 - ca) * Ca
        C = C / Ca
    want = (Ca * C + (1 - Ca) * bgg) ** float(np.float32(1.0 / g))
    assert np.allclose(r["image"][20, 20, :3], want, rtol=0, atol=1e-7), (r["image"][20, 20], want)


def test_threshold_of_two_thirds_and_more_gives_the_background():
    vox = np.full((16, 12, 12), 255, np.uint8)
    vox[::2] = 180
    for thr in (2.0 / 3.0, 0.7, 1.0):
        assert dm.depth_threshold(thr) >= 1.0
        r = dm.render(vox, _head_on(25, 25, threshold=thr), None, np.float64)
        assert not r["surface"].any()
        assert np.abs(r["image"][..., :3] - np.array([0.1, 0.2, 0.3])).max() <= 1e-7
    r = dm.render(vox, _head_on(25, 25, threshold=0.3), None, np.float64)
    assert np.abs(r["image"][12, 12, :3] - np.array([0.1, 0.2, 0.3])).max() > 0.1


# ---------------------------------------------------------------------------------------------------------------------- the cap
def test_cap_on_excused_pixels_on_the_model_alone():
    """For every case the GPU test renders: the float32 run of the model against its float64 run.  The fragile pixels
    (render_scenes.MARGIN_BOUND, K_BOUND, T_BOUND) are at most render_scenes.FRAGILE_CAP of the pixels that hit the box in every
    image, and outside them the two runs agree within the GPU test's tolerance."""
    scenes = ds.scenes()
    worst, worst_share, worst_case = 0.0, 0.0, None
    assert len(ds.cases()) == 2 * 8 * 2 * 2
    for case in ds.cases():
        st = ds.settings(*case)
        r64 = dm.render(scenes[case[0]], st, sc.LUT, np.float64)
        r32 = dm.render(scenes[case[0]], st, sc.LUT, np.float32)
        hit = int(r64["hit"].sum())
        assert hit >= 100, case
        # the mode shows something: a good part of the pixels that hit the box differ from the background
        lit = np.abs(r64["image"][..., :3] - np.asarray(st["background"])).max(axis=2) > 1e-3
        assert lit.sum() >= 0.25 * hit, case
        fr = rm.fragile(r64, sc.MARGIN_BOUND, sc.K_BOUND, sc.T_BOUND)
        share = fr.sum() / hit
        assert share <= sc.FRAGILE_CAP, (case, share)
        assert np.array_equal(r64["hit"] | fr, r32["hit"] | fr), case
        d = np.abs(r32["image"].astype(np.float64) - r64["image"])[..., :3].max(axis=2)
        diff = float(d[~fr].max())
        assert diff <= ds.GPU_TOLERANCE, (case, diff)
        if diff > worst:
            worst, worst_case = diff, case
        worst_share = max(worst_share, share)
        assert np.isfinite(r32["image"]).all() and r32["image"].min() >= 0.0 and r32["image"].max() <= 1.0
    print("OCT Depth model float32 against float64 over %d images: worst colour difference on non-fragile pixels %.3e (%s); largest "
          "fragile share %.4f; device tolerance %.3e" % (len(ds.cases()), worst, worst_case, worst_share, ds.GPU_TOLERANCE))
    # the constant beside the scenes is the measured value: within a few per cent of what this machine's libm gives
    assert worst <= 1.25 * ds.MODEL_F32_WORST
    assert ds.GPU_TOLERANCE == min(4.0 * ds.MODEL_F32_WORST, 1.0 / 255.0)


def test_scenes_are_what_they_claim():
    s = ds.scenes()
    assert s["phantom"].shape == (36, 56, 40) and np.array_equal(s["phantom"], sc.phantom())
    slab = s["slab"]
    assert slab.shape == (48, 36, 44) and max(slab.shape) <= 64
    m = dm.surface_map(slab, dm.depth_threshold(ds.SCENE_SETTINGS["slab"]["threshold"]))
    assert m.min() >= 15 and m.max() < dm.surface_start(48) and len(np.unique(m)) > 10  # tilted: the surface index varies, all inside
    below = slab[slab > 0] / 255.0
    assert (below > 0.9).any() and (below < 0.35).any()
    assert set(ds.VIEWS) <= set(sc.VIEWS) and len(ds.VIEWS) == 2
    seen = {(c[0], c[3], c[4], c[5]) for c in ds.cases()}
    assert len(seen) == 2 * 8

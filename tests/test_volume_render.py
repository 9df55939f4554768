"""Volume rendering without a device (include/octpipe.h "volume rendering"): the ABI surface, the status codes of calls that need no
device, the view matrix and the defaults against the model's restatement and closed forms, the numpy model (tests/render_model.py)
against first principles on scenes with known answers, the cap on excused pixels shown on the model alone for every case the GPU test
runs, and the register budget of the new kernels."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import render_model as rm
import render_scenes as sc
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT = 1

# measured by test_cap_on_excused_pixels_on_the_model_alone (1.46e-4) and four times that for the device (5.84e-4): render_scenes.py
MODEL_F32_WORST = sc.MODEL_F32_WORST
GPU_TOLERANCE = sc.GPU_TOLERANCE


# ---------------------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in ("octpipe_default_render_settings", "octpipe_render_view_matrix", "octpipe_update_render_lut", "octpipe_render_volume",
                 "octpipe_copy_rendered_to_host"):
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name), name
    assert re.search(r"\boctpipe_debug_render_volume\s*\(", dbg) and "octpipe_debug_render_volume" in _lib.OCTPIPE_DEBUG_SYMBOLS
    assert hasattr(L, "octpipe_debug_render_volume")
    for name, code in (("MIP", 0), ("DMIP", 1), ("XRAY", 2), ("ALPHA_BLENDING", 3), ("MIDA", 4), ("ISOSURFACE", 5)):
        assert re.search(r"OCTPIPE_RENDER_%s = %d\b" % (name, code), pub), name
        assert getattr(_lib, "RENDER_" + name) == code == getattr(rm, name)
    for name, code in (("RGBA_F32", 0), ("RGBA_U8", 1)):
        assert re.search(r"OCTPIPE_RENDER_%s = %d\b" % (name, code), pub)
        assert getattr(_lib, "RENDER_" + name) == code == getattr(rm, name)
    assert "OCTPIPE_RENDER_OCT_DEPTH" not in pub


def test_struct_layout():
    hdr = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    assert "42 x 4 = 168 bytes" in hdr and C.sizeof(_lib.RenderSettings) == 168
    body = hdr[hdr.index("typedef struct OctPipeRenderSettings"):hdr.index("} OctPipeRenderSettings;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", n.strip()) for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.RenderSettings._fields_]
    assert sorted(names) == sorted(rm.default_settings())
    assert _lib.RenderSettings.viewMatrix.offset == 12 and _lib.RenderSettings.fovDegrees.offset == 76
    assert _lib.RenderSettings.background.offset == 124 and _lib.RenderSettings.outputFormat.offset == 164


def _settings(**over):
    s = _lib.RenderSettings()
    _lib.lib().octpipe_default_render_settings(C.byref(s))
    for k, v in over.items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(s, k)[i] = x
        else:
            setattr(s, k, v)
    return s


def test_status_codes_without_a_device():
    L = _lib.lib()
    vox = np.zeros(8, np.uint8)
    dims = (C.c_uint32 * 3)(2, 2, 2)
    img, n, ms = C.c_void_p(), C.c_size_t(), C.c_double()

    def call(s, h=None, voxels=vox.ctypes.data, dm=dims):
        return L.octpipe_render_volume(h, voxels, 0, dm, C.byref(s) if s is not None else None, C.byref(img), C.byref(n))

    good = _settings()
    assert call(good) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    assert L.octpipe_debug_render_volume(None, vox.ctypes.data, 0, dims, C.byref(good), C.byref(img), C.byref(n), C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert b"null handle" in L.octpipe_last_error()
    nan = float("nan")
    singular = [0.0] * 16
    cases = [(None, b"settings"), (_settings(mode=6), b"mode"), (_settings(width=0), b"width"), (_settings(width=4097), b"width"),
             (_settings(height=0), b"height"), (_settings(height=5000), b"height"),
             (_settings(viewMatrix=[nan] + [0.0] * 15), b"viewMatrix"), (_settings(viewMatrix=singular), b"viewMatrix"),
             (_settings(fovDegrees=0.0), b"fovDegrees"), (_settings(fovDegrees=180.0), b"fovDegrees"), (_settings(fovDegrees=nan), b"fovDegrees"),
             (_settings(stretch=[1.0, 0.05, 1.0]), b"stretch"), (_settings(stretch=[1.0, 1.0, nan]), b"stretch"),
             (_settings(stepLength=0.0005), b"stepLength"), (_settings(stepLength=11.0), b"stepLength"), (_settings(stepLength=nan), b"stepLength"),
             (_settings(threshold=-0.1), b"threshold"), (_settings(threshold=nan), b"threshold"),
             (_settings(depthWeight=1.5), b"depthWeight"), (_settings(depthWeight=nan), b"depthWeight"),
             (_settings(alphaExponent=0.05), b"alphaExponent"), (_settings(alphaExponent=nan), b"alphaExponent"),
             (_settings(gamma=0.0), b"gamma"), (_settings(gamma=nan), b"gamma"),
             (_settings(smoothFactor=-1), b"smoothFactor"), (_settings(smoothFactor=4), b"smoothFactor"),
             (_settings(background=[0.0, 1.5, 0.0]), b"background"), (_settings(material=[nan, 0.0, 0.0]), b"material"),
             (_settings(lightPosition=[0.0, float("inf"), 0.0]), b"lightPosition"), (_settings(outputFormat=2), b"outputFormat")]
    for s, field in cases:
        assert call(s) == ERR_INVALID_ARGUMENT and field in L.octpipe_last_error(), (field, L.octpipe_last_error())
    assert call(good, dm=None) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()
    assert call(good, dm=(C.c_uint32 * 3)(2, 0, 2)) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()
    assert call(good, dm=(C.c_uint32 * 3)(2, 2, 5000)) == ERR_INVALID_ARGUMENT and b"dims" in L.octpipe_last_error()
    # the edges of the ranges are inside: what remains is the missing handle
    edge = _settings(width=4096, height=1, stepLength=10.0, threshold=1.0, depthWeight=0.0, alphaExponent=10.0, gamma=0.1, smoothFactor=3)
    assert call(edge) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    lut = np.zeros((4, 4), np.uint8)
    assert L.octpipe_update_render_lut(None, None, 4) == ERR_INVALID_ARGUMENT and b"rgba" in L.octpipe_last_error()
    assert L.octpipe_update_render_lut(None, lut.ctypes.data, 1) == ERR_INVALID_ARGUMENT and b"width" in L.octpipe_last_error()
    assert L.octpipe_update_render_lut(None, lut.ctypes.data, 4097) == ERR_INVALID_ARGUMENT and b"width" in L.octpipe_last_error()
    assert L.octpipe_update_render_lut(None, lut.ctypes.data, 4) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    assert L.octpipe_copy_rendered_to_host(None, None, 16) == ERR_INVALID_ARGUMENT and b"dst" in L.octpipe_last_error()
    assert L.octpipe_copy_rendered_to_host(None, lut.ctypes.data, 16) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    out = (C.c_float * 16)()
    q = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    assert L.octpipe_render_view_matrix(q, 0.0, 0.0, 0.0, out) == ERR_INVALID_ARGUMENT and b"quaternion" in L.octpipe_last_error()
    assert L.octpipe_render_view_matrix(None, 0.0, 0.0, 0.0, out) == ERR_INVALID_ARGUMENT
    q = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    assert L.octpipe_render_view_matrix(q, nan, 0.0, 0.0, out) == ERR_INVALID_ARGUMENT and b"viewX" in L.octpipe_last_error()
    assert L.octpipe_render_view_matrix(q, 0.0, 0.0, 1e9, out) == ERR_INVALID_ARGUMENT and b"distExp" in L.octpipe_last_error()
    assert L.octpipe_render_view_matrix(q, 0.0, 0.0, 0.0, None) == ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------- camera, defaults
def _view(q, x=0.0, y=0.0, dist=-500.0):
    out = (C.c_float * 16)()
    assert _lib.lib().octpipe_render_view_matrix((C.c_float * 4)(*q), x, y, dist, out) == 0
    return np.array(out, dtype=np.float32).reshape(4, 4)


def test_view_matrix_against_the_model_and_closed_forms():
    rng = np.random.default_rng(7)
    for _ in range(50):
        q = rng.standard_normal(4) * rng.uniform(0.1, 10)
        x, y, dist = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2800, 800)
        q32 = np.asarray(q, np.float32)
        got = _view(q32, x, y, dist)
        want = rm.view_matrix(q32.astype(np.float64), float(np.float32(x)), float(np.float32(y)), float(np.float32(dist)))
        assert np.array_equal(got, want)
    tz = np.float32(-4.0 * math.exp(-500.0 / 600.0))
    ident = _view((1, 0, 0, 0))
    assert np.array_equal(ident, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, tz], [0, 0, 0, 1]], np.float32))
    assert np.array_equal(_view((2, 0, 0, 0), 0.25, -0.5, 0.0)[:3, 3], np.array([0.25, -0.5, -4.0], np.float32))
    h = math.sqrt(0.5)
    # a quarter turn about x takes y to z, about y takes z to x, about z takes x to y (columns of the rotation are the images of the axes)
    for q, rot in (((h, h, 0, 0), [[1, 0, 0], [0, 0, -1], [0, 1, 0]]), ((h, 0, h, 0), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]),
                   ((h, 0, 0, h), [[0, -1, 0], [1, 0, 0], [0, 0, 1]])):
        m = _view(q)
        assert np.allclose(m[:3, :3], np.array(rot, np.float32), atol=1e-7), (q, m)
        assert np.array_equal(m[:3, 3], np.array([0, 0, tz], np.float32)) and np.array_equal(m[3], np.array([0, 0, 0, 1], np.float32))


def test_default_settings_equal_the_models():
    s = _settings()
    want = rm.default_settings()
    for name, _ in _lib.RenderSettings._fields_:
        got = getattr(s, name)
        if hasattr(got, "__len__"):
            assert np.array_equal(np.array(got, np.float32), np.asarray(want[name], np.float32).ravel()), name
        else:
            assert got == np.float32(want[name]) if isinstance(want[name], float) else got == want[name], name
    # the reference's start-up state, by value (glwindow3d.cpp:82-98, glwindow3d.h:206-236)
    assert (s.mode, s.stepLength, s.threshold, s.depthWeight, s.alphaExponent, s.smoothFactor, s.shadingEnabled, s.lutEnabled) == \
        (0, np.float32(0.01), 0.5, np.float32(0.7), 2.0, 1, 1, 0)
    assert (s.fovDegrees, s.gamma, tuple(s.lightPosition), tuple(s.material), tuple(s.background)) == \
        (50.0, np.float32(2.2), (1.0, 3.0, 3.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))


# ---------------------------------------------------------------------------------------------------------------------- the model
def _head_on(mode, w=41, h=41, **over):
    s = rm.default_settings()
    s.update(mode=mode, width=w, height=h, threshold=0.25, background=(0.1, 0.2, 0.3), jitterSeed=0)
    s.update(over)
    return s


def test_empty_volume_renders_the_background_in_every_mode():
    vox = np.zeros((12, 10, 14), np.uint8)
    for mode in range(6):
        # (the settings are float32 fields and background ^ gamma is rounded to float32 once: 1e-7 even in float64)
        for dt, tol in ((np.float64, 1e-7), (np.float32, 1e-6)):
            r = rm.render(vox, _head_on(mode, 33, 21, lutEnabled=1, jitterSeed=5), sc.LUT, dt)
            assert r["hit"].any() and not r["hit"].all()
            assert np.abs(r["image"][..., :3] - np.array([0.1, 0.2, 0.3])).max() <= tol, mode
            assert np.all(r["image"][..., 3] == 1.0)
    r = rm.render(vox, _head_on(rm.MIP, 8, 8, outputFormat=rm.RGBA_U8), None, np.float64)
    assert r["image"].dtype == np.uint8 and np.array_equal(r["image"][0, 0], [26, 51, 77, 255])  # (uint8)(c * 255 + 0.5)


def test_voxel_fetch_at_texel_centres_and_box_faces():
    rng = np.random.default_rng(11)
    vox = rng.integers(0, 256, size=(5, 6, 7), dtype=np.uint8)
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    p = [(x.ravel() + 0.5) / 7, (y.ravel() + 0.5) / 6, (z.ravel() + 0.5) / 5]
    assert np.allclose(rm.fetch(vox, p, np.float64), vox.ravel() / 255.0, rtol=0, atol=1e-12)
    assert np.allclose(rm.fetch(vox, [c.astype(np.float32) for c in p], np.float32), vox.ravel() / 255.0, rtol=0, atol=3e-5)
    # on the faces (and beyond them) the edge texels, exactly: both taps are the same texel
    for px_, xi in ((0.0, 0), (1.0, 6), (-3.0, 0), (7.5, 6)):
        q = [np.full(30, px_), (y[:, :, 0].ravel() + 0.5) / 6, (z[:, :, 0].ravel() + 0.5) / 5]
        assert np.allclose(rm.fetch(vox, q, np.float64), vox[:, :, xi].ravel() / 255.0, rtol=0, atol=1e-12)
    corner = rm.fetch(vox, [np.array([0.0, 1.0]), np.array([0.0, 1.0]), np.array([0.0, 1.0])], np.float64)
    assert np.array_equal(corner, np.array([vox[0, 0, 0], vox[4, 5, 6]]) / 255.0)
    # halfway between two texel centres: their mean
    mid = rm.fetch(vox, [np.array([2.0 / 7]), np.array([0.5 / 6]), np.array([0.5 / 5])], np.float64)
    assert np.allclose(mid, (float(vox[0, 0, 1]) + float(vox[0, 0, 2])) / 2 / 255.0, atol=1e-12)
    assert np.isfinite(rm.fetch(vox, [np.array([np.nan]), np.array([0.5]), np.array([0.5])], np.float64)).all()


def test_slab_head_on_gives_the_analytic_values_and_silhouette():
    n, v = 32, 200
    vox = np.zeros((n, n, n), np.uint8)
    vox[12:20] = v  # z = 12 .. 19: a slab facing the camera of the identity rotation
    w = 41
    focal = 1.0 / math.tan(math.radians(50.0) / 2)
    dist = 4.0 * math.exp(-500.0 / 600.0)
    c = 2.0 * (np.arange(w) + 0.5) / w - 1.0
    inside = np.abs(c) * (dist - 0.5) / focal < 0.5  # the front face, projected: diverging rays enter through it or not at all
    # the settings as the float32 fields hold them
    g, step = float(np.float32(2.2)), float(np.float32(0.01))
    bg = np.array([0.1, 0.2, 0.3], np.float32).astype(np.float64)
    bgg, inv_g = np.float32(bg ** g).astype(np.float64), float(np.float32(1.0 / g))
    # the central ray runs along -z: its samples sit at z = 1 - 0.01 k of the profile, interpolated between the texel centres
    zc = (np.arange(n) + 0.5) / n
    prof = np.interp(1.0 - step * np.arange(math.ceil(1.0 / step)), zc, vox[:, 0, 0] / 255.0)
    for mode, m in ((rm.MIP, v / 255.0), (rm.XRAY, math.sqrt(prof[prof > 0.25].mean()))):
        r = rm.render(vox, _head_on(mode, w, w), None, np.float64)
        assert np.array_equal(r["hit"], np.outer(inside, inside)), mode
        want = (m ** 2.0 * m + (1 - m ** 2.0) * bgg) ** inv_g
        assert np.allclose(r["image"][w // 2, w // 2, :3], want, rtol=0, atol=1e-7), (mode, r["image"][w // 2, w // 2], want)
        if mode == rm.MIP:  # every ray through the middle of the face crosses the plateau: one value
            mid = slice(w // 2 - 5, w // 2 + 6)
            assert np.allclose(r["image"][mid, mid, :3], want, rtol=0, atol=1e-7)
        assert np.array_equal(r["image"][~r["hit"]][:, :3], np.broadcast_to(bg, (int((~r["hit"]).sum()), 3)))
    # stretch: twice the spacing along x halves the other two extents; the silhouette follows
    r = rm.render(vox, _head_on(rm.MIP, w, w, stretch=(2.0, 1.0, 1.0)), None, np.float64)
    assert np.allclose(rm.box_top((n, n, n), (2.0, 1.0, 1.0)), [0.5, 0.25, 0.25])
    iy = np.abs(c) * (dist - 0.25) / focal < 0.25
    ix = np.abs(c) * (dist - 0.25) / focal < 0.5
    assert np.array_equal(r["hit"], np.outer(iy, ix))


def test_jitter_hash_is_the_headers():
    def one(px, py, seed):
        h = (px * 0x9E3779B1 + py * 0x85EBCA77 + seed * 0xC2B2AE3D) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
        h ^= h >> 12
        h = (h * 0x297A2D39) & 0xFFFFFFFF
        h ^= h >> 15
        return h >> 24
    px, py = np.meshgrid(np.arange(50), np.arange(40))
    got = rm.jitter(px.ravel(), py.ravel(), 0xDEADBEEF)
    assert [int(g) for g in got] == [one(int(a), int(b), 0xDEADBEEF) for a, b in zip(px.ravel(), py.ravel())]
    assert len(np.unique(got)) > 200  # spread over the byte


def test_isosurface_normals_of_a_ball():
    """the four-tap normal on the threshold surface of a soft-edged ball, quantised to uint8: within 5 degrees of the radial direction
    (the quantisation step of 1 / 255 against a gradient of about 33 codes per voxel bends it by 2 to 3 degrees at most)"""
    vox = sc.sphere()
    rng = np.random.default_rng(3)
    u = rng.standard_normal((500, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = [0.5 + 0.3 * u[:, i] for i in range(3)]
    for h in (0.001, 0.005):
        nrm = np.stack(rm.normal(vox, p, h, np.float64), axis=1)
        cosang = np.clip((nrm * u).sum(axis=1), -1, 1)
        assert np.degrees(np.arccos(cosang)).max() < 5.0, (h, np.degrees(np.arccos(cosang)).max())
    # ... and the rendered ball: lit from the light's side, the hit pixels form a disc
    s = _head_on(rm.ISOSURFACE, 61, 61, threshold=0.5, smoothFactor=1)
    r = rm.render(vox, s, None, np.float64)
    lum = r["image"][..., :3].sum(axis=2)
    ball = np.abs(lum - np.array([0.1, 0.2, 0.3], np.float32).astype(np.float64).sum()) > 1e-6
    assert 0.08 < ball.mean() < 0.14  # a disc of radius 0.3 / 1.74 x focal length = 0.37 of the half height
    yy, xx = np.nonzero(ball)
    assert abs(xx.mean() - 30) < 1.0 and abs(yy.mean() - 30) < 1.0
    assert lum[37, 32] > lum[23, 28] + 0.1  # the light sits above and a little to the right (1, 3, 3); row 0 is the bottom


# ---------------------------------------------------------------------------------------------------------------------- the cap
def _scenes():
    return {"blobs": sc.blobs(), "phantom": sc.phantom(), "pipeline": sc.pipeline_volume_from_oracle()}


def test_cap_on_excused_pixels_on_the_model_alone():
    """For every scene, mode, view, viewport and switch combination the GPU test renders: the float32 run of the model against its
    float64 run.  The fragile pixels (render_scenes.MARGIN_BOUND, K_BOUND, T_BOUND) are at most 2 % of the pixels that hit the box in
    every image, and outside them the two runs agree within the GPU test's tolerance.  (The pipeline-produced scene comes from the
    CPU oracle here; the GPU test renders the device's own voxels of the same input and checks the cap on them again.)"""
    scenes = _scenes()
    worst, worst_share, worst_case = 0.0, 0.0, None
    per_mode = {}
    for case in sc.cases():
        st = sc.settings(*case)
        r64 = rm.render(scenes[case[0]], st, sc.LUT, np.float64)
        r32 = rm.render(scenes[case[0]], st, sc.LUT, np.float32)
        hit = int(r64["hit"].sum())
        assert hit >= 100, case
        fr = rm.fragile(r64, sc.MARGIN_BOUND, sc.K_BOUND, sc.T_BOUND)
        share = fr.sum() / hit
        assert share <= sc.FRAGILE_CAP, (case, share)
        assert np.array_equal(r64["hit"] | fr, r32["hit"] | fr), case
        d = np.abs(r32["image"].astype(np.float64) - r64["image"])[..., :3].max(axis=2)
        diff = float(d[~fr].max())
        assert diff <= GPU_TOLERANCE, (case, diff)
        per_mode[case[1]] = max(per_mode.get(case[1], 0.0), diff)
        if diff > worst:
            worst, worst_case = diff, case
        worst_share = max(worst_share, share)
        assert np.isfinite(r32["image"]).all() and r32["image"].min() >= 0.0 and r32["image"].max() <= 1.0
    print("model float32 against float64 over %d images: worst colour difference on non-fragile pixels %.3e (%s), per mode %s; "
          "largest fragile share %.4f; device tolerance %.3e"
          % (len(sc.cases()), worst, worst_case, {rm.MODE_NAMES[k]: "%.2e" % v for k, v in sorted(per_mode.items())}, worst_share, GPU_TOLERANCE))
    # the constant in this file is the measured value: within a few per cent of what this machine's libm gives
    assert worst <= 1.25 * MODEL_F32_WORST


def test_scenes_are_what_they_claim():
    s = _scenes()
    assert s["blobs"].shape == (32, 40, 48) and s["blobs"].max() < 0.99 * 255 and s["blobs"].min() == 0
    assert s["phantom"].shape == (36, 56, 40) and s["phantom"].max() == 255
    assert s["pipeline"].shape == (64, 20, 24) and len(np.unique(s["pipeline"])) > 50
    assert len(sc.cases()) == 6 * 3 * 2 * 10
    seen = {(c[1], c[4], c[5], c[6]) for c in sc.cases() if c[0] == "blobs"}
    assert len(seen) == 6 * 8  # every mode x shading x LUT x jitter


# ---------------------------------------------------------------------------------------------------------------------- kernels
def test_render_kernels_need_no_scratch(tmp_path):
    """every instance of oct_render_kernel: no private memory (no spills in the march loop), at most 192 VGPRs (two waves per SIMD
    at least)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "volume_render.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "volume_render_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^(_ZN3oct17oct_render_kernelILi[0-5]ELb[01]ELb[01]EEEvNS_10RenderArgsE):", text, re.M)
    assert len(names) == 15, names
    for name in names:
        meta = text[text.index(name + ":"):]
        scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
        vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
        assert scratch == 0 and vgprs <= 192, (name, scratch, vgprs)

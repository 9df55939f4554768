"""Volume rendering on the MI355X (include/octpipe.h "volume rendering", csrc/volume_render.h, csrc/pipe_render.hip).

Every image of render_scenes.cases() -- every mode x {shading, colour table, jitter} x three views x two viewports on the blobs, every
mode from every view on the layered phantom and on a pipeline-produced volume -- is held against the float64 run of the numpy model
(tests/render_model.py).  Pixels whose closest decision is within render_scenes.MARGIN_BOUND / K_BOUND / T_BOUND of flipping are
excused from the colour comparison (at most 2 % of the pixels that hit the box, per image; tests/test_volume_render.py proves that cap
on the model alone); they must still be finite and inside [0, 1].  Then: the handle's own volume against the same bytes passed in,
geometry, determinism, no side effects, stream ordering and the errors that need a device."""
import ctypes as C

import numpy as np
import pytest

import render_model as rm
import render_scenes as sc
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

# The model's own float32-against-float64 worst colour difference on non-fragile pixels over these cases is 1.46e-4 (measured by
# tests/test_volume_render.py::test_cap_on_excused_pixels_on_the_model_alone, isosurface; render_scenes.MODEL_F32_WORST).  The device's
# bound is four times that, 5.84e-4: the margin covers its pow / rsqrt / exp2 and the fused multiply-adds of its blends.  It stays below
# 1 / 255, one code of the 8-bit image.
MODEL_F32_WORST = sc.MODEL_F32_WORST
GPU_TOLERANCE = sc.GPU_TOLERANCE
assert GPU_TOLERANCE == min(4.0 * 1.46e-4, 1.0 / 255.0)


def _dev(raw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def _fetch(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


@pytest.fixture(scope="module")
def pipe():
    """a handle that has processed the pipeline scene's two buffers: its volume view is the third scene"""
    p = sc.pipeline_params()
    h = Pipeline(p, device=0)
    for raw in sc.pipeline_raws():
        d = _dev(raw)
        h.process_device(d.data_ptr())
        h.synchronize()
    h.set_render_lut(sc.LUT)
    yield h
    h.close()


@pytest.fixture(scope="module")
def scenes(pipe):
    ptr, n = pipe.volume_view_buffer()
    assert n == 64 * 20 * 24
    own = _fetch(ptr, n, np.uint8).reshape(64, 20, 24)
    assert len(np.unique(own)) > 50
    return {"blobs": sc.blobs(), "phantom": sc.phantom(), "pipeline": own}


def _render(pipe, st, voxels, fmt=rm.RGBA_F32, device=False):
    import torch
    s = sc.to_ctypes(dict(st, outputFormat=fmt))
    keep = torch.from_numpy(voxels).to("cuda:0") if (device and voxels is not None) else voxels
    pipe.render_volume_device(s, keep)
    out = pipe.rendered_host(s)
    del keep
    return out


@pytest.mark.parametrize("mode", range(6), ids=[rm.MODE_NAMES[m] for m in range(6)])
@pytest.mark.parametrize("scene", ["blobs", "phantom", "pipeline"])
def test_every_mode_against_the_float64_model(pipe, scenes, scene, mode):
    worst, worst_share, n = 0.0, 0.0, 0
    for i, case in enumerate(c for c in sc.cases() if c[0] == scene and c[1] == mode):
        st = sc.settings(*case)
        vox = scenes[scene]
        want = rm.render(vox, st, sc.LUT, np.float64)
        # the pipeline scene is the handle's own buffer; the others alternate between a host array and a device tensor
        got = _render(pipe, st, None if scene == "pipeline" else vox, device=bool(i & 1))
        assert got.shape == want["image"].shape and got.dtype == np.float32
        assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0, case
        assert np.all(got[..., 3] == 1.0)
        fr = rm.fragile(want, sc.MARGIN_BOUND, sc.K_BOUND, sc.T_BOUND)
        hit = int(want["hit"].sum())
        share = fr.sum() / hit
        d = np.abs(got.astype(np.float64) - want["image"])[..., :3].max(axis=2)
        diff = float(d[~fr].max())
        print("%s: non-fragile worst %.3e, fragile %d of %d hit pixels (%.4f), worst on fragile %.3e"
              % (case, diff, int(fr.sum()), hit, share, float(d[fr].max()) if fr.any() else 0.0))
        assert hit >= 100 and share <= sc.FRAGILE_CAP, (case, share)
        assert diff <= GPU_TOLERANCE, (case, diff, np.unravel_index(np.argmax(np.where(fr, 0, d)), d.shape))
        # pixels that miss the box hold the background, exactly
        miss = ~want["hit"] & ~fr
        assert np.array_equal(got[miss][:, :3], np.broadcast_to(np.asarray(st["background"], np.float32), (int(miss.sum()), 3)))
        # RGBA_U8: the kernel's own float image quantised by the stated formula, exactly; within one code of the quantised model
        got8 = _render(pipe, st, None if scene == "pipeline" else vox, fmt=rm.RGBA_U8, device=not (i & 1))
        assert got8.dtype == np.uint8 and np.array_equal(got8, rm.quantise(got)), case
        d8 = np.abs(got8.astype(np.int32) - rm.quantise(want["image"]).astype(np.int32)).max(axis=2)
        assert d8[~fr].max() <= 1, case
        worst, worst_share, n = max(worst, diff), max(worst_share, share), n + 1
    assert n == (48 if scene == "blobs" else 6)
    print("%s %s: %d images, worst non-fragile colour difference %.3e (bound %.3e), largest fragile share %.4f"
          % (scene, rm.MODE_NAMES[mode], n, worst, GPU_TOLERANCE, worst_share))


def test_handles_own_volume_equals_the_same_bytes_passed_in(pipe, scenes):
    own = scenes["pipeline"]
    for mode in range(6):
        st = sc.settings("pipeline", mode, "oblique", "wide", 1, 1, 1)
        a = _render(pipe, st, None)
        b = _render(pipe, st, own)
        c = _render(pipe, st, own, device=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32)), mode
        assert len(np.unique(a[..., 0])) > 10
    # the python front end: the same picture through Pipeline.render_volume, flipped for image files on request
    st = sc.settings("pipeline", rm.MIP, "front", "wide", 0, 0, 0)
    v = sc.VIEWS["front"]
    kw = dict(size=(64, 40), view_matrix=st["viewMatrix"], threshold=st["threshold"], depth_weight=0.6, alpha_exponent=1.7,
              background=st["background"], material=st["material"])
    lower = pipe.render_volume("MIP", **kw)
    # (the quaternion goes through float32 on this path: the same picture up to that rounding)
    del kw["view_matrix"]
    byq = pipe.render_volume("MIP", rotation=v["q"], distance=v["dist"], view_pos=(v["x"], v["y"]), **kw)
    assert byq.shape == lower.shape and np.mean(np.abs(byq - lower) > 1e-3) < 0.02
    kw["view_matrix"] = st["viewMatrix"]
    assert np.array_equal(lower, _render(pipe, st, None))
    assert np.array_equal(pipe.render_volume("mip", origin="upper", **kw), lower[::-1])
    u8 = pipe.render_volume(_lib.RENDER_MIP, output="u8", **kw)
    assert u8.dtype == np.uint8 and np.array_equal(u8, rm.quantise(lower))


def test_quarter_turn_about_the_view_axis_rotates_a_square_image_exactly(pipe, scenes):
    for mode in range(6):
        st = sc.settings("phantom", mode, "oblique", (64, 64), 1, 1, 0)
        V = np.array(st["viewMatrix"], np.float32).reshape(4, 4).copy()
        V[:2, 3] = 0.0  # the view position would turn with the camera
        T = V.copy()
        T[0, :3], T[1, :3] = -V[1, :3], V[0, :3]  # rotation about the camera's z axis by a quarter turn, in front of V
        a = _render(pipe, dict(st, viewMatrix=V), scenes["phantom"])
        b = _render(pipe, dict(st, viewMatrix=T), scenes["phantom"])
        assert len(np.unique(a[..., 1])) > 20
        # (cx, cy) of the turned camera sees what (cy, -cx) saw: image b is image a turned by a quarter (rows are y, row 0 at the bottom)
        assert np.array_equal(np.rot90(a, 1, axes=(0, 1)).view(np.uint32), b.view(np.uint32)) or \
            np.array_equal(np.rot90(a, -1, axes=(0, 1)).view(np.uint32), b.view(np.uint32)), mode
        assert not np.array_equal(a, b)


def _head_on(w, h, **over):
    s = rm.default_settings()
    s.update(mode=rm.MIP, width=w, height=h, threshold=0.25, background=(0.1, 0.2, 0.3))
    s.update(over)
    return s


def test_stretch_changes_the_silhouette_as_extent_says(pipe):
    vox = np.full((16, 16, 16), 255, np.uint8)
    for stretch, top in (((1.0, 1.0, 1.0), (0.5, 0.5, 0.5)), ((2.0, 1.0, 1.0), (0.5, 0.25, 0.25)), ((1.0, 3.0, 1.5), (1 / 6, 0.5, 0.25))):
        assert np.allclose(rm.box_top((16, 16, 16), stretch), top)
        st = _head_on(81, 61, stretch=stretch)
        want = rm.render(vox, st, None, np.float64)
        got = _render(pipe, st, vox)
        lit = np.abs(got[..., :3] - np.asarray(st["background"], np.float32)).max(axis=2) > 0.5
        edge = want["tmargin"] < sc.T_BOUND
        assert np.array_equal(lit | edge, want["hit"] | edge), stretch
        # head-on the silhouette is the front face: a rectangle 2 top[0] by 2 top[1] at distance d - top[2]
        ys, xs = np.nonzero(lit)
        wpx, hpx = xs.max() - xs.min() + 1, ys.max() - ys.min() + 1
        assert abs(wpx / hpx - top[0] / top[1]) <= 2.0 / hpx * top[0] / top[1] + 2.0 / hpx, (stretch, wpx, hpx)


def test_each_axis_of_a_non_cubic_volume_lands_where_the_header_says(pipe):
    """dims = (x, y, z) = (24, 12, 40): extent 0.6 x 0.3 x 1.  Seen head-on (camera on +z, x to the right, y up), a bright block at high
    x shows on the right, one at high y at the top, and the silhouette is 0.6 wide by 0.3 high."""
    nx, ny, nz = 24, 12, 40
    base = np.full((nz, ny, nx), 60, np.uint8)
    st = _head_on(192, 128, threshold=0.1)
    bg = np.asarray(st["background"], np.float32)

    def centroid(vox):
        img = _render(pipe, st, vox)
        lum = img[..., :3].sum(axis=2)
        lit = np.abs(img[..., :3] - bg).max(axis=2) > 1e-3
        ys, xs = np.nonzero(lit)
        bright = lum > 0.5 * (lum[lit].max() + lum[lit].min())
        by, bx = np.nonzero(bright & lit)
        return (xs.min(), xs.max(), ys.min(), ys.max()), (bx.mean(), by.mean())

    box, _ = centroid(base)
    w, h = box[1] - box[0] + 1, box[3] - box[2] + 1
    assert abs(w / h - 2.0) < 0.15, box
    v = base.copy(); v[:, :, 18:] = 250
    (x0, x1, y0, y1), (cx, cy) = centroid(v)
    assert cx > (x0 + x1) / 2 + 0.15 * w and abs(cy - (y0 + y1) / 2) < 1.5
    v = base.copy(); v[:, 9:, :] = 250
    (x0, x1, y0, y1), (cx, cy) = centroid(v)
    assert cy > (y0 + y1) / 2 + 0.15 * h and abs(cx - (x0 + x1) / 2) < 1.5
    # z: a block at high z is nearest to the camera; DMIP darkens with depth, so the near block is brighter than the same block far away
    near, far = base.copy(), base.copy()
    near[34:, :, :] = 250
    far[:6, :, :] = 250
    sd = dict(st, mode=rm.DMIP, depthWeight=1.0)
    a, b = _render(pipe, sd, near), _render(pipe, sd, far)
    assert a[64, 96, 1] > b[64, 96, 1] + 0.2
    # the handle's volume: (A, B x buffersPerVolume, N / 2) = (24, 20, 64) along (x, y, z), as the header says for voxels = NULL
    ptr, n = pipe.volume_view_buffer()
    own = _fetch(ptr, n, np.uint8)
    st = sc.settings("pipeline", rm.XRAY, "behind", "odd", 0, 0, 0)
    want = _render(pipe, st, None)
    assert np.array_equal(want, _render(pipe, st, own.reshape(64, 20, 24)))
    s = sc.to_ctypes(st)
    pipe.render_volume_device(s, own, dims=(24, 20, 64))
    assert np.array_equal(want, pipe.rendered_host(s))
    pipe.render_volume_device(s, own, dims=(20, 24, 64))
    assert not np.array_equal(want, pipe.rendered_host(s))


def test_two_calls_give_identical_bytes(pipe, scenes):
    for mode in range(6):
        st = sc.settings("blobs", mode, "behind", "odd", 1, 1, 1)
        a = _render(pipe, st, scenes["blobs"])
        b = _render(pipe, st, scenes["blobs"])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode


def test_rendering_leaves_the_processing_chain_untouched():
    p = v180_benchmark_params(1024, 64, 2)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = 1
    p.bscanViewEnabled = 1
    p.enFaceViewEnabled = 1
    raws = [synthetic_raw(1024, 64, 2, seed=80 + k) for k in range(2)]
    pipe = Pipeline(p, device=0)
    pipe.set_render_lut(sc.LUT)
    devs = [_dev(r) for r in raws]

    def state():
        pipe.synchronize()
        (pb, nb), (pe, ne) = pipe.display_buffers()
        vp, vn = pipe.volume_view_buffer()
        return (pipe.processed_host(), pipe.mean_line(), _fetch(pb, nb, np.float32), _fetch(pe, ne, np.float32), _fetch(vp, vn, np.uint8))

    pipe.process_device(devs[0].data_ptr())
    before = state()
    for mode in range(6):
        img = pipe.render_volume(mode, size=(48, 32), threshold=0.2, lut=mode & 1, shading=1, jitter_seed=mode)
        assert img.shape == (32, 48, 4)
        pipe.render_volume(mode, size=(48, 32), voxels=sc.blobs(), output="u8")
    for x, y in zip(before, state()):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    pipe.process_device(devs[1].data_ptr())
    after = state()
    fresh = Pipeline(p, device=0)
    fresh.process_device(devs[0].data_ptr())
    fresh.synchronize()
    fresh.process_device(devs[1].data_ptr())
    fresh.synchronize()
    assert np.array_equal(after[0].view(np.uint32), fresh.processed_host().view(np.uint32))
    assert np.array_equal(after[1].view(np.uint32), fresh.mean_line().view(np.uint32))
    vp, vn = fresh.volume_view_buffer()
    assert np.array_equal(after[4], _fetch(vp, vn, np.uint8))
    fresh.close()
    pipe.close()


def test_render_queued_behind_process_device_sees_that_buffer():
    p = v180_benchmark_params(1024, 64, 4)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = 1
    pipe = Pipeline(p, device=0)
    devs = [_dev(synthetic_raw(1024, 64, 4, seed=90 + k)) for k in range(2)]
    st = rm.default_settings()
    st.update(width=64, height=48, threshold=0.2, mode=rm.XRAY, viewMatrix=rm.view_matrix(sc.VIEWS["oblique"]["q"], 0.0, 0.0, -500.0))
    s = sc.to_ctypes(st)
    pipe.process_device(devs[0].data_ptr())
    pipe.synchronize()
    pipe.render_volume_device(s)
    first = pipe.rendered_host(s)
    # no host synchronise between the processing call and the render
    pipe.process_device(devs[1].data_ptr())
    pipe.render_volume_device(s)
    second = pipe.rendered_host(s)
    pipe.synchronize()
    vp, vn = pipe.volume_view_buffer()
    vox = _fetch(vp, vn, np.uint8).reshape(512, 4, 64)
    pipe.render_volume_device(s, vox)
    assert np.array_equal(second.view(np.uint32), pipe.rendered_host(s).view(np.uint32))
    assert not np.array_equal(first, second)
    pipe.close()


def test_errors_that_need_a_device(scenes):
    p = v180_benchmark_params(256, 16, 2)
    p.volumeViewEnabled = 0
    pipe = Pipeline(p, device=0)
    s = sc.to_ctypes(sc.settings("blobs", rm.MIP, "front", "odd", 0, 0, 0))
    with pytest.raises(OctPipeError, match="volume view"):
        pipe.render_volume_device(s)
    with pytest.raises(OctPipeError, match="nothing rendered"):
        pipe.rendered_host(s)
    s.lutEnabled = 1
    with pytest.raises(OctPipeError, match="colour table"):
        pipe.render_volume_device(s, scenes["blobs"])
    s.mode = rm.ISOSURFACE  # the isosurface never reads the table
    ptr, n = pipe.render_volume_device(s, scenes["blobs"])
    assert ptr and n == 37 * 37 * 16
    out = np.empty(10, np.float32)
    assert pipe._lib.octpipe_copy_rendered_to_host(pipe._h, out.ctypes.data, out.nbytes) == 1
    assert b"bytes" in pipe._lib.octpipe_last_error()
    ptr2, n2, ms = pipe.render_volume_device(s, scenes["blobs"], timed=True)
    assert ptr2 == ptr and n2 == n and ms > 0.0
    s.mode, s.lutEnabled = rm.MIP, 1
    pipe.set_render_lut(sc.LUT)
    pipe.render_volume_device(s, scenes["blobs"])
    assert pipe.rendered_host(s).shape == (37, 37, 4)
    with pytest.raises(ValueError):
        pipe.set_render_lut(np.zeros((4, 3), np.uint8))
    pipe.close()

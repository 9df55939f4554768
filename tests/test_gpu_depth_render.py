"""The OCT Depth render mode and the surface map on the MI355X (include/octpipe.h "volume rendering", step 4 "OCT Depth";
csrc/volume_depth.h, csrc/pipe_render.hip).

The surface map is held bit for bit against numpy (tests/depth_render_model.py) on crafted and random volumes.  Every image of
depth_render_scenes.cases() -- the layered phantom and a tilted slab x {shading, colour table, jitter} x two views x two viewports --
is held against the float64 run of the numpy model; pixels whose closest decision is within render_scenes.MARGIN_BOUND / K_BOUND /
T_BOUND of flipping are excused from the colour comparison (tests/test_depth_render.py proves the cap on their share on the model
alone) and must still be finite and inside [0, 1].  Then quantisation, determinism, stream ordering and the absence of side effects."""
import ctypes as C

import numpy as np
import pytest

import depth_render_model as dm
import depth_render_scenes as ds
import render_model as rm
import render_scenes as sc
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

# min(4 x the model's float32-against-float64 figure, 1 / 255): depth_render_scenes.py
GPU_TOLERANCE = ds.GPU_TOLERANCE
assert GPU_TOLERANCE == min(4.0 * 1.05e-4, 1.0 / 255.0)


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
    """a handle that has processed the pipeline scene's two buffers, so that it has a volume view of its own"""
    h = Pipeline(sc.pipeline_params(), device=0)
    for raw in sc.pipeline_raws():
        d = _dev(raw)
        h.process_device(d.data_ptr())
        h.synchronize()
    h.set_render_lut(sc.LUT)
    yield h
    h.close()


@pytest.fixture(scope="module")
def scenes():
    return ds.scenes()


# ---------------------------------------------------------------------------------------------------------------------- the surface map
def _crafted(nx, ny, nz, T, seed):
    """random bytes that are no hit at T everywhere, then one crafted column after another (as many as the volume has room for)"""
    rng = np.random.default_rng(seed)
    start = dm.surface_start(nz)
    no_hit = [b for b in range(256) if not (np.float32(b) / np.float32(255.0) > np.float32(T))]
    hits = [b for b in range(256) if np.float32(b) / np.float32(255.0) > np.float32(T)]
    vox = rng.choice(np.array(no_hit, np.uint8), size=(nz, ny, nx))
    if not hits:
        vox[:] = 255  # T = 1.5 (or 1): nothing is above it
        return vox
    lo, hi, edge = hits[0], hits[-1], no_hit[-1]  # the smallest hit, the largest, and the largest byte that is none (153 at T = 0.6)
    cols = []
    cols.append({})                                               # nothing above T
    cols.append({0: hi})                                          # only index 0
    cols.append({i: hi for i in range(start + 1, nz)})            # only indices above start
    cols.append({start: lo})                                      # exactly at start
    cols.append({1: lo})                                          # exactly at index 1
    cols.append({i: edge for i in range(nz)})                     # b / 255 == T (T = 0.6) or just below: no hit
    cols.append({2: hi, start - 1: lo} if start >= 4 else {1: hi, start: lo})  # two hits: the larger index wins
    cols.append({0: hi, 1: lo, start: lo, **{i: hi for i in range(start + 1, nz)}})  # everything at once
    for c, col in enumerate(cols[:nx * ny]):
        y, x = divmod(c, nx)
        for i, b in col.items():
            if 0 <= i < nz:
                vox[i, y, x] = b
    return vox


@pytest.mark.parametrize("dims", [(19, 13, 40), (1, 1, 33), (48, 40, 64), (8, 8, 31)], ids=lambda d: "%dx%dx%d" % d)
def test_surface_map_bit_for_bit(pipe, dims):
    import torch
    nx, ny, nz = dims
    rng = np.random.default_rng(nx)
    volumes = []
    for T in (0.0, 0.6, 0.75, 1.5):
        if dims == (48, 40, 64):
            volumes.append((T, rng.integers(0, 256, size=(nz, ny, nx), dtype=np.uint8)))
        elif dims == (1, 1, 33):
            # one column: each crafted column in a volume of its own
            full = _crafted(8, 1, nz, T, 3)
            volumes += [(T, np.ascontiguousarray(full[:, :, c:c + 1])) for c in range(8)]
        else:
            volumes.append((T, _crafted(nx, ny, nz, T, 5)))
    seen = set()
    for k, (T, vox) in enumerate(volumes):
        want = dm.surface_map(vox, T)
        got = pipe.surface_map(T, vox if k & 1 else torch.from_numpy(vox).to("cuda:0"))
        assert got.dtype == np.uint16 and got.shape == (ny, nx)
        assert np.array_equal(got, want), (dims, T, np.argwhere(got != want)[:5])
        again = pipe.surface_map(T, torch.from_numpy(vox).to("cuda:0") if k & 1 else vox)  # the other kind of memory
        assert np.array_equal(again, want), (dims, T)
        seen |= set(np.unique(want).tolist())
        if T == 1.5:
            assert not want.any()
    start = dm.surface_start(nz)
    assert {0, start} <= seen and max(seen) == start, (dims, sorted(seen))
    if dims != (48, 40, 64):  # the crafted columns
        assert {1, start - 1} <= seen, (dims, sorted(seen))
    if dims == (8, 8, 31):
        assert start == 30 == nz - 1


def test_surface_map_of_the_handles_own_volume(pipe):
    ptr, n = pipe.volume_view_buffer()
    own = _fetch(ptr, n, np.uint8).reshape(64, 20, 24)
    for T in (0.0, 0.3, 0.75, 1.5):
        a = pipe.surface_map(T)
        assert a.shape == (20, 24) and np.array_equal(a, dm.surface_map(own, T)), T
        assert np.array_equal(a, pipe.surface_map(T, own))
        assert np.array_equal(a, pipe.surface_map(T, ptr, dims=(24, 20, 64)))
    assert len(np.unique(pipe.surface_map(0.3))) > 1  # not one constant
    with pytest.raises(OctPipeError, match="depthThreshold"):
        pipe.surface_map(1.6)
    # the python default is the reference's T for its start-up threshold of 0.5
    assert np.array_equal(pipe.surface_map(), pipe.surface_map(float(dm.depth_threshold(0.5))))


# ---------------------------------------------------------------------------------------------------------------------- the render
def _render(pipe, st, voxels, fmt=rm.RGBA_F32, device=False):
    import torch
    s = sc.to_ctypes(dict(st, outputFormat=fmt))
    keep = torch.from_numpy(voxels).to("cuda:0") if (device and voxels is not None) else voxels
    pipe.render_volume_device(s, keep)
    out = pipe.rendered_host(s)
    del keep
    return out


@pytest.mark.parametrize("view", ds.VIEWS)
@pytest.mark.parametrize("scene", ["phantom", "slab"])
def test_against_the_float64_model(pipe, scenes, scene, view):
    worst, worst_share, n = 0.0, 0.0, 0
    for i, case in enumerate(c for c in ds.cases() if c[0] == scene and c[1] == view):
        st = ds.settings(*case)
        vox = scenes[scene]
        want = dm.render(vox, st, sc.LUT, np.float64)
        got = _render(pipe, st, vox, device=bool(i & 1))
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
        got8 = _render(pipe, st, vox, fmt=rm.RGBA_U8, device=not (i & 1))
        assert got8.dtype == np.uint8 and np.array_equal(got8, rm.quantise(got)), case
        d8 = np.abs(got8.astype(np.int32) - rm.quantise(want["image"]).astype(np.int32)).max(axis=2)
        assert d8[~fr].max() <= 1, case
        worst, worst_share, n = max(worst, diff), max(worst_share, share), n + 1
    assert n == 16
    print("%s %s: %d images, worst non-fragile colour difference %.3e (bound %.3e), largest fragile share %.4f"
          % (scene, view, n, worst, GPU_TOLERANCE, worst_share))


def test_two_calls_give_identical_bytes_and_the_front_end_routes_the_mode(pipe, scenes):
    st = ds.settings("slab", "behind", "odd", 1, 1, 1)
    a = _render(pipe, st, scenes["slab"])
    b = _render(pipe, st, scenes["slab"], device=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(np.unique(a[..., 0])) > 20
    # another mode in between does not disturb it, and the other modes do not take this one
    other = _render(pipe, dict(st, mode=rm.ALPHA_BLENDING), scenes["slab"])
    assert not np.array_equal(a, other)
    assert np.array_equal(a.view(np.uint32), _render(pipe, st, scenes["slab"]).view(np.uint32))
    s = sc.to_ctypes(st)
    img, n = C.c_void_p(), C.c_size_t()
    vox = scenes["slab"]
    dims = (C.c_uint32 * 3)(*vox.shape[::-1])
    assert pipe._lib.octpipe_render_volume(pipe._h, vox.ctypes.data, 0, dims, C.byref(s), C.byref(img), C.byref(n)) == 1
    assert b"mode" in pipe._lib.octpipe_last_error()
    s.mode = rm.ALPHA_BLENDING
    assert pipe._lib.octpipe_render_oct_depth(pipe._h, vox.ctypes.data, 0, dims, C.byref(s), C.byref(img), C.byref(n)) == 1
    assert b"mode" in pipe._lib.octpipe_last_error()
    # Pipeline.render_volume(mode="OCT Depth")
    kw = dict(size=(37, 37), view_matrix=st["viewMatrix"], voxels=vox, threshold=st["threshold"], step_length=st["stepLength"],
              alpha_exponent=st["alphaExponent"], background=st["background"], shading=1, lut=1, jitter_seed=st["jitterSeed"])
    assert np.array_equal(pipe.render_volume("OCT Depth", **kw), a)
    assert np.array_equal(pipe.render_volume(_lib.RENDER_OCT_DEPTH, origin="upper", **kw), a[::-1])
    u8 = pipe.render_volume("oct depth", output="u8", **kw)
    assert u8.dtype == np.uint8 and np.array_equal(u8, rm.quantise(a))
    # the timed twin: the same picture, both kernels' times
    s.mode = _lib.RENDER_OCT_DEPTH
    ptr, nbytes, (pre_ms, ray_ms) = pipe.render_volume_device(s, vox, timed=True)
    assert nbytes == 37 * 37 * 16 and pre_ms > 0.0 and ray_ms > 0.0
    assert np.array_equal(pipe.rendered_host(s), a)
    # the handle's own volume against the same bytes passed in
    vp, vn = pipe.volume_view_buffer()
    own = _fetch(vp, vn, np.uint8).reshape(64, 20, 24)
    st = ds.settings("phantom", "oblique", "wide", 1, 1, 1)
    mine = _render(pipe, st, None)
    assert np.array_equal(mine.view(np.uint32), _render(pipe, st, own).view(np.uint32))
    assert np.array_equal(mine.view(np.uint32), _render(pipe, st, own, device=True).view(np.uint32))


def test_errors_that_need_a_device(scenes):
    p = v180_benchmark_params(256, 16, 2)
    p.volumeViewEnabled = 0
    pipe = Pipeline(p, device=0)
    s = sc.to_ctypes(ds.settings("slab", "oblique", "odd", 0, 0, 0))
    with pytest.raises(OctPipeError, match="volume view"):
        pipe.render_volume_device(s)
    with pytest.raises(OctPipeError, match="volume view"):
        pipe.surface_map(0.5)
    s.lutEnabled = 1
    with pytest.raises(OctPipeError, match="colour table") as e:
        pipe.render_volume_device(s, scenes["slab"])
    assert e.value.code == 2  # NOT_INITIALIZED
    pipe.set_render_lut(sc.LUT)
    ptr, n = pipe.render_volume_device(s, scenes["slab"])
    assert ptr and n == 37 * 37 * 16 and pipe.rendered_host(s).shape == (37, 37, 4)
    pipe.close()


def test_render_queued_behind_process_device_sees_that_buffer():
    p = v180_benchmark_params(1024, 64, 4)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = 1
    pipe = Pipeline(p, device=0)
    devs = [_dev(synthetic_raw(1024, 64, 4, seed=90 + k)) for k in range(2)]
    st = rm.default_settings()
    st.update(width=64, height=48, threshold=0.2, mode=dm.OCT_DEPTH, stepLength=0.02, shadingEnabled=0,
              viewMatrix=rm.view_matrix(sc.VIEWS["oblique"]["q"], 0.0, 0.0, -500.0))
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
    assert len(np.unique(second[..., 0])) > 10
    assert np.array_equal(pipe.surface_map(0.3), dm.surface_map(vox, 0.3))
    pipe.close()


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
    for k in range(4):
        img = pipe.render_volume("OCT Depth", size=(48, 32), threshold=0.2, lut=k & 1, shading=k >> 1, jitter_seed=k)
        assert img.shape == (32, 48, 4)
        pipe.render_volume("OCT Depth", size=(48, 32), voxels=ds.tilted_slab(), output="u8")
        pipe.surface_map(0.3)
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

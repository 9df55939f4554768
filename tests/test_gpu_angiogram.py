"""Angiography on the MI355X (include/octpipe.h "angiography", csrc/angiogram.h, csrc/pipe_angio.hip).

Every result is compared bit for bit against the numpy model of tests/angio_model.py, floats as uint32: there is no tolerance and nothing
is excused.  Small shapes through data= on handles with N = 256 (depth 128) and one with an odd depth; the en face call against the
model's projection of the volume call's own output; then the handle's own volume through detect -> smooth -> en face on the device,
sources, ordering, side effects and errors.

The contrast of a bin depends on its M values alone, so the model's volume is worked out once per (volume, M, method) over the whole
buffer, without the mask, and every region and mask setting is cut from it (the regions start at a multiple of M)."""
import ctypes as C

import numpy as np
import pytest
import torch

import angio_model as am
import surface_model as sm
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

METHODS = ((0, "variance"), (1, "decorrelation"), (2, "difference"))
MARK = -77.0


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        i = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %s (%#x), want %s (%#x)" % (
            what, len(i), g.size, tuple(i[0]), got[tuple(i[0])], g[tuple(i[0])], want[tuple(i[0])], w[tuple(i[0])]))


def _dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def _out(shape):
    """a device result buffer filled with a marker; the fill has finished before the handle's stream writes there"""
    out = torch.full(shape, MARK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return out


def _host(pipe, tensor):
    """a device result after the handle's stream has written it (a call with a device result does not wait)"""
    pipe.synchronize()
    return tensor.cpu().numpy()


def _noisy_volume(b, a, depth, seed):
    """standard normal values sprinkled with NaN, +-inf and zeros (pairs of zeros: the decorrelation's q = 0), two bins of tiny values"""
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((b, a, depth)).astype(np.float32)
    flat = vol.reshape(-1)
    k = max(4, flat.size // 40)
    where = rng.choice(flat.size, k, replace=False)
    flat[where[0::4]] = np.nan
    flat[where[1::4]] = np.inf
    flat[where[2::4]] = -np.inf
    flat[where[3::4]] = 0.0
    vol[:, :, depth // 2] = 0.0  # every repeat zero in one bin of every A-scan
    vol[0::2, :, depth // 2 + 1] = -0.0
    vol[1::2, :, depth // 2 + 2] = np.nan  # a NaN mean in every position: masked whatever the threshold
    # results in the float32 denormal range, where (float)c and (float)mu depend on the device keeping denormals: values near 1e-20
    # (their variance near 1e-40), and denormal values themselves (mean and difference denormal)
    vol[:, :, 3] = (rng.standard_normal((b, a)) * 1e-20).astype(np.float32)
    vol[:, :, 4] = (rng.standard_normal((b, a)) * 1e-41).astype(np.float32)
    return vol


def _holey_surface(rng, shape, lo, hi, holes=0.25):
    s = rng.integers(lo, hi, shape).astype(np.int32)
    s[rng.random(shape) < holes] = -1 - rng.integers(0, 5)
    return s


def _kw(region):
    b0, bn, a0, an, s0, sn = region
    return dict(bscans=(b0, bn), ascans=(a0, an), depth=(s0, sn))


def _odd_depth_handle(a, b):
    """N = 250 (depth 125: rows alternate in alignment) if the handle accepts it, else the smallest accepted N with an odd N / 2"""
    for n in [250] + list(range(6, 250, 4)):
        try:
            return Pipeline(v180_benchmark_params(n, a, b), device=0), n
        except OctPipeError:
            continue
    raise AssertionError("no samplesPerLine with an odd N / 2 is accepted")


# (N, A, B): the (M, (firstBscan, bscanCount)) of the handle -- bscanCount = M, 3 M and 16 all occur, every firstBscan a multiple of M
SHAPES = [
    (256, 1, 16, ((2, (0, 16)), (4, (0, 16)), (4, (4, 12)), (8, (0, 16)), (8, (8, 8)), (5, (0, 15)), (5, (10, 5)), (3, (3, 9)), (3, (6, 3)),
                 (6, (0, 12)), (7, (7, 7)))),  # (every repeat count has kernels of its own)
    (256, 67, 6, ((2, (0, 6)), (3, (0, 6)), (3, (3, 3)))),
    (256, 130, 4, ((2, (0, 4)), (2, (2, 2)), (4, (0, 4)))),
    ("odd", 9, 15, ((5, (0, 15)), (5, (5, 5)), (3, (0, 15)), (3, (6, 9)))),
]


class Small:
    def __init__(self, pipe, vol, combos):
        self.pipe, self.vol, self.combos = pipe, vol, combos
        self.dvol = torch.from_numpy(vol).cuda()
        self._ref = {}

    def reference(self, M, method):
        """the model's (contrast, mean) over the whole buffer without the mask, [B // M][A][depth]: computed once, never changed"""
        key = (M, method)
        if key not in self._ref:
            b, a, depth = self.vol.shape
            out, mean = am.angiogram(self.vol, (0, b // M * M, 0, a, 0, depth), M, method)
            out.setflags(write=False)
            mean.setflags(write=False)
            self._ref[key] = (out, mean)
        return self._ref[key]

    def expected(self, region, M, method, threshold=None, masked=0.0):
        b0, bn, a0, an, s0, sn = region
        assert b0 % M == 0 and bn % M == 0
        out, mean = self.reference(M, method)
        cut = (slice(b0 // M, (b0 + bn) // M), slice(a0, a0 + an), slice(s0, s0 + sn))
        out, mean = np.ascontiguousarray(out[cut]), np.ascontiguousarray(mean[cut])
        return (out if threshold is None else am.apply_mask(out, mean, threshold, masked)), mean


@pytest.fixture(scope="module", params=SHAPES, ids=["1x16", "67x6", "130x4", "odd-depth"])
def small(request):
    n, a, b, combos = request.param
    if n == "odd":
        pipe, n = _odd_depth_handle(a, b)
        assert (n // 2) % 2 == 1
    else:
        pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    yield Small(pipe, _noisy_volume(b, a, n // 2, seed=a * 7 + b), combos)
    pipe.close()


def _windows(depth):
    """the whole depth, firstSample 1, 2, 3 with sample counts that are 1, 3 and 2 (depth 128) or 2, 0 and 3 (depth 125) past a multiple
    of four, and a window shorter than one quad"""
    return [(0, depth), (1, depth - 3), (2, depth - 5), (3, depth - 6), (0, 3)]


def _ascans(a, k):
    return (0, a) if k % 2 == 0 or a < 4 else (1 + k % 3, a - 3 - k % 2)


# ---------------------------------------------------------------------------------------------------------------------- 1. the volume call
def test_volume_small_shapes(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    k = 0
    seen = set()
    for M, (b0, bn) in small.combos:
        for method, name in METHODS:
            mean_ref = small.reference(M, method)[1]
            finite = mean_ref[np.isfinite(mean_ref)]
            contained = float(np.sort(finite)[finite.size // 2])  # a mean the data contains: bins equal to the threshold are masked
            for window in _windows(depth):
                a0, an = _ascans(a, k)
                region = (b0, bn, a0, an) + window
                for thr, masked in ((None, 0.0), (contained, -0.0), (np.inf, np.nan), (-np.inf, 5.0)):
                    k += 1
                    want, want_mean = small.expected(region, M, method, thr, masked)
                    what = (region, M, name, thr, masked)
                    j = k + k // 4  # (every pairing of mean, memory and mask setting comes up)
                    with_mean, device = bool(j & 1), bool(j & 2)
                    seen.add((with_mean, device, thr is None))
                    kw = dict(threshold=thr, masked=masked, mean=with_mean, **_kw(region))
                    if device:
                        out = _out(want.shape)
                        got = pipe.angiogram(M, name, data=dvol, out=out, **kw)
                        got = (got,) if not with_mean else got
                        assert got[0] is out
                        got = tuple(_host(pipe, t) for t in got)
                    else:
                        got = pipe.angiogram(M, name, data=vol, **kw)
                        got = (got,) if not with_mean else got
                    _same(got[0], want, ("contrast",) + what)
                    if with_mean:
                        _same(got[1], want_mean, ("mean",) + what)
    assert len(seen) == 8


def test_volume_from_the_other_memory_and_nothing_else_written(small):
    """host source -> device result and device source -> host result; results that start off a 16-byte boundary (every row has a head, the
    source takes the dword loads, the mean's alignment differs from the contrast's) between markers that stay"""
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    M, (b0, bn) = small.combos[0]
    for k, window in enumerate(_windows(depth)):
        method, name = METHODS[k % 3]
        region = (b0, bn) + _ascans(a, k + 1) + window
        want, want_mean = small.expected(region, M, method, 0.0, np.nan)
        kw = dict(threshold=0.0, masked=np.nan, mean=True, **_kw(region))
        got = pipe.angiogram(M, name, data=dvol, **kw)
        _same(got[0], want, ("device -> host", region))
        _same(got[1], want_mean, ("device -> host, mean", region))
        count = want.size
        for skew, mean_skew in ((0, 0), (1, 3), (2, 2), (3, 0)):
            pad, mpad = _out((count + 8,)), _out((count + 8,))
            out = pad[4 + skew:4 + skew + count].view(want.shape)
            mean = mpad[mean_skew:mean_skew + count].view(want.shape)
            src = vol if skew & 1 else dvol
            res = pipe.angiogram(M, name, data=src, out=out, **dict(kw, mean=mean))
            assert res[0] is out and res[1] is mean
            _same(_host(pipe, out), want, ("skewed result", region, skew))
            _same(_host(pipe, mean), want_mean, ("skewed mean", region, mean_skew))
            hp, hm = pad.cpu().numpy(), mpad.cpu().numpy()
            assert np.all(hp[:4 + skew] == MARK) and np.all(hp[4 + skew + count:] == MARK), ("written outside the result", region, skew)
            assert np.all(hm[:mean_skew] == MARK) and np.all(hm[mean_skew + count:] == MARK), ("written outside the mean", region, mean_skew)
            # without mean= the mean is not written anywhere
            pipe.angiogram(M, name, data=src, out=out, **dict(kw, mean=False))
            pipe.synchronize()


# ---------------------------------------------------------------------------------------------------------------------- 2. the en face call
def test_enface_is_the_projection_of_the_volume_call(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    rng = np.random.default_rng(a + 31)
    k = 0
    for ci, (M, (b0, bn)) in enumerate(small.combos[:3]):
        for window in (((0, depth), (3, depth - 6), (1, depth - 3))[ci],):
            k += 1
            method, name = METHODS[k % 3]
            thr, masked = ((None, 0.0), (0.1, np.nan), (-0.3, -0.0))[(k // 2) % 3]
            region = (b0, bn) + _ascans(a, k) + window
            akw = dict(threshold=thr, masked=masked, **_kw(region))
            volume = pipe.angiogram(M, name, data=dvol, **akw)  # the volume call's own output ...
            _same(volume, small.expected(region, M, method, thr, masked)[0], ("volume", region, M, name))
            shape = (bn, region[3])
            surface = _holey_surface(rng, shape, 0, depth)
            dsurf = torch.from_numpy(surface).cuda()
            s0, sn = window
            # slabs inside the window, clipped at either end of it, wholly outside it at either end; 63 / 64 / 65 and 130 bins: one lane
            # short of a wave, a full wave, one and two bins per lane; the whole window
            slabs = ((0, 1), (-2, 16), (1, 63), (-40, 64), (-30, 65), (-depth, 130), (-64, 130), (-depth, 2 * depth + 1), (depth + 5, 3),
                     (-depth - 200, 64), (5, 4096))
            for i, (offset, thickness) in enumerate(slabs):
                for fn, fname in ((0, "average"), (1, "mip")):
                    fill = np.nan if (i + fn) & 1 else -1.5
                    ekw = dict(offset=offset, thickness=thickness, function=fname, fill=fill, **akw)
                    for given, model_surface in ((surface, surface), (dsurf, surface), (None, None)):
                        if given is None and i % 3:
                            continue
                        # ... projected by the model
                        want = am.project_volume(volume, region, M, model_surface, offset, thickness, fn, fill)
                        what = (region, M, name, thr, offset, thickness, fname, "no surface" if given is None else type(given).__name__)
                        if given is dsurf:
                            out = _out(want.shape)
                            assert pipe.angiogram_enface(M, name, surface=given, data=dvol, out=out, **ekw) is out
                            _same(_host(pipe, out), want, ("en face device",) + what)
                            # both forms of the kernel: one wave per A-scan, and teams of 16 lanes up to 64 bins
                            for form in (1, 2) if thickness <= 64 else (1,):
                                out = _out(want.shape)
                                got, ms = pipe.angiogram_enface_timed(M, name, surface=given, data=dvol, out=out, form=form, **ekw)
                                assert got is out and ms > 0.0
                                _same(_host(pipe, out), want, ("en face device, form %d" % form,) + what)
                        else:
                            _same(pipe.angiogram_enface(M, name, surface=given, data=vol, **ekw), want, ("en face host",) + what)
            # the fixed slab is the slab under a constant surface at firstSample
            const = np.full(shape, s0, np.int32)
            for fn in ("average", "mip"):
                ekw = dict(offset=7, thickness=70, function=fn, fill=0.0, data=dvol, **akw)
                _same(pipe.angiogram_enface(M, name, **ekw), pipe.angiogram_enface(M, name, surface=const, **ekw), ("fixed slab", region, fn))
                ekw["thickness"] = 40
                want = pipe.angiogram_enface(M, name, surface=const, **ekw)
                for form in (1, 2):
                    _same(pipe.angiogram_enface_timed(M, name, form=form, **ekw)[0], want, ("fixed slab", region, fn, form))


def test_enface_model_from_the_values(small):
    """one setting straight from the values (the model's own en face function, not the projection of a volume)"""
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    M, (b0, bn) = small.combos[-1]
    region = (b0, bn, 0, min(a, 12), 2, depth - 5)
    surface = _holey_surface(np.random.default_rng(3), (bn, region[3]), 0, depth)
    for (method, name), (fn, fname) in zip(METHODS, ((0, "average"), (1, "mip"), (0, "average"))):
        want = am.angiogram_enface(vol, region, M, method, surface, -3, 20, fn, -1.0, -0.2, 0.5)
        got = pipe.angiogram_enface(M, name, -0.2, 0.5, surface, -3, 20, fname, -1.0, data=dvol, **_kw(region))
        _same(got, want, ("en face from the values", region, M, name, fname))


# ---------------------------------------------------------------------------------------------------------------------- 3. the product
def test_detect_smooth_angiogram_enface_on_the_handles_own_volume():
    n, a, b, M = 1024, 48, 8, 4
    p = v180_benchmark_params(n, a, b, buffers_per_volume=2)
    raws = [synthetic_raw(n, a, b, seed=40 + i) for i in range(3)]
    pipe = Pipeline(p, device=0)
    for i in range(2):
        pipe.octCudaPipeline(raws[i])
        pipe.synchronize()
    _, _, last = pipe.processed_device()
    window = (9, 300)
    region = (0, b, 4, 40, 9, 300)
    kw = dict(bscans=(0, b), ascans=(4, 40), depth=window)
    images = []
    for slot in (0, 1):
        host = pipe.processed_host(slot=slot).reshape(b, a, n // 2).copy()
        thr = float(np.quantile(host[:, :, 9:309], 0.98))
        floor = float(np.quantile(host[:, :, 9:309], 0.3))
        # every step on the device: nothing leaves it before the image
        d_raw = torch.empty((b, 40), dtype=torch.int32, device="cuda")
        d_surf = torch.empty((b, 40), dtype=torch.int32, device="cuda")
        d_img = _out((b // M, 40))
        pipe.detect_surface(thr, 2, buffer=slot, out=d_raw, **kw)
        pipe.smooth_surface(d_raw, 1, out=d_surf)
        assert pipe.angiogram_enface(M, "difference", floor, 0.0, d_surf, 2, 16, "average", -1.0, buffer=slot, out=d_img, **kw) is d_img
        image = _host(pipe, d_img)
        surface = sm.smooth(sm.detect(host, region, thr, 2), 1)
        _same(d_surf.cpu().numpy(), surface, ("surface", slot))
        assert (surface[::M] >= 0).any()
        want = am.angiogram_enface(host, region, M, am.DIFFERENCE, surface, 2, 16, 0, -1.0, floor, 0.0)
        _same(image, want, ("chain", slot))
        images.append(image)
        # a repeated call, the host result, the caller's copy of the volume in either memory: the same bits
        args = (M, "difference", floor, 0.0, surface, 2, 16, "average", -1.0)
        for what, got in (("repeat", pipe.angiogram_enface(*args, buffer=slot, **kw)), ("host", pipe.angiogram_enface(*args, data=host, **kw)),
                          ("device", pipe.angiogram_enface(*args, data=torch.from_numpy(host).cuda(), **kw))):
            _same(got, want, (what, slot))
        # the volume call on the slot, every method, against the model and against the caller's copy
        sub = (0, b, 4, 6, 9, 61)
        skw = dict(bscans=(0, b), ascans=(4, 6), depth=(9, 61))
        for method, name in METHODS:
            out, mean = pipe.angiogram(M, name, floor, np.nan, mean=True, buffer=slot, **skw)
            wo, wm = am.angiogram(host, sub, M, method, floor, np.nan)
            _same(out, wo, ("volume on the slot", slot, name))
            _same(mean, wm, ("mean on the slot", slot, name))
            _same(pipe.angiogram(M, name, floor, np.nan, data=host, **skw), wo, ("volume from the host copy", slot, name))
    assert not np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))  # (the two slots differ)
    # no buffer= means the slot written last
    host = pipe.processed_host(slot=last).reshape(b, a, n // 2)
    _same(pipe.angiogram(M, "variance", **skw), am.angiogram(host, sub, M, am.VARIANCE)[0], "the slot written last")
    with pytest.raises(OctPipeError):
        pipe.angiogram(M, "variance", buffer=2, **skw)
    # the chain's next processed buffer is what a handle that never made these calls computes
    pipe.octCudaPipeline(raws[2])
    pipe.synchronize()
    fresh = Pipeline(p, device=0)
    for r in raws:
        fresh.octCudaPipeline(r)
        fresh.synchronize()
    for slot in (0, 1):
        assert np.array_equal(pipe.processed_host(slot=slot).view(np.uint32), fresh.processed_host(slot=slot).view(np.uint32)), slot
    assert np.array_equal(pipe.mean_line().view(np.uint32), fresh.mean_line().view(np.uint32))
    fresh.close()
    pipe.close()


def test_a_call_behind_process_device_sees_that_buffer():
    n, a, b, M = 1024, 32, 4, 2
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    devs = [_dev(synthetic_raw(n, a, b, seed=60 + k)) for k in range(2)]
    kw = dict(ascans=(0, 8), depth=(16, 50))
    pipe.process_device(devs[0].data_ptr())
    first = pipe.angiogram(M, "variance", **kw)
    pipe.process_device(devs[1].data_ptr())
    got = pipe.angiogram(M, "variance", **kw)  # no synchronise in between
    pipe.synchronize()
    second = pipe.processed_host().reshape(b, a, n // 2)
    _same(got, am.angiogram(second, (0, b, 0, 8, 16, 50), M, am.VARIANCE)[0], "behind process_device")
    assert not np.array_equal(got.view(np.uint32), first.view(np.uint32))
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. errors
def test_argument_errors_and_callbacks():
    n, a, b = 1024, 32, 6
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=1))
    pipe.synchronize()
    L, h = _lib.lib(), pipe.handle
    outf = np.zeros(b * a * (n // 2), np.float32)
    surf = np.zeros(a * b, np.int32)
    fp, sp = C.c_void_p(outf.ctypes.data), C.c_void_p(surf.ctypes.data)
    S, E = _lib.AngioSettings, _lib.SurfaceEnfaceSettings
    ok = _lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 0, n // 2)

    def volume(reg=ok, repeats=2, method=0):
        return L.octpipe_angiogram(h, None, 0, C.byref(reg), C.byref(S(repeats, method, 0, 0.0, 0.0)), fp, None, 0)

    def enface(reg=ok, repeats=2, method=0, thickness=4, fn=0, surface=sp):
        return L.octpipe_angiogram_enface(h, None, 0, C.byref(reg), C.byref(S(repeats, method, 0, 0.0, 0.0)), surface, 0,
                                          C.byref(E(0, thickness, fn, 0.0)), fp, 0)

    def refused(rc, field):
        assert rc == 1 and field in L.octpipe_last_error(), (rc, field, L.octpipe_last_error())

    for call in (volume, enface):
        assert call() == 0 and call(repeats=3) == 0 and call(repeats=6) == 0 and call(method=2) == 0
        refused(call(repeats=4), b"repeats")  # does not divide the 6 B-scans
        refused(call(repeats=1), b"repeats")
        refused(call(repeats=9), b"repeats")
        refused(call(method=3), b"method")
        assert call(_lib.StatsRegion(0xFFFFFFFF, 2, 4, 0, a, 0, 8), repeats=4) == 0
        for reg, field in ((_lib.StatsRegion(0xFFFFFFFF, 0, 0, 0, a, 0, 8), b"bscan"), (_lib.StatsRegion(0xFFFFFFFF, 2, b, 0, a, 0, 8), b"bscan"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 2, a, 1, 0, 8), b"Ascan"), (_lib.StatsRegion(0xFFFFFFFF, 0, 2, 0, 1, n // 2, 3), b"Sample"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 2, 0, 1, 0, n // 2 + 1), b"Sample"), (_lib.StatsRegion(1, 0, 2, 0, 1, 0, 8), b"buffer")):
            refused(call(reg), field)
    assert enface(thickness=4096) == 0 and enface(fn=1) == 0 and enface(surface=None) == 0
    refused(enface(thickness=0), b"thickness")
    refused(enface(thickness=4097), b"thickness")
    refused(enface(fn=2), b"function")
    with pytest.raises(OctPipeError, match="repeats"):
        pipe.angiogram(4)
    with pytest.raises(OctPipeError, match="repeats"):
        pipe.angiogram_enface(1)
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.extend([volume(), enface()])
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=3))
    pipe.synchronize()
    assert codes and set(codes) == {7}, codes
    pipe.close()

"""Depth-resolved attenuation on the MI355X (include/octpipe.h "attenuation", csrc/attenuation.h, csrc/pipe_attenuation.hip).

Every result is compared bit for bit against the numpy model of tests/attenuation_model.py, floats as uint32, the sums as uint64: there is
no tolerance and nothing is excused.  Small shapes through data= on handles with N = 256, 1024 and 2048 (depth 128, 512, 1024: less than one
chunk of 256 bins, exactly two, and four with the carry crossing three borders) and one with an odd depth; the en face call against
Pipeline.surface_enface on the volume call's own device output; then the handle's own volume with the map the handle's parameters give,
detect -> smooth -> en face on the device, sources, ordering, side effects and errors."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import attenuation_model as at
import surface_model as sm
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

MARK = -77.0
SCALES = ((at.INTENSITY, "intensity"), (at.AMPLITUDE, "amplitude"), (at.LOG2, "log2"))
PAYLOAD_NAN = np.array(0x7FC12345, np.uint32).view(np.float32)[()]
DELTA = 0.0049


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    as_int = np.uint64 if got.dtype == np.float64 else np.uint32
    g, w = got.view(as_int), want.view(as_int)
    if not np.array_equal(g, w):
        i = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %s (%#x), want %s (%#x)" % (
            what, len(i), g.size, tuple(i[0]), got[tuple(i[0])], g[tuple(i[0])], want[tuple(i[0])], w[tuple(i[0])]))


def _fetch(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def _dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def _out(shape, dtype=torch.float32):
    """a device result buffer filled with a marker; the fill has finished before the handle's stream writes there"""
    out = torch.full(shape, MARK, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return out


def _host(pipe, tensor):
    """a device result after the handle's stream has written it (a call with a device result does not wait)"""
    pipe.synchronize()
    return tensor.cpu().numpy()


def _wide(rng, shape):
    """chi-squared (one degree of freedom) speckle times exp(U(-20, 20)): positive, over seventeen decades"""
    return (rng.standard_normal(shape) ** 2 * np.exp(rng.uniform(-20.0, 20.0, shape))).astype(np.float32)


def _mixed(rng, wide):
    """a copy sprinkled with NaN, +-inf, negatives, +-0 and float32 denormals; an all-zero A-scan; an A-scan whose only non-zero bin is the
    last"""
    vol = wide.copy()
    flat = vol.reshape(-1)
    k = max(16, flat.size // 25)
    where = rng.choice(flat.size, k, replace=False)
    for i, value in enumerate((np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0, 3e-41, -7e-42)):
        flat[where[i::8]] = np.float32(value)
    rows = vol.reshape(-1, vol.shape[2])
    rows[1 % len(rows)] = 0.0
    last = rows[2 % len(rows)]
    last[:-1] = 0.0
    last[-1] = 3.5
    return vol


def _decibel(vol):
    """the same volume as 10 log10 of its positive values (the others stay what they are)"""
    with np.errstate(all="ignore"):
        return np.where(vol > 0, 10.0 * np.log10(vol.astype(np.float64)), vol).astype(np.float32)


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


SHAPES = [(256, 1, 4), (256, 67, 3), (1024, 130, 2), (2048, 9, 2), ("odd", 9, 3)]


class Small:
    def __init__(self, pipe, seed):
        self.pipe = pipe
        b, a, depth = int(pipe.params.bscansPerBuffer), int(pipe.params.ascansPerBscan), pipe.N // 2
        rng = np.random.default_rng(seed)
        wide = _wide(rng, (b, a, depth))
        mixed = _mixed(rng, wide)
        self.vols = {"wide": wide, "mixed": mixed, "wide dB": _decibel(wide), "mixed dB": _decibel(mixed)}
        for v in self.vols.values():
            v.setflags(write=False)
        self.dvols = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.vols.items()}
        self.shape = (b, a, depth)
        self.gain = (0.5 + rng.random(depth) * 2.0).astype(np.float32)
        self.gain[depth // 3] = -1.0  # a negative entry: that bin is +0
        self.gain[depth // 2] = 0.0

    def volume(self, scale, k):
        name = ("wide", "mixed")[(k * 2654435761 >> 7) & 1] + (" dB" if scale == at.LOG2 else "")
        return name, self.vols[name], self.dvols[name]

    def regions(self):
        """(firstSample, sampleCount) windows of the issue that fit the depth, with A-scan and B-scan sub-ranges"""
        b, a, depth = self.shape
        windows = [(0, depth), (1, depth - 1), (3, 257), (2, 256), (0, 255), (5, 1), (7, 4), (6, 5)]
        if depth == 1024:
            windows.append((509, 515))
        out = []
        for k, (s0, sn) in enumerate(w for w in windows if w[0] + w[1] <= depth):
            bs = (0, b) if k % 2 == 0 or b < 2 else (1, b - 1)
            asc = (0, a) if k % 3 == 0 or a < 4 else (1 + k % 3, a - 3 - k % 2)
            out.append(bs + asc + (s0, sn))
        return out


@pytest.fixture(scope="module", params=SHAPES, ids=["1x4", "67x3", "N1024", "N2048", "odd-depth"])
def small(request):
    n, a, b = request.param
    if n == "odd":
        pipe, n = _odd_depth_handle(a, b)
        assert (n // 2) % 2 == 1
    else:
        pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    yield Small(pipe, seed=a * 7 + b)
    pipe.close()


# what a scale is tried with: (a, b) that are not round numbers for the amplitude and the log form
MAPS = {at.INTENSITY: (0.731, 1e-9), at.AMPLITUDE: (0.37, -0.011), at.LOG2: (0.33219280948873626, 0.1234567)}


def _device(k):
    """whether the k-th combination runs from device memory into device memory"""
    return bool(k & 1)


def _settings(small, scale, k, window):
    """the k-th combination of noise, tail, gain and undefined: (model keywords, call keywords, undefined).  The bits of k % 16 switch the
    device path, the gain table, the noise and the tail on and off; every fifth combination has the map a = 1, b = 0."""
    s0, sn = window
    a, b = MAPS[scale] if k % 5 else (1.0, 0.0)
    noise = (1e-3, -0.25, 2.5)[k % 3] if k & 4 else 0.0
    tail = (0.75, 1e-9, 3e5)[(k // 2) % 3] if k & 8 else 0.0
    undefined = (np.float32(np.nan), np.float32(-0.0), PAYLOAD_NAN, np.float32(-1.0))[(k // 3) % 4]
    gain_kind = ("host", "device")[(k // 16) % 2] if k & 2 else None
    gain = None if gain_kind is None else small.gain[s0:s0 + sn].copy()
    model = dict(scale=scale, a=a, b=b, noise=noise, tail=tail, gain=gain)
    given = gain if gain_kind != "device" else torch.from_numpy(gain).cuda()
    call = dict(scale=dict(SCALES)[scale], map=(a, b), noise=noise, tail=tail, gain=given)
    return model, call, undefined


# ---------------------------------------------------------------------------------------------------------------------- 1. sums and volume
def test_sums_small_shapes(small):
    """the float64 sums below every bin: where the order of the summation shows in most bins"""
    pipe = small.pipe
    k = 0
    for region in small.regions():
        for scale, sname in SCALES:
            k += 1
            vname, vol, dvol = small.volume(scale, k)
            model, call, _ = _settings(small, scale, k, region[4:])
            want = at.sums(vol, region, **model)
            what = (region, sname, vname, k)
            if _device(k):
                out = _out(want.shape, torch.float64)
                assert pipe.attenuation_sums(DELTA, data=dvol, out=out, **call, **_kw(region)) is out
                _same(_host(pipe, out), want, ("sums, device",) + what)
            else:
                _same(pipe.attenuation_sums(DELTA, data=vol, **call, **_kw(region)), want, ("sums, host",) + what)


def test_volume_small_shapes(small):
    pipe = small.pipe
    k = 0
    seen = set()
    for region in small.regions():
        for scale, sname in SCALES:
            for _ in range(4):
                k += 1
                vname, vol, dvol = small.volume(scale, k)
                model, call, undefined = _settings(small, scale, k, region[4:])
                want = at.attenuation(vol, region, DELTA, undefined=undefined, **model)
                what = (region, sname, vname, k)
                device = _device(k)
                seen.add((device, model["gain"] is None, model["noise"] != 0.0, model["tail"] != 0.0))
                if device:
                    out = _out(want.shape)
                    assert pipe.attenuation(DELTA, undefined=undefined, data=dvol, out=out, **call, **_kw(region)) is out
                    _same(_host(pipe, out), want, ("volume, device",) + what)
                else:
                    _same(pipe.attenuation(DELTA, undefined=undefined, data=vol, **call, **_kw(region)), want, ("volume, host",) + what)
    assert len(seen) == 16


def test_volume_from_the_other_memory_and_nothing_else_written(small):
    """host source -> device result and device source -> host result; results that start off a 16-byte boundary (the dword stores) between
    markers that stay; a repeated call gives the same bits"""
    pipe = small.pipe
    for k, region in enumerate(small.regions()[:5]):
        scale, sname = SCALES[k % 3]
        vname, vol, dvol = small.volume(scale, k + 1)
        model, call, undefined = _settings(small, scale, 7 * k + 1, region[4:])
        want = at.attenuation(vol, region, DELTA, undefined=undefined, **model)
        kw = dict(undefined=undefined, **call, **_kw(region))
        _same(pipe.attenuation(DELTA, data=dvol, **kw), want, ("device -> host", region))
        count = want.size
        for skew in (0, 1, 2, 3):
            pad = _out((count + 8,))
            out = pad[4 + skew:4 + skew + count].view(want.shape)
            src = vol if skew & 1 else dvol
            for again in range(2):
                assert pipe.attenuation(DELTA, data=src, out=out, **kw) is out
                _same(_host(pipe, out), want, ("skewed result", region, skew, again))
            hp = pad.cpu().numpy()
            assert np.all(hp[:4 + skew] == MARK) and np.all(hp[4 + skew + count:] == MARK), ("written outside the result", region, skew)
        pad = _out((count + 4,), torch.float64)
        out = pad[1:1 + count].view(want.shape)
        pipe.attenuation_sums(DELTA, data=dvol, out=out, **call, **_kw(region))
        _same(_host(pipe, out), at.sums(vol, region, **model), ("sums between markers", region))
        hp = pad.cpu().numpy()
        assert hp[0] == MARK and np.all(hp[1 + count:] == MARK), ("written outside the sums", region)


# ---------------------------------------------------------------------------------------------------------------------- 2. the en face call
def test_enface_is_surface_enface_of_the_volume_call(small):
    pipe = small.pipe
    b, a, depth = small.shape
    rng = np.random.default_rng(a + 31)
    regions = small.regions()
    picks = [regions[0], regions[1], regions[-1]] + ([regions[2]] if depth >= 512 else [])
    for k, region in enumerate(picks):
        scale, sname = SCALES[k % 3]
        vname, vol, dvol = small.volume(scale, k + 1)
        model, call, undefined = _settings(small, scale, 3 * k + 1, region[4:])
        b0, bn, a0, an, s0, sn = region
        akw = dict(undefined=undefined, **call, **_kw(region))
        # the volume call's own device output, put where the region lies in a buffer of the handle's shape
        out = _out((bn, an, sn))
        pipe.attenuation(DELTA, data=dvol, out=out, **akw)
        _same(_host(pipe, out), at.attenuation(vol, region, DELTA, undefined=undefined, **model), ("volume", region, sname))
        full = torch.zeros((b, a, depth), dtype=torch.float32, device="cuda")
        full[b0:b0 + bn, a0:a0 + an, s0:s0 + sn] = out
        torch.cuda.synchronize()
        surface = _holey_surface(rng, (bn, an), 0, depth)
        dsurf = torch.from_numpy(surface).cuda()
        # slabs inside the window, pushed partly and wholly out of it at either end; 1, 16, 64, 300 and 4096 bins
        slabs = ((0, 1), (-2, 16), (3, 64), (-40, 64), (-150, 300), (-depth, 4096), (5, 4096), (depth + 5, 16), (-depth - 400, 300), (-depth - 70, 64))
        for i, (offset, thickness) in enumerate(slabs):
            for fn in ("average", "mip"):
                fill = np.nan if (i + (fn == "mip")) & 1 else -1.5
                ekw = dict(offset=offset, thickness=thickness, function=fn, fill=fill)
                want = pipe.surface_enface(dsurf, data=full, **ekw, **_kw(region))
                what = (region, sname, offset, thickness, fn)
                if i % 2:
                    img = _out((bn, an))
                    assert pipe.attenuation_enface(DELTA, dsurf, data=dvol, out=img, **ekw, **akw) is img
                    _same(_host(pipe, img), want, ("en face, device surface",) + what)
                else:
                    _same(pipe.attenuation_enface(DELTA, surface, data=vol, **ekw, **akw), want, ("en face, host surface",) + what)
        # no surface is the constant surface at firstSample
        const = np.full((bn, an), s0, np.int32)
        for fn in ("average", "mip"):
            for offset, thickness in ((0, 16), (7, 70), (-3, 9), (sn - 1, 5), (sn, 5)):
                ekw = dict(offset=offset, thickness=thickness, function=fn, fill=-2.0)
                want = pipe.surface_enface(const, data=full, **ekw, **_kw(region))
                _same(pipe.attenuation_enface(DELTA, None, data=dvol, **ekw, **akw), want, ("fixed slab", region, fn, offset, thickness))
                _same(pipe.attenuation_enface(DELTA, const, data=dvol, **ekw, **akw), want, ("constant surface", region, fn, offset, thickness))


def test_enface_model_from_the_values(small):
    """one setting straight from the model (its own en face function over the model's volume, no device result involved)"""
    pipe = small.pipe
    b, a, depth = small.shape
    region = small.regions()[1]
    bn, an = region[1], region[3]
    surface = _holey_surface(np.random.default_rng(3), (bn, an), 0, depth)
    for (scale, sname), (fn, fname) in zip(SCALES, ((0, "average"), (1, "mip"), (0, "average"))):
        vname, vol, dvol = small.volume(scale, 1)
        model, call, undefined = _settings(small, scale, 4, region[4:])
        want = at.attenuation_enface(vol, region, DELTA, surface, -3, 20, fn, -1.0, undefined=undefined, **model)
        got = pipe.attenuation_enface(DELTA, surface, -3, 20, fname, -1.0, undefined=undefined, data=dvol, **call, **_kw(region))
        _same(got, want, ("en face from the values", region, sname, fname))


# ---------------------------------------------------------------------------------------------------------------------- 3. the product
@pytest.mark.parametrize("log_scaling", [1, 0], ids=["log", "linear"])
def test_the_handles_own_volume_with_its_own_map(log_scaling):
    """one synthetic buffer processed with the log scaling on and off; scale=None takes the map from the handle's parameters.  Host source =
    device source = the handle's own slot, a repeated call, and detect -> smooth -> en face with nothing leaving the device."""
    n, a, b = 1024, 48, 4
    p = v180_benchmark_params(n, a, b, buffers_per_volume=2)
    p.signalLogScaling = log_scaling
    p.signalMultiplicator, p.signalAddend = 1.25, 0.125
    if not log_scaling:
        p.signalGrayscaleMax, p.signalGrayscaleMin = 40.0, 0.5
    pipe = Pipeline(p, device=0)
    for i in range(2):
        pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=90 + i))
        pipe.synchronize()
    sname, ma, mb = pipe.intensity_map()
    lo, hi, coeff, addend = float(p.signalGrayscaleMin), float(p.signalGrayscaleMax), 1.25, 0.125
    if log_scaling:
        assert (sname, ma, mb) == ("log2", (hi - lo) * math.log2(10.0) / (10.0 * coeff), (lo - addend * (hi - lo)) * math.log2(10.0) / 10.0)
    else:
        assert (sname, ma, mb) == ("amplitude", (hi - lo) / coeff, lo - addend * (hi - lo))
    scale = dict((v, k) for k, v in SCALES)[sname]
    region = (0, b, 4, 40, 9, 300)
    kw = dict(bscans=(0, b), ascans=(4, 40), depth=(9, 300))
    images = []
    for slot in (0, 1):
        host = pipe.processed_host(slot=slot).reshape(b, a, n // 2).copy()
        want = at.attenuation(host, region, DELTA, scale, ma, mb, noise=1e-6, tail=0.0)
        assert np.isfinite(want[:, :, :-1]).all() and (want[:, :, :-1] > 0).mean() > 0.9  # (the map gives intensities, not zeros)
        dhost = torch.from_numpy(host).cuda()
        calls = (("slot", dict(buffer=slot)), ("repeat", dict(buffer=slot)), ("host", dict(data=host, scale=sname, map=(ma, mb))),
                 ("device", dict(data=dhost, scale=sname, map=(ma, mb))))
        for what, src in calls:
            _same(pipe.attenuation(DELTA, noise=1e-6, **src, **kw), want, (what, slot))
        # every step on the device: nothing leaves it before the image
        thr = float(np.quantile(host[:, :, 9:309], 0.98))
        d_raw = torch.empty((b, 40), dtype=torch.int32, device="cuda")
        d_surf = torch.empty((b, 40), dtype=torch.int32, device="cuda")
        d_img = _out((b, 40))
        pipe.detect_surface(thr, 2, buffer=slot, out=d_raw, **kw)
        pipe.smooth_surface(d_raw, 1, out=d_surf)
        assert pipe.attenuation_enface(DELTA, d_surf, 2, 16, "average", -1.0, noise=1e-6, buffer=slot, out=d_img, **kw) is d_img
        image = _host(pipe, d_img)
        surface = sm.smooth(sm.detect(host, region, thr, 2), 1)
        _same(d_surf.cpu().numpy(), surface, ("surface", slot))
        assert (surface >= 0).any()
        _same(image, at.attenuation_enface(host, region, DELTA, surface, 2, 16, 0, -1.0, scale, ma, mb, noise=1e-6), ("chain", slot))
        for what, src in calls:
            _same(pipe.attenuation_enface(DELTA, surface, 2, 16, "average", -1.0, noise=1e-6, **src, **kw), image, ("en face " + what, slot))
        images.append(image)
    assert not np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))  # (the two slots differ)
    with pytest.raises(OctPipeError):
        pipe.attenuation(DELTA, buffer=2, **kw)
    pipe.close()


def test_a_call_behind_process_device_sees_that_buffer():
    n, a, b = 1024, 32, 2
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    devs = [_dev(synthetic_raw(n, a, b, seed=60 + k)) for k in range(2)]
    kw = dict(ascans=(0, 8), depth=(16, 50))
    pipe.process_device(devs[0].data_ptr())
    first = pipe.attenuation(DELTA, **kw)
    pipe.process_device(devs[1].data_ptr())
    got = pipe.attenuation(DELTA, **kw)  # no synchronise in between
    pipe.synchronize()
    second = pipe.processed_host().reshape(b, a, n // 2)
    sname, ma, mb = pipe.intensity_map()
    _same(got, at.attenuation(second, (0, b, 0, 8, 16, 50), DELTA, at.LOG2, ma, mb), "behind process_device")
    assert not np.array_equal(got.view(np.uint32), first.view(np.uint32))
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. side effects
def test_attenuation_leaves_the_processing_chain_untouched():
    n, a, b = 1024, 64, 2
    p = v180_benchmark_params(n, a, b)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = p.bscanViewEnabled = p.enFaceViewEnabled = 1
    devs = [_dev(synthetic_raw(n, a, b, seed=80 + k)) for k in range(2)]
    pipe = Pipeline(p, device=0)
    pipe.enable_kernel_timing(True)

    def state():
        pipe.synchronize()
        (pb, nb), (pe, ne) = pipe.display_buffers()
        vp, vn = pipe.volume_view_buffer()
        return (pipe.processed_host(), pipe.mean_line(), _fetch(pb, nb, np.float32), _fetch(pe, ne, np.float32), _fetch(vp, vn, np.uint8))

    pipe.process_device(devs[0].data_ptr())
    before = state()
    launches = pipe.kernel_timing(reset=False)[1]
    host = before[0].reshape(b, a, n // 2)
    gain = np.linspace(1.0, 2.0, 500).astype(np.float32)
    for src in (dict(), dict(data=host.copy(), scale="log2", map=pipe.intensity_map()[1:])):
        pipe.attenuation(DELTA, gain=gain, depth=(4, 500), **src)
        assert pipe.attenuation_timed(DELTA, depth=(4, 500), **src)[1] > 0.0
        pipe.attenuation_sums(DELTA, depth=(4, 500), **src)
        pipe.attenuation_enface(DELTA, None, 3, 16, "mip", depth=(4, 500), **src)
        assert pipe.attenuation_enface_timed(DELTA, None, 3, 300, "average", gain=gain, depth=(4, 500), **src)[1] > 0.0
    assert pipe.kernel_timing(reset=False)[1] == launches
    for x, y in zip(before, state()):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    pipe.process_device(devs[1].data_ptr())
    after = state()
    fresh = Pipeline(p, device=0)
    for d in devs:
        fresh.process_device(d.data_ptr())
        fresh.synchronize()
    assert np.array_equal(after[0].view(np.uint32), fresh.processed_host().view(np.uint32))
    assert np.array_equal(after[1].view(np.uint32), fresh.mean_line().view(np.uint32))
    fresh.close()
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. errors
def test_intensity_map_errors():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=1))
    pipe.synchronize()
    host = pipe.processed_host().reshape(b, a, n // 2).copy()
    assert pipe.intensity_map()[0] == "log2"
    with pytest.raises(ValueError, match="scale"):
        pipe.attenuation(DELTA, data=host)  # the caller says what their data is
    with pytest.raises(ValueError, match="scale"):
        pipe.attenuation_enface(DELTA, data=host)
    with pytest.raises(ValueError, match="map"):
        pipe.attenuation(DELTA, map=(1.0, 0.0))
    _same(pipe.attenuation(DELTA, "log2", data=host, ascans=(0, 2)), at.attenuation(host, (0, b, 0, 2, 0, n // 2), DELTA, at.LOG2), "map defaults to (1, 0)")
    p.signalMultiplicator = 0.0
    with pytest.raises(ValueError, match="signalMultiplicator"):
        pipe.intensity_map()
    with pytest.raises(ValueError, match="signalMultiplicator"):
        pipe.attenuation(DELTA)
    p.signalMultiplicator = 1.0
    p.postProcessBackgroundRemoval = 1
    with pytest.raises(ValueError, match="postProcessBackgroundRemoval"):
        pipe.intensity_map()
    with pytest.raises(ValueError, match="postProcessBackgroundRemoval"):
        pipe.attenuation_enface(DELTA)
    p.postProcessBackgroundRemoval = 0
    p.signalLogScaling = 0
    assert pipe.intensity_map()[0] == "amplitude"
    with pytest.raises(ValueError, match="gain"):
        pipe.attenuation(DELTA, "intensity", gain=np.ones(7, np.float32), data=host)
    pipe.close()


def test_argument_errors_and_callbacks():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=1))
    pipe.synchronize()
    L, h = _lib.lib(), pipe.handle
    outf = np.zeros(b * a * (n // 2), np.float64)
    surf = np.zeros(a * b, np.int32)
    fp, sp = C.c_void_p(outf.ctypes.data), C.c_void_p(surf.ctypes.data)
    E = _lib.SurfaceEnfaceSettings
    ok = _lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 0, n // 2)

    def S(scale=2, pixel=0.01):
        return _lib.AttenuationSettings(0.4, 0.0, scale, pixel, 0.0, 0.0, 0.0, 0)

    def volume(reg=ok, **kw):
        return L.octpipe_attenuation(h, None, 0, C.byref(reg), C.byref(S(**kw)), None, 0, fp, 0)

    def sums(reg=ok, **kw):
        return L.octpipe_debug_attenuation_sums(h, None, 0, C.byref(reg), C.byref(S(**kw)), None, 0, fp, 0)

    def enface(reg=ok, thickness=4, fn=0, surface=sp, **kw):
        return L.octpipe_attenuation_enface(h, None, 0, C.byref(reg), C.byref(S(**kw)), None, 0, surface, 0, C.byref(E(0, thickness, fn, 0.0)), fp, 0)

    def refused(rc, field):
        assert rc == 1 and field in L.octpipe_last_error(), (rc, field, L.octpipe_last_error())

    for call in (volume, sums, enface):
        assert call() == 0 and call(scale=0) == 0 and call(scale=1) == 0
        refused(call(scale=3), b"scale")
        refused(call(pixel=0.0), b"pixelSize")
        assert call(_lib.StatsRegion(0xFFFFFFFF, 1, 1, 3, 5, 500, 12)) == 0
        for reg, field in ((_lib.StatsRegion(0xFFFFFFFF, 0, 0, 0, a, 0, 8), b"bscan"), (_lib.StatsRegion(0xFFFFFFFF, 1, b, 0, a, 0, 8), b"bscan"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 2, a, 1, 0, 8), b"Ascan"), (_lib.StatsRegion(0xFFFFFFFF, 0, 2, 0, 1, n // 2, 3), b"Sample"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 2, 0, 1, 0, n // 2 + 1), b"Sample"), (_lib.StatsRegion(1, 0, 2, 0, 1, 0, 8), b"buffer")):
            refused(call(reg), field)
    assert enface(thickness=4096) == 0 and enface(fn=1) == 0 and enface(surface=None) == 0
    refused(enface(thickness=0), b"thickness")
    refused(enface(thickness=4097), b"thickness")
    refused(enface(fn=2), b"function")
    with pytest.raises(OctPipeError, match="pixelSize"):
        pipe.attenuation(-1.0)
    with pytest.raises(OctPipeError, match="scale"):
        pipe.attenuation_enface(DELTA, scale=5)
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.extend([volume(), sums(), enface()])
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=3))
    pipe.synchronize()
    assert codes and set(codes) == {7}, codes
    pipe.close()

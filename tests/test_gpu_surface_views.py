"""Surface views on the MI355X (include/octpipe.h "surface views", csrc/surface_views.h, csrc/pipe_surface.hip).

Every result is compared bit for bit against the numpy model of tests/surface_model.py, floats as uint32: there is no tolerance and
nothing is excused.  Small shapes through data= on handles with N = 256 (depth 128) and one with an odd depth, crafted A-scans at the
detection kernel's own chunk and step borders, then a tilted mirror through the whole chain on the handle's own volume, then sources,
ordering, side effects and errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import surface_model as sm
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

# the detection kernel's geometry (csrc/surface_views.h): a ballot covers DETECT_LANES bins, a step of its loop DETECT_STEP, both
# counted from firstSample; a run is joined across either border through the kernel's `carry`
DETECT_LANES, DETECT_STEP = 64, 256


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(np.uint32), want.view(np.uint32)
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


def _out(shape, dtype, n=None):
    """a device result buffer filled with a marker; the fill has finished before the handle's stream writes there"""
    out = torch.full(shape if n is None else (n,), -77, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return out


def _host(pipe, tensor):
    """a device result after the handle's stream has written it (a call with a device result does not wait)"""
    pipe.synchronize()
    return tensor.cpu().numpy()


def _noisy_volume(b, a, depth, seed):
    """standard normal values sprinkled with NaN and +-inf"""
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((b, a, depth)).astype(np.float32)
    flat = vol.reshape(-1)
    k = max(3, flat.size // 40)
    where = rng.choice(flat.size, k, replace=False)
    flat[where[0::3]] = np.nan
    flat[where[1::3]] = np.inf
    flat[where[2::3]] = -np.inf
    return vol


def _holey_surface(rng, shape, lo, hi, holes=0.3):
    s = rng.integers(lo, hi, shape).astype(np.int32)
    s[rng.random(shape) < holes] = -1 - rng.integers(0, 5)
    return s


def _kw(region):
    b0, bn, a0, an, s0, sn = region
    return dict(bscans=(b0, bn), ascans=(a0, an), depth=(s0, sn))


def _flat_kw(region):
    kw = _kw(region)
    kw["window"] = kw.pop("depth")
    return kw


def _regions(b, a, depth):
    """the whole buffer, and sub-regions whose firstSample is 0, 1, 2 and 3"""
    out = [(0, b, 0, a, 0, depth)]
    for s0 in range(4):
        bn, an = max(1, b - 1), max(1, a - 2 - s0)
        out.append((b - bn, bn, min(a - an, 1 + s0 % 2), an, s0, depth - s0 - (5 if s0 & 1 else 0)))
    return out


def _odd_depth_handle(a, b):
    """N = 250 (depth 125: rows alternate in alignment) if the handle accepts it, else the smallest accepted N with an odd N / 2"""
    for n in [250] + list(range(6, 250, 4)):
        try:
            return Pipeline(v180_benchmark_params(n, a, b), device=0), n
        except OctPipeError:
            continue
    raise AssertionError("no samplesPerLine with an odd N / 2 is accepted")


SHAPES = [(256, 1, 1), (256, 67, 3), (256, 130, 2), ("odd", 9, 4)]


@pytest.fixture(scope="module", params=SHAPES, ids=["1x1", "67x3", "130x2", "odd-depth"])
def small(request):
    n, a, b = request.param
    if n == "odd":
        pipe, n = _odd_depth_handle(a, b)
        assert (n // 2) % 2 == 1
    else:
        pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    vol = _noisy_volume(b, a, n // 2, seed=a * 7 + b)
    yield pipe, vol, torch.from_numpy(vol).cuda()
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 1. small shapes
def test_detect_small_shapes(small):
    pipe, vol, dvol = small
    b, a, depth = vol.shape
    for region in _regions(b, a, depth):
        for thr, run in ((0.5, 1), (-0.2, 2), (-1.0, 5), (-np.inf, min(64, region[5])), (np.inf, 1)):
            if run > region[5]:
                continue
            want = sm.detect(vol, region, thr, run)
            _same(pipe.detect_surface(thr, run, data=vol, **_kw(region)), want, ("detect host", region, thr, run))
            out = _out(want.shape, torch.int32)
            assert pipe.detect_surface(thr, run, data=dvol, out=out, **_kw(region)) is out
            _same(_host(pipe, out), want, ("detect device", region, thr, run))


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (37, 29), (6, 9)], ids=["1x1", "1x7", "5x1", "37x29", "all-holes"])
def test_smooth(deep, shape):
    pipe = deep
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    surface = _holey_surface(rng, shape, 0, 500, holes=1.0 if shape == (6, 9) else 0.3)
    for radius in range(4):
        want = sm.smooth(surface, radius)
        _same(pipe.smooth_surface(surface, radius), want, ("smooth host", shape, radius))
        out = _out(shape, torch.int32)
        assert pipe.smooth_surface(torch.from_numpy(surface).cuda(), radius, out=out) is out
        _same(_host(pipe, out), want, ("smooth device", shape, radius))
        _same(pipe.smooth_surface(torch.from_numpy(surface).cuda(), radius), want, ("smooth device -> host", shape, radius))
    if shape == (6, 9):
        assert np.all(sm.smooth(surface, 3) == -1)


def test_enface_small_shapes(small):
    pipe, vol, dvol = small
    b, a, depth = vol.shape
    rng = np.random.default_rng(a + 11)
    for region in _regions(b, a, depth):
        shape = (region[1], region[3])
        surface = _holey_surface(rng, shape, 0, depth)
        dsurf = torch.from_numpy(surface).cuda()
        # offsets that leave the slab inside the window, partly outside it (either end) and wholly outside it (either end)
        for k, (offset, thickness) in enumerate(((0, 1), (-1, 3), (2, 3), (-40, 64), (30, 64), (-depth, 4096), (-9, 4096), (depth + 5, 3), (-depth - 80, 64),
                                                 (-2 * depth - 4096, 4096))):
            for fn, name in ((0, "average"), (1, "mip")):
                fill = np.nan if (k + fn) & 1 else 0.0
                want = sm.enface(vol, region, surface, offset, thickness, fn, fill)
                what = (region, offset, thickness, name, fill)
                _same(pipe.surface_enface(surface, offset, thickness, name, fill, data=vol, **_kw(region)), want, ("enface host",) + what)
                out = _out(shape, torch.float32)
                assert pipe.surface_enface(dsurf, offset, thickness, name, fill, data=dvol, out=out, **_kw(region)) is out
                _same(_host(pipe, out), want, ("enface device",) + what)


def test_flatten_small_shapes(small):
    pipe, vol, dvol = small
    b, a, depth = vol.shape
    rng = np.random.default_rng(a + 23)
    for region in _regions(b, a, depth):
        shape = (region[1], region[3])
        window = region[5]
        surface = _holey_surface(rng, shape, 0, depth, holes=0.15)
        dsurf = torch.from_numpy(surface).cuda()
        # anchors negative, inside and beyond outDepth; outDepth 1, 5, the window and the window + 9
        for anchor, out_depth in ((0, 1), (-3, 5), (2, 5), (40, 5), (-17, window), (window // 2, window), (window + 30, window), (7, window + 9),
                                  (-window, window + 9), (2 * window + 20, window + 9)):
            want = sm.flatten(vol, region, surface, anchor, out_depth, np.nan)
            what = (region, anchor, out_depth)
            _same(pipe.flatten(surface, anchor, out_depth, np.nan, data=vol, **_flat_kw(region)), want, ("flatten host",) + what)
            for loads in (1, 2):
                out = _out(want.shape, torch.float32)
                got, ms = pipe.flatten_timed(dsurf, anchor, out_depth, np.nan, out=out, data=dvol, loads=loads, **_flat_kw(region))
                assert got is out and ms > 0.0
                _same(_host(pipe, out), want, ("flatten device, loads %d" % loads,) + what)
        # an output that starts off a 16-byte boundary: every row has a head
        count = int(np.prod(shape)) * window
        for skew in (1, 2, 3):
            pad = _out(None, torch.float32, count + 4)
            out = pad[skew:skew + count].view(shape + (window,))
            for loads in (1, 2):
                pipe.flatten_timed(dsurf, 5, window, np.nan, out=out, data=dvol, loads=loads, **_flat_kw(region))
                _same(_host(pipe, out), sm.flatten(vol, region, surface, 5, window, np.nan), ("flatten skewed output", region, skew, loads))
            assert float(pad[skew - 1]) == -77.0 and float(pad[skew + count]) == -77.0


def test_flatten_then_a_fixed_slab_is_the_surface_slab(small):
    pipe, vol, dvol = small
    b, a, depth = vol.shape
    region = (0, b, 0, a, 3, depth - 7)
    surface = _holey_surface(np.random.default_rng(5), (b, a), 20, depth - 30)
    for fn, name in ((0, "average"), (1, "mip")):
        for offset, thickness in ((-3, 9), (0, 1), (4, 16)):  # slabs inside the window: flattening puts no fill into them
            flat = pipe.flatten(surface, 12, 40, 0.0, data=dvol, **_flat_kw(region))
            got = pipe.surface_enface(surface, offset, thickness, name, 0.0, data=dvol, **_kw(region))
            _same(got, sm.fixed_slab(flat, 12 + offset, thickness, fn, 0.0), ("identity", name, offset, thickness))


# ---------------------------------------------------------------------------------------------------------------------- 2. crafted A-scans
def _crafted(run, depth):
    """A-scans (values 0 below, 2 above, threshold 1) for every firstSample 0 .. 3 and both borders of the kernel, as [rows][depth]
    with the surface the definition gives for the window [s0, depth - 1]: (row, s0, expected)"""
    rows, meta = [], []

    def add(s0, above, expect, patch=None):
        v = np.zeros(depth, np.float32)
        for lo, hi in above:
            v[max(lo, 0):hi] = 2.0
        for k, x in (patch or {}).items():
            v[k] = x
        rows.append(v)
        meta.append((s0, expect))

    for s0 in range(4):
        for border in (s0 + DETECT_LANES, s0 + DETECT_STEP):  # the first bin of the second ballot / of the second step
            add(s0, [(border, border + run)], border)                      # a run that starts exactly at the border
            add(s0, [(border - 1, border - 1 + run)], border - 1)          # ... one bin before it (run > 1: across it)
            add(s0, [(border - run + 1, border + 1)], border - run + 1)    # ... and ends with the border's bin
            # a run interrupted by one bin, the gap at the border's bin / at the last bin before it; the real run follows
            add(s0, [(border - run + 1, border), (border + 1, border + 1 + run)], border + 1)
            add(s0, [(border - run, border - 1), (border, border + run)], border)
        add(s0, [], -1)                                                    # no hit
        add(s0, [(s0, s0 + run)], s0)                                      # a hit at s0
        add(s0, [(s0 - 1, s0 - 1 + run)], -1)                              # one bin too early: bin s0 - 1 is outside the window
        add(s0, [(depth - run, depth)], depth - run)                       # a hit at the last admissible bin
        add(s0, [(depth - run + 1, depth)], -1)                            # one bin short at the end of the window
        add(s0, [(100, 100 + run), (300, 300 + run)], 300, {100 + run // 2: np.nan})          # NaN inside a run
        add(s0, [(100, 100 + run), (300, 300 + run)], 300, {100 + run - 1: 1.0})              # a value equal to the threshold
        add(s0, [(100, 100 + run)], 100, {100 + run // 2: np.inf})                            # +inf counts as above
        add(s0, [(100, 100 + run), (300, 300 + run)], 300, {100: -np.inf})
    return np.stack(rows), meta


@pytest.fixture(scope="module")
def deep():
    pipe = Pipeline(v180_benchmark_params(1024, 36, 4), device=0)  # depth 512: two steps of the detection loop
    yield pipe
    pipe.close()


@pytest.mark.parametrize("run", [1, 2, 5, 64])
def test_detect_crafted(deep, run):
    pipe, depth = deep, 512
    rows, meta = _crafted(run, depth)
    assert len(rows) <= 36 * 4
    vol = np.zeros((4, 36, depth), np.float32)
    vol.reshape(-1, depth)[:len(rows)] = rows
    dvol = torch.from_numpy(vol).cuda()
    for s0 in range(4):
        region = (0, 4, 0, 36, s0, depth - s0)
        want = sm.detect(vol, region, 1.0, run)
        for i, (row_s0, expect) in enumerate(meta):  # the closed forms, on the model first
            if row_s0 == s0:
                assert want.reshape(-1)[i] == expect, (run, s0, i, want.reshape(-1)[i], expect)
        _same(pipe.detect_surface(1.0, run, data=dvol, **_kw(region)), want, ("crafted", run, s0))
        _same(pipe.detect_surface(1.0, run, data=vol, **_kw(region)), want, ("crafted host", run, s0))
    # a shorter window moves the last admissible bin
    region = (1, 2, 3, 30, 2, 300)
    _same(pipe.detect_surface(1.0, run, data=dvol, **_kw(region)), sm.detect(vol, region, 1.0, run), ("crafted window", run))


# ---------------------------------------------------------------------------------------------------------------------- 3. the product
def _mirror_raw(n, z, amp=1500.0):
    """flat DC plus a Gaussian spectral envelope (sigma = N / 10) times a cosine at depth z (any shape of z)"""
    k = np.arange(n, dtype=np.float64)
    z = np.asarray(z, np.float64)[..., None]
    env = np.exp(-0.5 * ((k - n / 2) / (n / 10)) ** 2)
    return np.clip(np.rint(2048.0 + amp * env * np.cos(2 * np.pi * z * k / n)), 0, 4095).astype(np.uint16)


def _mirror_params(n, a, b):
    p = v180_benchmark_params(n, a, b)
    p.signalLogScaling, p.resampling, p.dispersionCompensation, p.fixedPatternNoiseRemoval = 0, 0, 0, 0
    p.update_all_curves()
    return p


# The scene run through the CPU oracle (oracle/octref.py) with these slopes: the mirror's peak is 2.74 .. 2.84 per A-scan, everything
# else from bin 16 on stays below 0.24 (the DC term sits in the first bins: the window starts at 16), the argmax of the A-scans runs
# from bin 120 to bin 172.  Threshold 1.0 with run 2 and a 3 x 3 median puts the surface 1.7 .. 3.1 bins in front of the peak; the argmax
# of the flattened A-scans takes two values.
MIRROR = dict(n=1024, a=128, b=3, z0=120.3, per_ascan=0.4, per_bscan=0.5, first=16, threshold=1.0, run=2, radius=1)


def test_tilted_mirror_through_the_chain():
    m = MIRROR
    n, a, b = m["n"], m["a"], m["b"]
    ai, bi = np.meshgrid(np.arange(a), np.arange(b))
    pipe = Pipeline(_mirror_params(n, a, b), device=0)
    pipe.octCudaPipeline(_mirror_raw(n, m["z0"] + m["per_ascan"] * ai + m["per_bscan"] * bi))
    pipe.synchronize()
    vol = pipe.processed_host().reshape(b, a, n // 2).copy()
    region = (0, b, 0, a, m["first"], n // 2 - m["first"])
    # on the device from end to end: no result leaves it before the last two
    d_raw = torch.empty((b, a), dtype=torch.int32, device="cuda")
    d_surf = torch.empty((b, a), dtype=torch.int32, device="cuda")
    d_flat = torch.empty((b, a, 64), dtype=torch.float32, device="cuda")
    pipe.detect_surface(m["threshold"], m["run"], depth=region[4:], out=d_raw)
    pipe.smooth_surface(d_raw, m["radius"], out=d_surf)
    pipe.flatten(d_surf, 20, 64, 0.0, out=d_flat, window=region[4:])
    image = pipe.surface_enface(d_surf, 1, 4, "mip", 0.0, depth=region[4:])
    pipe.synchronize()
    raw_surface = sm.detect(vol, region, m["threshold"], m["run"])
    surface = sm.smooth(raw_surface, m["radius"])
    flat = sm.flatten(vol, region, surface, 20, 64, 0.0)
    _same(d_raw.cpu().numpy(), raw_surface, "chain: detect")
    _same(d_surf.cpu().numpy(), surface, "chain: smooth")
    _same(d_flat.cpu().numpy(), flat, "chain: flatten")
    _same(image, sm.enface(vol, region, surface, 1, 4, 1, 0.0), "chain: en face")
    assert np.all(raw_surface >= 0)
    before = vol[:, :, m["first"]:].argmax(axis=2)
    after = flat.argmax(axis=2)
    print("tilted mirror: argmax of the A-scans %d .. %d, of the flattened A-scans %d .. %d; en face %.4f .. %.4f" % (
        before.min() + m["first"], before.max() + m["first"], after.min(), after.max(), image.min(), image.max()))
    assert before.max() - before.min() > 30
    assert after.max() - after.min() + 1 <= 2
    assert image.min() > 2.5  # the slab under the surface holds the mirror's peak everywhere
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. sources, ordering
def test_sources_and_determinism():
    n, a, b = 1024, 96, 2
    p = v180_benchmark_params(n, a, b, buffers_per_volume=2)
    pipe = Pipeline(p, device=0)
    for i in range(2):
        pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=70 + i))
        pipe.synchronize()
    _, _, last = pipe.processed_device()
    kw = dict(bscans=(0, 2), ascans=(5, 80), depth=(9, 400))
    fkw = dict(bscans=(0, 2), ascans=(5, 80), window=(9, 400))
    region = (0, 2, 5, 80, 9, 400)
    per_slot, thrs = [], []
    for s in (0, 1):
        host = pipe.processed_host(slot=s).reshape(b, a, n // 2).copy()
        thr = float(np.quantile(host[:, :, 9:409], 0.98))  # (two such bins in a row: early in some A-scans, late or never in others)
        thrs.append(thr)

        def run(**src):
            surf = pipe.detect_surface(thr, 2, **src, **kw)
            sms = pipe.smooth_surface(surf, 2)
            return [surf, sms, pipe.surface_enface(sms, 2, 16, "average", -1.0, **src, **kw),
                    pipe.surface_enface(sms, -4, 9, "mip", -1.0, **src, **kw), pipe.flatten(sms, 30, 100, np.nan, **src, **fkw)]

        ref = run(buffer=s)
        per_slot.append(ref)
        for what, got in (("repeat", run(buffer=s)), ("host", run(data=host)), ("device", run(data=torch.from_numpy(host).cuda()))):
            for x, y in zip(got, ref):
                _same(x, y, (what, s))
        surf = sm.detect(host, region, thr, 2)
        sms = sm.smooth(surf, 2)
        assert (surf >= 0).any()
        want = [surf, sms, sm.enface(host, region, sms, 2, 16, 0, -1.0), sm.enface(host, region, sms, -4, 9, 1, -1.0),
                sm.flatten(host, region, sms, 30, 100, np.nan)]
        for x, y in zip(ref, want):
            _same(x, y, ("model", s))
    _same(pipe.detect_surface(thrs[last], 2, **kw), per_slot[last][0], "the slot written last")
    with pytest.raises(OctPipeError):
        pipe.detect_surface(thrs[last], 2, buffer=2)
    pipe.close()


def test_host_sources_and_results_beyond_one_staging_slice():
    """75 MB of rows: a host source is staged in two slices (64 MiB each at most) and a flattened host result leaves in two; the bits
    are those of the device source, and the rows on either side of the slice border are the model's"""
    n, a, b = 4096, 1024, 9
    depth = n // 2
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    vol = np.random.default_rng(4).standard_normal((b, a, depth), dtype=np.float32)
    dvol = torch.from_numpy(vol).cuda()
    assert vol.nbytes > (64 << 20) and (64 << 20) // (4 * depth) == 8 * a  # the border: row 8192, the first A-scan of B-scan 8
    surf = pipe.detect_surface(2.0, 2, data=dvol, depth=(3, depth - 3))
    _same(pipe.detect_surface(2.0, 2, data=vol, depth=(3, depth - 3)), surf, "detect, host source in slices")
    sms = pipe.smooth_surface(surf, 1)
    d_flat = _out((b, a, depth), torch.float32)
    pipe.flatten(sms, 100, depth, np.nan, out=d_flat, data=dvol, window=(3, depth - 3))
    flat = pipe.flatten(sms, 100, depth, np.nan, data=vol, window=(3, depth - 3))
    _same(flat, _host(pipe, d_flat), "flatten, host source and host result in slices")
    image = pipe.surface_enface(sms, -2, 9, "average", np.nan, data=vol, depth=(3, depth - 3))
    _same(image, pipe.surface_enface(sms, -2, 9, "average", np.nan, data=dvol, depth=(3, depth - 3)), "en face, host source in slices")
    for bs, first in ((7, a - 4), (8, 0)):
        region = (bs, 1, first, 4, 3, depth - 3)
        part = sms[bs:bs + 1, first:first + 4]
        _same(surf[bs:bs + 1, first:first + 4], sm.detect(vol, region, 2.0, 2), ("detect at the border", bs))
        _same(flat[bs:bs + 1, first:first + 4], sm.flatten(vol, region, part, 100, depth, np.nan), ("flatten at the border", bs))
        _same(image[bs:bs + 1, first:first + 4], sm.enface(vol, region, part, -2, 9, 0, np.nan), ("en face at the border", bs))
    pipe.close()


def test_a_call_behind_process_device_sees_that_buffer():
    n, a, b = 1024, 64, 2
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    devs = [_dev(synthetic_raw(n, a, b, seed=90 + k)) for k in range(2)]
    pipe.process_device(devs[0].data_ptr())
    pipe.synchronize()
    first = pipe.processed_host().reshape(b, a, n // 2).copy()
    thr = float(np.quantile(first[:, :, 8:], 0.98))
    surface = sm.detect(first, (0, b, 0, a, 8, n // 2 - 8), thr, 1)
    pipe.process_device(devs[1].data_ptr())
    got = pipe.detect_surface(thr, 1, depth=(8, n // 2 - 8))  # no synchronise in between
    flat = pipe.flatten(got, 10, 32, 0.0, window=(8, n // 2 - 8))
    pipe.synchronize()
    second = pipe.processed_host().reshape(b, a, n // 2).copy()
    want = sm.detect(second, (0, b, 0, a, 8, n // 2 - 8), thr, 1)
    assert not np.array_equal(want, surface)  # (the two buffers differ where it matters)
    _same(got, want, "detect behind process_device")
    _same(flat, sm.flatten(second, (0, b, 0, a, 8, n // 2 - 8), want, 10, 32, 0.0), "flatten behind process_device")
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. side effects
def test_surface_views_leave_the_processing_chain_untouched():
    n, a, b = 1024, 64, 2
    p = v180_benchmark_params(n, a, b)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = p.bscanViewEnabled = p.enFaceViewEnabled = 1
    raws = [synthetic_raw(n, a, b, seed=80 + k) for k in range(2)]
    devs = [_dev(r) for r in raws]
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
    thr = float(np.quantile(host[:, :, 4:504], 0.98))
    for src in (dict(), dict(data=host.copy())):
        surf = pipe.detect_surface(thr, 2, depth=(4, 500), **src)
        sms = pipe.smooth_surface(surf, 3)
        pipe.surface_enface(sms, 0, 16, "mip", depth=(4, 500), **src)
        pipe.flatten(sms, 16, 128, window=(4, 500), **src)
        pipe.flatten_timed(sms, 16, 128, window=(4, 500), loads=2, **src)
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
    vp, vn = fresh.volume_view_buffer()
    assert np.array_equal(after[4], _fetch(vp, vn, np.uint8))
    fresh.close()
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 6. errors
def test_argument_errors_and_callbacks():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=1))
    pipe.synchronize()
    L, h = _lib.lib(), pipe.handle
    surf = np.zeros(a * b, np.int32)
    outi = np.zeros(a * b, np.int32)
    outf = np.zeros(a * b * 64, np.float32)
    sp, op, fp = (C.c_void_p(x.ctypes.data) for x in (surf, outi, outf))
    D, E, F = _lib.SurfaceDetectSettings, _lib.SurfaceEnfaceSettings, _lib.FlattenSettings
    ok = _lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 0, n // 2)

    def detect(reg=ok, thr=1.0, run=1, out=op):
        return L.octpipe_surface_detect(h, None, 0, C.byref(reg), C.byref(D(thr, run)), out, 0)

    def smooth(rows=b, cols=a, radius=1, src=sp, out=op):
        return L.octpipe_surface_smooth(h, src, 0, rows, cols, radius, out, 0)

    def enface(reg=ok, thickness=1, fn=0, surface=sp, out=fp):
        return L.octpipe_surface_enface(h, None, 0, C.byref(reg), surface, 0, C.byref(E(0, thickness, fn, 0.0)), out, 0)

    def flatten(reg=ok, out_depth=64, surface=sp, out=fp):
        return L.octpipe_flatten(h, None, 0, C.byref(reg), surface, 0, C.byref(F(0, out_depth, 0.0)), out, 0)

    def refused(rc, field):
        assert rc == 1 and field in L.octpipe_last_error(), (rc, field, L.octpipe_last_error())

    assert detect() == 0 and smooth() == 0 and enface() == 0 and flatten() == 0
    assert detect(run=64) == 0 and smooth(radius=0) == 0 and smooth(radius=3) == 0 and enface(thickness=4096) == 0 and flatten(out_depth=1) == 0
    refused(detect(run=0), b"run")
    refused(detect(run=65), b"run")
    refused(detect(thr=float("nan")), b"threshold")
    refused(detect(_lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 7, 5), run=6), b"run")  # run beyond the window
    assert detect(_lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 7, 5), run=5) == 0
    refused(detect(out=None), b"surface")
    refused(smooth(radius=4), b"radius")
    refused(smooth(out=sp), b"out")
    refused(smooth(rows=0), b"rows")
    refused(smooth(src=None), b"surface")
    refused(enface(thickness=0), b"thickness")
    refused(enface(thickness=4097), b"thickness")
    refused(enface(fn=2), b"function")
    refused(enface(surface=None), b"surface")
    refused(enface(out=None), b"out")
    refused(flatten(out_depth=0), b"outDepth")
    refused(flatten(out_depth=8193), b"outDepth")
    refused(flatten(surface=None), b"surface")
    refused(flatten(out=None), b"out")
    for call in (detect, enface, flatten):
        for reg, field in ((_lib.StatsRegion(0xFFFFFFFF, 0, 0, 0, a, 0, 8), b"bscan"), (_lib.StatsRegion(0xFFFFFFFF, 1, b, 0, a, 0, 8), b"bscan"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 1, a, 1, 0, 8), b"Ascan"), (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, n // 2, 3), b"Sample"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, n // 2 + 1), b"Sample"), (_lib.StatsRegion(1, 0, 1, 0, 1, 0, 8), b"buffer")):
            refused(call(reg), field)
    ms = C.c_double()
    refused(L.octpipe_debug_flatten(h, None, 0, C.byref(ok), sp, 0, C.byref(F(0, 64, 0.0)), fp, 0, 3, C.byref(ms)), b"loads")
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.extend([detect(), smooth(), enface(), flatten()])
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=3))
    pipe.synchronize()
    assert codes and set(codes) == {7}, codes
    pipe.close()

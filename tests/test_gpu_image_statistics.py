"""Image statistics on the MI355X (include/octpipe.h "image statistics", csrc/image_stats.h, csrc/pipe_stats.hip).

Histograms and every count are held bit-exact against the numpy model of tests/stats_model.py: on the product's own processed output,
on caller float buffers with crafted edge values, and on raw buffers of every sample format.  Moments within 1e-9 relative of numpy
float64 and bitwise equal across calls and sources.  Then slot selection, side effects and errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import stats_model as sm
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params
from octproz_amd.pipeline import ImageStatistics

pytestmark = pytest.mark.gpu

MOMENT_RTOL = 1e-9
COUNTS = ("count", "underflow", "overflow", "nonFinite")


def _check(got, want, what):
    assert np.array_equal(got.histogram, want["histogram"]), what
    for f in COUNTS:
        assert getattr(got, f) == want[f], (what, f, getattr(got, f), want[f])
    for f in ("lo", "hi", "binWidth"):
        g, w = getattr(got, f), want[f]
        assert (np.isnan(g) and np.isnan(w)) or g == w, (what, f, g, w)
    if want["count"] == 0:
        assert all(np.isnan(getattr(got, f)) for f in ("min", "max", "mean", "stddev")), what
        return
    assert got.min == want["min"] and got.max == want["max"], what
    scale = max(abs(want["mean"]), want["stddev"], 1e-300)
    assert abs(got.mean - want["mean"]) <= MOMENT_RTOL * scale, (what, got.mean, want["mean"])
    assert abs(got.stddev - want["stddev"]) <= MOMENT_RTOL * max(want["stddev"], 1e-300) or want["stddev"] == got.stddev == 0.0, \
        (what, got.stddev, want["stddev"])


def _same_bits(a, b, what):
    assert np.array_equal(a.histogram, b.histogram), what
    for f in ImageStatistics.FIELDS:
        x, y = np.float64(getattr(a, f)), np.float64(getattr(b, f))
        assert x.tobytes() == y.tobytes(), (what, f, x, y)


# ---------------------------------------------------------------------------------------------------------------------- 1. processed
@pytest.mark.parametrize("n", [1024, 1664, 1000])
@pytest.mark.parametrize("log,flip", [(1, 0), (0, 0), (1, 1)], ids=["log", "linear", "log-flip"])
def test_product_output_matches_the_model(n, log, flip):
    a, b = 64, 6
    p = v180_benchmark_params(n, a, b)
    p.signalLogScaling, p.bscanFlip = log, flip
    p.update_all_curves()
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=n + log))
    pipe.synchronize()
    vol = pipe.processed_host().reshape(b, a, n // 2)
    lo, hi = np.percentile(vol, [5, 95]).astype(np.float32)
    d_vol = torch.from_numpy(vol.copy()).cuda()
    regions = [(None, None, None), ((1, 4), (3, 51), (7, n // 2 - 20)), ((5, 1), (63, 1), (0, n // 2))]
    for bs, asc, dep in regions:
        reg = sm.region_of(vol, bs or (0, b), asc or (0, a), dep or (0, n // 2))
        for rng in (None, (float(lo), float(hi))):
            want = sm.processed(reg, 256, *(rng or (None, None)))
            got = pipe.processed_statistics(bscans=bs, ascans=asc, depth=dep, bins=256, range=rng)
            _check(got, want, (n, log, flip, bs, asc, dep, rng))
            again = pipe.processed_statistics(bscans=bs, ascans=asc, depth=dep, bins=256, range=rng)
            _same_bits(got, again, "repeat")
            host = pipe.processed_statistics(data=vol, bscans=bs, ascans=asc, depth=dep, bins=256, range=rng)
            dev = pipe.processed_statistics(data=d_vol, bscans=bs, ascans=asc, depth=dep, bins=256, range=rng)
            _same_bits(got, host, "host copy")
            _same_bits(got, dev, "device copy")
    pipe.close()


def _edge_buffer(n, a, b, rng):
    """a processed buffer full of the crafted values: exact edges of 0..8 in 8 bins, one ulp either side, -0.0, NaN, +-inf"""
    lo, hi = np.float32(0.0), np.float32(8.0)
    edges = np.arange(9, dtype=np.float32)
    crafted = np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(9)),
                              np.array([-0.0, np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)])
    vol = (rng.random((b, a, n // 2)) * 10 - 1).astype(np.float32)
    flat = vol.reshape(-1)
    idx = rng.choice(flat.size, size=flat.size // 3, replace=False)
    flat[idx] = crafted[rng.integers(0, crafted.size, size=idx.size)]
    return vol, lo, hi


@pytest.mark.parametrize("n", [1024, 1000])
def test_crafted_float_buffers_host_and_device(n):
    a, b = 32, 4
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    rng = np.random.default_rng(n)
    vol, lo, hi = _edge_buffer(n, a, b, rng)
    d_vol = torch.from_numpy(vol.copy()).cuda()
    for bs, asc, dep in [(None, None, None), ((1, 3), (5, 17), (3, 101))]:
        reg = sm.region_of(vol, bs or (0, b), asc or (0, a), dep or (0, n // 2))
        for bins, r in ((8, (float(lo), float(hi))), (1, (float(lo), float(hi))), (4096, (-0.5, 9.5)), (8, None)):
            want = sm.processed(reg, bins, *(r or (None, None)))
            h = pipe.processed_statistics(data=vol, bscans=bs, ascans=asc, depth=dep, bins=bins, range=r)
            d = pipe.processed_statistics(data=d_vol, bscans=bs, ascans=asc, depth=dep, bins=bins, range=r)
            _check(h, want, (n, bs, bins, r))
            _same_bits(h, d, "host vs device")
    # all-constant and all-non-finite buffers under autoRange
    const = np.full((b, a, n // 2), 3.25, np.float32)
    got = pipe.processed_statistics(data=const, bins=64)
    _check(got, sm.processed(const, 64), "constant")
    assert got.histogram[0] == const.size and got.stddev == 0.0
    bad = np.full((b, a, n // 2), np.nan, np.float32)
    bad[0, 0, :5] = np.inf
    got = pipe.processed_statistics(data=torch.from_numpy(bad).cuda(), bins=64)
    _check(got, sm.processed(bad, 64), "non-finite")
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. raw
@pytest.mark.parametrize("fmt,bit_depth", sm.FORMATS, ids=sm.FORMAT_IDS)
def test_raw_formats_match_the_model(fmt, bit_depth):
    n, a, b = 1024, 24, 4
    rng = np.random.default_rng(fmt * 7 + bit_depth)
    ints = sm.random_ints(rng, (b, a, n), fmt, bit_depth)
    raw, dec = sm.encode(ints, fmt, bit_depth)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    for bitshift in (0, 1):
        p = v180_benchmark_params(n, a, b)
        p.bitDepth, p.bitshift = bit_depth, bitshift
        p.update_all_curves()
        pipe = Pipeline(p, device=0, sample_format=fmt)
        val = sm.decoded(dec, fmt, bit_depth, bitshift)
        for bs, asc, smp in [(None, None, None), ((1, 3), (5, 17), (3, 1001)), ((0, 4), (1, 23), (9, 15))]:
            reg = sm.region_of(val, bs or (0, b), asc or (0, a), smp or (0, n))
            mid = int(np.median(reg))
            for bins, lo, width in ((4096, None, None), (256, mid - 300, 3), (7, int(reg.min()) + 5, 1000)):
                want = sm.raw(reg, bins, lo, width)
                h = pipe.raw_statistics(raw, bscans=bs, ascans=asc, samples=smp, bins=bins, lo=lo, bin_width=width)
                d = pipe.raw_statistics(d_raw, bscans=bs, ascans=asc, samples=smp, bins=bins, lo=lo, bin_width=width)
                _check(h, want, (fmt, bit_depth, bitshift, bs, asc, smp, bins, lo))
                _same_bits(h, d, "raw host vs device")
        pipe.close()


@pytest.mark.parametrize("n", [1000, 1001, 130])
def test_raw_lengths_without_vector_loads(n):
    """rows whose length or window does not allow the vector loads; packed 12 bit with an odd samplesPerLine and odd firstSample"""
    a, b = 9, 4
    for fmt, bit_depth in ((1, 12), (2, 12), (0, 12)):
        rng = np.random.default_rng(n + fmt)
        ints = sm.random_ints(rng, (b, a, n), fmt, bit_depth)
        raw, dec = sm.encode(ints, fmt, bit_depth)
        p = v180_benchmark_params(n, a, b)
        pipe = Pipeline(p, device=0, sample_format=fmt)
        for bs, asc, smp in [(None, None, None), ((1, 2), (3, 5), (1, n - 8)), ((0, 4), (0, 9), (7, 1))]:
            reg = sm.region_of(dec, bs or (0, b), asc or (0, a), smp or (0, n))
            want = sm.raw(reg, 4096, 0, 1)
            h = pipe.raw_statistics(raw, bscans=bs, ascans=asc, samples=smp, lo=0, bin_width=1)
            d = pipe.raw_statistics(torch.from_numpy(raw.copy()).cuda(), bscans=bs, ascans=asc, samples=smp, lo=0, bin_width=1)
            _check(h, want, (n, fmt, bs, asc, smp))
            _same_bits(h, d, "host vs device")
        pipe.close()


def test_saturation_count_of_twelve_bit_data():
    n, a, b = 1024, 64, 4
    rng = np.random.default_rng(3)
    ints = np.clip(rng.normal(3200, 700, size=(b, a, n)).round(), 0, 4095).astype(np.uint16)
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    s = pipe.raw_statistics(torch.from_numpy(ints.view(np.int16)).cuda())
    assert s.histogram[4095] == np.count_nonzero(ints == 4095) > 0
    assert s.count == ints.size and s.overflow == 0 and s.underflow == 0
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 3. slots
def test_slot_selection_with_two_buffers_per_volume():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b, buffers_per_volume=2)
    pipe = Pipeline(p, device=0)
    for i in range(3):
        pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=20 + i))
        pipe.synchronize()
        _, _, slot = pipe.processed_device()
        for s in (0, 1):
            data = pipe.processed_host(slot=s)
            got = pipe.processed_statistics(buffer=s, bins=64)
            _check(got, sm.processed(data, 64), ("slot", s))
        last = pipe.processed_statistics(bins=64)
        _same_bits(last, pipe.processed_statistics(buffer=slot, bins=64), "last slot")
    with pytest.raises(OctPipeError) as e:
        pipe.processed_statistics(buffer=2)
    assert e.value.code == 1
    pipe.close()


def test_float_streaming_double_buffer():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b)
    p.streamFloatToHost = 1
    pipe = Pipeline(p, device=0)
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])
    for i in range(3):
        pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=30 + i))
        pipe.synchronize()
        want = pipe.processed_host()
        got = pipe.processed_statistics(bins=128)
        _check(got, sm.processed(want, 128), ("float streaming", i))
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. side effects
def test_no_side_effects():
    n, a, b = 1024, 64, 2
    raws = [synthetic_raw(n, a, b, seed=40 + i) for i in range(2)]

    def run(with_stats):
        p = v180_benchmark_params(n, a, b)
        pipe = Pipeline(p, device=0)
        pipe.enable_kernel_timing(True)
        pipe.octCudaPipeline(raws[0])
        pipe.synchronize()
        before = pipe.kernel_timing(reset=False)[1]
        if with_stats:
            pipe.processed_statistics(bins=256)
            pipe.processed_statistics(bins=16, range=(0.0, 1.0), ascans=(3, 9))
            pipe.raw_statistics(raws[1])
            pipe.raw_statistics(torch.from_numpy(raws[1].view(np.int16)).cuda(), bins=100)
            assert pipe.kernel_timing(reset=False)[1] == before
        pipe.octCudaPipeline(raws[1])
        pipe.synchronize()
        out = (pipe.processed_host().copy(), pipe.mean_line().copy())
        pipe.close()
        return out

    ref, got = run(False), run(True)
    for x, y in zip(ref, got):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- 5. errors
def test_argument_errors_and_callbacks():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    L, h = _lib.lib(), pipe.handle
    st = _lib.ImageStatistics()
    raw = synthetic_raw(n, a, b, seed=1)

    def proc(reg, bins=16, auto=1, lo=0.0, hi=1.0):
        return L.octpipe_processed_statistics(h, None, 0, C.byref(reg), bins, auto, lo, hi, None, C.byref(st))

    def rawc(reg, bins=16, auto=1):
        return L.octpipe_raw_statistics(h, raw.ctypes.data, 0, C.byref(reg), bins, auto, 0, 1, None, C.byref(st))

    ok = _lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 0, n // 2)
    assert proc(ok) == 0 and rawc(_lib.StatsRegion(0, 0, b, 0, a, 0, n)) == 0
    for reg, field in ((_lib.StatsRegion(0xFFFFFFFF, 0, 0, 0, a, 0, 8), b"bscan"), (_lib.StatsRegion(0xFFFFFFFF, 1, b, 0, a, 0, 8), b"bscan"),
                       (_lib.StatsRegion(0xFFFFFFFF, 0, 1, a, 1, 0, 8), b"Ascan"), (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, n // 2, 1), b"Sample"),
                       (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, n // 2 + 1), b"Sample"), (_lib.StatsRegion(1, 0, 1, 0, 1, 0, 1), b"buffer")):
        assert proc(reg) == 1 and field in L.octpipe_last_error(), (field, L.octpipe_last_error())
    assert rawc(_lib.StatsRegion(0, 0, 1, 0, 1, 0, n + 1)) == 1 and b"Sample" in L.octpipe_last_error()
    assert rawc(_lib.StatsRegion(0, 0, 1, 0, 1, n - 1, 1)) == 0
    assert proc(ok, bins=4097) == 1 and proc(ok, auto=0, lo=1.0, hi=0.5) == 1
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.append(proc(ok))
        codes.append(rawc(_lib.StatsRegion(0, 0, b, 0, a, 0, n)))
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    assert codes and set(codes) == {7}, codes
    pipe.close()

"""Image statistics without a device (include/octpipe.h "image statistics"): the ABI surface, the status codes of calls that need no
device, the numpy model of the definition on crafted cases, ImageStatistics.quantile, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stats_model as sm
from octproz_amd import _lib
from octproz_amd.pipeline import ImageStatistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

PUBLIC = ["octpipe_processed_statistics", "octpipe_raw_statistics"]
DEBUG = ["octpipe_debug_processed_statistics", "octpipe_debug_raw_statistics"]
ERR_INVALID_ARGUMENT = 1


def f32(x):
    return np.float32(x)


def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name)
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name)


def test_struct_layouts():
    assert C.sizeof(_lib.StatsRegion) == 28
    assert C.sizeof(_lib.ImageStatistics) == 88
    assert [f[0] for f in _lib.StatsRegion._fields_] == ["buffer", "firstBscan", "bscanCount", "firstAscan", "ascanCount", "firstSample",
                                                         "sampleCount"]
    assert [f[0] for f in _lib.ImageStatistics._fields_] == ["count", "underflow", "overflow", "nonFinite", "min", "max", "mean", "stddev",
                                                             "lo", "hi", "binWidth"]
    hdr = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    assert "7 x uint32 = 28 bytes" in hdr and "11 x 8 = 88 bytes" in hdr


def _proc(L, h, region, bins=256, auto=0, lo=0.0, hi=1.0, out=True, data=None):
    st = _lib.ImageStatistics()
    hist = np.zeros(4096, np.uint64)
    return L.octpipe_processed_statistics(h, data, 0, C.byref(region) if region is not None else None, bins, auto, lo, hi, hist.ctypes.data,
                                          C.byref(st) if out else None)


def _raw(L, h, region, bins=256, auto=0, lo=0, width=1, raw=True, out=True):
    st = _lib.ImageStatistics()
    buf = np.zeros(64, np.uint8)
    return L.octpipe_raw_statistics(h, buf.ctypes.data if raw else None, 0, C.byref(region) if region is not None else None, bins, auto, lo,
                                    width, None, C.byref(st) if out else None)


def test_status_codes_without_a_device():
    L = _lib.lib()
    reg = _lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, 1)
    ms = C.c_double()
    assert _proc(L, None, reg) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    assert _raw(L, None, reg) == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    st = _lib.ImageStatistics()
    assert L.octpipe_debug_processed_statistics(None, None, 0, C.byref(reg), 16, 1, 0.0, 0.0, None, C.byref(st), C.byref(ms)) == 1
    assert L.octpipe_debug_raw_statistics(None, C.byref(reg), 0, C.byref(reg), 16, 1, 0, 0, None, C.byref(st), C.byref(ms)) == 1
    # arguments that are wrong whatever the handle: named before the handle is looked at
    cases = [(lambda: _proc(L, None, None), b"region"),
             (lambda: _proc(L, None, reg, out=False), b"out"),
             (lambda: _proc(L, None, reg, bins=0), b"bins"),
             (lambda: _proc(L, None, reg, bins=4097), b"bins"),
             (lambda: _proc(L, None, reg, lo=1.0, hi=1.0), b"lo < hi"),
             (lambda: _proc(L, None, reg, lo=2.0, hi=1.0), b"lo < hi"),
             (lambda: _proc(L, None, reg, lo=float("nan"), hi=1.0), b"lo < hi"),
             (lambda: _proc(L, None, reg, lo=0.0, hi=float("inf")), b"lo < hi"),
             (lambda: _proc(L, None, _lib.StatsRegion(1, 0, 1, 0, 1, 0, 1), data=np.zeros(4, np.float32).ctypes.data), b"buffer"),
             (lambda: _raw(L, None, reg, raw=False), b"raw"),
             (lambda: _raw(L, None, None), b"region"),
             (lambda: _raw(L, None, reg, out=False), b"out"),
             (lambda: _raw(L, None, reg, bins=0), b"bins"),
             (lambda: _raw(L, None, reg, bins=5000), b"bins"),
             (lambda: _raw(L, None, reg, width=0), b"binWidth")]
    for call, field in cases:
        assert call() == ERR_INVALID_ARGUMENT and field in L.octpipe_last_error(), (field, L.octpipe_last_error())
    # autoRange needs no lo / hi / binWidth
    assert _proc(L, None, reg, auto=1, lo=float("nan"), hi=float("nan")) == 1 and b"null handle" in L.octpipe_last_error()
    assert _raw(L, None, reg, auto=1, width=0) == 1 and b"null handle" in L.octpipe_last_error()


# ---------------------------------------------------------------------------------------------------------------------- the model
def test_processed_bins_at_the_edges():
    bins, lo, hi = 4, f32(0.0), f32(1.0)
    edge = f32(0.25)  # t = 1.0 exactly: bin 1
    v = np.array([lo, hi, edge, np.nextafter(edge, f32(0)), np.nextafter(edge, f32(1)), np.nextafter(hi, f32(2)),
                  np.nextafter(lo, f32(-1)), f32(-0.0), np.nan, np.inf, -np.inf, f32(0.75), f32(0.5)], np.float32)
    r = sm.processed(v, bins, lo, hi)
    # lo -> 0, hi -> 3 (last bin, as numpy), 0.25 -> 1, 0.25 - ulp -> 0, 0.25 + ulp -> 1, hi + ulp over, lo - ulp under, -0.0 -> 0,
    # 0.75 -> 3, 0.5 -> 2
    assert list(r["histogram"]) == [3, 2, 1, 2]
    assert (r["underflow"], r["overflow"], r["nonFinite"], r["count"]) == (1, 1, 3, 10)
    fin = v[np.isfinite(v)].astype(np.float64)
    assert r["min"] == fin.min() and r["max"] == fin.max() and r["mean"] == fin.mean() and r["stddev"] == fin.std()
    assert r["binWidth"] == 0.25


def test_processed_matches_numpy_histogram_where_edges_are_exact():
    rng = np.random.default_rng(1)
    v = (rng.random(100000) * 300 - 20).astype(np.float32)
    r = sm.processed(v, 256, 0.0, 256.0)
    want, _ = np.histogram(v, bins=256, range=(0.0, 256.0))
    assert np.array_equal(r["histogram"], want.astype(np.uint64))
    assert r["underflow"] == np.count_nonzero(v < 0) and r["overflow"] == np.count_nonzero(v > 256)


def test_processed_sub_and_mul_stay_separate():
    """a value where (v - lo) * scale and v * scale - lo * scale land in different bins: the definition takes the first"""
    bins, lo, hi = 100, f32(-3.3), f32(9.1)
    scale = sm.processed_scale(bins, lo, hi)
    rng = np.random.default_rng(5)
    v = (lo + rng.random(200000).astype(np.float32) * (hi - lo)).astype(np.float32)
    sep = np.floor((v - lo).astype(np.float32) * scale)
    fused = np.floor((v * scale).astype(np.float32) - (lo * scale).astype(np.float32))
    differ = np.nonzero(np.minimum(sep, bins - 1) != np.minimum(fused, bins - 1))[0]
    assert differ.size > 0
    x = v[differ[0]]
    r = sm.processed(np.array([x], np.float32), bins, lo, hi)
    assert int(np.argmax(r["histogram"])) == int(min(sep[differ[0]], bins - 1))


def test_processed_auto_range():
    v = np.array([3.0, 3.0, np.nan, 3.0], np.float32)
    r = sm.processed(v, 16)
    assert r["lo"] == r["hi"] == 3.0 and r["histogram"][0] == 3 and r["histogram"].sum() == 3 and r["stddev"] == 0.0
    r = sm.processed(np.array([np.nan, np.inf], np.float32), 16)
    assert np.isnan(r["lo"]) and np.isnan(r["hi"]) and r["histogram"].sum() == 0 and r["count"] == 0 and r["nonFinite"] == 2
    assert np.isnan(r["mean"]) and np.isnan(r["stddev"])
    v = np.array([-2.0, 0.5, 6.0], np.float32)
    r = sm.processed(v, 4)
    assert (r["lo"], r["hi"]) == (-2.0, 6.0) and list(r["histogram"]) == [1, 1, 0, 1]


def test_processed_scale_is_clamped():
    lo = f32(0.0)
    hi = np.nextafter(lo, f32(1))  # the smallest subnormal: bins / (hi - lo) overflows float32
    assert sm.processed_scale(4, lo, hi) == np.finfo(np.float32).max
    r = sm.processed(np.array([lo, hi], np.float32), 4, lo, hi)
    assert r["histogram"][0] == 2  # (hi - lo) * FLT_MAX = 4.8e-7: both values in bin 0


def test_raw_bins_with_negative_integers():
    x = np.array([-130, -129, -128, -1, 0, 5, 126, 127, 200], np.int64)
    r = sm.raw(x, 4, lo=-128, width=64)
    # [-128, -65) [-64, -1] [0, 63] [64, 127]; -130 / -129 under, 200 over
    assert list(r["histogram"]) == [1, 1, 2, 2] and (r["underflow"], r["overflow"]) == (2, 1)
    assert r["hi"] == -128 + 4 * 64 and r["nonFinite"] == 0 and r["count"] == 9
    r = sm.raw(x, 4)  # auto: lo = -130, width = ceil(331 / 4) = 83
    assert (r["lo"], r["binWidth"], r["underflow"], r["overflow"]) == (-130.0, 83.0, 0, 0) and r["histogram"].sum() == 9
    r = sm.raw(np.array([7, 7, 7]), 4096)
    assert (r["lo"], r["binWidth"]) == (7.0, 1.0) and r["histogram"][0] == 3


def test_raw_twelve_bit_saturation_count():
    rng = np.random.default_rng(2)
    x = np.clip(rng.normal(3000, 800, 50000).round(), 0, 4095).astype(np.int64)
    r = sm.raw(x, 4096, lo=0, width=1)
    assert r["histogram"][4095] == np.count_nonzero(x == 4095) > 0 and r["overflow"] == 0


@pytest.mark.parametrize("fmt,bit_depth", sm.FORMATS, ids=sm.FORMAT_IDS)
def test_encode_decode_round_trip(fmt, bit_depth):
    rng = np.random.default_rng(fmt)
    ints = sm.random_ints(rng, (4, 10), fmt, bit_depth)
    b, dec = sm.encode(ints, fmt, bit_depth)
    assert dec.shape == ints.shape
    if fmt in (1, 2):
        assert b.size == ints.size * 3 // 2
        want = ints & 0xFFF if fmt == 1 else ((ints & 0xFFF) ^ 0x800) - 0x800
        assert np.array_equal(dec, want)
    else:
        assert np.array_equal(dec, ints)
    assert np.array_equal(sm.decoded(dec, fmt, bit_depth, 1), dec if (fmt == 0 and bit_depth > 16) else dec >> 4)


# ---------------------------------------------------------------------------------------------------------------------- quantile
def test_quantile_on_a_known_histogram():
    st = _lib.ImageStatistics(count=10, lo=0.0, hi=4.0, binWidth=1.0)
    s = ImageStatistics(st, np.array([2, 0, 5, 3], np.uint64))
    assert list(s.edges) == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert s.quantile(0.0) == 0.0
    assert s.quantile(0.2) == 0.0   # cumulative 2 reaches 0.2 * 10 in bin 0
    assert s.quantile(0.21) == 2.0  # bin 1 adds nothing, bin 2 reaches 7
    assert s.quantile(0.7) == 2.0
    assert s.quantile(0.71) == 3.0
    assert s.quantile(1.0) == 3.0
    empty = ImageStatistics(_lib.ImageStatistics(lo=0.0, hi=4.0, binWidth=1.0), np.zeros(4, np.uint64))
    assert np.isnan(empty.quantile(0.5))
    with pytest.raises(ValueError):
        s.quantile(1.5)


# ---------------------------------------------------------------------------------------------------------------------- kernels
def _kernel_meta(text, name):
    start = text.index(name + ":")
    meta = text[start:]  # (the first resource comments after the label belong to this kernel)
    return int(re.search(r"; ScratchSize: (\d+)", meta).group(1)), int(re.search(r"; NumVgprs: (\d+)", meta).group(1))


def test_stats_kernels_need_no_scratch(tmp_path):
    """every (source, vector form) instance of oct_stats_kernel and the finish kernel: no private memory, at most 128 VGPRs (four waves
    per SIMD or more)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "image_stats.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "image_stats_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^(_ZN3oct16oct_stats_kernelILi\d+ELb[01]EEEvNS_9StatsArgsE):", text, re.M)
    assert len(names) == 18
    names += ["_ZN3oct23oct_stats_finish_kernelENS_15StatsFinishArgsE", "_ZN3oct25oct_stats_hist_sum_kernelEPKjjjPy"]
    for name in names:
        scratch, vgprs = _kernel_meta(text, name)
        assert scratch == 0 and vgprs <= 128, (name, scratch, vgprs)

"""Depth-resolved attenuation without a device (include/octpipe.h "attenuation"): the ABI surface, the status codes of calls that need no
device, the numpy model (tests/attenuation_model.py) against closed forms, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import attenuation_model as at
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT = 1
NAN_BITS = 0x7FC00000

PUBLIC = ("octpipe_attenuation", "octpipe_attenuation_enface")
DEBUG = ("octpipe_debug_attenuation", "octpipe_debug_attenuation_enface", "octpipe_debug_attenuation_sums")


# ---------------------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name), name
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name), name
    assert L.octpipe_abi_version() == 2  # the additions are additive


def test_struct_layout():
    struct, mirror, stated = "OctPipeAttenuationSettings", _lib.AttenuationSettings, "2 x 8 + 6 x 4 = 40 bytes"
    hdr = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    head = "typedef struct %s {" % struct
    line = hdr[hdr.index(head):].split("\n", 1)[0]
    assert stated in line and C.sizeof(mirror) == int(stated.split("=")[1].split()[0])
    body = hdr[hdr.index(head):hdr.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in mirror._fields_] == ["mapScale", "mapOffset", "scale", "pixelSize", "noise", "tail", "undefined", "reserved"]
    assert [C.sizeof(f[1]) for f in mirror._fields_] == [8, 8, 4, 4, 4, 4, 4, 4]  # the two doubles first: no padding
    assert [getattr(mirror, f[0]).offset for f in mirror._fields_] == [0, 8, 16, 20, 24, 28, 32, 36]


# ---------------------------------------------------------------------------------------------------------------------- status codes
def _err():
    return _lib.lib().octpipe_last_error().decode()


def test_argument_checks_come_before_the_handle():
    L = _lib.lib()
    reg = _lib.StatsRegion(0xFFFFFFFF, 0, 4, 0, 1, 0, 8)
    surf = np.zeros(4, np.int32)
    outf = np.zeros(64, np.float64)
    vol = np.zeros(64, np.float32)
    gain = np.ones(8, np.float32)
    sp, fp, vp, gp = (C.c_void_p(x.ctypes.data) for x in (surf, outf, vol, gain))
    E = _lib.SurfaceEnfaceSettings
    nan, inf = float("nan"), float("inf")

    def S(a=1.0, b=0.0, scale=0, pixel=0.01, noise=0.0, tail=0.0, undefined=nan, reserved=0):
        return _lib.AttenuationSettings(a, b, scale, pixel, noise, tail, undefined, reserved)

    good, slab = S(), E(0, 1, 0, 0.0)

    def ref(x):
        return None if x is None else C.byref(x)

    def volume(s=good, r=reg, out=fp, g=None, gdev=0):
        return L.octpipe_attenuation(None, vp, 0, ref(r), ref(s), g, gdev, out, 0)

    def sums(s=good, r=reg, out=fp, g=None, gdev=0):
        return L.octpipe_debug_attenuation_sums(None, vp, 0, ref(r), ref(s), g, gdev, out, 0)

    def enface(s=good, r=reg, out=fp, g=None, gdev=0, surface=sp, sdev=0, e=slab):
        return L.octpipe_attenuation_enface(None, vp, 0, ref(r), ref(s), g, gdev, surface, sdev, ref(e), out, 0)

    tiny = 2.0 ** -149  # the smallest float32 denormal
    common = (("scale", dict(s=S(scale=3))), ("scale", dict(s=S(scale=-1))),
              ("pixelSize", dict(s=S(pixel=0.0))), ("pixelSize", dict(s=S(pixel=-1.0))), ("pixelSize", dict(s=S(pixel=inf))),
              ("pixelSize", dict(s=S(pixel=nan))),
              ("noise", dict(s=S(noise=nan))), ("tail", dict(s=S(tail=nan))), ("tail", dict(s=S(tail=-tiny))),
              ("mapScale", dict(s=S(a=inf))), ("mapScale", dict(s=S(a=nan))), ("mapOffset", dict(s=S(b=-inf))), ("mapOffset", dict(s=S(b=nan))),
              ("reserved", dict(s=S(reserved=1))), ("depthGain", dict(g=None, gdev=1)),
              ("settings", dict(s=None)), ("region", dict(r=None)), ("out", dict(out=None)),
              ("buffer", dict(r=_lib.StatsRegion(3, 0, 4, 0, 1, 0, 8))))  # a slot with a caller buffer
    for call in (volume, sums, enface):
        for word, kw in common:
            assert call(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (call.__name__, word, _err())
        # the accepted ends of every range reach the handle check
        for s in (good, S(scale=2, pixel=tiny, noise=-inf, tail=inf, undefined=-0.0), S(scale=1, pixel=3e38, noise=inf, tail=0.0),
                  S(a=-1.7e308, b=1.7e308, noise=-1.0, tail=tiny), S(a=0.0, b=-0.0, undefined=inf)):
            assert call(s=s) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (call.__name__, _err())
        for kw in (dict(g=gp, gdev=0), dict(g=gp, gdev=1), dict(r=_lib.StatsRegion(0, 0, 4, 0, 1, 0, 8))):
            assert call(**kw) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (call.__name__, _err())
    for word, kw in (("thickness", dict(e=E(0, 0, 0, 0.0))), ("thickness", dict(e=E(0, 4097, 0, 0.0))), ("function", dict(e=E(0, 1, 2, 0.0))),
                     ("function", dict(e=E(0, 1, -1, 0.0))), ("settings", dict(e=None)), ("surface", dict(surface=None, sdev=1))):
        assert enface(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (word, _err())
    for kw in (dict(surface=None), dict(e=E(-5, 4096, 1, nan)), dict(e=E(2 ** 31 - 1, 1, 0, 0.0))):
        assert enface(**kw) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), _err()
    ms = C.c_double()
    assert L.octpipe_debug_attenuation(None, vp, 0, C.byref(reg), C.byref(S(scale=3)), None, 0, fp, 0, C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert "scale" in _err()
    assert L.octpipe_debug_attenuation(None, vp, 0, C.byref(reg), C.byref(good), None, 0, fp, 0, C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert _err().endswith("null handle")
    args = (None, vp, 0, C.byref(reg), C.byref(good), None, 0, sp, 0)
    assert L.octpipe_debug_attenuation_enface(*args, C.byref(E(0, 0, 0, 0.0)), fp, 0, C.byref(ms)) == ERR_INVALID_ARGUMENT and "thickness" in _err()
    assert L.octpipe_debug_attenuation_enface(*args, C.byref(slab), fp, 0, C.byref(ms)) == ERR_INVALID_ARGUMENT and _err().endswith("null handle")


# ---------------------------------------------------------------------------------------------------------------------- the model
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _homogeneous(mu, delta, n):
    q = np.exp(-2.0 * mu * delta)
    I = q ** np.arange(n, dtype=np.float64)
    return q, I


def test_homogeneous_medium():
    """I_i = q^i with q = exp(-2 mu Delta) and the exact tail I_{n-1} q / (1 - q): every bin gives (1 - q) / (2 Delta q), from intensity,
    amplitude and decibel input alike.  The bound is the float32 rounding of input, tail and output, a few 2^-24."""
    mu, delta, n = 2.0, 0.005, 300
    q, I = _homogeneous(mu, delta, n)
    want = (1.0 - q) / (2.0 * delta * q)
    tail = I[-1] * q / (1.0 - q)
    region = (0, 1, 0, 1, 0, n)
    inputs = (("intensity", at.INTENSITY, I, 1.0), ("amplitude", at.AMPLITUDE, np.sqrt(I), 1.0),
              ("log", at.LOG2, 10.0 * np.log10(I), np.log2(10.0) / 10.0))
    for name, scale, values, a in inputs:
        vol = values.astype(np.float32).reshape(1, 1, n)
        got = at.attenuation(vol, region, delta, scale, a=a, tail=tail).astype(np.float64)
        rel = float(np.max(np.abs(got / want - 1.0)))
        print("homogeneous medium, %s input: max relative error %.3g" % (name, rel))
        assert rel < 1e-6, (name, rel)
    # nothing known below the window: the last bin has nothing under it, the one above it only the last
    vol = I.astype(np.float32).reshape(1, 1, n)
    for undefined in (np.float32(-7.0), np.float32(-0.0), np.array(0x7FC12345, np.uint32).view(np.float32)):
        got = at.attenuation(vol, region, delta, undefined=undefined)[0, 0]
        assert _bits(got[-1]) == _bits(undefined)
        i2, i1 = np.float64(vol[0, 0, -2]), np.float64(vol[0, 0, -1])
        assert got[-2] == np.float32(i2 / ((2.0 * np.float64(np.float32(delta))) * i1))
        assert np.all(np.isfinite(got[:-1])) and np.all(got[:-1] > 0)


def test_pow2():
    rng = np.random.default_rng(5)
    y = rng.uniform(-60.0, 60.0, 200000)
    got, want = at.pow2(y), np.exp2(y)
    ulp = np.abs(got - want) / np.spacing(want)
    print("pow2 against numpy.exp2 on [-60, 60]: max %.2f ulp" % ulp.max())
    assert ulp.max() <= 4.0
    k = np.arange(-1000, 1024, dtype=np.float64)
    assert np.array_equal(at.pow2(k), np.ldexp(1.0, k.astype(np.int32)))  # exact at integers
    assert at.pow2(-0.0) == 1.0 and abs(at.pow2(0.5) - np.sqrt(2.0)) <= 2 * np.spacing(np.sqrt(2.0))
    # the guards
    assert at.pow2(1024.0) == np.inf and at.pow2(np.inf) == np.inf and at.pow2(np.nextafter(1024.0, 0.0)) < np.inf
    assert at.pow2(np.nextafter(-1000.0, -np.inf)) == 0.0 and at.pow2(-np.inf) == 0.0 and at.pow2(-1000.0) == np.ldexp(1.0, -1000)
    assert not np.signbit(at.pow2(-2000.0))
    assert np.isnan(at.pow2(np.nan))


def test_special_values():
    inf, nan = np.inf, np.nan
    # NaN, -inf, negatives and -0 are +0; +inf stays; the noise is subtracted before the clamp
    v = np.array([nan, -inf, -3.0, -0.0, 0.0, 2.0, inf], np.float32)
    assert np.array_equal(at.intensity(v), [0.0, 0.0, 0.0, 0.0, 0.0, 2.0, inf]) and not np.any(np.signbit(at.intensity(v)))
    assert np.array_equal(at.intensity(v, noise=2.0), [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf])
    assert np.array_equal(at.intensity(v, at.AMPLITUDE), [0.0, inf, 9.0, 0.0, 0.0, 4.0, inf])
    assert np.array_equal(at.intensity(v, at.LOG2), [0.0, 0.0, 0.125, 1.0, 1.0, 4.0, inf])
    # a NaN bin does not poison the A-scan above it
    vol = np.array([1.0, 2.0, nan, 4.0, 8.0], np.float32).reshape(1, 1, 5)
    region, delta = (0, 1, 0, 1, 0, 5), 0.5
    got = at.attenuation(vol, region, delta, undefined=-1.0)[0, 0]
    assert np.array_equal(got, np.array([1.0 / 14.0, 2.0 / 12.0, 0.0, 4.0 / 8.0, -1.0], np.float32))
    assert np.array_equal(at.sums(vol, region)[0, 0], [14.0, 12.0, 12.0, 8.0, 0.0])
    # an all-zero A-scan (-0 and values the noise removes included): every bin undefined, bits as given
    vol = np.array([0.0, -0.0, 0.5, -2.0, nan], np.float32).reshape(1, 1, 5)
    for undefined in (np.float32(-0.0), np.array(0xFFC00001, np.uint32).view(np.float32), np.float32(3.0)):
        got = at.attenuation(vol, region, delta, noise=0.5, undefined=undefined)
        assert np.all(at.bits(got) == _bits(undefined))
    # ... unless a tail lies below it
    got = at.attenuation(vol, region, delta, noise=0.5, tail=2.0, undefined=-1.0)
    assert np.all(at.bits(got) == 0)
    # two infinities: above the deeper one everything is finite / inf = +0 or inf / inf = NaN (canonical); the deeper one itself is inf /
    # finite = inf
    vol = np.array([1.0, inf, 3.0, inf, 5.0, 6.0], np.float32).reshape(1, 1, 6)
    got = at.attenuation(vol, (0, 1, 0, 1, 0, 6), delta, undefined=-1.0)[0, 0]
    assert [_bits(x) for x in got] == [0, NAN_BITS, 0, _bits(inf), _bits(5.0 / 6.0), _bits(-1.0)]
    # an inf tail: 0 for every finite bin
    got = at.attenuation(vol[:, :, 4:], (0, 1, 0, 1, 0, 2), delta, tail=inf)[0, 0]
    assert [_bits(x) for x in got] == [0, 0]
    # float32 denormal input and output
    d = np.float32(3e-41)
    vol = np.array([d, 1.0], np.float32).reshape(1, 1, 2)
    got = at.attenuation(vol, (0, 1, 0, 1, 0, 2), delta)[0, 0]
    assert got[0] == np.float32(np.float64(d)) and 0.0 < got[0] < np.finfo(np.float32).tiny


def test_gain_and_noise_in_the_defined_order():
    v = np.array([5.0, 3.0, 1.0], np.float32)
    g = np.array([2.0, -1.0, 0.5], np.float32)
    # (v - noise) * g, not v * g - noise; a negative gain gives +0
    assert np.array_equal(at.intensity(v, noise=2.0, gain=g), [6.0, 0.0, 0.0])
    assert np.array_equal(at.intensity(v, noise=-1.0, gain=g), [12.0, 0.0, 1.0])
    assert np.array_equal(at.intensity(v, at.AMPLITUDE, a=2.0, b=1.0, noise=9.0, gain=g), [224.0, 0.0, 0.0])  # ((2 v + 1)^2 - 9) g
    # inf * 0 is NaN is +0
    assert np.array_equal(at.intensity(np.array([np.inf], np.float32), gain=np.array([0.0], np.float32)), [0.0])
    # every product is rounded before it is added: v * a + b with a product that needs more than 53 bits
    a, b = 1.0 + 2.0 ** -30, -1.0
    v = np.float32(1.0 + 2.0 ** -23)
    fused = float(Fraction(float(v)) * Fraction(a) + Fraction(b))
    rounded = float(np.float64(v) * np.float64(a)) + b
    assert at.intensity(np.array([v], np.float32), a=a, b=b)[0] == rounded != fused
    vol = np.array([4.0, 2.0, 1.0], np.float32).reshape(1, 1, 3)
    got = at.attenuation(vol, (0, 1, 0, 1, 0, 3), 0.25, tail=1.0, gain=np.array([1.0, 2.0, 3.0], np.float32))[0, 0]
    assert np.array_equal(got, np.array([4.0 / (0.5 * 8.0), 4.0 / (0.5 * 4.0), 3.0 / 0.5], np.float32))


def wide_range_values(rng, shape):
    """chi-squared (one degree of freedom) speckle times exp(U(-20, 20)): positive, over seventeen decades"""
    return (rng.standard_normal(shape) ** 2 * np.exp(rng.uniform(-20.0, 20.0, shape))).astype(np.float32)


def test_the_defined_order_is_not_a_running_sum():
    """what gives the GPU test of the float64 sums its teeth: on that test's kind of data the defined order and one running sum from the deep
    end disagree in most bins"""
    I = at.intensity(wide_range_values(np.random.default_rng(11), (2000, 300)))
    a, b = at.below_sums(I, 0.25), at.running_sums(I, 0.25)
    differ = float(np.mean(a.view(np.uint64) != b.view(np.uint64)))
    print("defined order against a running sum: %.1f %% of the float64 sums differ" % (100 * differ))
    assert differ > 0.1
    assert np.allclose(a, b, rtol=1e-12, atol=0.0)  # (the same sums up to rounding)
    # lanes, pieces and chunks where the definition puts them: bin 256 k + 4 l + j, the carry crossing chunk borders
    n = 700
    I = np.zeros((1, n))
    I[0, [3, 255, 256, 511, 512, 699]] = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    s = at.below_sums(I, 64.0)[0]
    assert s[699] == 64.0 and s[698] == 96.0 and s[512] == 96.0 and s[511] == 112.0 and s[510] == 120.0 and s[256] == 120.0
    assert s[255] == 124.0 and s[254] == 126.0 and s[3] == 126.0 and s[2] == 127.0 and s[0] == 127.0


def test_enface_is_the_surface_views_enface_of_the_volume():
    import surface_model as sm
    rng = np.random.default_rng(3)
    vol = wide_range_values(rng, (3, 4, 90))
    vol[1, 2, 40] = np.nan
    region = (1, 2, 1, 3, 5, 80)
    surface = rng.integers(0, 90, (2, 3)).astype(np.int32)
    surface[0, 1] = -2
    kw = dict(scale=at.AMPLITUDE, a=0.5, b=0.1, noise=1e-3, tail=2.0)
    mu = np.zeros_like(vol)
    mu[1:3, 1:4, 5:85] = at.attenuation(vol, region, 0.01, **kw)
    for fn, offset, thickness in ((0, 0, 16), (1, 3, 70), (0, -4, 9), (1, 70, 65), (0, 90, 3), (0, -95, 9)):
        got = at.attenuation_enface(vol, region, 0.01, surface, offset, thickness, fn, -2.0, **kw)
        assert np.array_equal(at.bits(got), at.bits(sm.enface(mu, region, surface, offset, thickness, fn, -2.0))) and got.shape == (2, 3)
        assert got[0, 1] == -2.0
    const = np.full((2, 3), 5, np.int32)
    a = at.attenuation_enface(vol, region, 0.01, None, 7, 20, 0, -2.0, **kw)
    assert np.array_equal(at.bits(a), at.bits(at.attenuation_enface(vol, region, 0.01, const, 7, 20, 0, -2.0, **kw)))


# ---------------------------------------------------------------------------------------------------------------------- kernels
KERNELS = {  # mangled-name pattern: (instances, VGPR limit)
    r"_ZN3oct23oct_atten_volume_kernelILi[0-2]ELb[01]ELb[01]EEEv\w+": (3 * 2 * 2, 128),  # scale x gain x (mu32 | sums)
    r"_ZN3oct23oct_atten_enface_kernelILi[0-2]ELb[01]ELi[01]EEEv\w+": (3 * 2 * 2, 128),  # scale x gain x function
}


def test_attenuation_kernels_need_no_scratch(tmp_path):
    """every attenuation kernel: no private memory (the four intensities and sums of a lane stay in registers), at most 128 VGPRs for the
    volume kernels; the six steps of the lane scan are two 32-bit cross-lane moves each, plus one pair for t_{l+1}; no fused multiply-add
    outside the division's own sequence"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "attenuation.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "attenuation_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    for pattern, (count, limit) in KERNELS.items():
        names = re.findall(r"^(%s):" % pattern, text, re.M)
        assert len(names) == count, (pattern, names)
        for name in names:
            meta = text[text.index(name + ":"):]
            scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
            vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
            print(name, "VGPRs", vgprs, "SGPRs", int(re.search(r"; TotalNumSgprs: (\d+)", meta).group(1)))
            assert scratch == 0 and vgprs <= limit, (name, scratch, vgprs)
            body = meta[:meta.index("s_endpgm")]
            moves = len(re.findall(r"^\s+ds_bpermute_b32", body, re.M))  # (the compiler may lay the chunk's code out more than once)
            assert moves >= 14 and moves % 14 == 0, (name, moves)
            # the intensity, the sums and the product 2 Delta * below are separate multiplies and adds; what fused multiply-adds there
            # are belong to the four float64 divisions (and the one of the en face average)
            fused = len(re.findall(r"^\s+v_fma(c)?_f64", body, re.M))
            divisions = len(re.findall(r"^\s+v_div_fixup_f64", body, re.M))
            assert fused <= 7 * divisions, (name, fused, divisions)

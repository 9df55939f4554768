"""Angiography without a device (include/octpipe.h "angiography"): the ABI surface, the status codes of calls that need no device, the
numpy model (tests/angio_model.py) against closed forms, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import angio_model as am
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT = 1
NAN_BITS = 0x7FC00000

PUBLIC = ("octpipe_angiogram", "octpipe_angiogram_enface")
DEBUG = ("octpipe_debug_angiogram", "octpipe_debug_angiogram_enface")


# ---------------------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name), name
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name), name


def test_struct_layout():
    struct, mirror, stated = "OctPipeAngioSettings", _lib.AngioSettings, "5 x 4 = 20 bytes"
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
    assert names == [f[0] for f in mirror._fields_] == ["repeats", "method", "mask", "threshold", "masked"]
    assert all(C.sizeof(f[1]) == 4 for f in mirror._fields_)


# ---------------------------------------------------------------------------------------------------------------------- status codes
def _err():
    return _lib.lib().octpipe_last_error().decode()


def test_argument_checks_come_before_the_handle():
    L = _lib.lib()
    reg = _lib.StatsRegion(0xFFFFFFFF, 0, 4, 0, 1, 0, 8)
    surf = np.zeros(4, np.int32)
    outf = np.zeros(64, np.float32)
    vol = np.zeros(64, np.float32)
    sp, fp, vp = (C.c_void_p(x.ctypes.data) for x in (surf, outf, vol))
    S, E = _lib.AngioSettings, _lib.SurfaceEnfaceSettings
    good, slab = S(2, 0, 0, 0.0, 0.0), E(0, 1, 0, 0.0)
    nan = float("nan")

    def ref(x):
        return None if x is None else C.byref(x)

    def volume(s=good, r=reg, out=fp):
        return L.octpipe_angiogram(None, vp, 0, ref(r), ref(s), out, None, 0)

    def enface(s=good, r=reg, out=fp, surface=sp, sdev=0, e=slab):
        return L.octpipe_angiogram_enface(None, vp, 0, ref(r), ref(s), surface, sdev, ref(e), out, 0)

    common = (("repeats", dict(s=S(1, 0, 0, 0.0, 0.0))), ("repeats", dict(s=S(9, 0, 0, 0.0, 0.0))), ("repeats", dict(s=S(0, 0, 0, 0.0, 0.0))),
              ("repeats", dict(s=S(3, 0, 0, 0.0, 0.0))),  # 3 does not divide the 4 B-scans
              ("method", dict(s=S(2, 3, 0, 0.0, 0.0))), ("method", dict(s=S(2, -1, 0, 0.0, 0.0))),
              ("threshold", dict(s=S(2, 0, 1, nan, 0.0))), ("settings", dict(s=None)), ("region", dict(r=None)), ("out", dict(out=None)),
              ("buffer", dict(r=_lib.StatsRegion(3, 0, 4, 0, 1, 0, 8))))  # a slot with a caller buffer
    for call in (volume, enface):
        for word, kw in common:
            assert call(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (call.__name__, word, _err())
        # the accepted ends of every range reach the handle check
        for s in (good, S(8, 2, 0, nan, 0.0), S(4, 1, 1, float("inf"), nan), S(2, 0, 1, -float("inf"), 0.0)):
            r = _lib.StatsRegion(0, 0, 8, 0, 1, 0, 8)
            assert call(s=s, r=r) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (call.__name__, _err())
    for word, kw in (("thickness", dict(e=E(0, 0, 0, 0.0))), ("thickness", dict(e=E(0, 4097, 0, 0.0))), ("function", dict(e=E(0, 1, 2, 0.0))),
                     ("function", dict(e=E(0, 1, -1, 0.0))), ("settings", dict(e=None)), ("surface", dict(surface=None, sdev=1))):
        assert enface(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (word, _err())
    for kw in (dict(surface=None), dict(e=E(-5, 4096, 1, nan))):
        assert enface(**kw) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), _err()
    ms = C.c_double()
    assert L.octpipe_debug_angiogram(None, vp, 0, C.byref(reg), C.byref(S(9, 0, 0, 0.0, 0.0)), fp, None, 0, C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert "repeats" in _err()
    def debug_enface(e, form):
        return L.octpipe_debug_angiogram_enface(None, vp, 0, C.byref(reg), C.byref(good), sp, 0, C.byref(e), fp, 0, form, C.byref(ms))

    assert debug_enface(E(0, 0, 0, 0.0), 0) == ERR_INVALID_ARGUMENT and "thickness" in _err()
    for e, form in ((slab, 3), (E(0, 65, 0, 0.0), 2)):  # an unknown form; the team form beyond its 64 bins
        assert debug_enface(e, form) == ERR_INVALID_ARGUMENT and "form" in _err() and "null handle" not in _err(), (form, _err())
    for e, form in ((slab, 1), (slab, 2), (E(0, 64, 1, 0.0), 2), (E(0, 4096, 0, 0.0), 1)):
        assert debug_enface(e, form) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (form, _err())
    assert L.octpipe_debug_angiogram(None, vp, 0, C.byref(reg), C.byref(good), fp, None, 0, C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert _err().endswith("null handle")


# ---------------------------------------------------------------------------------------------------------------------- the model
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_equal_repeats_have_no_contrast():
    for M in range(2, 9):
        for value in (1.0, -3.25, 1e-30, 7e20):
            for method in (am.VARIANCE, am.DECORRELATION, am.DIFFERENCE):
                c, mu = am.bin_contrast([value] * M, method)
                assert c == 0.0 and mu == np.float32(value), (M, value, method, c, mu)


def test_repeats_one_and_three():
    assert am.bin_contrast([1.0, 3.0], am.VARIANCE) == (np.float32(1.0), np.float32(2.0))
    c, mu = am.bin_contrast([1.0, 3.0], am.DECORRELATION)
    assert c == np.float32(1.0 - 3.0 / 5.0) and mu == np.float32(2.0)
    assert am.bin_contrast([1.0, 3.0], am.DIFFERENCE)[0] == np.float32(2.0)
    # the neighbouring pairs of three repeats: (|3 - 1| + |0 - 3|) / 2; variance about the mean 4 / 3
    assert am.bin_contrast([1.0, 3.0, 0.0], am.DIFFERENCE)[0] == np.float32(2.5)
    mu = (np.float64(1.0) + 3.0 + 0.0) / 3.0
    want = (((1.0 - mu) * (1.0 - mu) + (3.0 - mu) * (3.0 - mu)) + (0.0 - mu) * (0.0 - mu)) / 3.0
    assert am.bin_contrast([1.0, 3.0, 0.0], am.VARIANCE)[0] == np.float32(want)
    # both values zero: t = 1, decorrelation 0
    assert _bits(am.bin_contrast([0.0, 0.0], am.DECORRELATION)[0]) == 0
    assert _bits(am.bin_contrast([0.0, -0.0, 0.0], am.DECORRELATION)[0]) == 0
    # one value zero: t = 0, decorrelation 1; opposite signs: t = -1, decorrelation 2
    assert am.bin_contrast([0.0, 5.0], am.DECORRELATION)[0] == np.float32(1.0)
    assert am.bin_contrast([2.0, -2.0], am.DECORRELATION)[0] == np.float32(2.0)


def test_nan_inf_and_the_mask():
    inf, nan = np.inf, np.nan
    for method in (am.VARIANCE, am.DECORRELATION, am.DIFFERENCE):
        c, mu = am.bin_contrast([1.0, nan, 2.0], method)
        assert _bits(c) == NAN_BITS and _bits(mu) == NAN_BITS
        c, mu = am.bin_contrast([1.0, inf], method)  # inf - inf in the variance, inf / inf in the decorrelation; |inf - 1| = inf
        assert (c == np.float32(inf) if method == am.DIFFERENCE else _bits(c) == NAN_BITS) and mu == np.float32(inf)
    c, mu = am.bin_contrast([inf, -inf], am.DIFFERENCE)
    assert c == np.float32(inf) and _bits(mu) == NAN_BITS
    # a float32 that overflows only when rounded to float32
    big = np.float32(3e38)
    assert am.bin_contrast([big, -big], am.VARIANCE)[0] == np.float32(inf) and am.bin_contrast([big, big], am.VARIANCE)[1] == big
    # the mask: a strict compare of mu32 with the threshold, `masked` as given
    assert am.bin_contrast([1.0, 3.0], am.VARIANCE, threshold=1.5, masked=-7.0)[0] == np.float32(1.0)
    assert am.bin_contrast([1.0, 3.0], am.VARIANCE, threshold=2.0, masked=-7.0)[0] == np.float32(-7.0)  # equal does not exceed
    assert _bits(am.bin_contrast([1.0, 3.0], am.VARIANCE, threshold=2.0, masked=-0.0)[0]) == 0x80000000
    assert _bits(am.bin_contrast([1.0, 3.0], am.VARIANCE, threshold=inf, masked=nan)[0]) == NAN_BITS
    assert am.bin_contrast([1.0, 3.0], am.VARIANCE, threshold=-inf, masked=-7.0)[0] == np.float32(1.0)
    assert am.bin_contrast([1.0, nan], am.VARIANCE, threshold=-inf, masked=-7.0)[0] == np.float32(-7.0)  # a NaN mean is masked
    assert am.bin_contrast([-inf, -inf], am.DIFFERENCE, threshold=-inf, masked=-7.0)[0] == np.float32(-7.0)  # -inf does not exceed -inf
    assert _bits(am.bin_contrast([inf, inf], am.VARIANCE, threshold=1.0, masked=-7.0)[0]) == NAN_BITS  # an inf mean passes
    # the volume form agrees with the bin form, masked or not
    vol = np.array([[[1.0, nan, 0.0, inf]], [[3.0, 2.0, 0.0, 1.0]]], np.float32)
    for method in (am.VARIANCE, am.DECORRELATION, am.DIFFERENCE):
        for thr in (None, 0.5, inf, -inf):
            out, mean = am.angiogram(vol, am.whole(vol), 2, method, thr, -0.0)
            for k in range(4):
                c, mu = am.bin_contrast([vol[0, 0, k], vol[1, 0, k]], method, thr, -0.0)
                assert _bits(out[0, 0, k]) == _bits(c) and _bits(mean[0, 0, k]) == _bits(mu), (method, thr, k)


def test_denormal_results_are_kept():
    tiny = float(np.finfo(np.float32).tiny)  # the smallest normal float32
    a, b = np.float32(1e-20), np.float32(3e-20)
    c, mu = am.bin_contrast([a, b], am.VARIANCE)
    m = (np.float64(a) + np.float64(b)) / 2.0
    assert 0.0 < c < tiny and c == np.float32(((a - m) * (a - m) + (b - m) * (b - m)) / 2.0)
    d0, d1 = np.float32(3e-41), np.float32(-5e-41)  # denormal inputs
    assert 0.0 < d0 < tiny
    c, mu = am.bin_contrast([d0, d1], am.DIFFERENCE)
    assert c == np.float32(np.float64(d0) - np.float64(d1)) and 0.0 < c < tiny
    assert mu == np.float32((np.float64(d0) + np.float64(d1)) / 2.0) and -tiny < mu < 0.0
    assert am.bin_contrast([d0, d0], am.DECORRELATION)[0] == 0.0  # the products are exact in float64: t = 1


def test_projection_partials_and_ties():
    # 65 bins: x_64 joins L_0 before the partials are added.  With x_0 = 1, x_64 = -1 and 2^-60 elsewhere the sum of the partials is
    # 63 * 2^-60 (L_0 = 0); one running sum in depth order would lose every 2^-60 against the 1 and end at 0.
    tiny = np.float32(2.0 ** -60)
    x = [tiny] * 65
    x[0], x[64] = np.float32(1.0), np.float32(-1.0)
    want = np.float32(np.float64(63 * 2.0 ** -60) / 65.0)
    assert am.project(x, 0) == want
    running = np.float64(0.0)
    for v in x:
        running = running + np.float64(v)
    assert np.float32(running / 65.0) != want
    # 64 bins: one bin per partial, added in increasing j
    x = [np.float32(1.0)] + [tiny] * 63
    assert am.project(x, 0) == np.float32(1.0 / 64.0)  # every 2^-60 is lost against the 1 that comes first
    assert _bits(am.project([np.float32(-0.0)], 0)) == 0x80000000  # the sum starts from the first value, not from +0
    assert _bits(am.project([np.float32(np.inf), np.float32(-np.inf)], 0)) == NAN_BITS
    # MIP: -0 against +0 by depth, NaN wins
    z, n = np.float32(0.0), np.float32(-0.0)
    assert _bits(am.project([n, z, n], 1)) == 0x80000000 and _bits(am.project([z, n], 1)) == 0
    assert _bits(am.project([np.float32(-1.0), n, z], 1)) == 0x80000000
    assert am.project([np.float32(1.0), np.float32(5.0), np.float32(5.0), np.float32(-np.inf)], 1) == np.float32(5.0)
    assert _bits(am.project([np.float32(1.0), np.float32(np.nan), np.float32(np.inf)], 1)) == NAN_BITS
    assert am.project([np.float32(-np.inf)], 1) == np.float32(-np.inf)


def test_fixed_slab_is_the_slab_under_a_constant_surface():
    rng = np.random.default_rng(7)
    vol = rng.standard_normal((6, 4, 90)).astype(np.float32)
    vol[2, 1, 30] = np.nan
    region = (0, 6, 1, 3, 5, 80)
    flat = np.full((6, 3), 5, np.int32)
    for method, fn, offset, thickness in ((0, 0, 0, 16), (1, 1, 3, 70), (2, 0, -4, 9), (0, 1, 70, 65), (2, 0, 80, 3), (1, 0, -9, 9)):
        a = am.angiogram_enface(vol, region, 3, method, None, offset, thickness, fn, -2.0, 0.1, 9.0)
        b = am.angiogram_enface(vol, region, 3, method, flat, offset, thickness, fn, -2.0, 0.1, 9.0)
        assert np.array_equal(am.bits(a), am.bits(b)) and a.shape == (2, 3)
        # ... and the projection of the contrast volume
        out, _ = am.angiogram(vol, region, 3, method, 0.1, 9.0)
        c = am.project_volume(out, region, 3, None, offset, thickness, fn, -2.0)
        assert np.array_equal(am.bits(a), am.bits(c)), (method, fn, offset, thickness)
    assert np.all(am.angiogram_enface(vol, region, 3, 0, None, 80, 3, 0, -2.0) == -2.0)  # wholly below the window
    # only the row of a position's first repeat counts, and a hole there gives the fill
    surface = np.full((6, 3), 20, np.int32)
    surface[1:3] = -1
    surface[3, 2] = -1
    img = am.angiogram_enface(vol, region, 3, 2, surface, 0, 4, 0, -2.0)
    assert img[1, 2] == -2.0 and np.all(img[0] != -2.0) and np.all(img[1, :2] != -2.0)


# ---------------------------------------------------------------------------------------------------------------------- kernels
KERNELS = {  # mangled-name pattern: instances (method [x function] x repeats 2 ... 8)
    r"_ZN3oct23oct_angio_volume_kernelILi[0-2]ELj[2-8]EEEv\w+": 3 * 7,
    r"_ZN3oct23oct_angio_enface_kernelILi[0-2]ELi[01]ELj[2-8]EEEv\w+": 6 * 7,
    r"_ZN3oct28oct_angio_enface_team_kernelILi[0-2]ELi[01]ELj[2-8]EEEv\w+": 6 * 7,
}


def test_angio_kernels_need_no_scratch(tmp_path):
    """every angiography kernel: no private memory (the 4 x M values of a step stay in registers), at most 128 VGPRs; no LDS at all.  In the
    volume kernel's body the M 16-byte loads of a step are issued before the first wait for any of them."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "angiogram.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "angiogram_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    for pattern, count in KERNELS.items():
        names = re.findall(r"^(%s):" % pattern, text, re.M)
        assert len(names) == count, (pattern, names)
        for name in names:
            meta = text[text.index(name + ":"):]
            scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
            lds = int(re.search(r"; LDSByteSize: (\d+)", meta).group(1))
            vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
            print(name, "VGPRs", vgprs, "SGPRs", int(re.search(r"; TotalNumSgprs: (\d+)", meta).group(1)))
            assert scratch == 0 and lds == 0 and vgprs <= 128, (name, scratch, lds, vgprs)
    # all M loads of a step in flight before the first arithmetic: in every volume kernel some run of M 16-byte loads has no wait inside
    for name in re.findall(r"^(_ZN3oct23oct_angio_volume_kernel\w+):", text, re.M):
        M = int(re.search(r"ELj(\d)E", name).group(1))
        body = text[text.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        ops = re.findall(r"^\s+(global_load_dwordx4|s_waitcnt vmcnt)", body, re.M)
        runs = "".join("L" if op.startswith("global") else "w" for op in ops)
        assert "L" * M + "w" in runs and "LwL" not in runs, (name, runs)

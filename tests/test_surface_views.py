"""Surface views without a device (include/octpipe.h "surface views"): the ABI surface, the status codes of calls that need no device,
the numpy model (tests/surface_model.py) against closed forms, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surface_model as sm
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT = 1

PUBLIC = ("octpipe_surface_detect", "octpipe_surface_smooth", "octpipe_surface_enface", "octpipe_flatten")
DEBUG = ("octpipe_debug_surface_detect", "octpipe_debug_surface_smooth", "octpipe_debug_surface_enface", "octpipe_debug_flatten")


# ---------------------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name), name
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name), name


@pytest.mark.parametrize("struct,mirror,stated", [("OctPipeSurfaceDetectSettings", _lib.SurfaceDetectSettings, "2 x 4 = 8 bytes"),
                                                  ("OctPipeSurfaceEnfaceSettings", _lib.SurfaceEnfaceSettings, "4 x 4 = 16 bytes"),
                                                  ("OctPipeFlattenSettings", _lib.FlattenSettings, "3 x 4 = 12 bytes")])
def test_struct_layouts(struct, mirror, stated):
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
    assert names == [f[0] for f in mirror._fields_]
    assert all(C.sizeof(f[1]) == 4 for f in mirror._fields_)


# ---------------------------------------------------------------------------------------------------------------------- status codes
def _err():
    return _lib.lib().octpipe_last_error().decode()


def test_argument_checks_come_before_the_handle():
    L = _lib.lib()
    reg = _lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, 8)
    surf = np.zeros(4, np.int32)
    outi = np.zeros(4, np.int32)
    outf = np.zeros(64, np.float32)
    vol = np.zeros(64, np.float32)
    sp, op, fp, vp = (C.c_void_p(x.ctypes.data) for x in (surf, outi, outf, vol))
    D, E, F = _lib.SurfaceDetectSettings, _lib.SurfaceEnfaceSettings, _lib.FlattenSettings

    def detect(s, r=reg, out=op):
        return L.octpipe_surface_detect(None, vp, 0, None if r is None else C.byref(r), None if s is None else C.byref(s), out, 0)

    for s, r, out, word in ((D(1.0, 0), reg, op, "run"), (D(1.0, 65), reg, op, "run"), (D(float("nan"), 1), reg, op, "threshold"),
                            (None, reg, op, "settings"), (D(1.0, 1), None, op, "region"), (D(1.0, 1), reg, None, "surface")):
        assert detect(s, r, out) == ERR_INVALID_ARGUMENT and word in _err(), word
    assert detect(D(1.0, 1)) == ERR_INVALID_ARGUMENT and "null handle" in _err()

    def smooth(rows, cols, radius, src=sp, out=op):
        return L.octpipe_surface_smooth(None, src, 0, rows, cols, radius, out, 0)

    for args, word in (((2, 2, 4), "radius"), ((0, 2, 1), "rows"), ((2, 0, 1), "cols"), ((1 << 15, 1 << 14, 1), "2^28"),
                       ((2, 2, 1, sp, sp), "out"), ((2, 2, 1, None, op), "surface"), ((2, 2, 1, sp, None), "out")):
        assert smooth(*args) == ERR_INVALID_ARGUMENT and word in _err(), word
    assert smooth(2, 2, 1) == ERR_INVALID_ARGUMENT and "null handle" in _err()

    def enface(s, surface=sp, out=fp):
        return L.octpipe_surface_enface(None, vp, 0, C.byref(reg), surface, 0, None if s is None else C.byref(s), out, 0)

    for s, surface, out, word in ((E(0, 0, 0, 0.0), sp, fp, "thickness"), (E(0, 4097, 0, 0.0), sp, fp, "thickness"), (E(0, 1, 2, 0.0), sp, fp, "function"),
                                  (E(0, 1, -1, 0.0), sp, fp, "function"), (None, sp, fp, "settings"), (E(0, 1, 0, 0.0), None, fp, "surface"),
                                  (E(0, 1, 0, 0.0), sp, None, "out")):
        assert enface(s, surface, out) == ERR_INVALID_ARGUMENT and word in _err(), word
    assert enface(E(0, 1, 0, 0.0)) == ERR_INVALID_ARGUMENT and "null handle" in _err()

    def flatten(s, surface=sp, out=fp):
        return L.octpipe_flatten(None, vp, 0, C.byref(reg), surface, 0, None if s is None else C.byref(s), out, 0)

    for s, surface, out, word in ((F(0, 0, 0.0), sp, fp, "outDepth"), (F(0, 8193, 0.0), sp, fp, "outDepth"), (None, sp, fp, "settings"),
                                  (F(0, 8, 0.0), None, fp, "surface"), (F(0, 8, 0.0), sp, None, "out")):
        assert flatten(s, surface, out) == ERR_INVALID_ARGUMENT and word in _err(), word
    assert flatten(F(0, 8, 0.0)) == ERR_INVALID_ARGUMENT and "null handle" in _err()
    ms = C.c_double()
    assert L.octpipe_debug_flatten(None, vp, 0, C.byref(reg), sp, 0, C.byref(F(0, 8, 0.0)), fp, 0, 3, C.byref(ms)) == ERR_INVALID_ARGUMENT and "loads" in _err()
    bad = _lib.StatsRegion(3, 0, 1, 0, 1, 0, 8)  # a slot with a caller buffer
    assert L.octpipe_flatten(None, vp, 0, C.byref(bad), sp, 0, C.byref(F(0, 8, 0.0)), fp, 0) == ERR_INVALID_ARGUMENT and "buffer" in _err()


# ---------------------------------------------------------------------------------------------------------------------- the model
def _volume(b=2, a=5, depth=40, seed=1):
    return np.random.default_rng(seed).standard_normal((b, a, depth)).astype(np.float32)


def test_flatten_with_a_constant_surface_at_the_anchor_is_the_identity_on_the_window():
    vol = _volume()
    region = (0, 2, 1, 3, 4, 30)
    for anchor in (4, 17, 33):  # the surface anywhere inside the window
        surface = np.full((2, 3), anchor, np.int32)
        flat = sm.flatten(vol, region, surface, anchor, 40, np.nan)
        assert np.array_equal(sm.bits(flat[:, :, 4:34]), sm.bits(vol[:, 1:4, 4:34]))
        assert np.isnan(flat[:, :, :4]).all() and np.isnan(flat[:, :, 34:]).all()  # outside the window: the fill
    # shifted by one: row j holds bin j + 1
    flat = sm.flatten(vol, sm.whole(vol), np.full((2, 5), 11, np.int32), 10, 40, -1.0)
    assert np.array_equal(flat[:, :, :39], vol[:, :, 1:]) and np.all(flat[:, :, 39] == -1.0)
    # no surface: the fill
    assert np.all(sm.flatten(vol, sm.whole(vol), np.full((2, 5), -7, np.int32), 0, 3, 5.0) == 5.0)


def test_a_slab_of_one_bin_at_the_surface_is_the_value_there():
    vol = _volume(seed=2)
    rng = np.random.default_rng(3)
    surface = rng.integers(0, 40, (2, 5)).astype(np.int32)
    want = np.take_along_axis(vol, surface[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    for fn in (0, 1):
        assert np.array_equal(sm.bits(sm.enface(vol, sm.whole(vol), surface, 0, 1, fn, 0.0)), sm.bits(want))
    # averaging is the float64 mean rounded once; the slab is clipped to the window; outside it the fill
    v = np.arange(40, dtype=np.float32)[None, None, :]
    s = np.array([[10]], np.int32)
    assert sm.enface(v, (0, 1, 0, 1, 0, 40), s, 2, 5, 0, 0.0)[0, 0] == np.float32(14.0)
    assert sm.enface(v, (0, 1, 0, 1, 0, 40), s, 2, 5, 1, 0.0)[0, 0] == np.float32(16.0)
    assert sm.enface(v, (0, 1, 0, 1, 5, 9), s, 2, 5, 0, 0.0)[0, 0] == np.float32(12.5)  # bins 12, 13 of the window 5 .. 13
    assert sm.enface(v, (0, 1, 0, 1, 5, 9), s, 4, 5, 0, -3.0)[0, 0] == np.float32(-3.0)
    assert sm.enface(v, (0, 1, 0, 1, 5, 9), np.array([[-1]], np.int32), 0, 5, 1, -3.0)[0, 0] == np.float32(-3.0)
    w = np.array([[[1.0, np.nan, 3.0, -0.0, 0.0, np.inf, -np.inf]]], np.float32)
    r = (0, 1, 0, 1, 0, 7)
    z = np.array([[0]], np.int32)
    assert sm.bits(sm.enface(w, r, z, 0, 3, 1, 0.0))[0, 0] == 0x7FC00000 and sm.bits(sm.enface(w, r, z, 0, 3, 0, 0.0))[0, 0] == 0x7FC00000
    assert sm.bits(sm.enface(w, r, z, 3, 2, 1, 1.0))[0, 0] == 0x80000000  # -0 first, +0 does not exceed it
    assert sm.bits(sm.enface(w, r, z, 5, 2, 0, 1.0))[0, 0] == 0x7FC00000  # inf - inf, canonical


def test_median_of_a_ramp():
    ramp = (3 * np.arange(9)[:, None] + np.arange(11)[None, :]).astype(np.int32)
    for radius in (0, 1, 2, 3):
        out = sm.smooth(ramp, radius)
        inner = (slice(radius, 9 - radius), slice(radius, 11 - radius))
        assert np.array_equal(out[inner], ramp[inner])  # a full window of a plane: its centre
    # a clipped window of even size takes the LOWER of the two middle entries; holes do not count
    line = np.array([[5, 1, 9, -1, 7]], np.int32)
    assert sm.smooth(line, 1).tolist() == [[1, 5, 1, 7, 7]]
    assert sm.smooth(line, 0).tolist() == [[5, 1, 9, -1, 7]]
    assert sm.smooth(np.array([[-5, -1], [-2, -9]], np.int32), 2).tolist() == [[-1, -1], [-1, -1]]
    assert sm.smooth(np.array([[-5, 4], [-2, -9]], np.int32), 1).tolist() == [[4, 4], [4, 4]]


def test_a_run_broken_by_one_bin():
    v = np.zeros((1, 1, 30), np.float32)
    v[0, 0, 5:9] = 2.0    # four bins above
    v[0, 0, 10:16] = 2.0  # one bin below, then six above
    r = sm.whole(v)
    assert [int(sm.detect(v, r, 1.0, run)[0, 0]) for run in (1, 4, 5, 6, 7)] == [5, 5, 10, 10, -1]
    assert int(sm.detect(v, r, 2.0, 1)[0, 0]) == -1  # equal to the threshold is not above it
    assert int(sm.detect(v, (0, 1, 0, 1, 6, 24), 1.0, 3)[0, 0]) == 6 and int(sm.detect(v, (0, 1, 0, 1, 7, 23), 1.0, 3)[0, 0]) == 10
    assert int(sm.detect(v, (0, 1, 0, 1, 0, 15), 1.0, 5)[0, 0]) == 10 and int(sm.detect(v, (0, 1, 0, 1, 0, 14), 1.0, 5)[0, 0]) == -1
    v[0, 0, 12] = np.nan
    assert int(sm.detect(v, r, 1.0, 3)[0, 0]) == 5 and int(sm.detect(v, r, 1.0, 5)[0, 0]) == -1
    v[0, 0, 12] = np.inf
    assert int(sm.detect(v, r, 1.0, 5)[0, 0]) == 10


def test_flatten_then_a_fixed_slab_is_the_surface_slab():
    vol = _volume(3, 6, 50, seed=5)
    surface = np.random.default_rng(6).integers(8, 30, (3, 6)).astype(np.int32)
    surface[1, 2] = -1
    for fn in (0, 1):
        flat = sm.flatten(vol, sm.whole(vol), surface, 12, 40, 0.0)
        assert np.array_equal(sm.bits(sm.fixed_slab(flat, 12 - 3, 9, fn, 0.0)), sm.bits(sm.enface(vol, sm.whole(vol), surface, -3, 9, fn, 0.0)))


# ---------------------------------------------------------------------------------------------------------------------- kernels
KERNELS = {  # mangled-name pattern: (instances, most VGPRs)
    r"_ZN3oct25oct_surface_detect_kernelE\w+": (1, 32),
    r"_ZN3oct25oct_surface_smooth_kernelILi[0-3]EEEv\w+": (4, 96),
    r"_ZN3oct25oct_surface_enface_kernelILi[01]EEEv\w+": (2, 32),
    r"_ZN3oct18oct_flatten_kernelILi[12]EEEv\w+": (2, 64),
}


def test_surface_kernels_need_no_scratch(tmp_path):
    """every surface view kernel: no private memory (the smoothing window of up to 49 entries stays in registers), no LDS, and few
    enough VGPRs for eight waves per SIMD (at most 64) in all but the widest smoothing windows"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "surface_views.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "surface_views_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    for pattern, (count, most) in KERNELS.items():
        names = re.findall(r"^(%s):" % pattern, text, re.M)
        assert len(names) == count, (pattern, names)
        for name in names:
            meta = text[text.index(name + ":"):]
            scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
            lds = int(re.search(r"; LDSByteSize: (\d+)", meta).group(1))
            vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
            print(name, "VGPRs", vgprs, "SGPRs", int(re.search(r"; TotalNumSgprs: (\d+)", meta).group(1)))
            assert scratch == 0 and lds == 0 and vgprs <= most, (name, scratch, lds, vgprs)

"""Repeat registration without a device (include/octpipe.h "repeat registration"): the ABI surface, the status codes of calls that need no
device, the numpy model (tests/register_model.py) against closed forms, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import angio_model as am
import register_model as rm
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = 1, 5

PUBLIC = ("octpipe_repeat_shifts", "octpipe_angiogram_registered", "octpipe_angiogram_enface_registered")
DEBUG = ("octpipe_debug_repeat_shifts", "octpipe_debug_angiogram_registered", "octpipe_debug_angiogram_enface_registered")


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


@pytest.mark.parametrize("struct,mirror,stated,fields", [
    ("OctPipeRepeatShiftSettings", "RepeatShiftSettings", "3 x 4 = 12 bytes", ["repeats", "ascansPerGroup", "maxShift"]),
    ("OctPipeAngioRegistration", "AngioRegistration", "2 x 4 = 8 bytes", ["ascansPerGroup", "fill"])])
def test_struct_layout(struct, mirror, stated, fields):
    mirror = getattr(_lib, mirror)
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
    assert names == [f[0] for f in mirror._fields_] == fields
    assert all(C.sizeof(f[1]) == 4 for f in mirror._fields_)


# ---------------------------------------------------------------------------------------------------------------------- status codes
def _err():
    return _lib.lib().octpipe_last_error().decode()


def _ref(x):
    return None if x is None else C.byref(x)


def test_estimate_argument_checks_come_before_the_handle():
    L = _lib.lib()
    S = _lib.RepeatShiftSettings
    vol, shifts, costs = np.zeros(64, np.float32), np.zeros(64, np.int32), np.zeros(4096, np.float64)
    vp, sp, cp = (C.c_void_p(x.ctypes.data) for x in (vol, shifts, costs))

    def region(bn=4, an=6, sn=40):
        return _lib.StatsRegion(0xFFFFFFFF, 0, bn, 0, an, 0, sn)

    def call(s=S(2, 3, 8), r=region(), out=sp, dev=0, c=cp):
        return L.octpipe_repeat_shifts(None, vp, 0, _ref(r), _ref(s), out, dev, c)

    refused = (("repeats", dict(s=S(1, 3, 8))), ("repeats", dict(s=S(9, 3, 8))), ("repeats", dict(s=S(3, 3, 8))),  # 3 does not divide 4
               ("ascansPerGroup", dict(s=S(2, 0, 8))), ("ascansPerGroup", dict(s=S(2, 4, 8))),  # 4 does not divide 6
               ("maxShift", dict(s=S(2, 3, 0))), ("maxShift", dict(s=S(2, 3, 65))),
               ("sampleCount", dict(r=region(sn=16))),  # 2R
               ("sampleCount", dict(s=S(2, 3, 1), r=region(sn=2))),  # 2R, and below 3
               ("shifts", dict(out=None)), ("shifts", dict(out=None, dev=1)), ("settings", dict(s=None)), ("region", dict(r=None)),
               ("buffer", dict(r=_lib.StatsRegion(3, 0, 4, 0, 6, 0, 40))))
    for word, kw in refused:
        assert call(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (word, kw, _err())
    assert call(r=region(sn=4097)) == ERR_UNSUPPORTED and "sampleCount" in _err()
    # the accepted ends of every range reach the handle check
    for kw in (dict(), dict(c=None), dict(s=S(8, 1, 1), r=region(bn=8, sn=3)), dict(s=S(4, 6, 64), r=region(sn=129)), dict(s=S(2, 6, 64), r=region(sn=4096)),
               dict(r=region(sn=17))):
        assert call(**kw) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (kw, _err())
    ms = C.c_double()
    assert L.octpipe_debug_repeat_shifts(None, vp, 0, C.byref(region()), C.byref(S(2, 3, 65)), sp, 0, None, C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert "maxShift" in _err()
    assert L.octpipe_debug_repeat_shifts(None, vp, 0, C.byref(region()), C.byref(S(2, 3, 8)), sp, 0, None, C.byref(ms)) == ERR_INVALID_ARGUMENT
    assert _err().endswith("null handle")


def test_registered_argument_checks_come_before_the_handle():
    L = _lib.lib()
    S, E, G = _lib.AngioSettings, _lib.SurfaceEnfaceSettings, _lib.AngioRegistration
    reg = _lib.StatsRegion(0xFFFFFFFF, 0, 4, 0, 6, 0, 8)
    surf, outf, vol, shifts = np.zeros(24, np.int32), np.zeros(256, np.float32), np.zeros(256, np.float32), np.zeros(64, np.int32)
    up, fp, vp, sp = (C.c_void_p(x.ctypes.data) for x in (surf, outf, vol, shifts))
    good, slab, grp = S(2, 0, 0, 0.0, 0.0), E(0, 1, 0, 0.0), G(3, 0.0)
    nan = float("nan")

    def volume(s=good, r=reg, out=fp, sh=sp, shdev=0, g=grp):
        return L.octpipe_angiogram_registered(None, vp, 0, _ref(r), _ref(s), out, None, 0, sh, shdev, _ref(g))

    def enface(s=good, r=reg, out=fp, sh=sp, shdev=0, g=grp, surface=up, sdev=0, e=slab):
        return L.octpipe_angiogram_enface_registered(None, vp, 0, _ref(r), _ref(s), surface, sdev, _ref(e), out, 0, sh, shdev, _ref(g))

    common = (("repeats", dict(s=S(1, 0, 0, 0.0, 0.0))), ("repeats", dict(s=S(9, 0, 0, 0.0, 0.0))), ("repeats", dict(s=S(3, 0, 0, 0.0, 0.0))),
              ("method", dict(s=S(2, 3, 0, 0.0, 0.0))), ("threshold", dict(s=S(2, 0, 1, nan, 0.0))), ("settings", dict(s=None)),
              ("region", dict(r=None)), ("out", dict(out=None)), ("buffer", dict(r=_lib.StatsRegion(3, 0, 4, 0, 6, 0, 8))),
              ("shifts", dict(sh=None)), ("shifts", dict(sh=None, shdev=1)), ("registration", dict(g=None)),
              ("ascansPerGroup", dict(g=G(0, 0.0))), ("ascansPerGroup", dict(g=G(4, 0.0))))
    for call in (volume, enface):
        for word, kw in common:
            assert call(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (call.__name__, word, _err())
        for kw in (dict(), dict(g=G(1, nan)), dict(g=G(6, -0.0)), dict(s=S(4, 2, 1, float("inf"), nan))):
            assert call(**kw) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (call.__name__, kw, _err())
    for word, kw in (("thickness", dict(e=E(0, 0, 0, 0.0))), ("thickness", dict(e=E(0, 4097, 0, 0.0))), ("function", dict(e=E(0, 1, 2, 0.0))),
                     ("settings", dict(e=None)), ("surface", dict(surface=None, sdev=1))):
        assert enface(**kw) == ERR_INVALID_ARGUMENT and word in _err() and "null handle" not in _err(), (word, _err())
    assert enface(surface=None) == ERR_INVALID_ARGUMENT and _err().endswith("null handle")
    ms = C.c_double()

    def debug_enface(e, form):
        return L.octpipe_debug_angiogram_enface_registered(None, vp, 0, C.byref(reg), C.byref(good), up, 0, C.byref(e), fp, 0, sp, 0, C.byref(grp), form,
                                                           C.byref(ms))

    for e, form in ((slab, 3), (E(0, 65, 0, 0.0), 2)):
        assert debug_enface(e, form) == ERR_INVALID_ARGUMENT and "form" in _err() and "null handle" not in _err(), (form, _err())
    for e, form in ((slab, 1), (slab, 2), (E(0, 4096, 0, 0.0), 1)):
        assert debug_enface(e, form) == ERR_INVALID_ARGUMENT and _err().endswith("null handle"), (form, _err())
    assert L.octpipe_debug_angiogram_registered(None, vp, 0, C.byref(reg), C.byref(good), fp, None, 0, None, 0, C.byref(grp), C.byref(ms)) == 1
    assert "shifts" in _err()
    assert L.octpipe_debug_angiogram_registered(None, vp, 0, C.byref(reg), C.byref(good), fp, None, 0, sp, 0, C.byref(grp), C.byref(ms)) == 1
    assert _err().endswith("null handle")


# ---------------------------------------------------------------------------------------------------------------------- the model
def _shifted_copies(rng, M, an, sn, R, deltas, s0=0, pad=0):
    """one position whose repeat m shows bin s of a long random profile (one per A-scan) at bin s + deltas[m]: float32 [M][an][pad + sn + pad]"""
    L = sn + 2 * pad
    long = rng.standard_normal((an, L + 2 * R)).astype(np.float32)
    vol = np.empty((M, an, L), np.float32)
    for m, d in enumerate(deltas):
        vol[m] = long[:, R - d:R - d + L]
    return vol


@pytest.mark.parametrize("G,an", [(1, 3), (3, 6), (130, 130)])
def test_known_offsets_are_recovered_with_zero_cost(G, an):
    rng = np.random.default_rng(G)
    R, sn, M = 5, 77, 4
    deltas = (0, 5, -5, 2)
    vol = _shifted_copies(rng, M, an, sn, R, deltas)
    region = (0, M, 0, an, 0, sn)
    shifts, costs, prof = rm.repeat_shifts(vol, region, M, G, R)
    assert shifts.shape == (1, M, an // G) and costs.shape == (1, M - 1, an // G, 2 * R + 1)
    for m, d in enumerate(deltas):
        assert np.all(shifts[0, m] == d), (m, d, shifts[0, m])
        if m:
            assert np.all(costs[0, m - 1, :, d + R] == 0.0)
            others = np.delete(costs[0, m - 1], d + R, axis=-1)
            assert np.all(others > 0.0)
        # the profile of the shifted copy is the shifted profile of the first repeat, bit for bit, where both exist
        lo, hi = max(0, d), min(sn, sn + d)
        assert np.array_equal(am.bits(prof[0, m, :, lo:hi]), am.bits(prof[0, 0, :, lo - d:hi - d]))
    if G == 130:  # two full chunks and a short one: the chunk partials first, then the partials in chunk order
        parts = []
        for c0 in (0, 64, 128):
            part = vol[0, c0].astype(np.float64)
            for a in range(c0 + 1, min(an, c0 + 64)):
                part = part + vol[0, a].astype(np.float64)
            parts.append(part)
        want = (((parts[0] + parts[1]) + parts[2]) / np.float64(130)).astype(np.float32)
        assert np.array_equal(am.bits(rm.averaged(vol[0])), am.bits(want)) and np.array_equal(am.bits(prof[0, 0, 0]), am.bits(want))


def test_tie_rule_constant_profiles_and_non_finite_values():
    R, sn, c = 4, 40, 20
    p0, p1 = np.zeros(sn, np.float32), np.zeros(sn, np.float32)
    p0[c] = 1.0
    p1[c - 2] = p1[c + 2] = 1.0
    costs = rm.lag_costs(p0, p1, R)
    want = np.full(2 * R + 1, 3.0)
    want[R - 2] = want[R + 2] = 1.0
    assert np.array_equal(costs, want) and rm.pick(costs, R) == -2
    vol = np.stack([p0, p1])[:, None, :]
    shifts, costs2, _ = rm.repeat_shifts(vol, (0, 2, 0, 1, 0, sn), 2, 1, R)
    assert shifts.tolist() == [[[0], [-2]]] and np.array_equal(costs2[0, 0, 0], want)
    # ties between |d| = 1 and |d| = 3 go to the smaller |d|; all lags equal: 0
    assert rm.pick(np.array([5.0, 1.0, 5.0, 5.0, 5.0, 1.0, 5.0, 1.0, 5.0]), 4) == 1
    assert rm.pick(np.array([1.0, 5.0, 5.0, 1.0, 5.0, 1.0, 5.0, 5.0, 5.0]), 4) == -1
    flat = np.full((3, 2, sn), 2.5, np.float32)
    shifts, costs, _ = rm.repeat_shifts(flat, (0, 3, 0, 2, 0, sn), 3, 1, R)
    assert not shifts.any() and not costs.any()
    # one inf in the window but outside the inner window: shift 0, every cost the canonical NaN; the other repeat is not affected
    rng = np.random.default_rng(5)
    vol = _shifted_copies(rng, 3, 2, sn, R, (0, 3, -1))
    vol[1, 0, 1] = np.inf  # bin 1 < R
    shifts, costs, _ = rm.repeat_shifts(vol, (0, 3, 0, 2, 0, sn), 3, 1, R)
    assert shifts[0, :, 0].tolist() == [0, 0, -1] and shifts[0, :, 1].tolist() == [0, 3, -1]
    assert np.all(costs[0, 0, 0].view(np.uint64) == rm.CANONICAL_NAN64) and costs[0, 1, 0, R - 1] == 0.0 and costs[0, 0, 1, R + 3] == 0.0
    vol[0, 1, sn - 1] = np.nan  # in P_0: every repeat of that group
    shifts, costs, _ = rm.repeat_shifts(vol, (0, 3, 0, 2, 0, sn), 3, 1, R)
    assert not shifts[0, :, 1].any() and np.all(costs[0, :, 1].view(np.uint64) == rm.CANONICAL_NAN64)
    # the partial scheme: 65 terms, t_64 = 1 joins L_0 = 2^-54 before the partials are added, and every other 2^-54 is then lost against
    # the 1; one running sum in depth order would reach 64 * 2^-54 first and keep it
    K, R1 = 65, 1
    p0 = np.zeros(K + 2, np.float32)
    p1 = np.full(K + 2, 2.0 ** -54, np.float32)
    p1[R1 + 64] = 1.0
    assert rm.lag_costs(p0, p1, R1)[R1] == 1.0
    running = np.float64(0.0)
    for v in p1[R1:R1 + K]:
        running = running + np.float64(v)
    assert running == 1.0 + 2.0 ** -48


def test_registered_contrast_of_shifted_copies():
    rng = np.random.default_rng(11)
    R, sn, M, an, G = 6, 50, 3, 4, 2
    deltas = (0, 6, -3)
    vol = _shifted_copies(rng, M, an, sn, R, deltas, pad=4)
    s0 = 4
    region = (0, M, 0, an, s0, sn)
    shifts, _, _ = rm.repeat_shifts(vol, region, M, G, R)
    assert shifts[0].tolist() == [[0, 0], [6, 6], [-3, -3]]
    lo, hi = rm.covered(deltas, s0, sn)
    assert (lo, hi) == (s0 + 3, s0 + sn - 1 - 6)
    fill = np.float32(-9.5)
    for method in (am.VARIANCE, am.DIFFERENCE):
        out, mean = rm.angiogram_registered(vol, region, M, method, shifts, G, fill)
        assert np.all(out[:, :, lo - s0:hi - s0 + 1] == 0.0) and np.all(out[:, :, :lo - s0] == fill) and np.all(out[:, :, hi - s0 + 1:] == fill)
        assert np.array_equal(mean[0, :, lo - s0:hi - s0 + 1], vol[0, :, lo:hi + 1]) and np.all(mean[:, :, :lo - s0] == fill)
        # without the registration most bins show contrast; with zero shifts the registered model is the angiography's, bit for bit
        zero = np.zeros_like(shifts)
        plain, plain_mean = am.angiogram(vol, region, M, method)
        out0, mean0 = rm.angiogram_registered(vol, region, M, method, zero, G, fill)
        assert np.array_equal(am.bits(out0), am.bits(plain)) and np.array_equal(am.bits(mean0), am.bits(plain_mean))
        assert np.count_nonzero(plain > 0.0) > 0.9 * plain.size
        # the en face slab is the projection of the registered volume restricted to Wc
        surface = np.array([[s0 + 1, -1, s0 + 30, s0 + sn - 2]] * M, np.int32)
        for fn, offset, thickness in ((0, 0, 16), (1, -3, 70), (0, 5, 1), (0, 48, 9)):
            a = rm.angiogram_enface_registered(vol, region, M, method, shifts, G, surface, offset, thickness, fn, -2.0, 0.0, 7.0)
            masked, _ = rm.angiogram_registered(vol, region, M, method, shifts, G, fill, 0.0, 7.0)
            b = rm.project_registered(masked, region, M, shifts, G, surface, offset, thickness, fn, -2.0)
            assert np.array_equal(am.bits(a), am.bits(b)), (method, fn, offset, thickness)
            assert a[0, 1] == -2.0
        assert rm.angiogram_enface_registered(vol, region, M, method, shifts, G, surface, 48, 9, 0, -2.0)[0, 3] == -2.0  # below Wc, inside W
        a = rm.angiogram_enface_registered(vol, region, M, method, zero, G, surface, -3, 20, 0, -2.0, 0.1, 3.0)
        assert np.array_equal(am.bits(a), am.bits(am.angiogram_enface(vol, region, M, method, surface, -3, 20, 0, -2.0, 0.1, 3.0)))


def test_covered_window():
    s0, sn = 10, 20
    assert rm.covered([0, 0], s0, sn) == (10, 29)
    assert rm.covered([0, 3, -2], s0, sn) == (12, 26)
    assert rm.covered([3, 3], s0, sn) == (10, 26)      # Wc = [7, 26]: a non-zero m = 0 shift moves it; only its part inside W counts
    assert rm.covered([-4, 0], s0, sn) == (14, 29)
    assert rm.covered([5, 0], s0, sn) == (10, 24)
    lo, hi = rm.covered([10, -10], s0, sn)
    assert lo > hi
    lo, hi = rm.covered([2 ** 31 - 1, -2 ** 31], s0, sn)
    assert lo > hi
    rng = np.random.default_rng(2)
    vol = rng.standard_normal((2, 2, 40)).astype(np.float32)
    region = (0, 2, 0, 2, s0, sn)
    shifts = np.array([[[3, 10], [3, -10]]], np.int32)  # group 0: both repeats 3 bins down; group 1: nothing covered
    out, mean = rm.angiogram_registered(vol, region, 2, am.DIFFERENCE, shifts, 1, 4.0)
    assert np.all(out[0, 1] == 4.0) and np.all(mean[0, 1] == 4.0)
    assert np.all(out[0, 0, 17:] == 4.0)
    want, _ = am.angiogram(vol, (0, 2, 0, 1, s0 + 3, sn - 3), 2, am.DIFFERENCE)
    assert np.array_equal(am.bits(out[0, 0, :17]), am.bits(want[0, 0]))
    img = rm.angiogram_enface_registered(vol, region, 2, 0, shifts, 1, None, 0, 4096, 1, -1.0)
    assert img[0, 1] == -1.0 and img[0, 0] != -1.0


# ---------------------------------------------------------------------------------------------------------------------- kernels
KERNELS = {  # mangled-name pattern: instances
    r"_ZN3oct26oct_register_search_kernelILb[01]EEEv\w+": 2,
    r"_ZN3oct26oct_register_volume_kernelILi[0-2]ELj[2-8]EEEv\w+": 3 * 7,
    r"_ZN3oct26oct_register_enface_kernelILi[0-2]ELi[01]ELj[2-8]EEEv\w+": 6 * 7,
    r"_ZN3oct31oct_register_enface_team_kernelILi[0-2]ELi[01]ELj[2-8]EEEv\w+": 6 * 7,
}


def test_register_kernels_need_no_scratch(tmp_path):
    """every repeat registration kernel: no private memory (the shifts, the row pointers and the 4 x M values of a step stay in registers),
    at most 128 VGPRs; only the search kernel uses LDS, and only the dynamic allocation its launcher sizes"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "repeat_register.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "repeat_register_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
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

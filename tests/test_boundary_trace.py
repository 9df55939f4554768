"""Boundary tracing without a device (include/octpipe.h "boundary tracing"): the ABI surface, the status codes of calls that need no
device, the numpy model (tests/boundary_model.py) against brute-force enumeration of every path and against a closed form, and the
resources of the new kernels against DESIGN.md 5.19."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boundary_model as bm
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = 1, 5


# ---------------------------------------------------------------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    name = "octpipe_trace_boundary"
    assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name)
    name = "octpipe_debug_trace_boundary"
    assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name)


def test_struct_layout():
    struct, mirror, stated = "OctPipeBoundaryTraceSettings", _lib.BoundaryTraceSettings, "6 x 4 = 24 bytes"
    hdr = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    head = "typedef struct %s {" % struct
    line = hdr[hdr.index(head):].split("\n", 1)[0]
    assert stated in line and C.sizeof(mirror) == 24
    body = hdr[hdr.index(head):hdr.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip().split() for d in body.split("{", 1)[1].split(";") if d.strip()]
    assert [d[1] for d in decls] == [f[0] for f in mirror._fields_]
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    assert [ctype[d[0]] for d in decls] == [f[1] for f in mirror._fields_]


# ---------------------------------------------------------------------------------------------------------------------- status codes
def _err():
    return _lib.lib().octpipe_last_error().decode()


def _call(settings, region=_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 4, 0, 8), guide=True, surface=True, guide_dev=0, form=None):
    L = _lib.lib()
    vol, g, out = np.zeros(64, np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    args = [None, C.c_void_p(vol.ctypes.data), 0, None if region is None else C.byref(region), C.c_void_p(g.ctypes.data) if guide else None,
            guide_dev, None if settings is None else C.byref(settings), C.c_void_p(out.ctypes.data) if surface else None, None, 0]
    if form is None:
        return L.octpipe_trace_boundary(*args)
    ms = C.c_double()
    return L.octpipe_debug_trace_boundary(*args, form, C.byref(ms))


def test_argument_checks_come_before_the_handle():
    S = _lib.BoundaryTraceSettings
    good = dict(bandLo=-4, bandHi=4, halfWidth=2, polarity=1, maxStep=1, smoothness=0.5)
    for change, word in ((dict(bandLo=5), "bandLo"), (dict(bandLo=-65537), "bandLo"), (dict(bandHi=65537), "bandHi"),
                         (dict(bandLo=65537, bandHi=65537), "bandLo"), (dict(halfWidth=0), "halfWidth"), (dict(halfWidth=9), "halfWidth"),
                         (dict(polarity=0), "polarity"), (dict(polarity=2), "polarity"), (dict(maxStep=0), "maxStep"), (dict(maxStep=8), "maxStep"),
                         (dict(smoothness=-0.5), "smoothness"), (dict(smoothness=float("nan")), "smoothness"),
                         (dict(smoothness=float("inf")), "smoothness")):
        assert _call(S(**dict(good, **change))) == ERR_INVALID_ARGUMENT and word in _err(), (change, _err())
    assert _call(None) == ERR_INVALID_ARGUMENT and "settings" in _err()
    assert _call(S(**good), region=None) == ERR_INVALID_ARGUMENT and "region" in _err()
    assert _call(S(**good), surface=False) == ERR_INVALID_ARGUMENT and "surface" in _err()
    assert _call(S(**good), guide=False, guide_dev=1) == ERR_INVALID_ARGUMENT and "guide" in _err()
    assert _call(S(**good), region=_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 65537, 0, 8)) == ERR_INVALID_ARGUMENT and "ascanCount" in _err()
    assert _call(S(**good), region=_lib.StatsRegion(3, 0, 1, 0, 4, 0, 8)) == ERR_INVALID_ARGUMENT and "buffer" in _err()
    for form in (5, 99):
        assert _call(S(**good), form=form) == ERR_INVALID_ARGUMENT and "form" in _err()
    # the band limits apply with a guide only
    assert _call(S(**dict(good, bandLo=9, bandHi=-9)), guide=False) == ERR_INVALID_ARGUMENT and "null handle" in _err()
    # the extremes of every limit pass the argument checks
    for change in (dict(bandLo=-65536, bandHi=-65536), dict(bandLo=65536, bandHi=65536), dict(halfWidth=1), dict(halfWidth=8), dict(polarity=-1),
                   dict(maxStep=7), dict(smoothness=0.0), dict(bandLo=0, bandHi=1023)):
        assert _call(S(**dict(good, **change))) == ERR_INVALID_ARGUMENT and "null handle" in _err(), change
    assert _call(S(**good), form=4) == ERR_INVALID_ARGUMENT and "null handle" in _err()


def test_more_than_1024_nodes_are_unsupported():
    S = _lib.BoundaryTraceSettings
    assert _call(S(0, 1024, 2, 1, 1, 0.0)) == ERR_UNSUPPORTED and "1025" in _err()
    assert _call(S(-65536, 65536, 2, 1, 1, 0.0)) == ERR_UNSUPPORTED and "131073" in _err()
    # without a guide the window is the band
    assert _call(S(0, 0, 2, 1, 1, 0.0), region=_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 4, 0, 1025), guide=False) == ERR_UNSUPPORTED and "1025" in _err()
    assert _call(S(0, 0, 2, 1, 1, 0.0), region=_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 4, 0, 1024), guide=False) == ERR_INVALID_ARGUMENT and "null handle" in _err()


# ---------------------------------------------------------------------------------------------------------------------- the model
def _both(vol, region, **kw):
    """the plain loops and the column-at-once form of the model, held equal bit for bit"""
    s, c = bm.trace(vol, region, **kw)
    sl, cl = bm.trace(vol, region, loops=True, **kw)
    assert np.array_equal(s, sl) and np.array_equal(bm.bits(c), bm.bits(cl))
    return s, c


@pytest.mark.parametrize("case", ["A4-H4-m1-integers", "A3-H5-m2", "A4-H4-m1-ties", "A3-H5-m2-guided"])
def test_model_against_every_path(case):
    rng = np.random.default_rng(len(case))
    for trial in range(6):
        guide, band, lam, k = None, (0, 0), [0.0, 0.5, 1.0][trial % 3], 1 + trial % 2
        if case == "A4-H4-m1-integers":
            an, H, m = 4, 4, 1
            vol = rng.integers(-5, 6, (1, an, H)).astype(np.float32)
        elif case == "A4-H4-m1-ties":  # almost every compare ties: the tie rules decide the path
            an, H, m = 4, 4, 1
            vol = rng.integers(0, 2, (1, an, H)).astype(np.float32)
        elif case == "A3-H5-m2":
            an, H, m, lam = 3, 5, 2, [0.0, 0.37][trial % 2]
            vol = rng.standard_normal((1, an, H)).astype(np.float32)
        else:
            an, H, m, lam = 3, 5, 2, 0.25
            vol = rng.integers(-4, 5, (1, an, 12)).astype(np.float32)
            guide = np.array([[4 + trial % 3, -1 if trial & 1 else 5, 1 + trial]], np.int32)  # a hole; part of the band outside the window
            band = (-2, 2)
        region = bm.whole(vol)
        s0, s1 = 0, vol.shape[2] - 1
        for polarity in (1, -1):
            got_s, got_c = _both(vol, region, guide=guide, band=band, half_width=k, polarity=polarity, max_step=m, smoothness=lam)
            lo, hi = (s0, s1) if guide is None else band
            assert hi - lo + 1 == H
            want_s, want_c = bm.brute_force(vol[0], None if guide is None else guide[0], lo, hi, s0, s1, k, polarity, m, lam)
            assert bm.bits(got_c)[0] == bm.bits(want_c), (case, trial, polarity, got_c, want_c)
            assert np.array_equal(got_s[0], want_s), (case, trial, polarity, got_s, want_s)


def test_model_recovers_a_tilted_step_exactly():
    A, N = 96, 128
    rng = np.random.default_rng(7)
    z = np.round(40 + 0.3 * np.arange(A)).astype(np.int32)
    vol = rng.uniform(0.0, 0.3, (1, A, N)).astype(np.float32)
    vol[0] += (np.arange(N)[None, :] >= z[:, None]).astype(np.float32)
    region = (0, 1, 0, A, 4, 120)
    s, c = bm.trace(vol, region, half_width=2, max_step=1, smoothness=0.05)
    assert np.array_equal(s[0], z)
    guide = (z - 7 + rng.integers(-1, 2, A)).astype(np.int32)[None, :]
    s, c = bm.trace(vol, region, guide=guide, band=(-12, 12), half_width=2, max_step=2, smoothness=0.05)
    assert np.array_equal(s[0], z)
    # the falling edge of the mirrored volume, found with the other polarity
    s, c = bm.trace(vol[:, :, ::-1], (0, 1, 0, A, 4, 120), polarity=-1, half_width=2, max_step=1, smoothness=0.05)
    assert np.array_equal(s[0], N - z)


def test_model_edge_rules():
    # a constant volume: every cost is -0 for polarity +1 (g = +0), every compare ties; the path stays on the first node
    vol = np.full((1, 5, 9), 2.0, np.float32)
    s, c = _both(vol, bm.whole(vol), half_width=3, max_step=2, smoothness=0.0)
    assert s.tolist() == [[0] * 5] and bm.bits(c)[0] == 0  # (-0 + +0) + -0 = +0 from the second A-scan on
    s, c = _both(vol[:, :1], (0, 1, 0, 1, 0, 9), half_width=3)
    assert s.tolist() == [[0]] and bm.bits(c)[0] == 0x80000000  # one A-scan: E = c = -0 with its own bits
    # a guide of holes only: every cost +0, every surface entry -1
    s, c = _both(vol, bm.whole(vol), guide=np.full((1, 5), -3, np.int32), band=(-1, 1))
    assert s.tolist() == [[-1] * 5] and bm.bits(c)[0] == 0
    # non-finite gradients cost +0
    v = np.zeros((1, 2, 6), np.float32)
    v[0, :, 3] = np.inf
    v[0, 1, 1] = np.nan
    assert bm.bits(bm.node_cost(v[0, 0], 3, 0, 5, 1, 1)) == 0 and bm.bits(bm.node_cost(v[0, 1], 2, 0, 5, 2, 1)) == 0
    _both(v, bm.whole(v), half_width=2, max_step=7)


# ---------------------------------------------------------------------------------------------------------------------- kernels
FORMS = {"Lb1ELb1E": "wave, choices in LDS", "Lb1ELb0E": "wave, choices in scratch", "Lb0ELb1E": "workgroup, choices in LDS",
         "Lb0ELb0E": "workgroup, choices in scratch"}


def test_trace_kernels_use_no_private_memory_and_match_the_design_table(tmp_path):
    """every instance: no private memory, static LDS within the CU's 160 KiB, and the registers and LDS bytes DESIGN.md 5.19 states"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "boundary_trace.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "boundary_trace_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5.19"):design.index("## 6. Measurement")]
    names = re.findall(r"^(_ZN3oct25oct_boundary_trace_kernelI(\w+?)EEvNS_9TraceArgsE):", text, re.M)
    assert sorted(n[1] for n in names) == sorted(FORMS), names
    for name, key in names:
        meta = text[text.index(name + ":"):]
        scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
        lds = int(re.search(r"; LDSByteSize: (\d+)", meta).group(1))
        vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
        sgprs = int(re.search(r"; TotalNumSgprs: (\d+)", meta).group(1))
        print(FORMS[key], "VGPRs", vgprs, "SGPRs", sgprs, "LDS", lds)
        assert scratch == 0 and lds <= 163840 and vgprs <= 128, (name, scratch, lds, vgprs)
        row = re.search(r"^\| %s \| (\d+) \| (\d+) \| ([\d ]+) \|$" % re.escape(FORMS[key]), section, re.M)
        assert row, FORMS[key]
        assert (int(row.group(1)), int(row.group(2)), int(row.group(3).replace(" ", ""))) == (vgprs, sgprs, lds), (FORMS[key], row.groups())

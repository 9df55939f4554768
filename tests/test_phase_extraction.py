"""Phase extraction without a device (include/octpipe.h "phase extraction"): the ABI surface, the float64 model of the library's
definition against analytic curves and an imaging check, and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import phase_model as pm
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

PUBLIC = ["octpipe_phase_reset", "octpipe_phase_accumulate", "octpipe_phase_mean", "octpipe_extract_resample_curve"]
DEBUG = ["octpipe_debug_phase_accumulate"]
LENGTHS = [256, 512, 1024, 2048, 4096]

# Recovery bound of the float64 model on [a, b] (a = b' = N/16 samples from each edge, Hann band, no raw window): measured at most
# 0.031 sample over N = 256 ... 4096 for this data (64 A-scans; what remains is the averaged sample reflectors and noise inside the
# band plus the band limit of the chirp near the anchors); 0.05 leaves room for the seed, and stays well below 0.1 sample.
RECOVERY_BOUND = 0.05


def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name)
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name)
    assert C.sizeof(_lib.PhaseExtraction) == 24
    assert [f[0] for f in _lib.PhaseExtraction._fields_] == ["peakStart", "peakEnd", "windowRaw", "hannPeak", "ignoreFirst", "ignoreLast"]


def test_null_handles_give_status_codes():
    L = _lib.lib()
    raw = np.zeros(16, np.uint16)
    out = np.zeros(16, np.float32)
    x = _lib.PhaseExtraction(2, 6, 0, 1, 0, 0)
    cnt, ms = C.c_uint64(), C.c_double()
    assert L.octpipe_phase_reset(None) == 1
    assert L.octpipe_phase_accumulate(None, raw.ctypes.data, 0, 0, 1) == 1
    assert L.octpipe_phase_mean(None, out.ctypes.data, C.byref(cnt)) == 1
    assert L.octpipe_extract_resample_curve(None, out.ctypes.data, C.byref(x), None, None, None, out.ctypes.data, None) == 1
    assert L.octpipe_debug_phase_accumulate(None, raw.ctypes.data, 0, 0, 1, C.byref(ms)) == 1
    assert b"null handle" in L.octpipe_last_error()


@pytest.mark.parametrize("n", LENGTHS)
def test_model_recovers_the_analytic_curve(n):
    raw = pm.calibration_raw(n, 64, seed=n)
    mean = raw.astype(np.float64).mean(axis=0)
    ig = n // 16
    r = pm.extract(mean, int(0.2 * n), int(0.4 * n), False, True, ig, ig)
    a, b = r["a"], r["b"]
    want = pm.analytic_curve(n, a, b)
    err = np.abs(r["curve"][a:b + 1] - want[a:b + 1]).max()
    assert err < RECOVERY_BOUND, err
    # the intermediate steps: psi is the anchor-referenced phase, the monotone psi is monotone and equal to psi inside a clean band
    assert r["psi"][a] == a and abs(r["psi"][b] - b) < 1e-9
    assert np.all(np.diff(r["psi_mono"]) >= 0)
    assert np.abs(r["psi_mono"][a:b + 1] - pm.psi_true(n, a, b)[a:b + 1]).max() < 2 * RECOVERY_BOUND


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_linear_k_gives_the_identity_curve(n):
    raw = pm.calibration_raw(n, 64, seed=2, kmap=lambda u: u)
    ig = n // 16
    r = pm.extract(raw.astype(np.float64).mean(axis=0), int(0.2 * n), int(0.4 * n), False, True, ig, ig)
    a, b = r["a"], r["b"]
    assert np.abs(r["curve"][a:b + 1] - np.arange(a, b + 1)).max() < RECOVERY_BOUND
    np.testing.assert_allclose(r["coeffs"], [0.0, n - 1.0, 0.0, 0.0], atol=0.05 * n / 256)


def test_cubic_curve_comes_back_through_the_fit():
    """a fringe whose resampling curve is the cubic C(j) (C(a) = a, C(b) = b, so the anchor normalisation is the identity on it): the
    fit returns C's coefficients in t = j / (N-1)"""
    n, ig = 1024, 64
    a, b = ig, n - 1 - ig
    beta = 0.4

    def C_(j):
        return j + beta * (j - a) * (j - b) * (j - 0.3 * n) / float(n) ** 2

    # the fringe is linear in j: sample n sits at j = C^{-1}(n), i.e. k(u_n) = C^{-1}(n) / (N-1)
    jj = np.linspace(-0.05 * n, 1.05 * n, 200001)
    def kmap(u):
        return np.interp(u * (n - 1), C_(jj), jj) / (n - 1)
    assert np.all(np.diff(C_(jj)) > 0)
    raw = pm.calibration_raw(n, 64, seed=9, kmap=kmap)
    r = pm.extract(raw.astype(np.float64).mean(axis=0), int(0.2 * n), int(0.4 * n), False, True, ig, ig)
    t = np.array([0.0, 1.0, 2.0, 3.0])
    # C in powers of t = j / (N-1): expand j = (N-1) t
    s = n - 1.0
    poly = np.polynomial.polynomial.polyfromroots([a, b, 0.3 * n]) * beta / float(n) ** 2  # (j-a)(j-b)(j-0.3n) beta / n^2
    want = np.array([poly[0], 1.0 + poly[1], poly[2], poly[3]]) * s ** t
    np.testing.assert_allclose(r["coeffs"], want, rtol=0, atol=0.5)
    assert np.abs(pm.poly_curve(r["coeffs"], n)[a:b + 1] - C_(np.arange(a, b + 1.0))).max() < 2 * RECOVERY_BOUND


def test_resampling_with_the_curve_restores_a_mirror():
    """imaging check: a mirror at depth 0.1 N, resampled with the model's curve (cubic interpolation) and transformed, reaches 0.9 of
    the peak of the same mirror sampled linearly in k with at most 1.2 x its width; unresampled it falls far below.  Measured for this
    data: curve 0.94 / 1.06, fitted coefficients 0.93 / 1.09, no resampling 0.38 / 7.0."""
    n = 1024
    raw = pm.calibration_raw(n, 64, seed=3)
    r = pm.extract(raw.astype(np.float64).mean(axis=0), int(0.2 * n), int(0.4 * n), False, True, 32, 32)
    depth = 0.1 * n
    h0, w0 = pm.peak_and_fwhm(pm.ascan(pm.mirror(n, depth, kmap=lambda u: u)))
    nl = pm.mirror(n, depth)
    for curve in (r["curve"], pm.poly_curve(r["coeffs"], n)):
        h, w = pm.peak_and_fwhm(pm.ascan(pm.resample_cubic(nl, curve)))
        assert h >= 0.9 * h0 and w <= 1.2 * w0, (h / h0, w / w0)
    h, w = pm.peak_and_fwhm(pm.ascan(nl))
    assert h < 0.5 * h0 and w > 3 * w0


def _kernel_meta(text, name):
    start = text.index(name + ":")
    meta = text[start:]  # (the first resource comments after the label belong to this kernel)
    return int(re.search(r"; ScratchSize: (\d+)", meta).group(1)), int(re.search(r"; NumVgprs: (\d+)", meta).group(1))


@pytest.mark.parametrize("log2n", [8, 9, 10, 11, 12])
def test_extract_kernel_needs_no_scratch(log2n, tmp_path):
    """oct_phase_extract_kernel<LOG2N> as csrc/Makefile builds it: no private memory at any supported length"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / ("phase_%d.s" % log2n))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-DOCT_LOG2N=%d" % log2n, "-S", "--cuda-device-only", "-o", out, "phase_extract_inst.hip"], cwd=CSRC,
                          stderr=subprocess.DEVNULL)
    scratch, vgprs = _kernel_meta(open(out).read(), "_ZN3oct24oct_phase_extract_kernelILi%dEEEvNS_16PhaseExtractArgsE" % log2n)
    assert scratch == 0 and vgprs <= 256


def test_accumulate_kernels_need_no_scratch(tmp_path):
    """every (format, vector form) instance of oct_phase_accumulate_kernel: no private memory"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "pipe_phase.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "pipe_phase.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^(_ZN3oct27oct_phase_accumulate_kernelILi\d+ELb[01]EEEvNS_12PhaseAccArgsE):", text, re.M)
    assert len(names) == 16
    for name in names:
        scratch, _ = _kernel_meta(text, name)
        assert scratch == 0, name

"""Peak analysis without a device (include/octpipe.h "peak analysis"): the ABI surface, the status codes of calls that need no device,
the numpy model of the definition on crafted cases and against independent implementations (tests/phase_model.peak_and_fwhm for the
crossings, scipy's Levenberg-Marquardt for the fit), and the register budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import peak_model as pm
import phase_model
from octproz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_INVALID_ARGUMENT = 1


def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    assert re.search(r"\boctpipe_peak_analysis\s*\(", pub) and "octpipe_peak_analysis" in _lib.OCTPIPE_SYMBOLS
    assert hasattr(L, "octpipe_peak_analysis")
    assert re.search(r"\boctpipe_debug_peak_analysis\s*\(", dbg) and "octpipe_debug_peak_analysis" in _lib.OCTPIPE_DEBUG_SYMBOLS
    assert hasattr(L, "octpipe_debug_peak_analysis")
    for name, bit in (("NO_PEAK", 1), ("NONFINITE", 2), ("WIDTH_UNDEFINED", 4), ("LEFT_OPEN", 8), ("RIGHT_OPEN", 16), ("FIT_CONVERGED", 256),
                      ("FIT_MAX_ITER", 512), ("FIT_STALLED", 1024), ("FIT_SKIPPED", 2048)):
        assert re.search(r"OCTPIPE_PEAK_%s = 1u << %d" % (name, bit.bit_length() - 1), pub), name
        assert getattr(_lib, "PEAK_" + name) == bit == getattr(pm, name)


def test_struct_layouts():
    assert C.sizeof(_lib.PeakSettings) == 20
    assert C.sizeof(_lib.Peak) == 104
    assert [f[0] for f in _lib.PeakSettings._fields_] == ["ascansPerGroup", "threshold", "fitGaussian", "fitHalfWidth", "maxIterations"]
    assert [f[0] for f in _lib.Peak._fields_] == ["status", "index", "value", "fitFirst", "fitCount", "iterations", "position", "left", "right",
                                                  "fwhm", "amplitude", "center", "sigma", "offset", "fitFwhm", "rms"]
    assert _lib.Peak.position.offset == 24 and _lib.Peak.rms.offset == 96
    hdr = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    assert "5 x 4 = 20 bytes" in hdr and "6 x 4 + 10 x 8 = 104 bytes" in hdr


def test_status_codes_without_a_device():
    L = _lib.lib()
    reg = _lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, 8)
    s = _lib.PeakSettings(1, float("-inf"), 1, 0, 0)
    peaks = (_lib.Peak * 4)()
    ms = C.c_double()

    def call(h=None, r=reg, st=s, out=peaks, data=None):
        return L.octpipe_peak_analysis(h, data, 0, C.byref(r) if r is not None else None, C.byref(st) if st is not None else None, out, None)

    assert call() == ERR_INVALID_ARGUMENT and b"null handle" in L.octpipe_last_error()
    assert L.octpipe_debug_peak_analysis(None, None, 0, C.byref(reg), C.byref(s), peaks, None, C.byref(ms)) == ERR_INVALID_ARGUMENT
    cases = [(lambda: call(r=None), b"region"),
             (lambda: call(st=None), b"settings"),
             (lambda: call(out=None), b"peaks"),
             (lambda: call(st=_lib.PeakSettings(1, float("nan"), 1, 0, 0)), b"threshold"),
             (lambda: call(st=_lib.PeakSettings(0, 0.0, 1, 0, 0)), b"ascansPerGroup"),
             (lambda: call(st=_lib.PeakSettings(1, 0.0, 1, 0, 1001)), b"maxIterations"),
             (lambda: call(r=_lib.StatsRegion(1, 0, 1, 0, 1, 0, 8), data=np.zeros(4, np.float32).ctypes.data), b"buffer")]
    for fn, field in cases:
        assert fn() == ERR_INVALID_ARGUMENT and field in L.octpipe_last_error(), (field, L.octpipe_last_error())
    # -inf is a threshold, 1000 iterations are allowed: what remains is the missing handle
    assert call(st=_lib.PeakSettings(1, float("-inf"), 1, 0, 1000)) == 1 and b"null handle" in L.octpipe_last_error()


# ---------------------------------------------------------------------------------------------------------------------- the model
def f32(x):
    return np.asarray(x, dtype=np.float32)


def test_ties_take_the_first_maximum():
    m = f32([0, 1, 5, 2, 5, 5, 1, 0])
    o = pm.analyse(m, s0=10)
    assert o["index"] == 12 and o["value"] == 5.0 and o["status"] == 0
    # -0.0 and 0.0 are equal: the first wins, its bits are reported
    o = pm.analyse(f32([-1, -0.0, 0.0, -2]))
    assert o["index"] == 1 and np.signbit(o["value"]) and o["status"] & pm.WIDTH_UNDEFINED


def test_threshold_is_strict():
    m = f32([0, 1, 3, 1, 0])
    o = pm.analyse(m, threshold=3.0)
    assert o["status"] == pm.NO_PEAK and o["index"] == 2 and o["value"] == 3.0
    assert all(np.isnan(o[f]) for f in ("position", "left", "right", "fwhm", "center"))
    assert pm.analyse(m, threshold=np.nextafter(np.float32(3), np.float32(0)))["status"] == 0


def test_peak_on_the_window_edge():
    o = pm.analyse(f32([9, 4, 1, 0, 0]), s0=7)
    assert o["position"] == 7.0 and o["status"] & pm.LEFT_OPEN and o["left"] == 7.0
    o = pm.analyse(f32([0, 0, 1, 4, 9]), s0=7)
    assert o["position"] == 11.0 and o["status"] & pm.RIGHT_OPEN and o["right"] == 11.0
    # inside the window the first maximum always has d < 0: two equal samples put the vertex halfway
    assert pm.analyse(f32([0, 4, 4, 0]))["position"] == 1.5


def test_open_flanks_are_flagged():
    o = pm.analyse(f32([3, 4, 5, 4, 3]))
    assert o["status"] == pm.LEFT_OPEN | pm.RIGHT_OPEN and (o["left"], o["right"]) == (0.0, 4.0) and o["fwhm"] == 4.0
    o = pm.analyse(f32([0, 1, 5, 4, 3]))
    assert o["status"] == pm.RIGHT_OPEN and o["left"] == 2 - (5 - 2.5) / (5 - 1)


def test_value_not_above_zero_leaves_the_width_undefined():
    o = pm.analyse(f32([-5, -3, -1, -3, -5]), fit=True)
    assert o["status"] & pm.WIDTH_UNDEFINED and np.isnan(o["fwhm"]) and np.isnan(o["left"])
    assert o["position"] == 2.0 and o["fitCount"] == 5  # w = 16, cut by the window
    o = pm.analyse(np.zeros(8, np.float32))
    assert o["status"] == pm.WIDTH_UNDEFINED and o["index"] == 0


def test_one_nan_marks_its_group_only():
    rng = np.random.default_rng(1)
    region = rng.random((2, 4, 32)).astype(np.float32)
    region[1, 2, 17] = np.nan
    avg, res = pm.analyse_region(region, 2)
    flags = [[r["status"] & pm.NONFINITE for r in row] for row in res]
    assert flags == [[0, 0], [0, pm.NONFINITE]]
    bad = res[1][1]
    assert np.isnan(bad["value"]) and bad["index"] == 0 and np.isnan(bad["position"])
    assert np.isnan(avg[1, 1, 17]) and np.isfinite(avg[1, 1, :17]).all()
    region[0, 0, 3] = np.inf
    assert pm.analyse_region(region, 2)[1][0][0]["status"] == pm.NONFINITE


def test_chunked_average():
    rng = np.random.default_rng(2)
    rows = (rng.random((64, 40)) * 1e4).astype(np.float32)
    rows[3] *= 1e6
    seq = np.zeros(40)
    for r in rows.astype(np.float64):
        seq = seq + r
    assert np.array_equal(pm.averaged(rows), (seq / 64).astype(np.float32))
    # G = 200: four chunk partials (64, 64, 64, 8) added in chunk order
    rows = (rng.standard_normal((200, 40)) * 10 ** rng.uniform(-3, 7, size=(200, 1))).astype(np.float32)
    parts = []
    for c in range(0, 200, 64):
        acc = np.zeros(40)
        for r in rows[c:c + 64].astype(np.float64):
            acc = acc + r
        parts.append(acc)
    t = parts[0]
    for p in parts[1:]:
        t = t + p
    assert np.array_equal(pm.averaged(rows), (t / 200).astype(np.float32))
    plain = np.zeros(40)
    for r in rows.astype(np.float64):
        plain = plain + r
    assert not np.array_equal(t, plain)  # (the data is chosen so that the order shows)


def test_crossings_equal_phase_model_peak_and_fwhm():
    rng = np.random.default_rng(3)
    for i in range(200):
        n = int(rng.integers(8, 600))
        z = np.arange(n)
        mu, sig = rng.uniform(-5, n + 5), rng.uniform(0.5, n / 3)
        a = (rng.uniform(0.1, 100) * np.exp(-0.5 * ((z - mu) / sig) ** 2) + rng.uniform(1e-3, 1) * rng.random(n) + 1e-3).astype(np.float32)
        o = pm.analyse(a)
        h, fw = phase_model.peak_and_fwhm(a.astype(np.float64), skip=0)
        assert o["value"] == h and o["fwhm"] == fw, (i, o["fwhm"], fw)


def _scipy_fit(z, y, p0):
    from scipy.optimize import least_squares
    return least_squares(lambda p: pm.gauss(z, p) - y, p0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000).x


def test_fit_agrees_with_scipy_on_noisy_gaussians():
    rng = np.random.default_rng(4)
    for i in range(40):
        n = 256
        z = np.arange(n, dtype=np.float64)
        mu, sig, amp, off = rng.uniform(60, 190), rng.uniform(1.5, 12), rng.uniform(10, 1000), rng.uniform(-2, 5)
        y = (amp * np.exp(-0.5 * ((z - mu) / sig) ** 2) + off + rng.normal(0, 0.02 * amp, n)).astype(np.float32)
        o = pm.analyse(y, fit=True)
        assert o["status"] & (pm.FIT_CONVERGED | pm.FIT_STALLED), o["status"]
        lo, cnt = o["fitFirst"], o["fitCount"]
        zz, yy = z[lo:lo + cnt], y[lo:lo + cnt].astype(np.float64)
        c0 = float(yy.min())
        p0 = [float(y[o["index"]]) - c0, o["position"], max(0.5, o["fwhm"] / pm.FWHM_PER_SIGMA), c0]
        ref = _scipy_fit(zz, yy, p0)
        got = np.array([o["amplitude"], o["center"], o["sigma"], o["offset"]])
        ref[2] = abs(ref[2])
        # relative to the parameter, and to the peak's own scale for the offset and the centre (amplitude, sigma)
        scale = np.maximum(np.abs(ref), [0.0, ref[2], 0.0, abs(ref[0])])
        assert np.all(np.abs(got - ref) <= 1e-6 * scale), (i, got, ref)


def test_fit_recovers_noise_free_gaussians():
    rng = np.random.default_rng(5)
    for i in range(40):
        n = 300
        z = np.arange(n, dtype=np.float64)
        mu, sig = rng.uniform(50, 250), rng.uniform(1.0, 20)
        y = (500.0 * np.exp(-0.5 * ((z - mu) / sig) ** 2) + 3.0).astype(np.float32)
        o = pm.analyse(y, fit=True)
        # (at the rounding floor of float32 data no step lowers the cost any more: converged or stalled there)
        assert o["status"] & (pm.FIT_CONVERGED | pm.FIT_STALLED)
        assert abs(o["center"] - mu) <= 1e-5 and abs(o["sigma"] - sig) <= 1e-5, (i, o["center"] - mu, o["sigma"] - sig)
        assert o["fitFwhm"] == pm.FWHM_PER_SIGMA * o["sigma"]


def test_fit_states():
    # a window below 5 samples
    o = pm.analyse(f32([0, 1, 5, 1]), fit=True)
    assert o["status"] & pm.FIT_SKIPPED and o["fitCount"] == 4 and np.isnan(o["center"])
    # fit off: no fit bit, fit fields NaN
    o = pm.analyse(f32([0, 1, 5, 1, 0, 0]))
    assert not o["status"] & pm.FIT_BITS and np.isnan(o["amplitude"]) and o["fitCount"] == 0
    # an exact Gaussian plus offset on a grid of dyadic values converges; one iteration is not enough from a poor start
    z = np.arange(64.0)
    y = f32(100 * np.exp(-0.5 * ((z - 30.3) / 4.0) ** 2) + 1)
    assert pm.analyse(y, fit=True, max_iterations=1)["status"] & pm.FIT_MAX_ITER
    o = pm.analyse(y, fit=True, fit_half_width=10)
    assert o["fitFirst"] == 20 and o["fitCount"] == 21 and o["status"] & pm.FIT_CONVERGED and o["iterations"] >= 1


# ---------------------------------------------------------------------------------------------------------------------- kernels
def _kernel_meta(text, name):
    start = text.index(name + ":")
    meta = text[start:]
    return int(re.search(r"; ScratchSize: (\d+)", meta).group(1)), int(re.search(r"; NumVgprs: (\d+)", meta).group(1))


def test_peak_kernels_need_no_scratch(tmp_path):
    """every instance of oct_peak_kernel and the partials kernel: no private memory, at most 128 VGPRs"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / "peak_analysis.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-S", "--cuda-device-only", "-o", out, "peak_analysis_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^(_ZN3oct15oct_peak_kernelILb[01]ELb[01]EEEvNS_8PeakArgsE):", text, re.M)
    assert len(names) == 4
    names.append("_ZN3oct24oct_peak_partials_kernelENS_8PeakArgsE")
    for name in names:
        scratch, vgprs = _kernel_meta(text, name)
        assert scratch == 0 and vgprs <= 128, (name, scratch, vgprs)

"""Dispersion estimation without a device: the ABI surface, the argument checks that need no GPU, the Python helpers' arithmetic, the
float64 metric model and the register budget of the sweep kernel (include/octpipe.h "dispersion estimation")."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dispersion_model as dm
from octproz_amd import _lib
from octproz_amd.pipeline import center_ascans, dispersion_metric_code, dispersion_range, first_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

PUBLIC = ["octpipe_dispersion_scores", "octpipe_estimate_dispersion"]
DEBUG = ["octpipe_debug_dispersion_metrics", "octpipe_debug_dispersion_phasors"]


def test_new_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    pub = open(os.path.join(ROOT, "include", "octpipe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "octpipe_debug.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in _lib.OCTPIPE_SYMBOLS and hasattr(L, name)
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and name in _lib.OCTPIPE_DEBUG_SYMBOLS and hasattr(L, name)
    # the metric struct mirror: 8 fields of 4 bytes, OCTPIPE_METRIC_* as in the header
    assert C.sizeof(_lib.DispersionMetric) == 32
    for name, value in (("SUM_ABOVE_THRESHOLD", 0), ("SAMPLES_ABOVE_THRESHOLD", 1), ("PEAK_VALUE", 2), ("MEAN_SOBEL", 3)):
        assert re.search(r"OCTPIPE_METRIC_%s = %d" % (name, value), pub)
        assert getattr(_lib, "METRIC_" + name) == value


def test_null_handles_give_status_codes():
    L = _lib.lib()
    m = _lib.DispersionMetric(0, 1, 0, 1, 2, 0.0, 0.0, 0.0)
    d = np.zeros(4, np.float32)
    raw = np.zeros(16, np.uint16)
    out = np.zeros(4, np.float32)
    b2, b3 = C.c_float(), C.c_float()
    assert L.octpipe_dispersion_scores(None, raw.ctypes.data, 0, C.byref(m), d.ctypes.data, d.ctypes.data, 4, out.ctypes.data) == 1
    assert L.octpipe_estimate_dispersion(None, raw.ctypes.data, 0, C.byref(m), -1.0, 1.0, -1.0, 1.0, 4, None, None, C.byref(b2), C.byref(b3)) == 1
    assert L.octpipe_debug_dispersion_metrics(None, raw.ctypes.data, 0, C.byref(m), d.ctypes.data, d.ctypes.data, 4, out.ctypes.data, None, None) == 1
    assert L.octpipe_debug_dispersion_phasors(None, 0.0, 0.0, d.ctypes.data, d.ctypes.data, 4, None, out.ctypes.data) == 1
    assert b"null handle" in L.octpipe_last_error()


def test_candidate_range_rule():
    c = dispersion_range(-100, 100, 50)
    assert c.dtype == np.float32 and len(c) == 50
    assert c[0] == np.float32(-100) and c[-1] == np.float32(100)
    for i in (0, 1, 17, 49):  # (float)(start + (end - start) * (double)i / (samples - 1))
        assert c[i] == np.float32(-100.0 + 200.0 * i / 49.0)
    assert list(dispersion_range(3.5, 9.0, 1)) == [np.float32(3.5)]
    assert dispersion_range(-100, 100, 51)[25] == 0.0  # an odd count puts 0 on the grid
    # end - start is a float32 subtraction
    s, e = np.float32(0.1), np.float32(1e8)
    assert dispersion_range(s, e, 3)[1] == np.float32(float(s) + float(np.float32(e - s)) * 0.5)
    with pytest.raises(ValueError):
        dispersion_range(0, 1, 0)


def test_centre_ascans_and_best_candidate():
    assert center_ascans(0, 512, 40) == 236
    assert center_ascans(3, 512, 40) == 3 * 512 + 236
    assert center_ascans(1, 64, 64) == 64
    assert center_ascans(0, 65, 40) == 12
    with pytest.raises(ValueError):
        center_ascans(0, 32, 40)
    assert first_max([1.0, 3.0, np.nan, 3.0]) == 1
    assert first_max([np.nan, -2.0, -1.0]) == 2
    assert first_max([np.nan, np.nan]) is None
    assert [dispersion_metric_code(n) for n in ("sum", "samples", "peak", "sobel")] == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        dispersion_metric_code("contrast")


@pytest.mark.parametrize("kind", dm.METRICS)
@pytest.mark.parametrize("ignore", [0, 1, 20])
def test_metric_model_agrees_with_a_per_bin_loop(kind, ignore):
    rng = np.random.default_rng(kind * 7 + ignore)
    v = rng.normal(0.0, 1.0, size=(5, 64))
    v[2, 30] = 9.0
    thr = 0.25
    np.testing.assert_allclose(dm.metric(v, kind, thr, ignore), dm.metric_naive(v, kind, thr, ignore), rtol=1e-12, atol=1e-12)


def test_metric_bounds_cover_perturbations_inside_the_per_bin_bound():
    rng = np.random.default_rng(11)
    v = rng.normal(0.0, 1.0, size=(6, 128))
    b = np.full_like(v, 1e-3)
    for kind in dm.METRICS:
        for _ in range(20):
            w = v + rng.uniform(-1.0, 1.0, size=v.shape) * b
            err = np.abs(dm.metric(w, kind, 0.1, 3) - dm.metric(v, kind, 0.1, 3))
            assert np.all(err <= dm.metric_bound(v, b, kind, 0.1, 3)), kind


def test_per_bin_bound_follows_the_amplitude_policy():
    import common
    from octproz_amd import OctAlgorithmParameters
    p = OctAlgorithmParameters()
    P = np.array([[1e6, 1e4, 1.0, 0.0]])
    lin = dm.per_bin_bound(P, p, 8, True)
    sA, _ = dm.grey_scaling(p, 8, True)
    assert np.allclose(lin - np.spacing(np.abs(dm.values_from_power(P, p, 8, True)).astype(np.float32)), sA * common.amp_rtol(8) * 1e3)
    log = dm.per_bin_bound(P, p, 8, False)
    assert np.isfinite(log[0, :3]).all() and np.isinf(log[0, 3])  # an amplitude inside the bound: no bound in dB
    assert log[0, 0] < log[0, 1] < log[0, 2]


@pytest.mark.parametrize("log2n", [8, 9, 10, 11, 12])
def test_sweep_kernel_needs_no_scratch(log2n, tmp_path):
    """oct_dispersion_sweep_kernel<LOG2N> as csrc/Makefile builds it: no private memory (spills) at any supported length"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path / ("sweep_%d.s" % log2n))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value",
                           "-DOCT_LOG2N=%d" % log2n, "-S", "--cuda-device-only", "-o", out, "dispersion_sweep_inst.hip"], cwd=CSRC,
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    name = "_ZN3oct27oct_dispersion_sweep_kernelILi%dEEEvNS_9SweepArgsE" % log2n
    start = text.index(name + ":")
    meta = text[start:text.index("s_endpgm", start) + 20000]
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; NumVgprs: (\d+)", meta).group(1)) <= 256

"""Dispersion estimation on the MI355X (include/octpipe.h "dispersion estimation", csrc/dispersion_sweep.h, csrc/pipe_dispersion.hip).

The sweep's per-(candidate, A-scan) metrics are held against a float64 model built from the oracle's stages (tests/dispersion_model.py)
and against the product's own processed image of the same candidate; bounds follow from the suite's frozen per-bin amplitude policy
(common.amp_rtol) as dispersion_model.py states.  Then: recovery of a known dispersion, no side effects on the processing chain,
determinism, argument errors and the device-built phasors."""
import ctypes as C

import numpy as np
import pytest

import dispersion_model as dm
from oracle import octref
from octproz_amd import INTERPOLATION, OctAlgorithmParameters, OctPipeError, Pipeline, WindowType, _lib, v180_benchmark_params
from octproz_amd.params import dispersion_curve
from octproz_amd.pipeline import dispersion_range

pytestmark = pytest.mark.gpu

LENGTHS = [256, 512, 1024, 2048, 4096]
INTERPS = [None, INTERPOLATION.LINEAR, INTERPOLATION.CUBIC, INTERPOLATION.LANCZOS]
CANDIDATES = [(0.0, 0.0), (30.0, -10.0), (-60.0, 45.0)]


def make_params(n, a=32, b=2, interp=None, roll=False, linear=False):
    p = OctAlgorithmParameters()
    p.samplesPerLine, p.ascansPerBscan, p.bscansPerBuffer, p.bitDepth = n, a, b, 12
    p.signalLogScaling = 0 if linear else 1
    p.signalGrayscaleMin, p.signalGrayscaleMax = -30.0, 100.0
    p.windowing, p.window, p.windowCenter, p.windowFillFactor = 1, WindowType.Hanning, 0.5, 0.95
    p.d0, p.d1 = 0.0, 20.0
    if interp is not None:
        s = n / 1024.0
        p.resampling, p.resamplingInterpolation = 1, int(interp)
        p.c0, p.c1, p.c2, p.c3 = 0.535239, 871.817574 * s, -170.633784 * s, 97.249716 * s
    p.backgroundRemoval, p.rollingAverageWindowSize = (1 if roll else 0), 8
    p.update_all_curves()
    return p


def _fetch(ptr, count, dtype):
    hip = C.CDLL("libamdhip64.so")
    out = np.empty(count, dtype=dtype)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def _check_matrix(got, v, b, kind, thr, ignore, what):
    want = dm.metric(v, kind, thr, ignore)
    bound = dm.metric_bound(v, b, kind, thr, ignore)
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)
    assert not bad.any(), "%s metric %d: got %s want %s bound %s" % (what, kind, got[bad][:4], want[bad][:4], bound[bad][:4])


# ---------------------------------------------------------------------------------------------------------------------- 1. model
@pytest.mark.parametrize("interp", INTERPS, ids=["none", "linear", "cubic", "lanczos"])
@pytest.mark.parametrize("n", LENGTHS)
def test_metric_matrix_matches_the_float64_model(n, interp):
    M = 8
    d2s = np.array([c[0] for c in CANDIDATES], np.float32)
    d3s = np.array([c[1] for c in CANDIDATES], np.float32)
    for roll in (False, True):
        p = make_params(n, interp=interp, roll=roll)
        raw = dm.layered_raw(p, 30.0, -10.0, seed=n + 3 * (interp or 0))
        pipe = Pipeline(p, device=0)
        lines = p.ascansPerBscan * p.bscansPerBuffer
        for first in (0, 28, lines - M):  # buffer line 0 (the Lanczos first-line offset), across a B-scan border, the last line
            P = [dm.model_power(raw, p, p.d0, p.d1, d2, d3, first, M) for d2, d3 in CANDIDATES]
            for linear in (True, False):
                v = [dm.values_from_power(x, p, n, linear) for x in P]
                b = [dm.per_bin_bound(x, p, n, linear) for x in P]
                thr = float(np.median(v[1]))
                for kind in dm.METRICS:
                    for ignore in (0, 20):
                        mat, sc, _ = pipe.dispersion_metrics(raw, d2s, d3s, first, M, kind, thr, ignore, linear)
                        for c in range(len(CANDIDATES)):
                            _check_matrix(mat[c], v[c], b[c], kind, thr, ignore,
                                          "N=%d interp=%s roll=%d first=%d lin=%d ignore=%d cand=%s" % (n, interp, roll, first, linear, ignore, CANDIDATES[c]))
                        np.testing.assert_allclose(sc, mat.astype(np.float64).mean(axis=1), rtol=1e-6, atol=1e-6)
        pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. product
@pytest.mark.parametrize("n,interp", [(1024, INTERPOLATION.CUBIC), (2048, INTERPOLATION.LANCZOS), (4096, INTERPOLATION.LINEAR), (512, None)])
def test_sweep_metrics_equal_the_products_image(n, interp):
    """candidate c's curve set on the handle, the buffer processed by the product: numpy metrics of those rows equal the sweep's
    per-A-scan metrics within the per-bin bound of each side"""
    a, bsc, M, first = 64, 2, 12, 40
    for linear in (False, True):
        p = make_params(n, a, bsc, interp=interp, roll=True, linear=linear)
        raw = dm.layered_raw(p, -20.0, 15.0, seed=n)
        pipe = Pipeline(p, device=0)
        for d2, d3 in CANDIDATES:
            mats = {}
            for kind in dm.METRICS:
                thr = 0.0
                mats[kind] = pipe.dispersion_metrics(raw, [d2], [d3], first, M, kind, thr, 20, linear)[0][0]
            p.dispersionCompensation, p.d2, p.d3 = 1, d2, d3
            p.fixedPatternNoiseRemoval = p.postProcessBackgroundRemoval = p.bscanFlip = p.sinusoidalScanCorrection = 0
            p.updateDispersionCurve()
            pipe.octCudaPipeline(raw)
            pipe.synchronize()
            rows = pipe.processed_host().reshape(a * bsc, n // 2)[first:first + M].astype(np.float64)
            P = dm.model_power(raw, p, p.d0, p.d1, d2, d3, first, M)
            v, b = dm.values_from_power(P, p, n, linear), dm.per_bin_bound(P, p, n, linear)
            for kind in dm.METRICS:
                thr = 0.0
                got = dm.metric(rows, kind, thr, 20)
                bound = 2.0 * dm.metric_bound(v, b, kind, thr, 20)  # both sides within the per-bin bound of the model
                assert np.all(np.abs(got - mats[kind]) <= bound), (n, linear, d2, d3, kind, got, mats[kind], bound)
            p.dispersionCompensation = 0
        pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 3. recovery
def _recovery_params():
    # (the rolling average removes the DC term: a constant times a chirped phasor is spread over every depth and outweighs the
    # reflectors at large |d2| -- in the extension's use the background removal is on for the same reason)
    p = make_params(1024, 64, 2, interp=None, roll=True, linear=False)
    p.d0, p.d1 = 0.0, 0.0
    return p


def test_estimate_recovers_a_known_dispersion():
    p = _recovery_params()
    c = dispersion_range(-100, 100, 51)  # step 4, 0 on the grid
    d2_true = float(c[35])
    assert d2_true == 40.0
    raw = dm.layered_raw(p, d2_true, 0.0, seed=21)
    pipe = Pipeline(p, device=0)
    # the product itself: its image is sharpest (PEAK) at (d2*, 0) against the grid neighbours
    first = (p.ascansPerBscan - 40) // 2
    peaks = {}
    for d2 in (d2_true - 4.0, d2_true, d2_true + 4.0):
        p.dispersionCompensation, p.d2, p.d3 = 1, d2, 0.0
        p.updateDispersionCurve()
        pipe.octCudaPipeline(raw)
        pipe.synchronize()
        rows = pipe.processed_host().reshape(-1, 512)[first:first + 40]
        peaks[d2] = dm.metric(rows, dm.PEAK, 0.0, 20).mean()
    p.dispersionCompensation = 0
    assert peaks[d2_true] > peaks[d2_true - 4.0] and peaks[d2_true] > peaks[d2_true + 4.0], peaks
    est = pipe.estimate_dispersion(raw, metric="peak", samples=51)
    assert (est.d2, est.d3) == (d2_true, 0.0), (est, est.d2_scores, est.d3_scores)
    assert len(est.d2_scores) == 51 and len(est.d3_scores) == 51
    assert int(np.argmax(est.d2_scores)) == 35
    # the axial-gradient metric on log values: on isolated point reflectors its maximum lies within one grid step of d2* (the
    # float64 model of tests/dispersion_model.py puts it at d2* - 4 for this sample: the ripple of a slightly defocused peak adds
    # gradient), and at d3 = 0
    est = pipe.estimate_dispersion(raw, metric="sobel", linear=False, samples=51)
    assert abs(est.d2 - d2_true) <= 4.0 and est.d3 == 0.0, (est, est.d2_scores, est.d3_scores)
    # d3* != 0: the full grid in one call
    d3_true = float(c[19])
    assert d3_true == -24.0
    raw3 = dm.layered_raw(p, d2_true, d3_true, seed=22)
    est = pipe.estimate_dispersion(raw3, metric="peak", samples=51, grid=True)
    assert est.grid.shape == (51, 51)
    assert (est.d2, est.d3) == (d2_true, d3_true), est
    # apply=True: the result reaches params and the handle's curve
    est = pipe.estimate_dispersion(raw, metric="peak", samples=51, apply=True)
    assert (p.d2, p.d3) == (d2_true, 0.0)
    np.testing.assert_array_equal(p.dispersionCurve, dispersion_curve(p.d0, p.d1, d2_true, 0.0, 1024))
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. side effects
def test_a_sweep_leaves_the_processing_chain_untouched():
    n, a, b = 1024, 64, 2
    p = v180_benchmark_params(n, a, b)
    p.volumeViewEnabled = 1
    p.continuousFixedPatternNoiseDetermination = 0
    raw = dm.layered_raw(p, 10.0, 0.0, seed=31)
    other = dm.layered_raw(p, -40.0, 5.0, seed=32)
    pipe = Pipeline(p, device=0)
    pipe.enable_kernel_timing(True)

    def state():
        pipe.synchronize()
        (pb, nb), (pe, ne) = pipe.display_buffers()
        vp, vn = pipe.volume_view_buffer()
        return (pipe.processed_host(), pipe.mean_line(), _fetch(pb, nb, np.float32), _fetch(pe, ne, np.float32), _fetch(vp, vn, np.uint8))

    pipe.octCudaPipeline(raw)
    before = state()
    _, launches = pipe.kernel_timing(reset=False)
    pipe.dispersion_scores(other, [-40.0, 0.0, 12.0], [5.0, 0.0, -3.0], 30, 40, "sobel", linear=False)
    pipe.estimate_dispersion(other, samples=9)
    assert pipe.kernel_timing(reset=False)[1] == launches
    pipe.octCudaPipeline(raw)
    after = state()
    for x, y in zip(before, after):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    assert pipe.kernel_timing(reset=False)[1] == launches + 1
    # a pending fixed-pattern-noise redetermination (one-shot) survives a sweep: the next buffer consumes it
    p.redetermineFixedPatternNoise = 1
    pipe._sync_params()
    pipe.dispersion_scores(raw, [0.0], [0.0], 0, 8, "peak")
    pipe.octCudaPipeline(other)
    pipe.synchronize()
    fresh = Pipeline(p, device=0)
    fresh.octCudaPipeline(other)
    fresh.synchronize()
    assert np.array_equal(pipe.mean_line().view(np.uint32), fresh.mean_line().view(np.uint32))
    assert not np.array_equal(pipe.mean_line().view(np.uint32), before[1].view(np.uint32))
    fresh.close()
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. determinism
def test_scores_are_deterministic_and_independent_of_chunking():
    import torch
    p = make_params(1024, 64, 2, interp=INTERPOLATION.CUBIC, roll=True)
    raw = dm.layered_raw(p, 25.0, -5.0, seed=41)
    pipe = Pipeline(p, device=0)
    c = dispersion_range(-100, 100, 64)
    d2, d3 = np.repeat(c, 64), np.tile(c, 64)
    for kind in ("sum", "samples", "peak", "sobel"):
        host = pipe.dispersion_scores(raw, d2, d3, 12, 40, kind, threshold=20.0, ignore_first=20, linear=False)
        again = pipe.dispersion_scores(raw, d2, d3, 12, 40, kind, threshold=20.0, ignore_first=20, linear=False)
        d_raw = torch.from_numpy(raw.view(np.int16)).to("cuda:0")
        torch.cuda.synchronize()
        dev = pipe.dispersion_scores(d_raw, d2, d3, 12, 40, kind, threshold=20.0, ignore_first=20, linear=False)
        parts = np.concatenate([pipe.dispersion_scores(raw, d2[i:i + 1024], d3[i:i + 1024], 12, 40, kind, threshold=20.0, ignore_first=20,
                                                       linear=False) for i in range(0, 4096, 1024)])
        for x in (again, dev, parts):
            assert np.array_equal(host.view(np.uint32), x.view(np.uint32)), kind
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 6. errors
def test_invalid_arguments_and_unsupported_lengths():
    n, a, b = 1024, 32, 2
    p = make_params(n, a, b, interp=INTERPOLATION.CUBIC)
    raw = dm.layered_raw(p, 0.0, 0.0, seed=51)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    want = pipe.processed_host()
    L = _lib.lib()
    d = np.zeros(2, np.float32)
    out = np.zeros(2, np.float32)

    def call(first, count, ignore, metric, k=2, raw_ptr=raw.ctypes.data):
        m = _lib.DispersionMetric(first, count, ignore, 1, metric, 0.0, 0.0, 0.0)
        return L.octpipe_dispersion_scores(pipe.handle, raw_ptr, 0, C.byref(m), d.ctypes.data, d.ctypes.data, k, out.ctypes.data)

    assert call(0, 8, 0, 2) == 0
    for args in [(60, 5, 0, 2), (0, 0, 0, 2), (0, 8, n // 2 - 2, 2), (0, 8, 0, 4), (0, 8, 0, -1)]:
        assert call(*args) == 1, args
        assert L.octpipe_last_error()
    assert call(0, 8, 0, 2, k=0) == 1
    assert call(0, 8, 0, 2, raw_ptr=None) == 1
    m = _lib.DispersionMetric(0, 8, 0, 1, 2, 0.0, 0.0, 0.0)
    b2, b3 = C.c_float(), C.c_float()
    assert L.octpipe_estimate_dispersion(pipe.handle, raw.ctypes.data, 0, C.byref(m), -1.0, 1.0, -1.0, 1.0, 0, None, None, C.byref(b2), C.byref(b3)) == 1
    assert L.octpipe_estimate_dispersion(pipe.handle, raw.ctypes.data, 0, C.byref(m), float("nan"), 1.0, -1.0, 1.0, 4, None, None, C.byref(b2), C.byref(b3)) == 1
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    assert np.array_equal(pipe.processed_host().view(np.uint32), want.view(np.uint32))
    pipe.close()
    for bad in (1664, 1000, 8192):
        q = make_params(bad, 8, 2)
        qp = Pipeline(q, device=0)
        qraw = np.full(bad * 16, 2000, np.uint16)
        with pytest.raises(OctPipeError) as e:
            qp.dispersion_scores(qraw, [0.0], [0.0], 0, 4)
        assert e.value.code == 5 and "256, 512, 1024, 2048 and 4096" in str(e.value)
        with pytest.raises(OctPipeError) as e:
            qp.estimate_dispersion(qraw, ascans_from_center=4, ignore_first=0, samples=3)
        assert e.value.code == 5
        qp.octCudaPipeline(qraw)  # the handle keeps processing
        qp.synchronize()
        qp.close()


def test_all_nan_scores_have_no_best_candidate():
    p = make_params(512, 16, 2)
    raw = dm.layered_raw(p, 0.0, 0.0, seed=52)
    pipe = Pipeline(p, device=0)
    sc = pipe.dispersion_scores(raw, [np.nan, np.inf], [0.0, 0.0], 0, 4, "peak")
    assert np.isnan(sc).all()
    L = _lib.lib()
    # d1 + d2 beyond the float range: theta overflows at the last samples, cos(inf) is NaN, every A-scan's peak is NaN
    m = _lib.DispersionMetric(0, 4, 0, 1, 2, 0.0, 0.0, 3.4e38)
    b2, b3 = C.c_float(), C.c_float()
    rc = L.octpipe_estimate_dispersion(pipe.handle, raw.ctypes.data, 0, C.byref(m), 3e38, 3.4e38, 0.0, 0.0, 3, None, None, C.byref(b2), C.byref(b3))
    assert rc == 1 and b"NaN" in L.octpipe_last_error()
    pipe.close()


def test_a_call_from_a_data_callback_is_refused():
    n, a, b = 1024, 32, 2
    p = make_params(n, a, b)
    p.streamFloatToHost = 1
    raw = dm.layered_raw(p, 0.0, 0.0, seed=53)
    pipe = Pipeline(p, device=0)
    S2 = n * a * b // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])
    seen = {}
    d = np.zeros(1, np.float32)
    out = np.zeros(1, np.float32)
    m = _lib.DispersionMetric(0, 4, 0, 1, 2, 0.0, 0.0, 0.0)

    def on_float(*args):
        L = _lib.lib()
        seen["scores"] = L.octpipe_dispersion_scores(pipe.handle, raw.ctypes.data, 0, C.byref(m), d.ctypes.data, d.ctypes.data, 1, out.ctypes.data)
        b2, b3 = C.c_float(), C.c_float()
        seen["estimate"] = L.octpipe_estimate_dispersion(pipe.handle, raw.ctypes.data, 0, C.byref(m), 0.0, 1.0, 0.0, 1.0, 2, None, None, C.byref(b2), C.byref(b3))

    pipe.set_callbacks(on_float_streaming=on_float)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    assert seen == {"scores": 7, "estimate": 7}
    pipe.dispersion_scores(raw, [0.0], [0.0], 0, 4)  # outside the callback: fine
    pipe.unregister_float_streaming_buffers()
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 7. phasors
@pytest.mark.parametrize("n", LENGTHS)
def test_device_phasors_equal_the_host_curve(n):
    p = make_params(n, 8, 2)
    pipe = Pipeline(p, device=0)
    rng = np.random.default_rng(n)
    d2 = np.concatenate([[0.0, -100.0, 100.0, 400.0], rng.uniform(-300, 300, 12)]).astype(np.float32)
    d3 = np.concatenate([[0.0, 100.0, -100.0, -250.0], rng.uniform(-300, 300, 12)]).astype(np.float32)
    d0, d1 = 1.5, 97.0
    theta, ph = pipe.dispersion_phasors(d2, d3, d0, d1)
    for c in range(len(d2)):
        curve = dispersion_curve(d0, d1, float(d2[c]), float(d3[c]), n)
        assert np.array_equal(theta[c].view(np.uint32), curve.view(np.uint32)), c
        host = octref.dispersive_phase(curve)
        assert np.abs(ph[c].real - host.real).max() <= 2.0 ** -22 and np.abs(ph[c].imag - host.imag).max() <= 2.0 ** -22, c
    pipe.close()

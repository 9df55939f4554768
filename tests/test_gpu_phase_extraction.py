"""Phase extraction on the MI355X (include/octpipe.h "phase extraction", csrc/phase_extract.h, csrc/pipe_phase.hip).

The accumulated mean is held bit-exact against numpy int64 sums in every sample format; spectrum, envelope, phase and curve against
the float64 model of tests/phase_model.py; the curve against the analytic one; and the product's own processed A-scan after
apply="curve" / "coeffs" against the imaging thresholds the CPU suite confirmed on the model.  Then: side effects, determinism and
argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import dispersion_model as dm
import phase_model as pm
from octproz_amd import INTERPOLATION, OctAlgorithmParameters, OctPipeError, Pipeline, VirtualOCTSystem, WindowType, _lib
from octproz_amd.pipeline import dispersion_range
from phase_cases import _encode, _random_ints

pytestmark = pytest.mark.gpu

LENGTHS = [256, 512, 1024, 2048, 4096]
# parity bounds of the device against the float64 model (float32 transforms; phase and curve in float64 on the device).  Measured
# maxima are recorded in DESIGN.md 5.10.
SPECTRUM_RTOL = 1e-5   # of the spectrum's maximum
CURVE_ATOL = 1e-3      # samples
RECOVERY_BOUND = 0.05  # tests/test_phase_extraction.py


def make_params(n, a=32, b=2, bit_depth=12):
    p = OctAlgorithmParameters()
    p.samplesPerLine, p.ascansPerBscan, p.bscansPerBuffer, p.bitDepth = n, a, b, bit_depth
    p.update_all_curves()
    return p


# ---------------------------------------------------------------------------------------------------------------------- 1. accumulate
FORMATS = [(0, 8), (0, 12), (0, 32), (1, 12), (2, 12), (3, 8), (4, 16), (5, 32)]


@pytest.mark.parametrize("fmt,bit_depth", FORMATS, ids=["u8", "u16", "u32", "p12u", "p12s", "i8", "i16", "i32"])
def test_mean_is_bit_exact_in_every_format(fmt, bit_depth):
    n, a, b = 1024, 64, 8
    lines = a * b
    rng = np.random.default_rng(fmt * 10 + bit_depth)
    for bitshift in (0, 1):
        p = make_params(n, a, b, bit_depth)
        p.bitshift = bitshift
        pipe = Pipeline(p, device=0, sample_format=fmt)
        bufs = []
        for i in range(3):
            raw, dec = _encode(_random_ints(rng, (lines, n), fmt, bit_depth), fmt, bit_depth)
            bufs.append((raw, dec))
        u32 = fmt == 0 and bit_depth > 16
        val = [d if (not bitshift or u32) else (d >> 4) for _, d in bufs]
        scale = 2.0 ** -32 if (u32 and bitshift) else 1.0
        # host raw, device raw, several buffers; the first over 8 calls of 64 A-scans
        pipe.phase_reset()
        for q in range(8):
            pipe.phase_accumulate(bufs[0][0], q * 64, 64)
        m8, c8 = pipe.phase_mean()
        pipe.phase_reset()
        pipe.phase_accumulate(torch.from_numpy(bufs[0][0].reshape(-1).view(np.uint8).copy()).cuda(), 0, lines)
        m1, c1 = pipe.phase_mean()
        assert c8 == c1 == lines
        want = ((val[0].sum(axis=0) / lines) * scale).astype(np.float32)
        assert np.array_equal(m8.view(np.uint32), m1.view(np.uint32))
        assert np.array_equal(m1.view(np.uint32), want.view(np.uint32)), (fmt, bit_depth, bitshift)
        pipe.phase_accumulate(bufs[1][0])
        pipe.phase_accumulate(torch.from_numpy(bufs[2][0].reshape(-1).view(np.uint8).copy()).cuda(), 100, 300)
        m, c = pipe.phase_mean()
        tot = val[0].sum(axis=0) + val[1].sum(axis=0) + val[2][100:400].sum(axis=0)
        assert c == 2 * lines + 300
        assert np.array_equal(m.view(np.uint32), ((tot / c) * scale).astype(np.float32).view(np.uint32))
        pipe.close()


@pytest.mark.parametrize("n", [1000, 1664, 130])
def test_accumulate_works_at_lengths_without_extraction(n):
    """every samplesPerLine accumulates, and extract answers UNSUPPORTED.  Rows of 1000 and 1664 uint16 samples are multiples of 16
    bytes and take the vector form from the staged copy and from the aligned tensor; only N = 130 (260 bytes) takes the scalar
    form here.  tests/test_gpu_phase_crafted.py runs the scalar form in every format."""
    p = make_params(n, 16, 2)
    rng = np.random.default_rng(n)
    raw = rng.integers(0, 4096, size=(32, n)).astype(np.uint16)
    pipe = Pipeline(p, device=0)
    pipe.phase_reset()
    pipe.phase_accumulate(raw, 3, 20)
    pipe.phase_accumulate(torch.from_numpy(raw).cuda())
    m, c = pipe.phase_mean()
    want = ((raw[3:23].astype(np.int64).sum(axis=0) + raw.astype(np.int64).sum(axis=0)) / 52.0).astype(np.float32)
    assert c == 52 and np.array_equal(m, want)
    with pytest.raises(OctPipeError) as e:
        pipe.extract_resample_curve(peak=(10, 40))
    assert e.value.code == 5  # OCTPIPE_ERR_UNSUPPORTED
    pipe.close()


def test_mean_of_the_buffers_the_acquisition_loop_delivers():
    n, a, b, nbuf = 1024, 64, 4, 5
    p = make_params(n, a, b)
    data = np.concatenate([pm.calibration_raw(n, a * b, seed=40 + i).reshape(-1) for i in range(nbuf)])
    system = VirtualOCTSystem(12, a, b, n, data=data, buffers_from_file=nbuf)
    pipe = Pipeline(p, device=0)
    pipe.phase_reset()
    got = []
    bytes_ = a * b * n * 2

    def consume(ptr, nr):
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(bytes_,)).view(np.uint16).copy()
        got.append(arr)
        pipe.phase_accumulate(arr)
        return 0

    system.startAcquisition()
    rc, stats = system.run_processing(consume, max_buffers=nbuf)
    system.stopAcquisition()
    system.close()
    assert rc == 0
    m, c = pipe.phase_mean()
    assert c == len(got) * a * b and len(got) >= 1
    want = (np.sum([g.reshape(-1, n).astype(np.int64).sum(axis=0) for g in got], axis=0) / c).astype(np.float32)
    assert np.array_equal(m, want)
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. model
@pytest.mark.parametrize("n", LENGTHS)
def test_extraction_matches_the_float64_model(n):
    p = make_params(n, 32, 2)
    raw = pm.calibration_raw(n, 64, seed=n + 1)
    pipe = Pipeline(p, device=0)
    ig = n // 16
    worst = {}
    for window_raw in (False, True):
        for hann in (False, True):
            res = pipe.extract_resample_curve(raws=raw, peak=(int(0.2 * n), int(0.4 * n)), window_raw=window_raw, hann_peak=hann,
                                              ignore_first=ig, ignore_last=ig)
            want = pm.extract(res.mean, int(0.2 * n), int(0.4 * n), window_raw, hann, ig, ig)
            a, b = want["a"], want["b"]
            assert np.array_equal(res.mean, raw.astype(np.float64).mean(axis=0).astype(np.float32))
            smax = want["spectrum"].max()
            es = np.abs(res.spectrum - want["spectrum"]).max() / smax
            ee = np.abs(res.envelope - want["envelope"]).max() / want["envelope"].max()
            ep = np.abs(res.phase[a:b + 1] - want["phase"][a:b + 1]).max()
            ec = np.abs(res.curve[a:b + 1] - want["curve"][a:b + 1]).max()
            worst[(window_raw, hann)] = (es, ee, ep, ec)
            assert es <= SPECTRUM_RTOL and ee <= SPECTRUM_RTOL * 10, (n, window_raw, hann, es, ee)
            assert ec <= CURVE_ATOL, (n, window_raw, hann, ec)
            # one float32 ulp at the largest phase of the case: the output is rounded to float32 (half an ulp), the float32 transforms
            # account for the rest (2.5e-4 rad at N = 4096, where the ulp is 4.9e-4)
            assert ep <= np.spacing(np.float32(np.abs(want["phase"]).max())), (n, window_raw, hann, ep)
            np.testing.assert_allclose(res.coeffs, pm.fit_cubic(res.curve, a, b), rtol=1e-5, atol=1e-3)
    print("N=%d parity (spectrum rel, envelope rel, phase rad, curve samples):" % n, worst)
    pipe.close()


@pytest.mark.parametrize("n", LENGTHS)
def test_curve_recovers_the_analytic_curve(n):
    p = make_params(n, 32, 2)
    pipe = Pipeline(p, device=0)
    ig = n // 16
    res = pipe.extract_resample_curve(raws=pm.calibration_raw(n, 64, seed=n), peak=(int(0.2 * n), int(0.4 * n)), ignore_first=ig, ignore_last=ig)
    a, b = ig, n - 1 - ig
    err = np.abs(res.curve[a:b + 1] - pm.analytic_curve(n, a, b)[a:b + 1]).max()
    print("N=%d recovery %.4f" % (n, err))
    assert err <= RECOVERY_BOUND + CURVE_ATOL
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 3. product
def _mirror_raw(n, lines, depth, kmap=pm.k_map):
    return np.rint(2048.0 + 800.0 * pm.mirror(n, depth, kmap)[None, :].repeat(lines, axis=0)).astype(np.uint16)


def _image_params(n, a, b):
    p = make_params(n, a, b)
    p.signalLogScaling = 0
    p.signalGrayscaleMin, p.signalAddend = 0.0, 0.0
    p.windowing, p.window, p.windowCenter, p.windowFillFactor = 1, WindowType.Hanning, 0.5, 1.0
    p.resamplingInterpolation = INTERPOLATION.CUBIC
    p.update_all_curves()
    return p


def _peak(pipe, raw, n):
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    return pm.peak_and_fwhm(pipe.processed_host().reshape(-1, n // 2)[5].astype(np.float64))


def test_apply_restores_the_products_image_and_enables_dispersion_estimation():
    n, a, b = 1024, 64, 2
    depth = 0.1 * n
    calib = pm.calibration_raw(n, a * b, seed=7)
    ref_p = _image_params(n, a, b)
    ref = Pipeline(ref_p, device=0)
    h0, w0 = _peak(ref, _mirror_raw(n, a * b, depth, kmap=lambda u: u), n)
    ref.close()
    for apply in ("curve", "coeffs"):
        p = _image_params(n, a, b)
        pipe = Pipeline(p, device=0)
        hn, wn = _peak(pipe, _mirror_raw(n, a * b, depth), n)
        assert hn < 0.5 * h0
        res = pipe.extract_resample_curve(raws=calib, peak=(int(0.2 * n), int(0.4 * n)), ignore_first=32, ignore_last=32, apply=apply)
        assert p.resampling == 1 and p.useCustomResampleCurve == (apply == "curve")
        if apply == "coeffs":
            assert (p.c0, p.c1, p.c2, p.c3) == tuple(float(c) for c in res.coeffs)
        h, w = _peak(pipe, _mirror_raw(n, a * b, depth), n)
        print("apply=%s: peak %.3f, FWHM %.3f of the linear-k mirror (none: %.3f)" % (apply, h / h0, w / w0, hn / h0))
        assert h >= 0.9 * h0 and w <= 1.2 * w0, (apply, h / h0, w / w0)
        if apply == "coeffs":
            # (the cubic fit of this k-map's curve leaves up to ~1.3 samples at the edges -- its inverse is not a cubic -- which is
            # enough to move a d2 estimate on reflectors at 0.3 N by two grid steps: the dispersion check runs on the measured curve)
            pipe.close()
            continue
        # calibration, then dispersion: a layered sample with d2 = 40 recorded through the same k-nonlinearity
        lp = dm.layered_raw(p, 0.0, 0.0, seed=1)  # (shape only)
        u = np.arange(n, dtype=np.float64) / (n - 1)
        jpos = (n - 1) * pm.k_map(u)  # the linear-k position each raw sample sees
        d2_true = 40.0
        rng = np.random.default_rng(3)
        theta = p.d0 + p.d1 * jpos / (n - 1) + d2_true * (jpos / (n - 1)) ** 2
        sig = 1800.0 + sum(amp * np.cos(2.0 * np.pi * round(z * n) * jpos / n + theta) for z, amp in ((0.09, 350.0), (0.17, 250.0), (0.31, 300.0)))
        raw = np.clip(np.rint(sig[None, :] + rng.normal(0.0, 4.0, size=lp.shape)), 0, 4095).astype(np.uint16)
        p.backgroundRemoval, p.rollingAverageWindowSize = 1, 8
        p.signalLogScaling = 1
        est = pipe.estimate_dispersion(raw, metric="peak", samples=51)
        print("apply=%s: d2 estimate %g" % (apply, est.d2))
        assert abs(est.d2 - d2_true) <= float(dispersion_range(-100, 100, 51)[1] - dispersion_range(-100, 100, 51)[0]), est
        pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. side effects
def test_no_side_effects_and_determinism():
    n, a, b = 1024, 64, 2
    from octproz_amd import v180_benchmark_params
    p = v180_benchmark_params(n, a, b)
    p.continuousFixedPatternNoiseDetermination = 0
    raw = pm.calibration_raw(n, a * b, seed=11)
    pipe = Pipeline(p, device=0)
    pipe.enable_kernel_timing(True)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    before = (pipe.processed_host().copy(), pipe.mean_line().copy())
    _, launches = pipe.kernel_timing(reset=False)
    curve = p.resampleCurve.copy()
    r1 = pipe.extract_resample_curve(raws=[raw, raw], peak=(200, 400), ignore_first=32, ignore_last=32)
    r2 = pipe.extract_resample_curve(peak=(200, 400), ignore_first=32, ignore_last=32)
    for f in ("spectrum", "envelope", "phase", "curve", "coeffs"):
        assert np.array_equal(getattr(r1, f).view(np.uint32), getattr(r2, f).view(np.uint32)), f
    assert r1.count == 2 * a * b
    assert pipe.kernel_timing(reset=False)[1] == launches
    assert np.array_equal(p.resampleCurve, curve)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    after = (pipe.processed_host(), pipe.mean_line())
    for x, y in zip(before, after):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. errors
def test_argument_errors():
    n = 1024
    p = make_params(n, 32, 2)
    pipe = Pipeline(p, device=0)
    L, h = _lib.lib(), pipe.handle
    mean = np.zeros(n, np.float32)
    curve = np.zeros(n, np.float32)
    cnt = C.c_uint64()
    assert L.octpipe_phase_reset(h) == 0
    assert L.octpipe_phase_mean(h, mean.ctypes.data, C.byref(cnt)) == 1  # count 0
    assert L.octpipe_extract_resample_curve(h, None, C.byref(_lib.PhaseExtraction(200, 400, 0, 1, 0, 0)), None, None, None, curve.ctypes.data, None) == 1
    raw = pm.calibration_raw(n, 64, seed=1)
    assert L.octpipe_phase_accumulate(h, raw.ctypes.data, 0, 60, 5) == 1  # past A*B
    assert L.octpipe_phase_accumulate(h, raw.ctypes.data, 0, 0, 0) == 1
    assert L.octpipe_phase_accumulate(h, None, 0, 0, 1) == 1
    good = raw.astype(np.float64).mean(axis=0).astype(np.float32)

    def ex(m, x, out=curve):
        return L.octpipe_extract_resample_curve(h, m.ctypes.data, C.byref(x), None, None, None, out.ctypes.data if out is not None else None, None)

    assert ex(good, _lib.PhaseExtraction(200, 400, 0, 1, 32, 32)) == 0
    for x, field in ((_lib.PhaseExtraction(1, 400, 0, 1, 0, 0), b"peakStart"), (_lib.PhaseExtraction(200, 201, 0, 1, 0, 0), b"peakEnd"),
                     (_lib.PhaseExtraction(200, 512, 0, 1, 0, 0), b"peakEnd"), (_lib.PhaseExtraction(200, 400, 0, 1, 1000, 20), b"ignore")):
        assert ex(good, x) == 1 and field in L.octpipe_last_error(), field
    assert ex(good, _lib.PhaseExtraction(200, 400, 0, 1, 0, 0), out=None) == 1
    bad = good.copy()
    bad[17] = np.nan
    assert ex(bad, _lib.PhaseExtraction(200, 400, 0, 1, 0, 0)) == 1 and b"mean" in L.octpipe_last_error()
    flat = np.full(n, 2048.0, np.float32)
    assert ex(flat, _lib.PhaseExtraction(200, 400, 0, 1, 0, 0)) == 1 and b"no calibration signal" in L.octpipe_last_error()
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.append(L.octpipe_phase_accumulate(h, raw.ctypes.data, 0, 0, 1))
        codes.append(L.octpipe_phase_reset(h))
        codes.append(L.octpipe_extract_resample_curve(h, good.ctypes.data, C.byref(_lib.PhaseExtraction(200, 400, 0, 1, 0, 0)), None, None, None,
                                                      curve.ctypes.data, None))
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    assert codes and set(codes) == {7}, codes
    pipe.close()

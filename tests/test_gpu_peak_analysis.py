"""Peak analysis on the MI355X (include/octpipe.h "peak analysis", csrc/peak_analysis.h, csrc/pipe_peak.hip).

The averaged A-scans, index, value, position, left, right, fwhm and the status bits of steps 1 to 4 are held bit-exact against the
numpy model of tests/peak_model.py on the product's own processed output; the fit against the model and scipy on the groups where it
is well posed.  Then the physics: a mirror's axial PSF, a roll-off sweep in one call, a tilted mirror's surface map.  Then sources,
determinism, side effects and errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import peak_model as pm
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

EXACT = ("index", "position", "left", "right", "fwhm")
FIT = ("amplitude", "center", "sigma", "offset")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check_exact(got, avg, res, what):
    """got: PeakAnalysis with .averaged; avg / res: the model's averaged A-scans and per-group dicts"""
    assert np.array_equal(got.averaged.view(np.uint32), avg.view(np.uint32)), what
    for i, row in enumerate(res):
        for j, o in enumerate(row):
            assert (int(got.status[i, j]) & pm.STEP4_BITS) == o["status"] & pm.STEP4_BITS, (what, i, j, got.status[i, j], o["status"])
            assert _same(got.value[i, j], np.float32(o["value"])), (what, i, j)
            for f in EXACT:
                assert _same(getattr(got, f)[i, j], o[f]), (what, i, j, f, getattr(got, f)[i, j], o[f])


def _check_fit(got, avg, res, s0, what):
    """fits where both ends converged and the peak stands 10 x above the median of its depth window (not a noise-only group): model
    within 1e-7, scipy within 1e-5 (relative to the parameter, for the centre and the offset to the peak's sigma and amplitude)"""
    from scipy.optimize import least_squares
    compared = differ = scipy_done = 0
    worst = 0.0
    for i, row in enumerate(res):
        for j, o in enumerate(row):
            gs = int(got.status[i, j])
            if (gs & pm.FIT_BITS) != (o["status"] & pm.FIT_BITS):
                differ += 1
            if not (gs & o["status"] & pm.FIT_CONVERGED):
                continue
            assert got.fitFirst[i, j] == o["fitFirst"] and got.fitCount[i, j] == o["fitCount"], what
            lo, cnt = o["fitFirst"] - s0, o["fitCount"]
            y = avg[i, j, lo:lo + cnt].astype(np.float64)
            if not o["value"] >= 10.0 * np.median(avg[i, j]):
                continue
            ref = np.array([o[f] for f in FIT])
            g = np.array([getattr(got, f)[i, j] for f in FIT])
            scale = np.maximum(np.abs(ref), [0.0, ref[2], 0.0, abs(ref[0])])
            worst = max(worst, float(np.max(np.abs(g - ref) / scale)))
            assert np.all(np.abs(g - ref) <= 1e-7 * scale), (what, i, j, g, ref)
            compared += 1
            if scipy_done < 8:
                z = np.arange(o["fitFirst"], o["fitFirst"] + cnt, dtype=np.float64)
                c0 = float(y.min())
                p0 = [o["value"] - c0, o["position"], max(0.5, o["fwhm"] / pm.FWHM_PER_SIGMA) if np.isfinite(o["fwhm"]) else 1.0, c0]
                sp = least_squares(lambda p: pm.gauss(z, p) - y, p0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15).x
                sp[2] = abs(sp[2])
                sscale = np.maximum(np.abs(sp), [0.0, sp[2], 0.0, abs(sp[0])])
                assert np.all(np.abs(g - sp) <= 1e-5 * sscale), (what, i, j, g, sp)
                scipy_done += 1
    print("%s: %d fits compared (worst %.2e of scale), %d groups with another fit end state" % (what, compared, worst, differ))
    return compared


# ---------------------------------------------------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("n,log,flip", [(1024, 0, 0), (1024, 1, 1), (1664, 0, 0), (1000, 1, 0)], ids=["1024-lin", "1024-log-flip", "1664-lin", "1000-log"])
def test_product_output_matches_the_model(n, log, flip):
    a, b = 128, 3
    p = v180_benchmark_params(n, a, b)
    p.signalLogScaling, p.bscanFlip = log, flip
    if not log:
        p.signalGrayscaleMin = 0.0  # (linear values without an offset: the background's median is near zero)
    p.update_all_curves()
    pipe = Pipeline(p, device=0)
    # the product's test signal plus a mirror whose depth moves with the A-scan (the mean-line subtraction keeps it): well-posed fits
    ai, bi = np.meshgrid(np.arange(a), np.arange(b))
    mirror = _mirror_raw(n, 0.15 * n + 0.37 * ai + 11.0 * bi + 0.3, 900.0).astype(np.float64) - 2048.0
    raw = np.clip(synthetic_raw(n, a, b, seed=n + log).astype(np.float64) + mirror, 0, 4095).astype(np.uint16)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    vol = pipe.processed_host().reshape(b, a, n // 2).copy()
    fitted = 0
    cases = [(None, None, None, None), ((1, 2), (8, 96), (13, n // 2 - 40), 8), (None, None, (20, 300), 1), ((0, 2), (0, 128), (5, 200), 128)]
    for bs, asc, dep, g in cases:
        fb, nb = bs or (0, b)
        fa, na = asc or (0, a)
        fs, ns = dep or (0, n // 2)
        region = vol[fb:fb + nb, fa:fa + na, fs:fs + ns]
        G = na if g is None else g
        avg, res = pm.analyse_region(region, G, s0=fs, fit=True)
        got = pipe.peak_analysis(bscans=bs, ascans=asc, depth=dep, ascans_per_group=g, averaged=True)
        what = (n, log, flip, bs, asc, dep, G)
        _check_exact(got, avg, res, what)
        fitted += _check_fit(got, avg, res, fs, what)
    if not log:
        assert fitted > 0
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. physics
def _mirror_params(n, a, b):
    p = v180_benchmark_params(n, a, b)
    p.signalLogScaling, p.resampling, p.dispersionCompensation, p.fixedPatternNoiseRemoval = 0, 0, 0, 0
    p.update_all_curves()
    return p


def _mirror_raw(n, z, amp=1500.0):
    """flat DC plus a Gaussian spectral envelope (sigma = N / 10) times a cosine at depth z (any shape of z)"""
    k = np.arange(n, dtype=np.float64)
    z = np.asarray(z, np.float64)[..., None]
    env = np.exp(-0.5 * ((k - n / 2) / (n / 10)) ** 2)
    amp = np.asarray(amp, np.float64)
    amp = amp[..., None] if amp.ndim else amp
    return np.clip(np.rint(2048.0 + amp * env * np.cos(2 * np.pi * z * k / n)), 0, 4095).astype(np.uint16)


def test_mirror_psf():
    n, a, b = 1024, 64, 2
    z0 = 0.21 * n + 0.37
    p = _mirror_params(n, a, b)
    raw = np.broadcast_to(_mirror_raw(n, z0), (b, a, n)).copy()
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    got = pipe.peak_analysis(depth=(16, n // 2 - 16))
    assert np.all(got.fit_converged | got.fit_stalled), got.status
    # the expected PSF: float64 magnitude of the same windowed spectrum, fitted by scipy over the window the GPU reports
    from scipy.optimize import least_squares
    mag = np.abs(np.fft.fft(raw[0, 0].astype(np.float64) * np.asarray(p.windowCurve, np.float64)))[:n // 2]
    lo, cnt = int(got.fitFirst[0, 0]), int(got.fitCount[0, 0])
    z = np.arange(lo, lo + cnt, dtype=np.float64)
    y = mag[lo:lo + cnt]
    sp = least_squares(lambda q: pm.gauss(z, q) - y, [y.max() - y.min(), z0, 2.0, y.min()], method="lm", xtol=1e-15, ftol=1e-15).x
    want_fwhm = pm.FWHM_PER_SIGMA * abs(sp[2])
    print("PSF: GPU fitFwhm %.5f centre %.5f, expected %.5f / %.5f (mirror at %.3f), half-max width %.4f" % (
        got.fitFwhm[0, 0], got.center[0, 0], want_fwhm, sp[1], z0, got.fwhm[0, 0]))
    assert np.all(np.abs(got.fitFwhm / want_fwhm - 1.0) <= 0.005)
    assert np.all(np.abs(got.center - sp[1]) <= 0.01)
    pipe.close()


def test_roll_off_in_one_call():
    n, a, b = 1024, 64, 16
    zb = np.linspace(0.05 * n, 0.4 * n, b) + 0.29
    amp = np.exp(-zb / (0.4 * n))
    p = _mirror_params(n, a, b)
    raw = np.broadcast_to(_mirror_raw(n, zb, 1500.0 * amp)[:, None, :], (b, a, n)).copy()
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(raw)
    pipe.synchronize()
    got = pipe.peak_analysis(depth=(16, n // 2 - 16), ascans_per_group=a)
    assert got.shape == (b, 1) and np.all(got.fit_converged | got.fit_stalled)
    centre = got.center[:, 0]
    ratio = got.amplitude[:, 0] / got.amplitude[0, 0]
    print("roll-off: worst centre error %.4f bins, worst amplitude ratio error %.4f" % (np.max(np.abs(centre - zb)),
                                                                                      np.max(np.abs(ratio / (amp / amp[0]) - 1))))
    assert np.all(np.abs(centre - zb) <= 0.02)
    assert np.all(np.abs(ratio / (amp / amp[0]) - 1.0) <= 0.01)
    pipe.close()


def test_surface_map_of_a_tilted_mirror():
    n, a, b = 1024, 64, 8
    ai, bi = np.meshgrid(np.arange(a), np.arange(b))
    plane = 100.3 + 0.7 * ai + 3.1 * bi
    p = _mirror_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(_mirror_raw(n, plane))
    pipe.synchronize()
    fit = pipe.peak_analysis(depth=(16, n // 2 - 16), ascans_per_group=1, fit=True)
    nofit = pipe.peak_analysis(depth=(16, n // 2 - 16), ascans_per_group=1, fit=False)
    # (at the rounding floor of float32 data a fit may end stalled rather than converged: same parameters)
    assert fit.shape == (b, a) and np.all(fit.fit_converged | fit.fit_stalled)
    print("surface: %d of %d converged, the others stalled" % (int(fit.fit_converged.sum()), fit.status.size))
    print("surface: worst fit centre error %.4f, worst parabola error %.4f" % (np.max(np.abs(fit.center - plane)),
                                                                            np.max(np.abs(fit.position - plane))))
    assert np.all(np.abs(fit.center - plane) <= 0.02)
    assert np.all(np.abs(fit.position - plane) <= 0.15)
    for f in ("index", "value", "position", "left", "right", "fwhm"):
        assert _same(getattr(fit, f), getattr(nofit, f)), f
    assert np.array_equal(fit.status & pm.STEP4_BITS, nofit.status) and not np.any(nofit.status & pm.FIT_BITS)
    assert np.all(np.isnan(nofit.center)) and np.all(nofit.fitCount == 0)
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 3. sources
def _bits(r):
    return [np.ascontiguousarray(getattr(r, f)).view(np.uint8).tobytes() for f in r.FIELDS] + [r.averaged.view(np.uint8).tobytes()]


def test_sources_and_determinism():
    n, a, b = 1024, 128, 2
    p = v180_benchmark_params(n, a, b, buffers_per_volume=2)
    p.signalLogScaling = 0
    p.update_all_curves()
    pipe = Pipeline(p, device=0)
    for i in range(2):
        pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=50 + i))
        pipe.synchronize()
    _, _, last = pipe.processed_device()
    for g in (1, 8, 128):
        kw = dict(depth=(9, 400), ascans_per_group=g, averaged=True)
        per_slot = []
        for s in (0, 1):
            host = pipe.processed_host(slot=s).reshape(b, a, n // 2).copy()
            ref = pipe.peak_analysis(buffer=s, **kw)
            per_slot.append(ref)
            want = _bits(ref)
            assert _bits(pipe.peak_analysis(buffer=s, **kw)) == want, ("repeat", g, s)
            assert _bits(pipe.peak_analysis(data=host, **kw)) == want, ("host", g, s)
            assert _bits(pipe.peak_analysis(data=torch.from_numpy(host).cuda(), **kw)) == want, ("device", g, s)
            avg, res = pm.analyse_region(host[:, :, 9:409], g, s0=9)
            _check_exact(ref, avg, res, ("slot", s, g))
        assert _bits(pipe.peak_analysis(**kw)) == _bits(per_slot[last]), ("last slot", g)
    # the same values in another slot give the same bits
    vol = pipe.processed_host(slot=0).reshape(b, a, n // 2).copy()
    d_vol = torch.from_numpy(np.concatenate([vol, vol])).cuda()  # (two B-scan blocks: rows of the second start mid-buffer)
    two = Pipeline(v180_benchmark_params(n, a, 2 * b), device=0)
    x = two.peak_analysis(data=d_vol, bscans=(b, b), depth=(9, 400), ascans_per_group=8, averaged=True)
    y = pipe.peak_analysis(buffer=0, depth=(9, 400), ascans_per_group=8, averaged=True)
    assert _bits(x) == _bits(y)
    two.close()
    with pytest.raises(OctPipeError):
        pipe.peak_analysis(buffer=2)
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. side effects
def test_no_side_effects():
    n, a, b = 1024, 64, 2
    raws = [synthetic_raw(n, a, b, seed=60 + i) for i in range(2)]

    def run(with_peaks):
        p = v180_benchmark_params(n, a, b)
        pipe = Pipeline(p, device=0)
        pipe.enable_kernel_timing(True)
        pipe.octCudaPipeline(raws[0])
        pipe.synchronize()
        before = pipe.kernel_timing(reset=False)[1]
        if with_peaks:
            pipe.peak_analysis(averaged=True)
            pipe.peak_analysis(ascans_per_group=1, fit=False, depth=(3, 300))
            pipe.peak_analysis(data=pipe.processed_host(), ascans_per_group=8)
            assert pipe.kernel_timing(reset=False)[1] == before
        disp = pipe.display_bscan_host() if hasattr(pipe, "display_bscan_host") else None
        pipe.octCudaPipeline(raws[1])
        pipe.synchronize()
        out = [pipe.processed_host().copy(), pipe.mean_line().copy()]
        if disp is not None:
            out.append(np.asarray(disp).copy())
        pipe.close()
        return out

    ref, got = run(False), run(True)
    assert len(ref) == len(got)
    for x, y in zip(ref, got):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- 5. errors
def test_argument_errors_and_callbacks():
    n, a, b = 1024, 32, 2
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=1))
    pipe.synchronize()
    L, h = _lib.lib(), pipe.handle
    peaks = (_lib.Peak * 4096)()

    def call(reg, g=1, thr=float("-inf"), it=0):
        s = _lib.PeakSettings(g, thr, 1, 0, it)
        return L.octpipe_peak_analysis(h, None, 0, C.byref(reg), C.byref(s), peaks, None)

    ok = _lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 0, n // 2)
    assert call(ok) == 0 and call(ok, g=a) == 0 and call(ok, g=8) == 0
    assert call(ok, g=5) == 1 and b"divide" in L.octpipe_last_error()
    for reg, field in ((_lib.StatsRegion(0xFFFFFFFF, 0, 0, 0, a, 0, 8), b"bscan"), (_lib.StatsRegion(0xFFFFFFFF, 1, b, 0, a, 0, 8), b"bscan"),
                       (_lib.StatsRegion(0xFFFFFFFF, 0, 1, a, 1, 0, 8), b"Ascan"), (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, n // 2, 3), b"Sample"),
                       (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, n // 2 + 1), b"Sample"), (_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, 2), b"at least 3"),
                       (_lib.StatsRegion(1, 0, 1, 0, 1, 0, 8), b"buffer")):
        assert call(reg) == 1 and field in L.octpipe_last_error(), (field, L.octpipe_last_error())
    assert call(_lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 1, 0, 3)) == 0
    assert call(ok, thr=float("nan")) == 1 and b"threshold" in L.octpipe_last_error()
    # a depth window beyond 4096: UNSUPPORTED (N = 16384, the library-route length)
    big = Pipeline(v180_benchmark_params(16384, 8, 1), device=0)
    s = _lib.PeakSettings(1, float("-inf"), 0, 0, 0)
    r = _lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 8, 0, 8192)
    big.octCudaPipeline(synthetic_raw(16384, 8, 1, seed=2))
    big.synchronize()
    assert L.octpipe_peak_analysis(big.handle, None, 0, C.byref(r), C.byref(s), peaks, None) == 5
    r = _lib.StatsRegion(0xFFFFFFFF, 0, 1, 0, 8, 100, 4096)
    assert L.octpipe_peak_analysis(big.handle, None, 0, C.byref(r), C.byref(s), peaks, None) == 0
    big.close()
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.append(call(ok))
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=3))
    pipe.synchronize()
    assert codes and set(codes) == {7}, codes
    pipe.close()

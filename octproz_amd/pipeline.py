"""Thin Python handle around the C ABI of the pipeline (include/octpipe.h).

The three calls a user of the reference knows are kept by name:
    initializeCuda(h_buffer1, h_buffer2, params)   kernels.h:63  -> Pipeline(...)/initializeCuda
    octCudaPipeline(h_inputSignal)                 kernels.h:64  -> Pipeline.octCudaPipeline
    cleanupCuda()                                  kernels.h:67  -> Pipeline.cleanupCuda
Dirty-flag handling follows cu:1433-1445: a curve is pushed to the device when its
`*Updated` flag is set and the stage is enabled, then the flag is cleared.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check
from .params import OctAlgorithmParameters, dispersion_curve

# metric names of the dispersion estimation (OCTPIPE_METRIC_*, include/octpipe.h)
DISPERSION_METRICS = {"sum": _lib.METRIC_SUM_ABOVE_THRESHOLD, "samples": _lib.METRIC_SAMPLES_ABOVE_THRESHOLD,
                      "peak": _lib.METRIC_PEAK_VALUE, "sobel": _lib.METRIC_MEAN_SOBEL}


# rendering modes of the volume view (OCTPIPE_RENDER_*, include/octpipe.h), by the reference's names
RENDER_MODES = {"MIP": _lib.RENDER_MIP, "DMIP": _lib.RENDER_DMIP, "X-ray": _lib.RENDER_XRAY, "Alpha blending": _lib.RENDER_ALPHA_BLENDING,
                "MIDA": _lib.RENDER_MIDA, "Isosurface": _lib.RENDER_ISOSURFACE, "OCT Depth": _lib.RENDER_OCT_DEPTH}
# keyword of Pipeline.render_volume -> field of OctPipeRenderSettings
_RENDER_FIELDS = {"fov": "fovDegrees", "stretch": "stretch", "step_length": "stepLength", "threshold": "threshold", "depth_weight": "depthWeight",
                  "alpha_exponent": "alphaExponent", "gamma": "gamma", "smooth_factor": "smoothFactor", "shading": "shadingEnabled",
                  "lut": "lutEnabled", "background": "background", "material": "material", "light_position": "lightPosition",
                  "jitter_seed": "jitterSeed", "view_matrix": "viewMatrix"}


def render_mode_code(mode):
    """"MIP" / "DMIP" / "X-ray" / "Alpha blending" / "MIDA" / "Isosurface" / "OCT Depth" (case and blanks ignored) or an OCTPIPE_RENDER_* number"""
    if isinstance(mode, str):
        key = mode.replace(" ", "").replace("-", "").replace("_", "").lower()
        for name, code in RENDER_MODES.items():
            if name.replace(" ", "").replace("-", "").lower() == key:
                return code
        raise ValueError("unknown rendering mode %r (one of %s)" % (mode, ", ".join(RENDER_MODES)))
    return int(mode)


def default_render_settings():
    """octpipe_default_render_settings: the reference's start-up state as a RenderSettings"""
    s = _lib.RenderSettings()
    _lib.lib().octpipe_default_render_settings(C.byref(s))
    return s


def render_view_matrix(rotation=(1.0, 0.0, 0.0, 0.0), view_pos=(0.0, 0.0), distance=-500.0):
    """octpipe_render_view_matrix: the 4 x 4 view matrix (row-major numpy float32) of the quaternion (w, x, y, z), the view position and
    the reference's distExp (the camera sits 4 exp(distance / 600) in front of the volume's centre)"""
    q = (C.c_float * 4)(*[float(v) for v in rotation])
    out = (C.c_float * 16)()
    check(_lib.lib().octpipe_render_view_matrix(q, float(view_pos[0]), float(view_pos[1]), float(distance), out))
    return np.array(out, dtype=np.float32).reshape(4, 4)


def dispersion_metric_code(metric):
    """"peak" / "sum" / "samples" / "sobel" or an OCTPIPE_METRIC_* number"""
    if isinstance(metric, str):
        if metric not in DISPERSION_METRICS:
            raise ValueError("unknown dispersion metric %r (one of %s)" % (metric, ", ".join(DISPERSION_METRICS)))
        return DISPERSION_METRICS[metric]
    return int(metric)


def dispersion_range(start, end, samples):
    """The candidates of a range as octpipe_estimate_dispersion samples it: (float)(start + (end - start) * (double)i / (samples - 1))
    with float32 start / end (start alone for samples == 1)."""
    samples = int(samples)
    if samples < 1:
        raise ValueError("samples must be >= 1")
    s, e = np.float32(start), np.float32(end)
    if samples == 1:
        return np.array([s], dtype=np.float32)
    diff = float(np.float32(e - s))  # (a float subtraction in the C ABI)
    i = np.arange(samples, dtype=np.float64)
    return (float(s) + diff * i / float(samples - 1)).astype(np.float32)


def center_ascans(frame, ascans_per_bscan, count):
    """Buffer-local index of the first of `count` A-scans taken from the centre of B-scan `frame` (the extension's selection)."""
    if count < 1 or count > ascans_per_bscan:
        raise ValueError("need 1 <= count <= A-scans per B-scan")
    return int(frame) * int(ascans_per_bscan) + (int(ascans_per_bscan) - int(count)) // 2


def first_max(scores):
    """Index of the first maximum; a NaN never wins.  None when every score is NaN."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    ok = ~np.isnan(s)
    if not ok.any():
        return None
    return int(np.flatnonzero(s == np.max(s[ok]))[0])


class DispersionEstimate:
    """Result of Pipeline.estimate_dispersion: the best (d2, d3) and the scores behind it.  Two-step search: d2_candidates /
    d2_scores (d3 = 0), then d3_candidates / d3_scores (with the best d2).  grid=True: `grid` holds the scores [i2, i3] of every
    pair (d2_candidates[i2], d3_candidates[i3]) and the two curves are None."""

    def __init__(self, d2, d3, d2_candidates, d3_candidates, d2_scores=None, d3_scores=None, grid=None):
        self.d2, self.d3 = float(d2), float(d3)
        self.d2_candidates, self.d3_candidates = d2_candidates, d3_candidates
        self.d2_scores, self.d3_scores, self.grid = d2_scores, d3_scores, grid

    def __repr__(self):
        return "DispersionEstimate(d2=%g, d3=%g%s)" % (self.d2, self.d3, ", grid %dx%d" % self.grid.shape if self.grid is not None else "")


class PhaseExtraction:
    """Result of Pipeline.extract_resample_curve (include/octpipe.h "phase extraction"): the averaged interferogram `mean` [N] of
    `count` A-scans, `spectrum` [N/2] (|X[k]|, the depth bins of a processed A-scan), `envelope` and unwrapped `phase` [N] of the
    selected band, the resampling `curve` [N] and its cubic fit `coeffs` (c0..c3 of octpipe_resample_curve)."""

    def __init__(self, mean, count, spectrum, envelope, phase, curve, coeffs):
        self.mean, self.count, self.spectrum, self.envelope, self.phase, self.curve = mean, count, spectrum, envelope, phase, curve
        self.coeffs = coeffs

    def __repr__(self):
        return "PhaseExtraction(count=%d, coeffs=%s)" % (self.count, np.array2string(self.coeffs, precision=6))


class ImageStatistics:
    """Result of Pipeline.processed_statistics / raw_statistics (include/octpipe.h "image statistics"): `histogram` (uint64 [bins]),
    `edges` (float64 [bins + 1]: lo + i * binWidth), and the fields of OctPipeImageStatistics: count, underflow, overflow, nonFinite,
    min, max, mean, stddev (population), lo, hi, binWidth."""

    FIELDS = ("count", "underflow", "overflow", "nonFinite", "min", "max", "mean", "stddev", "lo", "hi", "binWidth")

    def __init__(self, st, histogram):
        for f in self.FIELDS:
            setattr(self, f, getattr(st, f))
        self.histogram = histogram
        bins = len(histogram)
        if np.isfinite(self.lo) and np.isfinite(self.binWidth):
            self.edges = self.lo + self.binWidth * np.arange(bins + 1, dtype=np.float64)
            self.edges[-1] = self.hi
        else:
            self.edges = np.full(bins + 1, np.nan)

    def quantile(self, q):
        """The q-quantile from the histogram: the lower edge of the first bin at which the cumulative in-range count reaches
        q * the in-range total (under- and overflow are not part of either).  NaN when no value is in range."""
        if not 0.0 <= q <= 1.0:
            raise ValueError("q must lie in [0, 1]")
        cum = np.cumsum(self.histogram.astype(np.float64))
        total = cum[-1] if len(cum) else 0.0
        if total == 0:
            return float("nan")
        return float(self.edges[int(np.argmax(cum >= q * total))])

    def __repr__(self):
        return "ImageStatistics(count=%d, mean=%g, stddev=%g, min=%g, max=%g, bins=%d over [%g, %g])" % (
            self.count, self.mean, self.stddev, self.min, self.max, len(self.histogram), self.lo, self.hi)


class PeakAnalysis:
    """Result of Pipeline.peak_analysis (include/octpipe.h "peak analysis"): one numpy array per field of OctPipePeak, shaped
    (bscanCount, ascanCount // G) -- status, index, value, fitFirst, fitCount, iterations, position, left, right, fwhm, amplitude,
    center, sigma, offset, fitFwhm, rms -- the status bits decoded as boolean arrays (no_peak, nonfinite, width_undefined, left_open,
    right_open, fit_converged, fit_max_iter, fit_stalled, fit_skipped), and `averaged` shaped (..., sampleCount) when asked for."""

    FIELDS = tuple(f[0] for f in _lib.Peak._fields_)
    BITS = (("no_peak", _lib.PEAK_NO_PEAK), ("nonfinite", _lib.PEAK_NONFINITE), ("width_undefined", _lib.PEAK_WIDTH_UNDEFINED),
            ("left_open", _lib.PEAK_LEFT_OPEN), ("right_open", _lib.PEAK_RIGHT_OPEN), ("fit_converged", _lib.PEAK_FIT_CONVERGED),
            ("fit_max_iter", _lib.PEAK_FIT_MAX_ITER), ("fit_stalled", _lib.PEAK_FIT_STALLED), ("fit_skipped", _lib.PEAK_FIT_SKIPPED))

    def __init__(self, records, shape, averaged=None):
        for f in self.FIELDS:
            setattr(self, f, records[f].reshape(shape).copy())
        for name, bit in self.BITS:
            setattr(self, name, (self.status & bit) != 0)
        self.found = (self.status & (_lib.PEAK_NO_PEAK | _lib.PEAK_NONFINITE)) == 0
        self.averaged = None if averaged is None else averaged.reshape(shape + (averaged.shape[-1],))
        self.shape = shape

    def __repr__(self):
        return "PeakAnalysis(groups=%s, found=%d, fit_converged=%d)" % (self.shape, int(self.found.sum()), int(self.fit_converged.sum()))


class Pipeline:
    def __init__(self, params: OctAlgorithmParameters, device=0, h_buffer1=None, h_buffer2=None, sample_format=0, route=0):
        self.params = params
        self._h = C.c_void_p()
        self._lib = _lib.lib()
        _lib.drain_deferred()
        acq = params.acquisition()
        pod = params.pod()
        self._keep = (h_buffer1, h_buffer2)
        b1 = h_buffer1.ctypes.data if h_buffer1 is not None else None
        b2 = h_buffer2.ctypes.data if h_buffer2 is not None else None
        # sample_format: OCTPIPE_FORMAT_* (0 = the reference's rule, 1/2 packed 12 bit, 3/4/5 int8/int16/int32)
        # route: OCTPIPE_ROUTE_* flags (tests / A-B measurements; include/octpipe_debug.h); the FFT-backend flags are read at creation
        if route:
            rc = self._lib.octpipe_debug_create(C.byref(self._h), device, C.byref(acq), C.byref(pod), b1, b2, int(sample_format), int(route))
        else:
            rc = self._lib.octpipe_create_with_format(C.byref(self._h), device, C.byref(acq), C.byref(pod), b1, b2, int(sample_format))
        if rc != 0:
            msg = self._lib.octpipe_last_error()
            if self._h:
                self._lib.octpipe_destroy(self._h)
                self._h = C.c_void_p()
            raise _lib.OctPipeError(rc, msg.decode() if msg else "")
        self.N = int(params.samplesPerLine)
        self.S = params.samplesPerBuffer
        self._callbacks = None
        self._sync_params(force_curves=True)

    # reference-named entry points ------------------------------------------------------------
    @classmethod
    def initializeCuda(cls, h_buffer1, h_buffer2, params, device=0, sample_format=0, route=0):
        return cls(params, device, h_buffer1, h_buffer2, sample_format, route)

    def octCudaPipeline(self, h_inputSignal):
        self._sync_params()
        a = np.ascontiguousarray(h_inputSignal)
        check(self._lib.octpipe_process(self._h, a.ctypes.data))

    def cleanupCuda(self):
        if self._h:
            _lib.destroy_or_defer("pipeline", self._h)  # (a finaliser may run on a callback thread: destroyed later then)
            self._h = C.c_void_p()

    close = cleanupCuda

    def __del__(self):
        try:
            self.cleanupCuda()
        except Exception:
            pass

    # -------------------------------------------------------------------------------------------
    def _sync_params(self, force_curves=False):
        p = self.params
        if p.resampling and (p.resamplingUpdated or force_curves) and p.resampleCurve is not None:
            c = np.ascontiguousarray(p.resampleCurve, dtype=np.float32)
            check(self._lib.octpipe_update_resample_curve(self._h, c.ctypes.data, len(c)))
            p.resamplingUpdated = False
        if p.dispersionCompensation and (p.dispersionUpdated or force_curves) and p.dispersionCurve is not None:
            c = np.ascontiguousarray(p.dispersionCurve, dtype=np.float32)
            check(self._lib.octpipe_update_dispersion_curve(self._h, c.ctypes.data, len(c)))
            p.dispersionUpdated = False
        if p.windowing and (p.windowUpdated or force_curves) and p.windowCurve is not None:
            c = np.ascontiguousarray(p.windowCurve, dtype=np.float32)
            check(self._lib.octpipe_update_window_curve(self._h, c.ctypes.data, len(c)))
            p.windowUpdated = False
        if p.postProcessBackgroundRemoval and p.postProcessBackgroundUpdated and p.postProcessBackground is not None:
            c = np.ascontiguousarray(p.postProcessBackground, dtype=np.float32)
            check(self._lib.octpipe_update_postprocess_background(self._h, c.ctypes.data, len(c)))
            p.postProcessBackgroundUpdated = False
        pod = p.pod()
        check(self._lib.octpipe_set_params(self._h, C.byref(pod)))
        # one-shot requests are consumed by the pipeline (cu:1524, cu:1561)
        p.redetermineFixedPatternNoise = 0
        p.postProcessBackgroundRecordingRequested = 0

    def process_device(self, d_raw_ptr, sync_params=True):
        """Run the chain on a raw buffer already resident in HBM (plain device pointer)."""
        if sync_params:
            self._sync_params()
        check(self._lib.octpipe_process_device(self._h, C.c_void_p(d_raw_ptr)))

    def synchronize(self):
        check(self._lib.octpipe_synchronize(self._h))

    def processed_device(self):
        ptr, nbytes, nr = C.c_void_p(), C.c_size_t(), C.c_uint()
        check(self._lib.octpipe_get_processed_device(self._h, C.byref(ptr), C.byref(nbytes), C.byref(nr)))
        return ptr.value, nbytes.value, nr.value

    def processed_host(self, slot=None):
        """float32 [B*A, N/2] of the slot written last (or of `slot`)."""
        _, _, nr = self.processed_device()
        if slot is None:
            slot = nr
        n = self.S // 2
        out = np.empty(n, dtype=np.float32)
        check(self._lib.octpipe_copy_processed_to_host(self._h, out.ctypes.data, n, n * slot))
        return out

    def stream_ptr(self):
        s = C.c_void_p()
        check(self._lib.octpipe_get_stream(self._h, C.byref(s)))
        return s.value or 0

    def set_stream(self, stream_ptr):
        check(self._lib.octpipe_set_stream(self._h, C.c_void_p(stream_ptr)))

    def mean_line(self):
        m = np.empty(self.N, dtype=np.complex64)
        check(self._lib.octpipe_get_mean_line(self._h, m.ctypes.data))
        return m

    def set_mean_line(self, m, pin=True):
        m = np.ascontiguousarray(m, dtype=np.complex64)
        assert m.size == self.N
        check(self._lib.octpipe_set_mean_line(self._h, m.ctypes.data, 1 if pin else 0))

    def min_variance_mean(self, z, width, height):
        z = np.ascontiguousarray(z, dtype=np.complex64)
        out = np.empty(width, dtype=np.complex64)
        check(self._lib.octpipe_min_variance_mean(self._h, z.ctypes.data, 0, width, height, out.ctypes.data))
        return out

    def debug_spectrum(self, d_raw_ptr, lines):
        self._sync_params()
        out = np.empty(lines * self.N, dtype=np.complex64)
        check(self._lib.octpipe_debug_spectrum(self._h, C.c_void_p(d_raw_ptr), lines, out.ctypes.data))
        return out

    def raw_buffer_bytes(self):
        n = C.c_size_t()
        check(self._lib.octpipe_raw_buffer_bytes(self._h, C.byref(n)))
        return n.value

    def debug_unpack(self, d_raw_ptr, count):
        self._sync_params()
        out = np.empty(count, dtype=np.float32)
        check(self._lib.octpipe_debug_unpack(self._h, C.c_void_p(d_raw_ptr), count, out.ctypes.data))
        return out

    def debug_force_prepared(self, on=True):
        check(self._lib.octpipe_debug_force_prepared(self._h, 1 if on else 0))

    def set_route(self, flags):
        """OCTPIPE_ROUTE_* of an existing handle (takes effect with the next buffer)"""
        check(self._lib.octpipe_debug_set_route(self._h, int(flags)))

    def set_sinus_blocks_per_wave(self, k):
        """MODE_SINUS: blocks of the work list per wave (0 = library default); measurement / test knob (octpipe_debug.h)"""
        check(self._lib.octpipe_debug_set_sinus_blocks_per_wave(self._h, int(k)))

    def last_path(self):
        """_lib.PATH_* bits of the implementation the last buffer's image launch took"""
        n = C.c_uint()
        check(self._lib.octpipe_debug_last_path(self._h, C.byref(n)))
        return n.value

    def lane_stats(self):
        """(overlapped, joins) of the compute lanes (csrc/lanes.h): buffers that went out on the lane of their slot with no join in front,
        and how often the compute stream had to be ordered behind the second lane"""
        o, j = C.c_uint64(), C.c_uint64()
        check(self._lib.octpipe_debug_lane_stats(self._h, C.byref(o), C.byref(j)))
        return o.value, j.value

    def rtc_status(self):
        """run-time compiled kernel of this handle's length (csrc/mixedn_rtc.hip): {"uses_it", "radices", "compiled_in_process",
        "compile_seconds", "message"}; message = why the length keeps another route / why the last compilation failed"""
        uses, n, sec = C.c_int(), C.c_int(), C.c_double()
        rad = (C.c_int * 5)()
        msg = C.create_string_buffer(2048)
        check(self._lib.octpipe_debug_rtc_status(self._h, C.byref(uses), rad, C.byref(n), C.byref(sec), msg, C.c_size_t(2048)))
        return {"uses_it": bool(uses.value), "radices": [r for r in rad if r], "compiled_in_process": n.value,
                "compile_seconds": sec.value, "message": msg.value.decode(errors="replace")}

    def last_grid(self):
        n = C.c_int()
        check(self._lib.octpipe_debug_last_grid(self._h, C.byref(n)))
        return n.value

    def postprocess_background(self):
        out = np.empty(self.N // 2, dtype=np.float32)
        check(self._lib.octpipe_copy_postprocess_background_to_host(self._h, out.ctypes.data, self.N // 2))
        return out

    def export_calibration(self):
        n = self._lib.octpipe_calibration_size(self._h)
        blob = np.empty(n, dtype=np.uint8)
        check(self._lib.octpipe_export_calibration(self._h, blob.ctypes.data, n))
        return blob

    def import_calibration(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        check(self._lib.octpipe_import_calibration(self._h, blob.ctypes.data, blob.size))

    def register_streaming_buffers(self, b1, b2):
        self._stream_keep = (b1, b2)
        check(self._lib.octpipe_register_streaming_buffers(self._h, b1.ctypes.data, b2.ctypes.data, b1.nbytes))

    def unregister_streaming_buffers(self):
        check(self._lib.octpipe_unregister_streaming_buffers(self._h))

    def register_float_streaming_buffers(self, b1, b2):
        self._fstream_keep = (b1, b2)
        check(self._lib.octpipe_register_float_streaming_buffers(self._h, b1.ctypes.data, b2.ctypes.data, b1.nbytes))

    def unregister_float_streaming_buffers(self):
        check(self._lib.octpipe_unregister_float_streaming_buffers(self._h))

    def set_callbacks(self, on_streaming=None, on_float_streaming=None, on_background=None):
        noop_d = lambda *a: None
        noop_e = lambda *a: None
        cbs = (_lib.DATA_CALLBACK(on_streaming or noop_d), _lib.DATA_CALLBACK(on_float_streaming or noop_d),
               _lib.EVENT_CALLBACK(on_background or noop_e))
        self._callbacks = cbs  # keep alive
        check(self._lib.octpipe_set_callbacks(self._h, cbs[0], cbs[1], cbs[2], None))

    def change_displayed_bscan_frame(self, frame_nr, frames, fn):
        check(self._lib.octpipe_change_displayed_bscan_frame(self._h, frame_nr, frames, fn))

    def change_displayed_enface_frame(self, frame_nr, frames, fn):
        check(self._lib.octpipe_change_displayed_enface_frame(self._h, frame_nr, frames, fn))

    def display_buffers(self):
        pb, nb, pe, ne = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        check(self._lib.octpipe_get_display_buffers(self._h, C.byref(pb), C.byref(nb), C.byref(pe), C.byref(ne)))
        return (pb.value, nb.value), (pe.value, ne.value)

    def volume_view_buffer(self):
        """(device pointer, bytes) of the uint8 volume view [N/2][B*buffersPerVolume][A] (cu:914-941 into a plain buffer)"""
        ptr, n = C.c_void_p(), C.c_size_t()
        check(self._lib.octpipe_get_volume_view_buffer(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def postprocess_background_host(self):
        """the host shadow filled in-stream before the backgroundRecorded callback (no HIP call: callable from it)"""
        out = np.empty(self.N // 2, dtype=np.float32)
        check(self._lib.octpipe_get_postprocess_background_host(self._h, out.ctypes.data, self.N // 2))
        return out

    def enable_kernel_timing(self, on=True, every=1):
        """HIP events around the dominant kernel of every launch (`every` = n > 1: of every n-th launch only)"""
        check(self._lib.octpipe_enable_kernel_timing(self._h, 1 if on else 0))
        if on and int(every) > 1:
            check(self._lib.octpipe_set_kernel_timing_stride(self._h, int(every)))

    def kernel_timing(self, reset=True):
        ms, n = C.c_double(), C.c_uint()
        check(self._lib.octpipe_kernel_timing(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    # dispersion estimation (include/octpipe.h) ----------------------------------------------------
    def _raw_arg(self, raw):
        """(pointer, is_device, keep-alive) of a raw buffer: numpy array (host), torch tensor (its memory) or a device pointer (int)"""
        if isinstance(raw, np.ndarray):
            a = np.ascontiguousarray(raw)
            if a.nbytes < self.raw_buffer_bytes():
                raise ValueError("raw buffer holds %d bytes, the handle's layout needs %d" % (a.nbytes, self.raw_buffer_bytes()))
            return a.ctypes.data, 0, a
        if hasattr(raw, "data_ptr"):
            if not raw.is_contiguous():
                raise ValueError("raw tensor must be contiguous")
            if raw.is_cuda:
                return raw.data_ptr(), 1, raw
            return self._raw_arg(raw.numpy())
        return int(raw), 1, None

    def _metric(self, first_ascan, ascan_count, metric, threshold, ignore_first, linear, d0, d1):
        p = self.params
        return _lib.DispersionMetric(int(first_ascan), int(ascan_count), int(ignore_first), 1 if linear else 0, dispersion_metric_code(metric),
                                     float(threshold), float(p.d0 if d0 is None else d0), float(p.d1 if d1 is None else d1))

    def dispersion_scores(self, raw, d2, d3, first_ascan, ascan_count, metric="peak", threshold=0.0, ignore_first=0, linear=True, d0=None, d1=None):
        """Score[c] of the candidates (d2[c], d3[c]) on A-scans first_ascan .. first_ascan + ascan_count - 1 of `raw` (float32 [K])."""
        self._sync_params()
        ptr, dev, keep = self._raw_arg(raw)
        d2 = np.ascontiguousarray(np.atleast_1d(d2), dtype=np.float32)
        d3 = np.ascontiguousarray(np.atleast_1d(d3), dtype=np.float32)
        if d2.shape != d3.shape:
            raise ValueError("d2 and d3 need the same length")
        m = self._metric(first_ascan, ascan_count, metric, threshold, ignore_first, linear, d0, d1)
        out = np.empty(len(d2), dtype=np.float32)
        check(self._lib.octpipe_dispersion_scores(self._h, C.c_void_p(ptr), dev, C.byref(m), d2.ctypes.data, d3.ctypes.data, len(d2), out.ctypes.data))
        del keep
        return out

    def dispersion_metrics(self, raw, d2, d3, first_ascan, ascan_count, metric="peak", threshold=0.0, ignore_first=0, linear=True, d0=None, d1=None):
        """octpipe_debug_dispersion_metrics: (metric matrix float32 [K, M], scores [K], device ms of the sweep kernel)"""
        self._sync_params()
        ptr, dev, keep = self._raw_arg(raw)
        d2 = np.ascontiguousarray(np.atleast_1d(d2), dtype=np.float32)
        d3 = np.ascontiguousarray(np.atleast_1d(d3), dtype=np.float32)
        m = self._metric(first_ascan, ascan_count, metric, threshold, ignore_first, linear, d0, d1)
        mat = np.empty((len(d2), int(ascan_count)), dtype=np.float32)
        sc = np.empty(len(d2), dtype=np.float32)
        ms = C.c_double()
        check(self._lib.octpipe_debug_dispersion_metrics(self._h, C.c_void_p(ptr), dev, C.byref(m), d2.ctypes.data, d3.ctypes.data, len(d2),
                                                         mat.ctypes.data, sc.ctypes.data, C.byref(ms)))
        del keep
        return mat, sc, ms.value

    def dispersion_phasors(self, d2, d3, d0=None, d1=None):
        """octpipe_debug_dispersion_phasors: (theta float32 [K, N], phasors complex64 [K, N])"""
        d2 = np.ascontiguousarray(np.atleast_1d(d2), dtype=np.float32)
        d3 = np.ascontiguousarray(np.atleast_1d(d3), dtype=np.float32)
        K = len(d2)
        theta = np.empty((K, self.N), dtype=np.float32)
        ph = np.empty((K, self.N), dtype=np.complex64)
        p = self.params
        check(self._lib.octpipe_debug_dispersion_phasors(self._h, float(p.d0 if d0 is None else d0), float(p.d1 if d1 is None else d1),
                                                         d2.ctypes.data, d3.ctypes.data, K, theta.ctypes.data, ph.ctypes.data))
        return theta, ph

    def estimate_dispersion(self, raw, frame=0, ascans_from_center=40, ignore_first=20, linear=True, metric="peak", threshold=0.0,
                            d2_range=(-100.0, 100.0), d3_range=(-100.0, 100.0), samples=50, grid=False, apply=False):
        """The Dispersion Estimator's search on one grabbed raw buffer (defaults: the extension's).  Two steps -- d2 with d3 = 0, then d3
        with the best d2 -- or, grid=True, every samples x samples pair in one call.  apply=True writes the result into params (d2, d3)
        and pushes the dispersion curve to the handle."""
        self._sync_params()
        first = center_ascans(frame, self.params.ascansPerBscan, ascans_from_center)
        m = self._metric(first, ascans_from_center, metric, threshold, ignore_first, linear, None, None)
        c2, c3 = dispersion_range(d2_range[0], d2_range[1], samples), dispersion_range(d3_range[0], d3_range[1], samples)
        if grid:
            scores = self.dispersion_scores(raw, np.repeat(c2, len(c3)), np.tile(c3, len(c2)), first, ascans_from_center, metric, threshold,
                                            ignore_first, linear)
            best = first_max(scores)
            if best is None:
                raise _lib.OctPipeError(1, "dispersion estimate: every score of the grid is NaN")
            res = DispersionEstimate(c2[best // len(c3)], c3[best % len(c3)], c2, c3, grid=scores.reshape(len(c2), len(c3)))
        else:
            ptr, dev, keep = self._raw_arg(raw)
            s2, s3 = np.empty(len(c2), dtype=np.float32), np.empty(len(c3), dtype=np.float32)
            b2, b3 = C.c_float(), C.c_float()
            check(self._lib.octpipe_estimate_dispersion(self._h, C.c_void_p(ptr), dev, C.byref(m), float(d2_range[0]), float(d2_range[1]),
                                                        float(d3_range[0]), float(d3_range[1]), int(samples), s2.ctypes.data, s3.ctypes.data,
                                                        C.byref(b2), C.byref(b3)))
            del keep
            res = DispersionEstimate(b2.value, b3.value, c2, c3, d2_scores=s2, d3_scores=s3)
        if apply:
            p = self.params
            p.d2, p.d3 = res.d2, res.d3
            p.dispersionCurve = dispersion_curve(p.d0, p.d1, p.d2, p.d3, int(p.samplesPerLine))
            c = np.ascontiguousarray(p.dispersionCurve, dtype=np.float32)
            check(self._lib.octpipe_update_dispersion_curve(self._h, c.ctypes.data, len(c)))
            p.dispersionUpdated = False
        return res

    # phase extraction / k-linearisation calibration (include/octpipe.h) ---------------------------
    def phase_reset(self):
        """Clear the handle's phase accumulator."""
        check(self._lib.octpipe_phase_reset(self._h))

    def phase_accumulate(self, raw, first_ascan=0, ascan_count=None):
        """Add A-scans first_ascan .. first_ascan + ascan_count - 1 of one raw buffer (numpy, torch tensor or device pointer; None: all
        A*B) to the accumulator, decoded with the current bitshift."""
        self._sync_params()
        if ascan_count is None:
            ascan_count = int(self.params.ascansPerBscan) * int(self.params.bscansPerBuffer) - int(first_ascan)
        ptr, dev, keep = self._raw_arg(raw)
        check(self._lib.octpipe_phase_accumulate(self._h, C.c_void_p(ptr), dev, int(first_ascan), int(ascan_count)))
        del keep

    def phase_accumulate_timed(self, raw, first_ascan=0, ascan_count=None):
        """octpipe_debug_phase_accumulate: phase_accumulate, returning the device time of its work in ms"""
        self._sync_params()
        if ascan_count is None:
            ascan_count = int(self.params.ascansPerBscan) * int(self.params.bscansPerBuffer) - int(first_ascan)
        ptr, dev, keep = self._raw_arg(raw)
        ms = C.c_double()
        check(self._lib.octpipe_debug_phase_accumulate(self._h, C.c_void_p(ptr), dev, int(first_ascan), int(ascan_count), C.byref(ms)))
        del keep
        return ms.value

    def phase_mean(self):
        """(mean float32 [N], A-scan count) of the accumulator"""
        mean = np.empty(self.N, dtype=np.float32)
        count = C.c_uint64()
        check(self._lib.octpipe_phase_mean(self._h, mean.ctypes.data, C.byref(count)))
        return mean, count.value

    def extract_resample_curve(self, raws=None, mean=None, ascans=None, peak=None, window_raw=False, hann_peak=True,
                               ignore_first=0, ignore_last=0, apply=None):
        """The Phase Extraction Extension on the device.  raws: one raw buffer or a list of them; the accumulator is reset and every
        buffer's A-scans ascans = (first, last) (inclusive, the extension's range; None: all) are accumulated.  Or mean: an averaged
        interferogram [N] of your own.  Neither: the accumulator as it stands.  peak = (peakStart, peakEnd), inclusive depth bins of
        the calibration peak.  apply="coeffs" is *Transfer coeffs* (params.c0..c3 from the fit, resampling on, the polynomial
        curve pushed); apply="curve" is *Transfer curve* (the measured curve as the custom curve, pushed).  *Save curve* is
        octproz_amd.params.save_curve_csv(path, result.curve).  Returns a PhaseExtraction."""
        if peak is None:
            raise ValueError("peak = (peakStart, peakEnd) is required")
        if apply not in (None, "coeffs", "curve"):
            raise ValueError("apply must be None, 'coeffs' or 'curve'")
        if raws is not None and mean is not None:
            raise ValueError("pass raws or mean, not both")
        first, count = 0, None
        if ascans is not None:
            first, last = int(ascans[0]), int(ascans[1])
            if last < first:
                raise ValueError("ascans = (first, last) needs last >= first")
            count = last - first + 1
        if raws is not None:
            self.phase_reset()
            for raw in (raws if isinstance(raws, (list, tuple)) else [raws]):
                self.phase_accumulate(raw, first, count)
        n = self.N
        if mean is None:
            mean, cnt = self.phase_mean()
        else:
            mean, cnt = np.ascontiguousarray(mean, dtype=np.float32).ravel(), 0
            if len(mean) != n:
                raise ValueError("mean needs %d samples" % n)
        x = _lib.PhaseExtraction(int(peak[0]), int(peak[1]), 1 if window_raw else 0, 1 if hann_peak else 0, int(ignore_first), int(ignore_last))
        spectrum, envelope = np.empty(n // 2, np.float32), np.empty(n, np.float32)
        phase, curve, coeffs = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(4, np.float32)
        check(self._lib.octpipe_extract_resample_curve(self._h, mean.ctypes.data, C.byref(x), spectrum.ctypes.data, envelope.ctypes.data,
                                                       phase.ctypes.data, curve.ctypes.data, coeffs.ctypes.data))
        p = self.params
        if apply == "coeffs":
            p.c0, p.c1, p.c2, p.c3 = (float(c) for c in coeffs)
            p.resampling, p.useCustomResampleCurve = 1, False
        elif apply == "curve":
            p.loadCustomResampleCurve(curve)
            p.resampling, p.useCustomResampleCurve = 1, True
        if apply is not None:
            p.updateResampleCurve()
            c = np.ascontiguousarray(p.resampleCurve, dtype=np.float32)
            check(self._lib.octpipe_update_resample_curve(self._h, c.ctypes.data, len(c)))
            p.resamplingUpdated = False
        return PhaseExtraction(mean, cnt, spectrum, envelope, phase, curve, coeffs)

    # image statistics (include/octpipe.h) -------------------------------------------------------------
    def _stats_region(self, buffer, bscans, ascans, samples, depth_extent):
        p = self.params
        ext = (int(p.bscansPerBuffer), int(p.ascansPerBscan), int(depth_extent))
        out = []
        for pair, e in zip((bscans, ascans, samples), ext):
            out.extend((0, e) if pair is None else (int(pair[0]), int(pair[1])))
        return _lib.StatsRegion(0xFFFFFFFF if buffer is None else int(buffer), *out)

    def _float_arg(self, data):
        """(pointer, is_device, keep-alive) of one processed buffer [B][A][N/2] of float32: numpy array, torch tensor or device pointer"""
        need = self.S // 2
        if hasattr(data, "data_ptr"):
            if not data.is_contiguous():
                raise ValueError("data tensor must be contiguous")
            if data.is_cuda:
                if str(data.dtype) != "torch.float32" or data.numel() < need:
                    raise ValueError("data tensor must hold %d float32 values" % need)
                return data.data_ptr(), 1, data
            data = data.numpy()
        if isinstance(data, np.ndarray):
            a = np.ascontiguousarray(data, dtype=np.float32)
            if a.size < need:
                raise ValueError("data holds %d values, one processed buffer is %d" % (a.size, need))
            return a.ctypes.data, 0, a
        return int(data), 1, None

    def _processed_statistics(self, data, buffer, bscans, ascans, depth, bins, range, timed):
        if data is not None and buffer not in (None, 0):
            raise ValueError("with data, buffer must be None or 0")
        r = self._stats_region(buffer, bscans, ascans, depth, self.N // 2)
        ptr, dev, keep = (None, 0, None) if data is None else self._float_arg(data)
        auto, lo, hi = (1, 0.0, 0.0) if range is None else (0, float(range[0]), float(range[1]))
        hist, st, ms = np.zeros(int(bins), np.uint64), _lib.ImageStatistics(), C.c_double()
        args = [self._h, C.c_void_p(ptr), dev, C.byref(r), int(bins), auto, lo, hi, hist.ctypes.data, C.byref(st)]
        if timed:
            check(self._lib.octpipe_debug_processed_statistics(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_processed_statistics(*args))
        del keep
        return ImageStatistics(st, hist), ms.value

    def processed_statistics(self, data=None, buffer=None, bscans=None, ascans=None, depth=None, bins=256, range=None):
        """Histogram and moments of a region of processed data (the Image Statistics extension).  data: None (the handle's processed
        volume, slot `buffer`, None = the slot the last process call wrote), or one buffer [B][A][N/2] of float32 (numpy, torch
        tensor or device pointer).  bscans / ascans / depth: (first, count) pairs, None = the whole extent.  range: (lo, hi), None =
        autoRange (min / max of the region's finite values).  Returns an ImageStatistics."""
        return self._processed_statistics(data, buffer, bscans, ascans, depth, bins, range, False)[0]

    def processed_statistics_timed(self, data=None, buffer=None, bscans=None, ascans=None, depth=None, bins=256, range=None):
        """octpipe_debug_processed_statistics: (ImageStatistics, device time of the call's work in ms)"""
        return self._processed_statistics(data, buffer, bscans, ascans, depth, bins, range, True)

    def _raw_statistics(self, raw, bscans, ascans, samples, bins, lo, bin_width, timed):
        self._sync_params()
        r = self._stats_region(None, bscans, ascans, samples, self.N)
        ptr, dev, keep = self._raw_arg(raw)
        auto = 1 if lo is None else 0
        lo = 0 if lo is None else int(lo)
        bw = 1 if bin_width is None else int(bin_width)
        hist, st, ms = np.zeros(int(bins), np.uint64), _lib.ImageStatistics(), C.c_double()
        args = [self._h, C.c_void_p(ptr), dev, C.byref(r), int(bins), auto, lo, bw, hist.ctypes.data, C.byref(st)]
        if timed:
            check(self._lib.octpipe_debug_raw_statistics(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_raw_statistics(*args))
        del keep
        return ImageStatistics(st, hist), ms.value

    def raw_statistics(self, raw, bscans=None, ascans=None, samples=None, bins=4096, lo=None, bin_width=None):
        """Histogram and moments of a region of one raw buffer (numpy, torch tensor or device pointer) in the handle's sample format,
        decoded with the current bitshift.  lo / bin_width: the integer range (bin_width None = 1); lo None = autoRange (lo = min,
        binWidth = max(1, ceil((max - min + 1) / bins))).  Returns an ImageStatistics."""
        return self._raw_statistics(raw, bscans, ascans, samples, bins, lo, bin_width, False)[0]

    def raw_statistics_timed(self, raw, bscans=None, ascans=None, samples=None, bins=4096, lo=None, bin_width=None):
        """octpipe_debug_raw_statistics: (ImageStatistics, device time of the call's work in ms)"""
        return self._raw_statistics(raw, bscans, ascans, samples, bins, lo, bin_width, True)

    # peak analysis (include/octpipe.h) -------------------------------------------------------------------
    def _peak_analysis(self, data, buffer, bscans, ascans, depth, ascans_per_group, threshold, fit, fit_half_width, max_iterations,
                       averaged, timed):
        if data is not None and buffer not in (None, 0):
            raise ValueError("with data, buffer must be None or 0")
        r = self._stats_region(buffer, bscans, ascans, depth, self.N // 2)
        g = int(r.ascanCount) if ascans_per_group is None else int(ascans_per_group)
        if g < 1 or r.ascanCount % g:
            raise ValueError("ascans_per_group = %d must divide the region's %d A-scans" % (g, r.ascanCount))
        s = _lib.PeakSettings(g, float(threshold), 1 if fit else 0, int(fit_half_width), int(max_iterations))
        shape = (int(r.bscanCount), int(r.ascanCount) // g)
        peaks = (_lib.Peak * (shape[0] * shape[1]))()
        avg = np.zeros((shape[0] * shape[1], int(r.sampleCount)), np.float32) if averaged else None
        ptr, dev, keep = (None, 0, None) if data is None else self._float_arg(data)
        ms = C.c_double()
        args = [self._h, C.c_void_p(ptr), dev, C.byref(r), C.byref(s), peaks, None if avg is None else avg.ctypes.data]
        if timed:
            check(self._lib.octpipe_debug_peak_analysis(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_peak_analysis(*args))
        del keep
        rec = np.ctypeslib.as_array(peaks)
        return PeakAnalysis(rec, shape, avg), ms.value

    def peak_analysis(self, data=None, buffer=None, bscans=None, ascans=None, depth=None, ascans_per_group=None, threshold=-np.inf, fit=True,
                      fit_half_width=0, max_iterations=0, averaged=False):
        """Averaged A-scans of groups of a region of processed data, their peak, half-maximum width and Gaussian fit (the Peak Detector
        and Axial PSF Analyzer extensions).  data / buffer / bscans / ascans / depth: as processed_statistics.  ascans_per_group: G,
        None = the whole A-scan range (one averaged A-scan per B-scan, as the extensions); 1 = one result per A-scan.  threshold: the
        minimum peak value.  fit: the Gaussian fit (fit_half_width 0: from the width; max_iterations 0: 100).  averaged: also return
        the averaged A-scans.  Returns a PeakAnalysis."""
        return self._peak_analysis(data, buffer, bscans, ascans, depth, ascans_per_group, threshold, fit, fit_half_width, max_iterations,
                                   averaged, False)[0]

    def peak_analysis_timed(self, data=None, buffer=None, bscans=None, ascans=None, depth=None, ascans_per_group=None, threshold=-np.inf,
                            fit=True, fit_half_width=0, max_iterations=0, averaged=False):
        """octpipe_debug_peak_analysis: (PeakAnalysis, device time of the call's work in ms)"""
        return self._peak_analysis(data, buffer, bscans, ascans, depth, ascans_per_group, threshold, fit, fit_half_width, max_iterations,
                                   averaged, True)

    # surface views (include/octpipe.h) ---------------------------------------------------------------------
    def _surface_arg(self, surface, entries, what="surface", of="the region has %d A-scans"):
        """(pointer, is_device, keep-alive) of a surface (or another map) of `entries` int32: numpy array, CUDA int32 tensor or device pointer"""
        if hasattr(surface, "data_ptr"):
            if not surface.is_contiguous():
                raise ValueError("%s tensor must be contiguous" % what)
            if surface.is_cuda:
                if str(surface.dtype) != "torch.int32" or surface.numel() != entries:
                    raise ValueError("%s tensor must hold %d int32 entries" % (what, entries))
                return surface.data_ptr(), 1, surface
            surface = surface.numpy()
        if isinstance(surface, np.ndarray):
            a = np.ascontiguousarray(surface, dtype=np.int32)
            if a.size != entries:
                raise ValueError(("%s holds %d entries, " + of) % (what, a.size, entries))
            return a.ctypes.data, 0, a
        return int(surface), 1, None

    @staticmethod
    def _result_arg(out, shape, dtype):
        """(pointer, is_device, what the call returns) of a result: None = a new numpy array, or a CUDA tensor of that many elements"""
        if out is None:
            a = np.empty(shape, dtype)
            return a.ctypes.data, 0, a
        if not (hasattr(out, "data_ptr") and out.is_cuda and out.is_contiguous()):
            raise ValueError("out must be None or a contiguous CUDA tensor")
        if str(out.dtype) != "torch." + np.dtype(dtype).name or out.numel() != int(np.prod(shape)):
            raise ValueError("out must hold %d %s values" % (int(np.prod(shape)), np.dtype(dtype).name))
        return out.data_ptr(), 1, out

    def _source(self, data, buffer, bscans, ascans, depth):
        if data is not None and buffer not in (None, 0):
            raise ValueError("with data, buffer must be None or 0")
        r = self._stats_region(buffer, bscans, ascans, depth, self.N // 2)
        ptr, dev, keep = (None, 0, None) if data is None else self._float_arg(data)
        return r, C.c_void_p(ptr), dev, keep

    def _detect_surface(self, threshold, run, data, buffer, bscans, ascans, depth, out, timed):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        s = _lib.SurfaceDetectSettings(float(threshold), int(run))
        optr, odev, res = self._result_arg(out, (int(r.bscanCount), int(r.ascanCount)), np.int32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.byref(s), C.c_void_p(optr), odev]
        if timed:
            check(self._lib.octpipe_debug_surface_detect(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_surface_detect(*args))
        del keep
        return res, ms.value

    def detect_surface(self, threshold, run=1, data=None, buffer=None, bscans=None, ascans=None, depth=None, out=None):
        """The first interface of every A-scan of a region of processed data: the smallest depth bin inside the window `depth` at which
        `run` consecutive values exceed `threshold`, -1 where there is none.  data / buffer / bscans / ascans / depth: as
        processed_statistics.  Returns an int32 array [bscans][ascans] of absolute depth bins; with out = a CUDA int32 tensor the
        surface stays on the device (the tensor is returned; the work is queued on the handle's stream and the call does not wait:
        synchronize() before another stream reads the tensor)."""
        return self._detect_surface(threshold, run, data, buffer, bscans, ascans, depth, out, False)[0]

    def detect_surface_timed(self, threshold, run=1, data=None, buffer=None, bscans=None, ascans=None, depth=None, out=None):
        """octpipe_debug_surface_detect: (surface, device time of the call's work in ms)"""
        return self._detect_surface(threshold, run, data, buffer, bscans, ascans, depth, out, True)

    def _smooth_surface(self, surface, radius, out, timed):
        shape = tuple(int(x) for x in surface.shape)
        if len(shape) != 2:
            raise ValueError("surface must be two-dimensional (pass a numpy array or a tensor)")
        sptr, sdev, keep = self._surface_arg(surface, shape[0] * shape[1])
        optr, odev, res = self._result_arg(out, shape, np.int32)
        ms = C.c_double()
        args = [self._h, C.c_void_p(sptr), sdev, shape[0], shape[1], int(radius), C.c_void_p(optr), odev]
        if timed:
            check(self._lib.octpipe_debug_surface_smooth(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_surface_smooth(*args))
        del keep
        return res, ms.value

    def smooth_surface(self, surface, radius=1, out=None):
        """The lower median of the valid (non-negative) entries in the (2 radius + 1)^2 neighbourhood of every entry of a surface (numpy
        array or CUDA int32 tensor, two-dimensional); holes are filled from their neighbours, -1 where the neighbourhood has none.
        out: as detect_surface."""
        return self._smooth_surface(surface, radius, out, False)[0]

    def smooth_surface_timed(self, surface, radius=1, out=None):
        """octpipe_debug_surface_smooth: (surface, device time of the call's work in ms)"""
        return self._smooth_surface(surface, radius, out, True)

    def _surface_enface(self, surface, offset, thickness, function, fill, data, buffer, bscans, ascans, depth, out, timed):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        fn = {"average": 0, "mip": 1}.get(function, function)
        shape = (int(r.bscanCount), int(r.ascanCount))
        s = _lib.SurfaceEnfaceSettings(int(offset), int(thickness), int(fn), float(fill))
        sptr, sdev, skeep = self._surface_arg(surface, shape[0] * shape[1])
        optr, odev, res = self._result_arg(out, shape, np.float32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.c_void_p(sptr), sdev, C.byref(s), C.c_void_p(optr), odev]
        if timed:
            check(self._lib.octpipe_debug_surface_enface(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_surface_enface(*args))
        del keep, skeep
        return res, ms.value

    def surface_enface(self, surface, offset=0, thickness=1, function="average", fill=0.0, data=None, buffer=None, bscans=None, ascans=None,
                       depth=None, out=None):
        """An en face image that follows a surface: per A-scan the average ("average") or the maximum ("mip") of the `thickness` bins
        from surface + offset on, as far as they lie inside the window `depth`; `fill` where there is no surface or no such bin.
        surface: numpy array, CUDA int32 tensor or device pointer, [bscans][ascans] of the region.  The other keywords as
        detect_surface.  Returns a float32 array [bscans][ascans] (out = a CUDA float32 tensor: the image stays on the device)."""
        return self._surface_enface(surface, offset, thickness, function, fill, data, buffer, bscans, ascans, depth, out, False)[0]

    def surface_enface_timed(self, surface, offset=0, thickness=1, function="average", fill=0.0, data=None, buffer=None, bscans=None,
                             ascans=None, depth=None, out=None):
        """octpipe_debug_surface_enface: (image, device time of the call's work in ms)"""
        return self._surface_enface(surface, offset, thickness, function, fill, data, buffer, bscans, ascans, depth, out, True)

    def _flatten(self, surface, anchor, depth, fill, out, data, buffer, bscans, ascans, window, loads, timed):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, window)
        rows = int(r.sampleCount) if depth is None else int(depth)
        shape = (int(r.bscanCount), int(r.ascanCount), rows)
        s = _lib.FlattenSettings(int(anchor), rows, float(fill))
        sptr, sdev, skeep = self._surface_arg(surface, shape[0] * shape[1])
        optr, odev, res = self._result_arg(out, shape, np.float32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.c_void_p(sptr), sdev, C.byref(s), C.c_void_p(optr), odev]
        if timed:
            check(self._lib.octpipe_debug_flatten(*args, int(loads), C.byref(ms)))
        else:
            check(self._lib.octpipe_flatten(*args))
        del keep, skeep
        return res, ms.value

    def flatten(self, surface, anchor=0, depth=None, fill=0.0, out=None, data=None, buffer=None, bscans=None, ascans=None, window=None):
        """The region with every A-scan shifted so that its surface lands in row `anchor`: a float32 array [bscans][ascans][depth]
        (depth: rows of the output, None = the size of the depth window) whose row j holds bin surface - anchor + j where that lies
        inside the window, else `fill`.  window: the (first, count) depth window the other calls name `depth`.  surface, out and the
        other keywords as surface_enface."""
        return self._flatten(surface, anchor, depth, fill, out, data, buffer, bscans, ascans, window, 0, False)[0]

    def flatten_timed(self, surface, anchor=0, depth=None, fill=0.0, out=None, data=None, buffer=None, bscans=None, ascans=None, window=None,
                      loads=0):
        """octpipe_debug_flatten: (volume, device time of the call's work in ms); loads: 0 the product's form, 1 dword loads, 2 aligned
        16-byte loads with a cross-lane shift"""
        return self._flatten(surface, anchor, depth, fill, out, data, buffer, bscans, ascans, window, loads, True)

    # boundary tracing (include/octpipe.h) ------------------------------------------------------------------
    def _trace_boundary(self, guide, band, half_width, polarity, max_step, smoothness, cost, out, data, buffer, bscans, ascans, depth, form,
                        timed):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        pol = {"rising": 1, "falling": -1}.get(polarity, polarity)
        shape = (int(r.bscanCount), int(r.ascanCount))
        s = _lib.BoundaryTraceSettings(int(band[0]), int(band[1]), int(half_width), int(pol), int(max_step), float(smoothness))
        gptr, gdev, gkeep = (None, 0, None) if guide is None else self._surface_arg(guide, shape[0] * shape[1], "guide")
        optr, odev, res = self._result_arg(out, shape, np.int32)
        costs, cptr = None, None
        if cost and odev:
            import torch
            costs = torch.empty(shape[0], dtype=torch.float32, device=out.device)
            cptr = costs.data_ptr()
        elif cost:
            costs = np.empty(shape[0], np.float32)
            cptr = costs.ctypes.data
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.c_void_p(gptr), gdev, C.byref(s), C.c_void_p(optr), C.c_void_p(cptr), odev]
        if timed:
            check(self._lib.octpipe_debug_trace_boundary(*args, int(form), C.byref(ms)))
        else:
            check(self._lib.octpipe_trace_boundary(*args))
        del keep, gkeep
        return ((res, costs) if cost else res), ms.value

    def trace_boundary(self, guide=None, band=(-16, 16), half_width=2, polarity=1, max_step=1, smoothness=0.0, cost=False, out=None,
                       data=None, buffer=None, bscans=None, ascans=None, depth=None):
        """A layer boundary by graph search: per B-scan of the region the path from its first to its last A-scan that minimises the
        summed vertical gradient cost (`half_width` bins below minus `half_width` bins above the node; polarity 1 / "rising": dark above
        and bright below, -1 / "falling": the reverse) plus `smoothness` per bin of depth change, which is at most `max_step` bins
        between neighbouring A-scans.  guide: None (every bin of the window `depth` is a node, at most 1024), or a surface
        [bscans][ascans] (numpy array, CUDA int32 tensor or device pointer; negative = none) around which the nodes are the bins
        guide + band[0] ... guide + band[1].  Returns an int32 array [bscans][ascans] of absolute depth bins (-1 where the guide has
        a hole or the path leaves the window); with cost=True (surface, float32 path cost per B-scan).  out and the other keywords as
        detect_surface; with out the costs are a CUDA tensor as well."""
        return self._trace_boundary(guide, band, half_width, polarity, max_step, smoothness, cost, out, data, buffer, bscans, ascans, depth,
                                    0, False)[0]

    def trace_boundary_timed(self, guide=None, band=(-16, 16), half_width=2, polarity=1, max_step=1, smoothness=0.0, cost=False, out=None,
                             data=None, buffer=None, bscans=None, ascans=None, depth=None, form=0):
        """octpipe_debug_trace_boundary: (result, device time of the call's work in ms); form: 0 the product's pick, 1 / 2 one wave per
        B-scan with the choices in LDS / in scratch, 3 / 4 one workgroup per B-scan likewise"""
        return self._trace_boundary(guide, band, half_width, polarity, max_step, smoothness, cost, out, data, buffer, bscans, ascans, depth,
                                    form, True)

    # angiography (include/octpipe.h) -----------------------------------------------------------------------
    @staticmethod
    def _angio_settings(repeats, method, threshold, masked):
        code = {"variance": _lib.ANGIO_VARIANCE, "decorrelation": _lib.ANGIO_DECORRELATION, "difference": _lib.ANGIO_DIFFERENCE}.get(method, method)
        if threshold is None:
            return _lib.AngioSettings(int(repeats), int(code), 0, 0.0, float(masked))
        return _lib.AngioSettings(int(repeats), int(code), 1, float(threshold), float(masked))

    def _registration(self, r, repeats, shifts, ascans_per_group, fill):
        """(pointer, is_device, OctPipeAngioRegistration, keep-alive) of the shifts of a registered angiography call"""
        g = int(r.ascanCount) if ascans_per_group is None else int(ascans_per_group)
        if g < 1 or r.ascanCount % g:
            raise ValueError("ascans_per_group = %d must divide the region's %d A-scans" % (g, r.ascanCount))
        entries = int(r.bscanCount) // max(1, int(repeats)) * int(repeats) * (int(r.ascanCount) // g)
        ptr, dev, keep = self._surface_arg(shifts, entries, "shifts", "positions x repeats x groups is %d")
        return C.c_void_p(ptr), dev, _lib.AngioRegistration(g, float(fill)), keep

    def _angiogram(self, repeats, method, threshold, masked, mean, data, buffer, bscans, ascans, depth, out, timed, shifts=None,
                   ascans_per_group=None, uncovered=0.0):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        s = self._angio_settings(repeats, method, threshold, masked)
        shape = (int(r.bscanCount) // max(1, int(repeats)), int(r.ascanCount), int(r.sampleCount))
        optr, odev, res = self._result_arg(out, shape, np.float32)
        mptr, mres = None, None
        if mean is not False and mean is not None:
            if odev and mean is True:
                mean = out.new_empty(out.shape)
            if (not hasattr(mean, "data_ptr")) if odev else (mean is not True):
                raise ValueError("mean must be False or True, or with out= a CUDA tensor a CUDA tensor like it")
            mptr, _, mres = self._result_arg(mean if odev else None, shape, np.float32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.byref(s), C.c_void_p(optr), C.c_void_p(mptr), odev]
        if shifts is not None:
            sptr, sdev, reg, skeep = self._registration(r, repeats, shifts, ascans_per_group, uncovered)
            args += [sptr, sdev, C.byref(reg)]
            if timed:
                check(self._lib.octpipe_debug_angiogram_registered(*args, C.byref(ms)))
            else:
                check(self._lib.octpipe_angiogram_registered(*args))
            del skeep
        elif timed:
            check(self._lib.octpipe_debug_angiogram(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_angiogram(*args))
        del keep
        return (res if mres is None else (res, mres)), ms.value

    def angiogram(self, repeats, method="variance", threshold=None, masked=0.0, mean=False, data=None, buffer=None, bscans=None, ascans=None,
                  depth=None, out=None, shifts=None, ascans_per_group=None, uncovered=0.0):
        """OCT angiography: the contrast between the `repeats` consecutive B-scans of every slow-axis position of a region of processed
        data, a float32 array [bscans / repeats][ascans][depth].  method: "variance" (speckle variance), "decorrelation" (amplitude
        decorrelation of neighbouring repeats) or "difference" (mean absolute difference of neighbouring repeats).  threshold: None =
        no mask; otherwise the contrast is replaced by `masked` wherever the mean of the repeats does not exceed it.  mean=True: returns
        (angiogram, mean of the repeats).  data / buffer / bscans / ascans / depth: as processed_statistics.  out = a CUDA float32
        tensor: the result stays on the device (as detect_surface; the mean then is a CUDA tensor too, mean= may name it).
        shifts: None = bin against the same bin; otherwise what register_repeats returned for the same region, repeats and
        ascans_per_group (numpy array, CUDA int32 tensor or device pointer): every repeat is read at its shifted bins, and the bins of
        the window that not every repeat covers hold `uncovered` in the angiogram and in the mean."""
        return self._angiogram(repeats, method, threshold, masked, mean, data, buffer, bscans, ascans, depth, out, False, shifts,
                               ascans_per_group, uncovered)[0]

    def angiogram_timed(self, repeats, method="variance", threshold=None, masked=0.0, mean=False, data=None, buffer=None, bscans=None,
                        ascans=None, depth=None, out=None, shifts=None, ascans_per_group=None, uncovered=0.0):
        """octpipe_debug_angiogram / octpipe_debug_angiogram_registered: (what angiogram returns, device time of the call's work in ms)"""
        return self._angiogram(repeats, method, threshold, masked, mean, data, buffer, bscans, ascans, depth, out, True, shifts,
                               ascans_per_group, uncovered)

    def _angiogram_enface(self, repeats, method, threshold, masked, surface, offset, thickness, function, fill, data, buffer, bscans, ascans,
                          depth, out, form, timed, shifts=None, ascans_per_group=None):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        s = self._angio_settings(repeats, method, threshold, masked)
        fn = {"average": 0, "mip": 1}.get(function, function)
        slab = _lib.SurfaceEnfaceSettings(int(offset), int(thickness), int(fn), float(fill))
        shape = (int(r.bscanCount) // max(1, int(repeats)), int(r.ascanCount))
        sptr, sdev, skeep = (None, 0, None) if surface is None else self._surface_arg(surface, int(r.bscanCount) * int(r.ascanCount))
        optr, odev, res = self._result_arg(out, shape, np.float32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.byref(s), C.c_void_p(sptr), sdev, C.byref(slab), C.c_void_p(optr), odev]
        if shifts is not None:
            hptr, hdev, reg, hkeep = self._registration(r, repeats, shifts, ascans_per_group, 0.0)
            args += [hptr, hdev, C.byref(reg)]
            if timed:
                check(self._lib.octpipe_debug_angiogram_enface_registered(*args, int(form), C.byref(ms)))
            else:
                check(self._lib.octpipe_angiogram_enface_registered(*args))
            del hkeep
        elif timed:
            check(self._lib.octpipe_debug_angiogram_enface(*args, int(form), C.byref(ms)))
        else:
            check(self._lib.octpipe_angiogram_enface(*args))
        del keep, skeep
        return res, ms.value

    def angiogram_enface(self, repeats, method="variance", threshold=None, masked=0.0, surface=None, offset=0, thickness=1, function="average",
                         fill=0.0, data=None, buffer=None, bscans=None, ascans=None, depth=None, out=None, shifts=None, ascans_per_group=None):
        """An en face angiogram: the contrast of angiogram() inside a slab of `thickness` bins, averaged ("average") or its maximum
        ("mip"), a float32 array [bscans / repeats][ascans]; the contrast volume is never written.  surface: None = the slab starts
        `offset` bins below the first bin of the window `depth`; otherwise what detect_surface / smooth_surface return for the same
        region ([bscans][ascans]: numpy array, CUDA int32 tensor or device pointer), every position using the row of its first repeat.
        `fill` where there is no surface or no bin of the slab inside the window.  shifts / ascans_per_group: as angiogram (the slab
        then is clipped to the bins that every repeat covers).  The other keywords as angiogram."""
        return self._angiogram_enface(repeats, method, threshold, masked, surface, offset, thickness, function, fill, data, buffer, bscans,
                                      ascans, depth, out, 0, False, shifts, ascans_per_group)[0]

    def angiogram_enface_timed(self, repeats, method="variance", threshold=None, masked=0.0, surface=None, offset=0, thickness=1,
                               function="average", fill=0.0, data=None, buffer=None, bscans=None, ascans=None, depth=None, out=None, form=0,
                               shifts=None, ascans_per_group=None):
        """octpipe_debug_angiogram_enface: (image, device time of the call's work in ms); form: 0 the product's choice, 1 one wave per
        A-scan, 2 teams of 16 lanes with four A-scans per wave (thickness <= 64)"""
        return self._angiogram_enface(repeats, method, threshold, masked, surface, offset, thickness, function, fill, data, buffer, bscans,
                                      ascans, depth, out, form, True, shifts, ascans_per_group)

    # repeat registration (include/octpipe.h) ---------------------------------------------------------------
    def _register_repeats(self, repeats, ascans_per_group, max_shift, costs, data, buffer, bscans, ascans, depth, out, timed):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        g = int(r.ascanCount) if ascans_per_group is None else int(ascans_per_group)
        if g < 1 or r.ascanCount % g:
            raise ValueError("ascans_per_group = %d must divide the region's %d A-scans" % (g, r.ascanCount))
        M, R = int(repeats), int(max_shift)
        s = _lib.RepeatShiftSettings(M, g, R)
        P, Qp = int(r.bscanCount) // max(1, M), int(r.ascanCount) // g
        optr, odev, res = self._result_arg(out, (P, M, Qp), np.int32)
        cptr, cres = None, None
        if costs is not False and costs is not None:
            if odev and costs is True:
                import torch
                costs = torch.empty((P, max(M - 1, 0), Qp, 2 * R + 1), dtype=torch.float64, device=out.device)
            if (not hasattr(costs, "data_ptr")) if odev else (costs is not True):
                raise ValueError("costs must be False or True, or with out= a CUDA tensor a CUDA float64 tensor")
            cptr, _, cres = self._result_arg(costs if odev else None, (P, max(M - 1, 0), Qp, 2 * R + 1), np.float64)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.byref(s), C.c_void_p(optr), odev, C.c_void_p(cptr)]
        if timed:
            check(self._lib.octpipe_debug_repeat_shifts(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_repeat_shifts(*args))
        del keep
        return (res if cres is None else (res, cres)), ms.value

    def register_repeats(self, repeats, ascans_per_group=None, max_shift=8, costs=False, data=None, buffer=None, bscans=None, ascans=None,
                         depth=None, out=None):
        """Bulk-motion registration of the `repeats` consecutive B-scans of every slow-axis position: the axial shift, in depth bins within
        +-max_shift, of every repeat against the first one, an int32 array [bscans / repeats][repeats][ascans / ascans_per_group] (entry 0 of
        every position is 0).  One shift per group of ascans_per_group A-scans, estimated on the group's averaged A-scan (that of
        peak_analysis); None = the whole A-scan range, one shift per B-scan.  costs=True: returns (shifts, costs), costs a float64 array
        [bscans / repeats][repeats - 1][groups][2 max_shift + 1] of the summed absolute differences per lag.  data / buffer / bscans /
        ascans / depth: as processed_statistics.  out = a CUDA int32 tensor: the shifts stay on the device (as detect_surface; the costs
        then are a CUDA float64 tensor, costs= may name it) and can be handed to angiogram(shifts=) / angiogram_enface(shifts=)."""
        return self._register_repeats(repeats, ascans_per_group, max_shift, costs, data, buffer, bscans, ascans, depth, out, False)[0]

    def register_repeats_timed(self, repeats, ascans_per_group=None, max_shift=8, costs=False, data=None, buffer=None, bscans=None, ascans=None,
                               depth=None, out=None):
        """octpipe_debug_repeat_shifts: (what register_repeats returns, device time of the call's work in ms)"""
        return self._register_repeats(repeats, ascans_per_group, max_shift, costs, data, buffer, bscans, ascans, depth, out, True)

    # attenuation (include/octpipe.h) -----------------------------------------------------------------------
    def intensity_map(self):
        """(scale, a, b) that turns the handle's processed values back into what the attenuation works on, from the current parameters: the
        grey-scale mapping v = coeff * ((y - min) / (max - min) + addend) of the last stage of the chain (cu:718 / cu:739) inverted, y = v * a'
        + b'.  signalLogScaling on: y = 10 log10 of the power, so ("log2", a' log2(10) / 10, b' log2(10) / 10); off: y is the amplitude,
        ("amplitude", a', b').  ValueError naming the field where no such map exists: postProcessBackgroundRemoval on (that stage saturates)
        or signalMultiplicator == 0."""
        p = self.params
        if p.postProcessBackgroundRemoval:
            raise ValueError("postProcessBackgroundRemoval is on: the processed values are saturated, no map gives the intensity back")
        coeff, addend = float(p.signalMultiplicator), float(p.signalAddend)
        lo, hi = float(p.signalGrayscaleMin), float(p.signalGrayscaleMax)
        if coeff == 0.0:
            raise ValueError("signalMultiplicator is 0: the processed values do not depend on the signal")
        if p.signalLogScaling:
            return "log2", (hi - lo) * math.log2(10.0) / (10.0 * coeff), (lo - addend * (hi - lo)) * math.log2(10.0) / 10.0
        return "amplitude", (hi - lo) / coeff, lo - addend * (hi - lo)

    def _gain_arg(self, gain, entries):
        """(pointer, is_device, keep-alive) of a gain table of `entries` float32: numpy array, CUDA float32 tensor or device pointer"""
        if hasattr(gain, "data_ptr"):
            if not gain.is_contiguous():
                raise ValueError("gain tensor must be contiguous")
            if gain.is_cuda:
                if str(gain.dtype) != "torch.float32" or gain.numel() != entries:
                    raise ValueError("gain tensor must hold %d float32 entries" % entries)
                return gain.data_ptr(), 1, gain
            gain = gain.numpy()
        if isinstance(gain, np.ndarray):
            a = np.ascontiguousarray(gain, dtype=np.float32)
            if a.size != entries:
                raise ValueError("gain holds %d entries, the depth window has %d bins" % (a.size, entries))
            return a.ctypes.data, 0, a
        return int(gain), 1, None

    def _attenuation_settings(self, pixel_size, scale, map, noise, tail, undefined, data):
        if scale is None:
            if data is not None:
                raise ValueError('with data, say what it holds: scale="intensity", "amplitude" or "log2" (and map=(a, b))')
            if map is not None:
                raise ValueError("map= goes with scale=; scale=None takes both from intensity_map()")
            scale, a, b = self.intensity_map()
        else:
            a, b = (1.0, 0.0) if map is None else map
        code = {"intensity": _lib.ATTENUATION_INTENSITY, "amplitude": _lib.ATTENUATION_AMPLITUDE, "log2": _lib.ATTENUATION_LOG2}.get(scale, scale)
        s = _lib.AttenuationSettings(float(a), float(b), int(code), float(pixel_size), float(noise), float(tail), 0.0, 0)
        # `undefined` keeps its bits: a float32 NaN payload would not survive the way through a Python float
        bits = np.asarray(undefined, dtype=np.float32).reshape(1)
        C.memmove(C.addressof(s) + _lib.AttenuationSettings.undefined.offset, bits.ctypes.data, 4)
        return s

    def _attenuation(self, pixel_size, scale, map, noise, tail, gain, undefined, data, buffer, bscans, ascans, depth, out, timed, sums=False):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        s = self._attenuation_settings(pixel_size, scale, map, noise, tail, undefined, data)
        gptr, gdev, gkeep = (None, 0, None) if gain is None else self._gain_arg(gain, int(r.sampleCount))
        shape = (int(r.bscanCount), int(r.ascanCount), int(r.sampleCount))
        optr, odev, res = self._result_arg(out, shape, np.float64 if sums else np.float32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.byref(s), C.c_void_p(gptr), gdev, C.c_void_p(optr), odev]
        if sums:
            check(self._lib.octpipe_debug_attenuation_sums(*args))
        elif timed:
            check(self._lib.octpipe_debug_attenuation(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_attenuation(*args))
        del keep, gkeep
        return res, ms.value

    def attenuation(self, pixel_size, scale=None, map=None, noise=0.0, tail=0.0, gain=None, undefined=np.nan, data=None, buffer=None,
                    bscans=None, ascans=None, depth=None, out=None):
        """The depth-resolved attenuation coefficient (Vermeer et al. 2014) of every bin of a region of processed data, mu[i] = I[i] /
        (2 pixel_size * sum of the I below bin i), a float32 array [bscans][ascans][depth] in the inverse unit of pixel_size (the length of
        one depth bin in the sample).  The intensity of a bin is its value v mapped by x = v * a + b, map = (a, b), and read according to
        scale: "intensity" (x), "amplitude" (x * x) or "log2" (2 ** x); then `noise` is subtracted, the result multiplied by the bin's entry of
        `gain` (a roll-off correction of one float32 per bin of the depth window: numpy array, CUDA tensor or device pointer) and clamped at
        0.  scale=None (the handle's own volume only): scale and map are intensity_map().  tail: the intensity below the window, 0 if
        unknown.  undefined: what the bins hold that have nothing below them.  data / buffer / bscans / ascans / depth: as
        processed_statistics.  out = a CUDA float32 tensor: the result stays on the device (as detect_surface)."""
        return self._attenuation(pixel_size, scale, map, noise, tail, gain, undefined, data, buffer, bscans, ascans, depth, out, False)[0]

    def attenuation_timed(self, pixel_size, scale=None, map=None, noise=0.0, tail=0.0, gain=None, undefined=np.nan, data=None, buffer=None,
                          bscans=None, ascans=None, depth=None, out=None):
        """octpipe_debug_attenuation: (volume, device time of the call's work in ms)"""
        return self._attenuation(pixel_size, scale, map, noise, tail, gain, undefined, data, buffer, bscans, ascans, depth, out, True)

    def attenuation_sums(self, pixel_size, scale=None, map=None, noise=0.0, tail=0.0, gain=None, data=None, buffer=None, bscans=None,
                         ascans=None, depth=None, out=None):
        """octpipe_debug_attenuation_sums: the float64 sum of the intensities below every bin, [bscans][ascans][depth], in the order the
        attenuation defines (out = a CUDA float64 tensor: it stays on the device)"""
        return self._attenuation(pixel_size, scale, map, noise, tail, gain, np.nan, data, buffer, bscans, ascans, depth, out, False, True)[0]

    def _attenuation_enface(self, pixel_size, surface, offset, thickness, function, fill, scale, map, noise, tail, gain, undefined, data, buffer,
                            bscans, ascans, depth, out, timed):
        r, ptr, dev, keep = self._source(data, buffer, bscans, ascans, depth)
        s = self._attenuation_settings(pixel_size, scale, map, noise, tail, undefined, data)
        gptr, gdev, gkeep = (None, 0, None) if gain is None else self._gain_arg(gain, int(r.sampleCount))
        fn = {"average": 0, "mip": 1}.get(function, function)
        slab = _lib.SurfaceEnfaceSettings(int(offset), int(thickness), int(fn), float(fill))
        shape = (int(r.bscanCount), int(r.ascanCount))
        sptr, sdev, skeep = (None, 0, None) if surface is None else self._surface_arg(surface, shape[0] * shape[1])
        optr, odev, res = self._result_arg(out, shape, np.float32)
        ms = C.c_double()
        args = [self._h, ptr, dev, C.byref(r), C.byref(s), C.c_void_p(gptr), gdev, C.c_void_p(sptr), sdev, C.byref(slab), C.c_void_p(optr), odev]
        if timed:
            check(self._lib.octpipe_debug_attenuation_enface(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_attenuation_enface(*args))
        del keep, gkeep, skeep
        return res, ms.value

    def attenuation_enface(self, pixel_size, surface=None, offset=0, thickness=1, function="average", fill=0.0, scale=None, map=None, noise=0.0,
                           tail=0.0, gain=None, undefined=np.nan, data=None, buffer=None, bscans=None, ascans=None, depth=None, out=None):
        """An en face attenuation map: the coefficient of attenuation() inside a slab of `thickness` bins, averaged ("average") or its
        maximum ("mip"), a float32 array [bscans][ascans] -- what surface_enface() returns for the volume attenuation() writes, without that
        volume ever being written.  surface: None = the slab starts `offset` bins below the first bin of the window `depth`; otherwise what
        detect_surface / smooth_surface return for the same region (numpy array, CUDA int32 tensor or device pointer).  `fill` where
        there is no surface or no bin of the slab inside the window.  The other keywords as attenuation."""
        return self._attenuation_enface(pixel_size, surface, offset, thickness, function, fill, scale, map, noise, tail, gain, undefined, data,
                                        buffer, bscans, ascans, depth, out, False)[0]

    def attenuation_enface_timed(self, pixel_size, surface=None, offset=0, thickness=1, function="average", fill=0.0, scale=None, map=None,
                                 noise=0.0, tail=0.0, gain=None, undefined=np.nan, data=None, buffer=None, bscans=None, ascans=None, depth=None,
                                 out=None):
        """octpipe_debug_attenuation_enface: (image, device time of the call's work in ms)"""
        return self._attenuation_enface(pixel_size, surface, offset, thickness, function, fill, scale, map, noise, tail, gain, undefined, data,
                                        buffer, bscans, ascans, depth, out, True)

    # volume rendering (include/octpipe.h) ------------------------------------------------------------------
    def render_settings(self, mode="MIP", size=(512, 512), rotation=(1.0, 0.0, 0.0, 0.0), distance=-500.0, view_pos=(0.0, 0.0), output="f32",
                        **settings):
        """A RenderSettings from the reference's defaults and the keywords of render_volume"""
        s = default_render_settings()
        s.mode = render_mode_code(mode)
        s.width, s.height = int(size[0]), int(size[1])
        if output not in ("f32", "u8"):
            raise ValueError("output must be 'f32' or 'u8'")
        s.outputFormat = _lib.RENDER_RGBA_U8 if output == "u8" else _lib.RENDER_RGBA_F32
        if "view_matrix" not in settings:
            settings["view_matrix"] = render_view_matrix(rotation, view_pos, distance).ravel()
        for key, value in settings.items():
            if key not in _RENDER_FIELDS:
                raise TypeError("unknown render setting %r (one of %s)" % (key, ", ".join(sorted(_RENDER_FIELDS))))
            field = _RENDER_FIELDS[key]
            if field in ("stretch", "background", "material", "lightPosition", "viewMatrix"):
                cur = getattr(s, field)
                vals = [float(v) for v in np.asarray(value, dtype=np.float64).ravel()]
                if len(vals) != len(cur):
                    raise ValueError("%s needs %d values" % (key, len(cur)))
                for i, v in enumerate(vals):
                    cur[i] = v
            elif field in ("smoothFactor", "shadingEnabled", "lutEnabled", "jitterSeed"):
                setattr(s, field, int(value))
            else:
                setattr(s, field, float(value))
        return s

    def _voxel_arg(self, voxels, dims):
        """(pointer, is_device, dims array, keep-alive) of a uint8 volume: numpy [z][y][x], torch tensor, or a device pointer with dims"""
        if voxels is None:
            return None, 0, None, None
        if hasattr(voxels, "data_ptr"):
            if not voxels.is_contiguous() or str(voxels.dtype) != "torch.uint8":
                raise ValueError("voxel tensor must be contiguous uint8")
            if voxels.is_cuda:
                if dims is None:
                    if voxels.dim() != 3:
                        raise ValueError("voxel tensor must be [z][y][x] (or pass dims = (x, y, z))")
                    dims = tuple(voxels.shape)[::-1]
                return voxels.data_ptr(), 1, (C.c_uint32 * 3)(*[int(d) for d in dims]), voxels
            voxels = voxels.numpy()
        if isinstance(voxels, np.ndarray):
            a = np.ascontiguousarray(voxels, dtype=np.uint8)
            if dims is None:
                if a.ndim != 3:
                    raise ValueError("voxels must be [z][y][x] (or pass dims = (x, y, z))")
                dims = a.shape[::-1]
            if int(np.prod([int(d) for d in dims])) != a.size:
                raise ValueError("voxels hold %d bytes, dims %s need %d" % (a.size, tuple(dims), int(np.prod(dims))))
            return a.ctypes.data, 0, (C.c_uint32 * 3)(*[int(d) for d in dims]), a
        if dims is None:
            raise ValueError("a device pointer needs dims = (x, y, z)")
        return int(voxels), 1, (C.c_uint32 * 3)(*[int(d) for d in dims]), None

    def render_volume_device(self, settings, voxels=None, dims=None, timed=False):
        """octpipe_render_volume with a RenderSettings: enqueues the render and returns (device pointer, bytes) of the image without
        waiting for it (timed=True: octpipe_debug_render_volume, waits, returns (pointer, bytes, kernel ms)).  settings.mode =
        RENDER_OCT_DEPTH goes to octpipe_render_oct_depth (timed=True: (pointer, bytes, (pre-pass ms, ray cast ms)))"""
        ptr, dev, dm, keep = self._voxel_arg(voxels, dims)
        img, n, ms = C.c_void_p(), C.c_size_t(), C.c_double()
        args = [self._h, C.c_void_p(ptr), dev, dm, C.byref(settings), C.byref(img), C.byref(n)]
        if settings.mode == _lib.RENDER_OCT_DEPTH:
            pre = C.c_double()
            if timed:
                check(self._lib.octpipe_debug_render_oct_depth(*args, C.byref(pre), C.byref(ms)))
            else:
                check(self._lib.octpipe_render_oct_depth(*args))
            del keep
            return (img.value, n.value, (pre.value, ms.value)) if timed else (img.value, n.value)
        if timed:
            check(self._lib.octpipe_debug_render_volume(*args, C.byref(ms)))
        else:
            check(self._lib.octpipe_render_volume(*args))
        del keep
        return (img.value, n.value, ms.value) if timed else (img.value, n.value)

    def rendered_host(self, settings, origin="lower"):
        """octpipe_copy_rendered_to_host: the last image as numpy [height][width][4], float32 or uint8 by settings.outputFormat;
        origin="lower": row 0 is the bottom of the picture, as the device holds it; "upper": flipped, as image files want it"""
        if origin not in ("lower", "upper"):
            raise ValueError("origin must be 'lower' or 'upper'")
        dt = np.uint8 if settings.outputFormat == _lib.RENDER_RGBA_U8 else np.float32
        out = np.empty((int(settings.height), int(settings.width), 4), dt)
        check(self._lib.octpipe_copy_rendered_to_host(self._h, out.ctypes.data, out.nbytes))
        return out[::-1].copy() if origin == "upper" else out

    def render_volume(self, mode="MIP", size=(512, 512), rotation=(1.0, 0.0, 0.0, 0.0), distance=-500.0, view_pos=(0.0, 0.0), voxels=None,
                      dims=None, output="f32", origin="lower", **settings):
        """Ray-cast the 8-bit volume view of the last processed volume (params.volumeViewEnabled), or `voxels` (uint8 [z][y][x]: numpy,
        torch, or a device pointer with dims = (x, y, z)), into an RGBA image (the reference's volume window).  mode: "MIP", "DMIP",
        "X-ray", "Alpha blending", "MIDA", "Isosurface", "OCT Depth" (colour by depth below the detected surface, surface_map).  size = (width, height); rotation = quaternion (w, x, y, z); distance = the
        reference's distExp; settings: fov, stretch, step_length, threshold, depth_weight, alpha_exponent, gamma, smooth_factor, shading,
        lut, background, material, light_position, jitter_seed, view_matrix (16 values, instead of rotation / distance / view_pos).
        Returns numpy [height][width][4], float32 (output="f32") or uint8 ("u8")."""
        s = self.render_settings(mode, size, rotation, distance, view_pos, output, **settings)
        self.render_volume_device(s, voxels, dims)
        return self.rendered_host(s, origin)

    def surface_map(self, threshold=0.75, voxels=None, dims=None):
        """octpipe_volume_surface_map: per (x, y) column of the volume view (or `voxels`, as in render_volume) the largest depth index
        whose voxel / 255 exceeds `threshold` (0 ... 1.5; the OCT Depth mode uses 1.5 x its render threshold), 0 without one; the top
        1 / 32 of the depth range and index 0 are not examined.  Returns numpy uint16 [y][x]."""
        ptr, dev, dm, keep = self._voxel_arg(voxels, dims)
        if dm is None:
            p = self.params
            nx, ny = int(p.ascansPerBscan), int(p.bscansPerBuffer) * int(p.buffersPerVolume)
        else:
            nx, ny = int(dm[0]), int(dm[1])
        out = np.empty((ny, nx), np.uint16)
        check(self._lib.octpipe_volume_surface_map(self._h, C.c_void_p(ptr), dev, dm, float(threshold), out.ctypes.data))
        del keep
        return out

    def set_render_lut(self, rgba):
        """octpipe_update_render_lut: the 1-D colour table of the volume view, uint8 [width][4] (RGBA), 2 ... 4096 entries"""
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("rgba must be [width][4] uint8")
        check(self._lib.octpipe_update_render_lut(self._h, a.ctypes.data, a.shape[0]))

    @property
    def handle(self):
        return self._h


class PipelineGroup:
    """octpipe_group_* (include/octpipe.h): one buffer per call, B-scan slabs over several GPUs of the node from one process."""

    def __init__(self, params: OctAlgorithmParameters, devices, h_buffer1=None, h_buffer2=None, flags=0):
        self.params = params
        self._lib = _lib.lib()
        _lib.drain_deferred()
        self._g = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        acq, pod = params.acquisition(), params.pod()
        self._keep = (h_buffer1, h_buffer2)
        b1 = h_buffer1.ctypes.data if h_buffer1 is not None else None
        b2 = h_buffer2.ctypes.data if h_buffer2 is not None else None
        # flags: _lib.GROUP_* (octpipe_group_create_ex); on failure the library has released everything and *out is NULL
        if flags:
            rc = self._lib.octpipe_group_create_ex(C.byref(self._g), devs, len(devices), C.byref(acq), C.byref(pod), b1, b2, int(flags))
        else:
            rc = self._lib.octpipe_group_create(C.byref(self._g), devs, len(devices), C.byref(acq), C.byref(pod), b1, b2)
        if rc != 0:
            msg = self._lib.octpipe_group_last_error()
            assert not self._g
            raise _lib.OctPipeError(rc, msg.decode() if msg else "")
        self.N, self.S = int(params.samplesPerLine), params.samplesPerBuffer
        self._sync_params(force_curves=True)

    def _check(self, rc):
        if rc != 0:
            raise _lib.OctPipeError(rc, (self._lib.octpipe_group_last_error() or b"").decode())

    def _sync_params(self, force_curves=False):
        p = self.params
        for flag, upd, curve, setter in (("resampling", "resamplingUpdated", "resampleCurve", self._lib.octpipe_group_update_resample_curve),
                                         ("dispersionCompensation", "dispersionUpdated", "dispersionCurve", self._lib.octpipe_group_update_dispersion_curve),
                                         ("windowing", "windowUpdated", "windowCurve", self._lib.octpipe_group_update_window_curve)):
            c = getattr(p, curve)
            if getattr(p, flag) and (getattr(p, upd) or force_curves) and c is not None:
                c = np.ascontiguousarray(c, dtype=np.float32)
                self._check(setter(self._g, c.ctypes.data, len(c)))
                setattr(p, upd, False)
        if p.postProcessBackgroundRemoval and p.postProcessBackgroundUpdated and p.postProcessBackground is not None:
            c = np.ascontiguousarray(p.postProcessBackground, dtype=np.float32)
            self._check(self._lib.octpipe_group_update_postprocess_background(self._g, c.ctypes.data, len(c)))
            p.postProcessBackgroundUpdated = False
        pod = p.pod()
        self._check(self._lib.octpipe_group_set_params(self._g, C.byref(pod)))
        p.redetermineFixedPatternNoise = 0
        p.postProcessBackgroundRecordingRequested = 0

    @property
    def backend(self):
        return self._lib.octpipe_group_backend(self._g).decode()

    @property
    def broadcasts(self):
        return int(self._lib.octpipe_group_broadcast_count(self._g))

    @property
    def size(self):
        return self._lib.octpipe_group_size(self._g)

    def set_submit_threads(self, enable=True):
        """one submitting host thread per member (opt-in; the default is the calling thread)"""
        self._check(self._lib.octpipe_group_set_submit_threads(self._g, 1 if enable else 0))

    @property
    def info(self):
        t, n = C.c_int(), C.c_int()
        self._check(self._lib.octpipe_group_info(self._g, C.byref(t), C.byref(n)))
        return {"submit_threads": t.value, "slabs_placed_on_gpu_node": n.value,
                "serial_submits": int(self._lib.octpipe_group_serial_submit_count(self._g))}

    def slab(self, i):
        f, n = C.c_uint(), C.c_uint()
        self._check(self._lib.octpipe_group_slab(self._g, i, C.byref(f), C.byref(n)))
        return f.value, n.value

    def octCudaPipeline(self, h_inputSignal):
        self._sync_params()
        a = np.ascontiguousarray(h_inputSignal)
        self._check(self._lib.octpipe_group_process(self._g, a.ctypes.data))

    def process_device(self, slab_ptrs):
        self._sync_params()
        arr = (C.c_void_p * len(slab_ptrs))(*slab_ptrs)
        self._check(self._lib.octpipe_group_process_device(self._g, arr))

    def set_mean_line(self, m, pin=True):
        m = np.ascontiguousarray(m, dtype=np.complex64)
        self._check(self._lib.octpipe_group_set_mean_line(self._g, m.ctypes.data, 1 if pin else 0))

    def synchronize(self):
        self._check(self._lib.octpipe_group_synchronize(self._g))

    def processed_host(self):
        out = np.empty(self.S // 2, dtype=np.float32)
        self._check(self._lib.octpipe_group_copy_processed_to_host(self._g, out.ctypes.data))
        return out

    @property
    def handle(self):
        return self._g

    def close(self):
        if self._g:
            _lib.destroy_or_defer("group", self._g)
            self._g = C.c_void_p()

    cleanupCuda = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
